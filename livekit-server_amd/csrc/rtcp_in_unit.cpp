// rtcp_in_unit.cpp — CPU unit tests of the RTCP ingress parse
// (rtcp_in_device.h): the framing walk, the per-type size checks and the NACK
// pair expansion the kernels k_rtcp_in_count / k_rtcp_in_write compile, and the
// entry rules of include/lkfwd.h on top of them.  Built with the host compiler
// alone (make rtcp_in_unit; address + undefined sanitizers).  Every compound
// packet is parsed from a heap block of exactly its length, so a read past
// the entry trips the sanitizer.
//   rtcp_in_unit --list          the case names
//   rtcp_in_unit <name>          one case ("PASS <name>" / exit 1)
//   rtcp_in_unit                 every case
//   rtcp_in_unit --replay        a script on stdin, results on stdout:
//     e <ssrc> <hex | ->         one entry for a DownTrack with that SSRC; prints
//       e status= reports= nacks= plis= firs= fb=<lsn:lost:jitter:lsr:dlsr:fraction:flags:nacks:plis:firs,..|->
//         sns=<sn,..|-> refs=<kind:off:len,..|->
//   rtcp_in_unit --bench <n> <reps>   the host path's parse, single thread: n compounds (RR + NACK with
//                                     three pairs + SDES, one per DownTrack) into lkf_rtcp_fb[] / lkf_nack[];
//                                     prints "bench n= fb= nacks= ms_min= ms_median= ms_max=" over reps
//   rtcp_in_unit --bench <n> <reps> step   the same, one rep per line read from stdin, "ms=<that rep>" printed
//                                     after each (a caller alternates it with another path, tick by tick)
#define __host__
#define __device__
#include <algorithm>
#include <chrono>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "rtcp_in_device.h"

using namespace lkf;
using namespace lkf::rtcpin;
using Bytes = std::vector<u8>;

static_assert(sizeof(lkf_rtcp_raw) == 12 && sizeof(lkf_rtcp_in_result) == 48 && sizeof(lkf_rtcp_ref) == 16,
              "RTCP ingress records");

static int g_fail = 0;
#define CHECK(c)                                                         \
  do {                                                                   \
    if (!(c)) {                                                          \
      std::printf("  check failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
      g_fail++;                                                          \
    }                                                                    \
  } while (0)

// what one entry yields (the write pass's lists, per entry)
struct Entry {
  u32 status = LKF_RTCP_IN_MALFORMED;
  u32 reports = 0, nacks = 0, plis = 0, firs = 0;
  std::vector<lkf_rtcp_fb> fb;
  std::vector<u16> sns;
  std::vector<lkf_rtcp_ref> refs;
};
struct Collect {
  Entry *e;
  void report(const u8 *b) {
    lkf_rtcp_fb f;
    std::memset(&f, 0, sizeof(f));
    f.flags = LKF_FB_HAS_RR;
    read_report(b, f);
    e->fb.push_back(f);
    e->reports++;
  }
  void pair(u32 pid, u32 blp) {
    const size_t before = e->sns.size();
    pair_expand(pid, blp, [&](u16 sn) { e->sns.push_back(sn); });
    CHECK(e->sns.size() - before == pair_count(blp));
  }
  void pli() { e->plis++; }
  void fir() { e->firs++; }
  void ref(u32 kind, u32 at, u32 size) { e->refs.push_back({0, kind, at, size}); }
};

static Entry parse(const Bytes &src, u32 ssrc) {
  u8 *blk = static_cast<u8 *>(std::malloc(src.size() ? src.size() : 1));  // exactly the entry (1 B when empty: never read)
  if (!src.empty()) std::memcpy(blk, src.data(), src.size());
  Entry e;
  Collect c{&e};
  Counts n;
  const u32 len = u32(src.size());
  const u32 st = walk(src.empty() ? blk + 1 : blk, len, ssrc, c);
  CHECK(walk(src.empty() ? blk + 1 : blk, len, ssrc, n) == st);  // the count pass sees what the write pass writes
  std::free(blk);
  if (st != LKF_RTCP_IN_OK) return Entry();  // the whole entry is void
  CHECK(n.reports == e.reports && n.nacks == e.sns.size() && n.plis == e.plis && n.firs == e.firs &&
        n.refs == e.refs.size());
  e.status = st;
  e.nacks = u32(e.sns.size());
  if (e.fb.empty()) {  // max(1, reports) records, the counts on the last
    lkf_rtcp_fb f;
    std::memset(&f, 0, sizeof(f));
    e.fb.push_back(f);
  }
  e.fb.back().nacks = e.nacks;
  e.fb.back().plis = e.plis;
  e.fb.back().firs = e.firs;
  return e;
}

// ---- a small marshaller for the cases ----
static void put16(Bytes &b, u32 v) { b.push_back(u8(v >> 8)), b.push_back(u8(v)); }
static void put32(Bytes &b, u32 v) { put16(b, v >> 16), put16(b, v & 0xffff); }
static Bytes pkt(u32 count, u32 pt, const Bytes &body, int lengthAdjust = 0, u32 version = 2) {
  Bytes b;
  b.push_back(u8((version << 6) | (count & 31)));
  b.push_back(u8(pt));
  put16(b, u32(int(body.size() / 4) + lengthAdjust));
  b.insert(b.end(), body.begin(), body.end());
  return b;
}
static Bytes block(u32 ssrc, u32 fraction, u32 lost, u32 lsn, u32 jitter, u32 lsr, u32 dlsr) {
  Bytes b;
  put32(b, ssrc);
  put32(b, (fraction << 24) | (lost & 0xffffff));
  put32(b, lsn), put32(b, jitter), put32(b, lsr), put32(b, dlsr);
  return b;
}
static Bytes cat(std::initializer_list<Bytes> parts) {
  Bytes b;
  for (const Bytes &p : parts) b.insert(b.end(), p.begin(), p.end());
  return b;
}
static Bytes rr(u32 sender, std::initializer_list<Bytes> blocks) {
  Bytes body;
  put32(body, sender);
  for (const Bytes &k : blocks) body.insert(body.end(), k.begin(), k.end());
  return pkt(u32(blocks.size()), 201, body);
}
static Bytes nack(u32 media, std::initializer_list<std::pair<u32, u32>> pairs) {
  Bytes body;
  put32(body, 7), put32(body, media);
  for (auto &p : pairs) put16(body, p.first), put16(body, p.second);
  return pkt(1, 205, body);
}
static Bytes psfb(u32 fmt, u32 media, const Bytes &fci = {}) {
  Bytes body;
  put32(body, 7), put32(body, media);
  body.insert(body.end(), fci.begin(), fci.end());
  return pkt(fmt, 206, body);
}
static Bytes remb(const char *id, u32 numSsrc, u32 listed) {
  Bytes fci(id, id + 4);
  fci.push_back(u8(numSsrc)), fci.push_back(0x12), fci.push_back(0x34), fci.push_back(0x56);
  for (u32 i = 0; i < listed; i++) put32(fci, 100 + i);
  return psfb(15, 0, fci);
}
static Bytes twcc(u32 media, u32 extraWords) {
  Bytes body;
  put32(body, 7), put32(body, media);
  for (u32 i = 0; i < extraWords; i++) put32(body, 0x01020304);
  return pkt(15, 205, body);
}

constexpr u32 kSsrc = 0x11223344;
static bool void_entry(const Entry &e) {
  return e.status == LKF_RTCP_IN_MALFORMED && e.fb.empty() && e.sns.empty() && e.refs.empty() && !e.reports &&
         !e.nacks && !e.plis && !e.firs;
}

static void t_empty() { CHECK(void_entry(parse({}, kSsrc))); }
static void t_three_bytes() { CHECK(void_entry(parse({0x80, 201, 0}, kSsrc))); }
static void t_bad_version() {
  Bytes body;
  put32(body, 1);
  CHECK(void_entry(parse(pkt(0, 201, body, 0, 1), kSsrc)));
  CHECK(void_entry(parse(pkt(0, 201, body, 0, 3), kSsrc)));
  CHECK(parse(pkt(0, 201, body), kSsrc).status == LKF_RTCP_IN_OK);
}
static void t_length_past_end() {
  Bytes body;
  put32(body, 1);
  CHECK(void_entry(parse(pkt(0, 201, body, +1), kSsrc)));
  // one word short: the packet ends early and four stray bytes follow, which are no packet of version 2
  body.assign(8, 0);
  CHECK(void_entry(parse(pkt(0, 201, body, -1), kSsrc)));
}
static void t_rr_rc0() {
  const Entry e = parse(rr(5, {}), kSsrc);
  CHECK(e.status == LKF_RTCP_IN_OK && e.reports == 0 && e.fb.size() == 1 && e.fb[0].flags == 0);
}
static void t_rr_rc1() {
  const Entry e = parse(rr(5, {block(kSsrc, 0xAB, 0xFFFFFE, 0x00010203, 77, 0xDEADBEEF, 0x10000)}), kSsrc);
  CHECK(e.status == LKF_RTCP_IN_OK && e.reports == 1 && e.fb.size() == 1);
  const lkf_rtcp_fb &f = e.fb[0];
  CHECK(f.flags == LKF_FB_HAS_RR && f.fraction_lost == 0xAB && f.total_lost == 0xFFFFFE &&
        f.last_sequence_number == 0x00010203 && f.jitter == 77 && f.last_sender_report == 0xDEADBEEF &&
        f.delay == 0x10000);
}
static void t_rr_rc31() {
  Bytes body;
  put32(body, 5);
  for (u32 i = 0; i < 31; i++) {
    const Bytes k = block(i == 30 ? kSsrc : 900 + i, 0, i, 1000 + i, i, 0, 0);
    body.insert(body.end(), k.begin(), k.end());
  }
  const Entry e = parse(pkt(31, 201, body), kSsrc);
  CHECK(e.status == LKF_RTCP_IN_OK && e.reports == 1 && e.fb[0].last_sequence_number == 1030);
  // a profile extension behind the blocks is ignored
  put32(body, 0xCAFEF00D);
  CHECK(parse(pkt(31, 201, body), kSsrc).reports == 1);
}
static void t_rr_truncated_block() {
  Bytes p = rr(5, {block(kSsrc, 0, 0, 10, 0, 0, 0), block(kSsrc, 0, 0, 11, 0, 0, 0)});
  p.resize(p.size() - 4);  // the second block loses a word: the header's length points past the end
  CHECK(void_entry(parse(p, kSsrc)));
  p[3] = u8(p.size() / 4 - 1);  // ... and with the length mended the count needs more than the size
  CHECK(void_entry(parse(p, kSsrc)));
}
static void t_two_rr() {
  const Entry e = parse(cat({rr(5, {block(kSsrc, 0, 1, 10, 0, 0, 0)}), rr(6, {block(kSsrc, 0, 2, 11, 0, 0, 0)})}), kSsrc);
  CHECK(e.status == LKF_RTCP_IN_OK && e.reports == 2 && e.fb.size() == 2);
  CHECK(e.fb[0].last_sequence_number == 10 && e.fb[1].last_sequence_number == 11);
}
static void t_rr_two_matching_blocks() {
  const Entry e = parse(cat({rr(5, {block(kSsrc, 0, 1, 10, 0, 0, 0), block(9, 0, 0, 99, 0, 0, 0),
                                    block(kSsrc, 0, 2, 12, 0, 0, 0)}),
                             psfb(1, kSsrc)}),
                        kSsrc);
  CHECK(e.reports == 2 && e.fb.size() == 2 && e.fb[0].last_sequence_number == 10 && e.fb[1].last_sequence_number == 12);
  CHECK(e.fb[0].plis == 0 && e.fb[1].plis == 1);  // the counts ride on the last record
}
static void t_sr_matching_block_ignored() {
  Bytes body;
  put32(body, 5);
  for (int i = 0; i < 5; i++) put32(body, 0);
  const Bytes k = block(kSsrc, 0, 0, 10, 0, 0, 0);
  body.insert(body.end(), k.begin(), k.end());
  const Entry e = parse(pkt(1, 200, body), kSsrc);
  CHECK(e.status == LKF_RTCP_IN_OK && e.reports == 0 && e.fb.size() == 1 && e.fb[0].flags == 0);
  CHECK(void_entry(parse(pkt(2, 200, body), kSsrc)));  // two blocks announced, one present
}
static void t_nack_blp0() {
  const Entry e = parse(nack(kSsrc, {{500, 0}}), kSsrc);
  CHECK(e.nacks == 1 && e.sns == std::vector<u16>({500}) && e.fb[0].nacks == 1);
}
static void t_nack_blp_ffff() {
  const Entry e = parse(nack(999 /* another SSRC: not compared */, {{100, 0xFFFF}, {7, 0x8001}}), kSsrc);
  std::vector<u16> want;
  for (u32 i = 0; i <= 16; i++) want.push_back(u16(100 + i));
  want.insert(want.end(), {7, 8, 23});
  CHECK(e.nacks == 20 && e.sns == want);
}
static void t_nack_pid_wrap() {
  const Entry e = parse(nack(kSsrc, {{65535, 0x0003}}), kSsrc);
  CHECK(e.sns == std::vector<u16>({65535, 0, 1}));
}
static void t_nack_no_pairs() {
  const Entry e = parse(nack(kSsrc, {}), kSsrc);
  CHECK(e.status == LKF_RTCP_IN_OK && e.nacks == 0 && e.sns.empty());
  Bytes body;
  put32(body, 7);
  CHECK(void_entry(parse(pkt(1, 205, body), kSsrc)));  // 8 bytes: below the 12 a NACK needs
}
static void t_fir_bad_remainder() {
  Bytes fci(8, 0);
  CHECK(parse(psfb(4, 0, fci), kSsrc).firs == 1);
  fci.resize(16);
  CHECK(parse(psfb(4, 0, fci), kSsrc).firs == 1);  // per packet, not per entry of it
  fci.resize(12);
  CHECK(void_entry(parse(psfb(4, 0, fci), kSsrc)));
}
static void t_remb_bad_id() {
  const Entry e = parse(remb("REMB", 2, 2), kSsrc);
  CHECK(e.status == LKF_RTCP_IN_OK && e.refs.size() == 1 && e.refs[0].kind == LKF_RTCP_REF_REMB &&
        e.refs[0].off == 0 && e.refs[0].len == 28);
  CHECK(void_entry(parse(remb("REMC", 2, 2), kSsrc)));
  CHECK(void_entry(parse(psfb(15, 0, Bytes(4, 'R')), kSsrc)));  // 16 bytes: below the 20 a REMB needs
}
static void t_remb_numssrc_beyond() {
  CHECK(void_entry(parse(remb("REMB", 3, 2), kSsrc)));
  CHECK(void_entry(parse(remb("REMB", 255, 0), kSsrc)));
  CHECK(parse(remb("REMB", 0, 0), kSsrc).refs.size() == 1);
}
static void t_twcc_16_bytes() {
  CHECK(void_entry(parse(twcc(kSsrc, 1), kSsrc)));
  const Entry e = parse(cat({psfb(1, 0), twcc(kSsrc, 2)}), kSsrc);
  CHECK(e.refs.size() == 1 && e.refs[0].kind == LKF_RTCP_REF_TWCC && e.refs[0].off == 12 && e.refs[0].len == 20);
}
static void t_twcc_other_ssrc() {
  const Entry e = parse(twcc(kSsrc + 1, 3), kSsrc);
  CHECK(e.status == LKF_RTCP_IN_OK && e.refs.empty());
}
static void t_unknown_pt_skipped() {
  Bytes junk(12, 0xFF);
  const Entry e = parse(cat({pkt(3, 202, junk), pkt(0, 222, junk), pkt(9, 205, junk), pkt(2, 206, junk),
                             pkt(0, 207, junk), nack(kSsrc, {{9, 0}})}),
                        kSsrc);
  CHECK(e.status == LKF_RTCP_IN_OK && e.sns == std::vector<u16>({9}) && e.reports == 0 && e.refs.empty());
  // the P bit is ignored: pad bytes belong to the body
  Bytes p = nack(kSsrc, {{9, 0}});
  p[0] |= 0x20;
  CHECK(parse(p, kSsrc).sns == std::vector<u16>({9}));
}
static void t_malformed_after_valid() {
  const Bytes good = cat({rr(5, {block(kSsrc, 0, 1, 10, 0, 0, 0)}), nack(kSsrc, {{3, 1}}), psfb(1, 0), remb("REMB", 0, 0)});
  CHECK(parse(good, kSsrc).status == LKF_RTCP_IN_OK);
  CHECK(void_entry(parse(cat({good, psfb(4, 0, Bytes(4, 0))}), kSsrc)));
  CHECK(void_entry(parse(cat({good, Bytes({0x80, 201})}), kSsrc)));
}

struct Case {
  const char *name;
  void (*fn)();
};
static const Case kCases[] = {
    {"empty", t_empty},
    {"three_bytes", t_three_bytes},
    {"bad_version", t_bad_version},
    {"length_past_end", t_length_past_end},
    {"rr_rc0", t_rr_rc0},
    {"rr_rc1", t_rr_rc1},
    {"rr_rc31", t_rr_rc31},
    {"rr_truncated_block", t_rr_truncated_block},
    {"two_rr", t_two_rr},
    {"rr_two_matching_blocks", t_rr_two_matching_blocks},
    {"sr_matching_block_ignored", t_sr_matching_block_ignored},
    {"nack_blp0", t_nack_blp0},
    {"nack_blp_ffff", t_nack_blp_ffff},
    {"nack_pid_wrap", t_nack_pid_wrap},
    {"nack_no_pairs", t_nack_no_pairs},
    {"fir_bad_remainder", t_fir_bad_remainder},
    {"remb_bad_id", t_remb_bad_id},
    {"remb_numssrc_beyond", t_remb_numssrc_beyond},
    {"twcc_16_bytes", t_twcc_16_bytes},
    {"twcc_other_ssrc", t_twcc_other_ssrc},
    {"unknown_pt_skipped", t_unknown_pt_skipped},
    {"malformed_after_valid", t_malformed_after_valid},
};

static int replay() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string op, hex;
    u32 ssrc = 0;
    if (!(in >> op)) continue;
    if (op != "e") {
      std::fprintf(stderr, "unknown op: %s\n", op.c_str());
      return 2;
    }
    in >> ssrc >> hex;
    if (hex == "-") hex.clear();
    Bytes d(hex.size() / 2);
    for (size_t i = 0; i < d.size(); i++) d[i] = u8(std::stoul(hex.substr(2 * i, 2), nullptr, 16));
    const Entry e = parse(d, ssrc);
    std::printf("e status=%u reports=%u nacks=%u plis=%u firs=%u fb=", e.status, e.reports, e.nacks, e.plis, e.firs);
    for (size_t i = 0; i < e.fb.size(); i++) {
      const lkf_rtcp_fb &f = e.fb[i];
      std::printf("%s%u:%u:%u:%u:%u:%u:%u:%u:%u:%u", i ? "," : "", f.last_sequence_number, f.total_lost, f.jitter,
                  f.last_sender_report, f.delay, u32(f.fraction_lost), f.flags, f.nacks, f.plis, f.firs);
    }
    std::printf("%s sns=", e.fb.empty() ? "-" : "");
    for (size_t i = 0; i < e.sns.size(); i++) std::printf("%s%u", i ? "," : "", u32(e.sns[i]));
    std::printf("%s refs=", e.sns.empty() ? "-" : "");
    for (size_t i = 0; i < e.refs.size(); i++)
      std::printf("%s%u:%u:%u", i ? "," : "", e.refs[i].kind, e.refs[i].off, e.refs[i].len);
    std::printf("%s\n", e.refs.empty() ? "-" : "");
  }
  return g_fail ? 1 : 0;
}

// The host path the engine offered before lkf_rtcp_ingest: walk every
// compound, filter, expand and group into lkf_rtcp_fb[] and lkf_nack[].
struct BenchSink {
  std::vector<lkf_rtcp_fb> *fb;
  std::vector<lkf_nack> *nk;
  int32_t dt;
  u32 reports = 0, nacks = 0, plis = 0, firs = 0;
  void report(const u8 *b) {
    lkf_rtcp_fb f;
    std::memset(&f, 0, sizeof(f));
    f.dt = dt;
    f.flags = LKF_FB_HAS_RR;
    read_report(b, f);
    fb->push_back(f);
    reports++;
  }
  void pair(u32 pid, u32 blp) {
    pair_expand(pid, blp, [&](u16 sn) {
      nk->push_back({dt, sn, 0});
      nacks++;
    });
  }
  void pli() { plis++; }
  void fir() { firs++; }
  void ref(u32, u32, u32) {}
};
static int bench(u32 n, u32 reps, bool step) {
  Bytes arena;
  std::vector<lkf_rtcp_raw> raws(n);
  const Bytes sdes = pkt(1, 202, Bytes({0, 0, 0, 1, 1, 6, 'c', 'n', 'a', 'm', 'e', '0', 0, 0, 0, 0}));
  for (u32 i = 0; i < n; i++) {
    const u32 ssrc = 1000 + i;
    const Bytes c = cat({rr(ssrc ^ 0x5a5a, {block(ssrc, 1, i & 0xff, 5000 + i, i & 0x3ff, 0, 0)}),
                         nack(ssrc, {{i & 0xffff, 0x0005}, {(i + 40) & 0xffff, 0}, {(i + 90) & 0xffff, 0x8000}}), sdes});
    raws[i] = {int32_t(i), u32(arena.size()), u32(c.size())};
    arena.insert(arena.end(), c.begin(), c.end());
  }
  std::vector<double> times;
  size_t nfb = 0, nnk = 0;
  std::string line;
  for (u32 r = 0; r < reps; r++) {
    if (step && !std::getline(std::cin, line)) break;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<lkf_rtcp_fb> fb;
    std::vector<lkf_nack> nk;
    fb.reserve(n), nk.reserve(size_t(n) * 6);
    for (u32 i = 0; i < n; i++) {
      const size_t f0 = fb.size(), n0 = nk.size();
      BenchSink s{&fb, &nk, raws[i].dt};
      if (walk(arena.data() + raws[i].off, raws[i].len, 1000 + i, s) != LKF_RTCP_IN_OK) {
        fb.resize(f0), nk.resize(n0);
        continue;
      }
      if (fb.size() == f0) {
        lkf_rtcp_fb f;
        std::memset(&f, 0, sizeof(f));
        f.dt = raws[i].dt;
        fb.push_back(f);
      }
      fb.back().nacks = s.nacks, fb.back().plis = s.plis, fb.back().firs = s.firs;
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    times.push_back(ms);
    nfb = fb.size(), nnk = nk.size();
    if (step) {
      std::printf("ms=%.4f\n", ms);
      std::fflush(stdout);
    }
  }
  if (times.empty()) return 1;
  std::sort(times.begin(), times.end());
  std::printf("bench n=%u arena_bytes=%zu fb=%zu nacks=%zu ms_min=%.4f ms_median=%.4f ms_max=%.4f\n", n, arena.size(), nfb,
              nnk, times.front(), times[times.size() / 2], times.back());
  return 0;
}

int main(int argc, char **argv) {
  const std::string arg = argc > 1 ? argv[1] : "";
  if (arg == "--list") {
    for (const Case &c : kCases) std::printf("%s\n", c.name);
    return 0;
  }
  if (arg == "--replay") return replay();
  if (arg == "--bench") return bench(argc > 2 ? u32(std::atoi(argv[2])) : 100000, argc > 3 ? u32(std::atoi(argv[3])) : 5,
                                   argc > 4 && std::string(argv[4]) == "step");
  bool found = false;
  for (const Case &c : kCases) {
    if (!arg.empty() && arg != c.name) continue;
    found = true;
    const int before = g_fail;
    c.fn();
    std::printf("%s %s\n", g_fail == before ? "PASS" : "FAIL", c.name);
  }
  if (!found) {
    std::fprintf(stderr, "no such case: %s\n", arg.c_str());
    return 2;
  }
  return g_fail ? 1 : 0;
}
