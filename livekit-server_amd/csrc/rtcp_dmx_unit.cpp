// rtcp_dmx_unit.cpp — CPU unit tests of the RTCP demultiplexing
// (rtcp_dmx_device.h): the destination-SSRC walk and the routing-table lookup
// the kernel k_rtcp_dmx_mark compiles, and the table / output rules of
// include/lkfwd.h on top of them, with the kernels' bitmap row per datagram
// and scanned per-DownTrack offsets.  Built with the host compiler alone (make
// rtcp_dmx_unit; address + undefined sanitizers).  Every datagram is walked
// from a heap block of exactly its length, so a read past it trips the
// sanitizer.
//   rtcp_dmx_unit --list          the case names
//   rtcp_dmx_unit <name>          one case ("PASS <name>" / exit 1)
//   rtcp_dmx_unit                 every case
//   rtcp_dmx_unit --replay        a script on stdin, results on stdout:
//     d <transport> <ssrc> <dt>   an active DownTrack bound to the transport
//     g <transport> <hex | ->     one datagram of the call
//     run                         demultiplexes the datagrams since the last run; prints per datagram
//       r status= dests= unrouted= entries=
//                                 and one line  x <dt:dgram,..|->
//   rtcp_dmx_unit --bench <n> <transports> <reps>   the host path's demux, single thread: n DownTracks over
//                                 the transports, one compound (RR + NACK with three pairs + SDES) each, into
//                                 lkf_rtcp_entry[]; prints "bench n= entries= ms_min= ms_median= ms_max="
//   rtcp_dmx_unit --bench <n> <transports> <reps> step   the same, one rep per line read from stdin, "ms=<that
//                                 rep>" printed after each (a caller alternates it with another path)
#define __host__
#define __device__
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <tuple>
#include <vector>

#include "rtcp_dmx_device.h"

using namespace lkf;
using namespace lkf::rtcpdmx;
using Bytes = std::vector<u8>;

static_assert(sizeof(lkf_rtcp_dmx_result) == 16 && sizeof(lkf_rtcp_entry) == 8 && sizeof(Row) == 12, "RTCP demux records");

static int g_fail = 0;
#define CHECK(c)                                                         \
  do {                                                                   \
    if (!(c)) {                                                          \
      std::printf("  check failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
      g_fail++;                                                          \
    }                                                                    \
  } while (0)

// ---- the routing table and one call, as the engine's host side and kernels do them ----
struct Table {
  std::vector<Row> rows;     // by (transport, ssrc), one per key
  std::vector<u32> tFirst;   // ntransports + 1
  std::vector<u32> byDt;     // row indices, DownTrack ascending
};
static Table build(std::vector<Row> rows, u32 ntransports) {
  Table t;
  std::sort(rows.begin(), rows.end(), [](const Row &a, const Row &b) {
    return std::tie(a.transport, a.ssrc, a.dt) < std::tie(b.transport, b.ssrc, b.dt);
  });
  for (size_t i = 0; i < rows.size(); i++)  // the highest handle of a key
    if (i + 1 == rows.size() || rows[i + 1].transport != rows[i].transport || rows[i + 1].ssrc != rows[i].ssrc)
      t.rows.push_back(rows[i]);
  t.tFirst.assign(ntransports + 1, 0);
  for (const Row &r : t.rows) t.tFirst[r.transport + 1]++;
  for (u32 k = 0; k < ntransports; k++) t.tFirst[k + 1] += t.tFirst[k];
  t.byDt.resize(t.rows.size());
  for (u32 i = 0; i < t.byDt.size(); i++) t.byDt[i] = i;
  std::sort(t.byDt.begin(), t.byDt.end(), [&](u32 a, u32 b) { return t.rows[a].dt < t.rows[b].dt; });
  return t;
}

struct Dgram {
  u32 transport;
  const u8 *p;  // len bytes
  u32 len;
};
struct Out {
  std::vector<lkf_rtcp_dmx_result> res;
  std::vector<lkf_rtcp_entry> entries;
};
static Out demux(const Table &t, const std::vector<Dgram> &in) {
  const u32 n = u32(in.size()), nt = u32(t.tFirst.size() - 1);
  Out o;
  o.res.resize(n);
  std::vector<u32> bmOff(n + 1, 0);
  for (u32 i = 0; i < n; i++) {
    const bool live = in[i].len && in[i].transport < nt;
    bmOff[i + 1] = bmOff[i] + (live ? row_words(t.tFirst[in[i].transport + 1] - t.tFirst[in[i].transport]) : 0);
  }
  // the bitmap rows in one heap block of exactly their words: a bit past a row's end trips the sanitizer
  u32 *bits = static_cast<u32 *>(std::calloc(bmOff[n] ? bmOff[n] : 1, sizeof(u32)));
  for (u32 i = 0; i < n; i++) {  // the mark pass
    lkf_rtcp_dmx_result r = {LKF_RTCP_DMX_EMPTY, 0, 0, 0};
    if (in[i].len) {
      r.status = LKF_RTCP_DMX_MALFORMED;
      const u32 tr = in[i].transport;
      if (tr < nt) {
        const u32 nw = bmOff[i + 1] - bmOff[i];
        Mark m{t.rows.data(), t.tFirst[tr], t.tFirst[tr + 1], bits + bmOff[i], nw};
        if (walk(in[i].p, in[i].len, m) == LKF_RTCP_DMX_OK) {
          r.status = LKF_RTCP_DMX_OK;
          r.dests = m.dests;
          r.unrouted = m.unrouted;
          for (u32 w = 0; w < nw; w++) r.entries += u32(__builtin_popcount(bits[bmOff[i] + w]));
        } else {
          for (u32 w = 0; w < nw; w++) bits[bmOff[i] + w] = 0;
        }
      }
    }
    o.res[i] = r;
  }
  // The count / scan / write passes: DownTrack ascending, datagram ascending.
  // (A host walks each datagram's set bits instead of each row's datagrams:
  // the same counts and the same places, by the cheaper loop for one thread.)
  std::vector<u32> cnt(t.rows.size(), 0), off(t.rows.size(), 0);
  auto each_bit = [&](auto &&f) {
    for (u32 i = 0; i < n; i++)
      for (u32 w = bmOff[i]; w < bmOff[i + 1]; w++)
        for (u32 v = bits[w]; v; v &= v - 1)
          f(t.tFirst[in[i].transport] + 32 * (w - bmOff[i]) + u32(__builtin_ctz(v)), i);
  };
  each_bit([&](u32 row, u32) { cnt[row]++; });
  u32 total = 0;
  for (u32 k : t.byDt) off[k] = total, total += cnt[k];
  o.entries.resize(total);
  each_bit([&](u32 row, u32 i) { o.entries[off[row]++] = {t.rows[row].dt, i}; });
  std::free(bits);
  return o;
}

// a call over byte vectors: every datagram in a heap block of exactly its length
static Out run(const Table &t, const std::vector<std::pair<u32, Bytes>> &dgrams) {
  std::vector<Dgram> in;
  std::vector<u8 *> blocks;
  for (const auto &d : dgrams) {
    u8 *blk = static_cast<u8 *>(std::malloc(d.second.size() ? d.second.size() : 1));
    if (!d.second.empty()) std::memcpy(blk, d.second.data(), d.second.size());
    blocks.push_back(blk);
    in.push_back({d.first, d.second.empty() ? blk + 1 : blk, u32(d.second.size())});  // (an empty one is never read)
  }
  Out o = demux(t, in);
  for (u8 *b : blocks) std::free(b);
  return o;
}

// ---- a small marshaller for the cases ----
static void put16(Bytes &b, u32 v) { b.push_back(u8(v >> 8)), b.push_back(u8(v)); }
static void put32(Bytes &b, u32 v) { put16(b, v >> 16), put16(b, v & 0xffff); }
static Bytes pkt(u32 count, u32 pt, const Bytes &body, int lengthAdjust = 0) {
  Bytes b;
  b.push_back(u8(0x80 | (count & 31)));
  b.push_back(u8(pt));
  put16(b, u32(int(body.size() / 4) + lengthAdjust));
  b.insert(b.end(), body.begin(), body.end());
  return b;
}
static Bytes words(std::initializer_list<u32> w) {
  Bytes b;
  for (u32 v : w) put32(b, v);
  return b;
}
static Bytes cat(std::initializer_list<Bytes> parts) {
  Bytes b;
  for (const Bytes &p : parts) b.insert(b.end(), p.begin(), p.end());
  return b;
}
static Bytes rr(u32 sender, std::initializer_list<u32> blocks) {
  Bytes body = words({sender});
  for (u32 s : blocks) {
    const Bytes k = words({s, 0, 0, 0, 0, 0});
    body.insert(body.end(), k.begin(), k.end());
  }
  return pkt(u32(blocks.size()), 201, body);
}
static Bytes sr(u32 sender, std::initializer_list<u32> blocks) {
  Bytes body = words({sender, 0, 0, 0, 0, 0});
  for (u32 s : blocks) {
    const Bytes k = words({s, 0, 0, 0, 0, 0});
    body.insert(body.end(), k.begin(), k.end());
  }
  return pkt(u32(blocks.size()), 200, body);
}
static Bytes fb(u32 pt, u32 fmt, u32 media, const Bytes &fci = {}) { return pkt(fmt, pt, cat({words({7, media}), fci})); }
static Bytes remb(u32 numSsrc, std::initializer_list<u32> listed) {
  Bytes fci = {'R', 'E', 'M', 'B', u8(numSsrc), 0x12, 0x34, 0x56};
  for (u32 s : listed) put32(fci, s);
  return fb(206, 15, 0, fci);
}
static Bytes sdes(u32 ssrc) { return pkt(1, 202, cat({words({ssrc}), Bytes({1, 5, 'c', 'n', 'a', 'm', 'e', 0})})); }

// the table of the cases: transport 0 holds SSRC 100 -> dt 0 and 200 -> dt 1, transport 1 holds 100 -> dt 2
static Table small() { return build({{0, 100, 0}, {0, 200, 1}, {1, 100, 2}}, 3); }
static std::vector<std::pair<int32_t, u32>> pairs(const Out &o) {
  std::vector<std::pair<int32_t, u32>> v;
  for (const auto &x : o.entries) v.push_back({x.dt, x.dgram});
  return v;
}
using P = std::vector<std::pair<int32_t, u32>>;
static bool is(const lkf_rtcp_dmx_result &r, u32 status, u32 dests, u32 unrouted, u32 entries) {
  return r.status == status && r.dests == dests && r.unrouted == unrouted && r.entries == entries;
}

static void t_empty() {
  const Out o = run(small(), {{0, {}}});
  CHECK(is(o.res[0], LKF_RTCP_DMX_EMPTY, 0, 0, 0) && o.entries.empty());
}
static void t_rr_blocks() {
  const Out o = run(small(), {{0, rr(100 /* the sender is no destination */, {200, 999, 100})}});
  CHECK(is(o.res[0], LKF_RTCP_DMX_OK, 3, 1, 2) && pairs(o) == P({{0, 0}, {1, 0}}));
  CHECK(is(run(small(), {{0, rr(100, {})}}).res[0], LKF_RTCP_DMX_OK, 0, 0, 0));
}
static void t_sr_blocks_then_sender() {
  const Out o = run(small(), {{0, sr(200, {999})}, {0, sr(5, {100})}});
  CHECK(is(o.res[0], LKF_RTCP_DMX_OK, 2, 1, 1) && is(o.res[1], LKF_RTCP_DMX_OK, 2, 1, 1));
  CHECK(pairs(o) == P({{0, 1}, {1, 0}}));
  struct Seen {
    std::vector<u32> v;
    void dest(u32 s) { v.push_back(s); }
  } s;
  const Bytes p = sr(7, {8, 9});
  CHECK(walk(p.data(), u32(p.size()), s) == LKF_RTCP_DMX_OK && s.v == std::vector<u32>({8, 9, 7}));
}
static void t_nack_twcc_pli_media() {
  const Out o = run(small(), {{0, fb(205, 1, 100, words({0x00050000}))},
                              {0, fb(205, 15, 200, words({1, 2}))},
                              {0, fb(206, 1, 100)},
                              {0, fb(205, 15, 200, words({1}))}});  // a 16-byte TransportLayerCC: malformed
  CHECK(is(o.res[0], LKF_RTCP_DMX_OK, 1, 0, 1) && is(o.res[1], LKF_RTCP_DMX_OK, 1, 0, 1) &&
        is(o.res[2], LKF_RTCP_DMX_OK, 1, 0, 1) && is(o.res[3], LKF_RTCP_DMX_MALFORMED, 0, 0, 0));
  CHECK(pairs(o) == P({{0, 0}, {0, 2}, {1, 1}}));
}
static void t_rrr_sli_media() {
  const Out o = run(small(), {{0, fb(205, 5, 100)}, {0, fb(206, 2, 200, words({0}))}});
  CHECK(is(o.res[0], LKF_RTCP_DMX_OK, 1, 0, 1) && is(o.res[1], LKF_RTCP_DMX_OK, 1, 0, 1));
  CHECK(pairs(o) == P({{0, 0}, {1, 1}}));
}
static void t_rrr_sli_short() {  // size 8: no destination, still OK
  const Out o = run(small(), {{0, pkt(5, 205, words({100}))}, {0, pkt(2, 206, words({100}))}, {0, pkt(2, 206, {})}});
  for (int i = 0; i < 3; i++) CHECK(is(o.res[i], LKF_RTCP_DMX_OK, 0, 0, 0));
  CHECK(o.entries.empty());
}
static void t_fir_entries() {  // the media SSRC field is not a destination
  const Out o = run(small(), {{0, fb(206, 4, 100, words({200, 0, 999, 0, 200, 0}))}, {0, fb(206, 4, 100)}});
  CHECK(is(o.res[0], LKF_RTCP_DMX_OK, 3, 1, 1) && is(o.res[1], LKF_RTCP_DMX_OK, 0, 0, 0));
  CHECK(pairs(o) == P({{1, 0}}));
  CHECK(run(small(), {{0, fb(206, 4, 100, words({200}))}}).res[0].status == LKF_RTCP_DMX_MALFORMED);
}
static void t_remb_list() {
  const Out o = run(small(), {{0, remb(4, {100, 5, 200, 6})}, {0, remb(0, {})}, {0, remb(1, {100, 200})}});
  CHECK(is(o.res[0], LKF_RTCP_DMX_OK, 4, 2, 2) && is(o.res[1], LKF_RTCP_DMX_OK, 0, 0, 0));
  CHECK(is(o.res[2], LKF_RTCP_DMX_OK, 1, 0, 1));  // numSSRC below the words present: the first alone
  CHECK(pairs(o) == P({{0, 0}, {0, 2}, {1, 0}}));
  CHECK(run(small(), {{0, remb(3, {100, 200})}}).res[0].status == LKF_RTCP_DMX_MALFORMED);  // inflated
  CHECK(run(small(), {{0, remb(255, {})}}).res[0].status == LKF_RTCP_DMX_MALFORMED);
}
static void t_others_none() {
  const Bytes junk = words({100, 100, 100});
  const Out o = run(small(), {{0, cat({sdes(100), pkt(1, 203, words({100})), pkt(0, 204, junk), pkt(0, 207, junk),
                                       pkt(11, 205, junk), pkt(3, 206, junk), pkt(0, 192, junk)})}});
  CHECK(is(o.res[0], LKF_RTCP_DMX_OK, 0, 0, 0) && o.entries.empty());
}
static void t_duplicate_ssrc_one_entry() {
  const Out o = run(small(), {{0, cat({fb(205, 1, 100, words({0x00050000})), fb(206, 1, 100), rr(1, {100, 100})})}});
  CHECK(is(o.res[0], LKF_RTCP_DMX_OK, 4, 0, 1) && pairs(o) == P({{0, 0}}));
}
static void t_malformed_after_valid() {
  const Bytes good = rr(1, {100, 200});
  CHECK(run(small(), {{0, good}}).res[0].entries == 2);
  for (const Bytes &tail : {Bytes({0x80, 201}), fb(206, 4, 0, words({1})), Bytes({0x40, 201, 0, 0})}) {
    const Out o = run(small(), {{0, cat({good, tail})}, {0, good}});
    CHECK(is(o.res[0], LKF_RTCP_DMX_MALFORMED, 0, 0, 0) && pairs(o) == P({{0, 1}, {1, 1}}));
  }
}
static void t_unrouted_other_transport() {
  const Out o = run(small(), {{1, rr(1, {200})}, {2, rr(1, {100})}});
  CHECK(is(o.res[0], LKF_RTCP_DMX_OK, 1, 1, 0) && is(o.res[1], LKF_RTCP_DMX_OK, 1, 1, 0) && o.entries.empty());
}
static void t_same_ssrc_two_transports() {
  const Out o = run(small(), {{1, rr(1, {100})}, {0, rr(1, {100})}});
  CHECK(pairs(o) == P({{0, 1}, {2, 0}}));
}
static void t_highest_handle_wins() {
  const Table t = build({{0, 100, 4}, {0, 100, 9}, {0, 100, 2}, {0, 50, 3}}, 1);
  CHECK(t.rows.size() == 2 && t.rows[0].dt == 3 && t.rows[1].dt == 9);
  const Out o = run(t, {{0, rr(1, {100, 50})}});
  CHECK(is(o.res[0], LKF_RTCP_DMX_OK, 2, 0, 2) && pairs(o) == P({{3, 0}, {9, 0}}));
}
static void t_bitmap_word_boundaries() {  // 0, 1, 32, 33, 64, 65 and 70 rows: every row's last bit and word
  for (u32 n : {0u, 1u, 31u, 32u, 33u, 63u, 64u, 65u, 70u}) {
    std::vector<Row> rows;
    for (u32 i = 0; i < n; i++) rows.push_back({1, 1000 + 7 * i, int32_t(n - 1 - i)});  // (handles against the SSRC order)
    rows.push_back({0, 1000, 500}), rows.push_back({2, 1000, 501});                    // neighbours on both sides
    const Table t = build(rows, 3);
    CHECK(row_words(n) == (n + 31) / 32);
    for (u32 i = 0; i < n; i++) {
      const Out o = run(t, {{0, rr(1, {1000})}, {1, rr(1, {1000 + 7 * i, 1000 + 7 * i + 1})}, {2, rr(1, {1000})}});
      CHECK(is(o.res[1], LKF_RTCP_DMX_OK, 2, 1, 1));
      CHECK(pairs(o) == (int32_t(n - 1 - i) < 500 ? P({{int32_t(n - 1 - i), 1}, {500, 0}, {501, 2}}) : P()));
    }
    const Out none = run(t, {{1, rr(1, {999, 1000 + 7 * n})}});
    CHECK(is(none.res[0], LKF_RTCP_DMX_OK, 2, 2, 0));
  }
}
static void t_order_by_dt_then_dgram() {
  const Table t = build({{0, 10, 5}, {0, 20, 1}, {1, 10, 3}}, 2);
  const Out o = run(t, {{0, rr(1, {10, 20})}, {1, rr(1, {10})}, {0, {}}, {0, rr(1, {20})}, {1, rr(1, {10})}, {0, rr(1, {10})}});
  CHECK(pairs(o) == P({{1, 0}, {1, 3}, {3, 1}, {3, 4}, {5, 0}, {5, 5}}));
  u32 sum = 0;
  for (const auto &r : o.res) sum += r.entries;
  CHECK(sum == o.entries.size() && o.res[2].status == LKF_RTCP_DMX_EMPTY);
}
static void t_find_edges() {
  const Row rows[] = {{0, 0, 0}, {0, 5, 1}, {0, 0xffffffffu, 2}, {1, 5, 3}};
  CHECK(find(rows, 0, 3, 0) == 0 && find(rows, 0, 3, 5) == 1 && find(rows, 0, 3, 0xffffffffu) == 2);
  CHECK(find(rows, 0, 3, 4) == ~0u && find(rows, 0, 3, 6) == ~0u && find(rows, 3, 4, 5) == 3);
  CHECK(find(rows, 0, 0, 5) == ~0u && find(rows, 3, 3, 5) == ~0u && find(rows, 3, 4, 0) == ~0u);
}

struct Case {
  const char *name;
  void (*fn)();
};
static const Case kCases[] = {
    {"empty", t_empty},
    {"rr_blocks", t_rr_blocks},
    {"sr_blocks_then_sender", t_sr_blocks_then_sender},
    {"nack_twcc_pli_media", t_nack_twcc_pli_media},
    {"rrr_sli_media", t_rrr_sli_media},
    {"rrr_sli_short", t_rrr_sli_short},
    {"fir_entries", t_fir_entries},
    {"remb_list", t_remb_list},
    {"others_none", t_others_none},
    {"duplicate_ssrc_one_entry", t_duplicate_ssrc_one_entry},
    {"malformed_after_valid", t_malformed_after_valid},
    {"unrouted_other_transport", t_unrouted_other_transport},
    {"same_ssrc_two_transports", t_same_ssrc_two_transports},
    {"highest_handle_wins", t_highest_handle_wins},
    {"bitmap_word_boundaries", t_bitmap_word_boundaries},
    {"order_by_dt_then_dgram", t_order_by_dt_then_dgram},
    {"find_edges", t_find_edges},
};

static int replay() {
  std::vector<Row> rows;
  std::vector<std::pair<u32, Bytes>> dgrams;
  u32 nt = 0;
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string op, hex;
    if (!(in >> op)) continue;
    if (op == "d") {
      Row r;
      in >> r.transport >> r.ssrc >> r.dt;
      rows.push_back(r);
      nt = std::max(nt, r.transport + 1);
    } else if (op == "g") {
      u32 t = 0;
      in >> t >> hex;
      if (hex == "-") hex.clear();
      Bytes d(hex.size() / 2);
      for (size_t i = 0; i < d.size(); i++) d[i] = u8(std::stoul(hex.substr(2 * i, 2), nullptr, 16));
      dgrams.push_back({t, d});
      nt = std::max(nt, t + 1);
    } else if (op == "run") {
      const Out o = run(build(rows, nt), dgrams);
      for (const auto &r : o.res)
        std::printf("r status=%u dests=%u unrouted=%u entries=%u\n", r.status, r.dests, r.unrouted, r.entries);
      std::printf("x ");
      for (size_t i = 0; i < o.entries.size(); i++) std::printf("%s%d:%u", i ? "," : "", o.entries[i].dt, o.entries[i].dgram);
      std::printf("%s\n", o.entries.empty() ? "-" : "");
      dgrams.clear();
    } else {
      std::fprintf(stderr, "unknown op: %s\n", op.c_str());
      return 2;
    }
  }
  return g_fail ? 1 : 0;
}

// The host path the demux calls replace: walk every decrypted compound, look
// its destinations up, regroup by DownTrack into lkf_rtcp_entry[].
static int bench(u32 n, u32 nt, u32 reps, bool step) {
  if (!nt) nt = 1;
  std::vector<Row> rows;
  Bytes arena;
  std::vector<Dgram> in(n);
  std::vector<u32> offs(n);
  for (u32 i = 0; i < n; i++) {
    const u32 ssrc = 1000 + i;
    rows.push_back({i % nt, ssrc, int32_t(i)});
    const Bytes c = cat({rr(ssrc ^ 0x5a5a, {ssrc}),
                         fb(205, 1, ssrc, words({((i & 0xffff) << 16) | 5, ((i + 40) & 0xffff) << 16, (((i + 90) & 0xffff) << 16) | 0x8000})),
                         sdes(ssrc ^ 0x5a5a)});
    offs[i] = u32(arena.size());
    in[i] = {i % nt, nullptr, u32(c.size())};
    arena.insert(arena.end(), c.begin(), c.end());
  }
  for (u32 i = 0; i < n; i++) in[i].p = arena.data() + offs[i];
  const Table t = build(rows, nt);  // (kept between ticks, as the engine keeps its table: not part of a tick)
  std::vector<double> times;
  size_t entries = 0;
  std::string line;
  for (u32 r = 0; r < reps; r++) {
    if (step && !std::getline(std::cin, line)) break;
    const auto t0 = std::chrono::steady_clock::now();
    const Out o = demux(t, in);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    times.push_back(ms);
    entries = o.entries.size();
    if (step) {
      std::printf("ms=%.4f\n", ms);
      std::fflush(stdout);
    }
  }
  if (times.empty()) return 1;
  std::sort(times.begin(), times.end());
  std::printf("bench n=%u transports=%u arena_bytes=%zu entries=%zu ms_min=%.4f ms_median=%.4f ms_max=%.4f\n", n, nt,
              arena.size(), entries, times.front(), times[times.size() / 2], times.back());
  return 0;
}

int main(int argc, char **argv) {
  const std::string arg = argc > 1 ? argv[1] : "";
  if (arg == "--list") {
    for (const Case &c : kCases) std::printf("%s\n", c.name);
    return 0;
  }
  if (arg == "--replay") return replay();
  if (arg == "--bench")
    return bench(argc > 2 ? u32(std::atoi(argv[2])) : 100000, argc > 3 ? u32(std::atoi(argv[3])) : 1000,
                 argc > 4 ? u32(std::atoi(argv[4])) : 5, argc > 5 && std::string(argv[5]) == "step");
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
