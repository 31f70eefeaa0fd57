// srtp_rx_unit.cpp — CPU unit tests of the SRTP receive recurrence
// (srtp_rx_device.h): the datagram parse, the packet-index estimate across
// sequence-number wraps, the 64-packet replay window and its commit.  Built
// with the host compiler alone (make srtp_rx_unit; address + undefined
// sanitizers).
//   srtp_rx_unit --list     the case names
//   srtp_rx_unit <name>     one case ("PASS <name>" / exit 1)
//   srtp_rx_unit            every case
//   srtp_rx_unit --replay   a script on stdin (below), results on stdout
//
// --replay script, one op per line, integers in decimal:
//   p <seq> <malformed> <auth>        one datagram of the stream: prints "p st=<status> v=<index>"
//   d <tag> <off> <arena_len> <hex>   parse of the datagram <hex> placed at <off> of an arena of
//                                     <arena_len> bytes: prints "d malformed=<0|1> seq=<seq> h=<h>"
//   state                             prints the state
//   reset                             prints the state, then a fresh stream (the next script)
#define __host__
#define __device__
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "srtp_rx_device.h"

using namespace lkf;
using namespace lkf::srtprx;

static_assert(sizeof(lkf_srtp_rx_result) == 16, "lkf_srtp_rx_result is 16 B");
static_assert(sizeof(lkf_stream_srtp) == 56, "lkf_stream_srtp is 56 B");

static int g_fail = 0;
#define CHECK(c)                                                         \
  do {                                                                   \
    if (!(c)) {                                                          \
      std::printf("  check failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
      g_fail++;                                                          \
    }                                                                    \
  } while (0)

static SrtpRx fresh() {
  SrtpRx s;
  std::memset(&s, 0, sizeof(s));
  s.tp1 = 1;
  return s;
}
static u32 feed(SrtpRx &s, u32 seq, bool auth = true, u64 *vout = nullptr) {
  u64 v = 0;
  const u32 st = step(s, false, seq, auth, v);
  if (vout) *vout = v;
  return st;
}

static void t_first_packet() {
  SrtpRx s = fresh();
  u64 v;
  CHECK(feed(s, 65500, true, &v) == LKF_SRTP_RX_OK);
  CHECK(v == 65500 && s.started == 1 && s.sl == 65500 && s.mask == 1 && s.accepted == 1);
}
static void t_in_order() {
  SrtpRx s = fresh();
  for (u32 q = 10; q < 20; q++) CHECK(feed(s, q) == LKF_SRTP_RX_OK);
  CHECK(s.sl == 19 && s.mask == 0x3ff && s.accepted == 10);
}
static void t_wrap_forward() {
  SrtpRx s = fresh();
  u64 v;
  feed(s, 65534);
  feed(s, 65535);
  CHECK(feed(s, 0, true, &v) == LKF_SRTP_RX_OK && v == 65536);
  CHECK(feed(s, 1, true, &v) == LKF_SRTP_RX_OK && v == 65537);
  CHECK(s.sl == 65537 && s.mask == 0xf);
}
static void t_reorder_across_wrap() {
  SrtpRx s = fresh();
  u64 v;
  feed(s, 65533);
  CHECK(feed(s, 2, true, &v) == LKF_SRTP_RX_OK && v == 65538);  // ahead, over the wrap
  CHECK(feed(s, 65535, true, &v) == LKF_SRTP_RX_OK && v == 65535);  // late, the old rollover count
  CHECK(feed(s, 0, true, &v) == LKF_SRTP_RX_OK && v == 65536);
  CHECK(s.sl == 65538 && s.mask == ((1ull << 0) | (1ull << 2) | (1ull << 3) | (1ull << 5)));
}
static void t_dup() {
  SrtpRx s = fresh();
  feed(s, 100);
  feed(s, 101);
  CHECK(feed(s, 101) == LKF_SRTP_RX_REPLAY_DUP);
  CHECK(feed(s, 100) == LKF_SRTP_RX_REPLAY_DUP);
  CHECK(s.replay == 2 && s.accepted == 2 && s.mask == 3);
}
static void t_behind_63() {
  SrtpRx s = fresh();
  feed(s, 1000);
  feed(s, 1100);
  u64 v;
  CHECK(feed(s, 1037, true, &v) == LKF_SRTP_RX_OK && v == 1037);
  CHECK(s.mask == ((1ull << 63) | 1));
}
static void t_behind_64() {
  SrtpRx s = fresh();
  feed(s, 1000);
  feed(s, 1100);
  CHECK(feed(s, 1036) == LKF_SRTP_RX_REPLAY_OLD);
  CHECK(s.replay == 1 && s.mask == 1);
}
static void t_jump_shift_64() {
  SrtpRx s = fresh();
  feed(s, 5);
  feed(s, 5 + 63);
  CHECK(s.mask == ((1ull << 63) | 1));
  feed(s, 5 + 63 + 64);  // shift of exactly 64: the whole window leaves
  CHECK(s.mask == 1);
  feed(s, 5 + 63 + 64 + 1000);
  CHECK(s.mask == 1 && s.sl == 5 + 63 + 64 + 1000);
}
static void t_auth_no_state_change() {
  SrtpRx s = fresh();
  feed(s, 7);
  const SrtpRx before = s;
  u64 v;
  CHECK(feed(s, 30000, false, &v) == LKF_SRTP_RX_AUTH && v == 30000);
  CHECK(s.sl == before.sl && s.mask == before.mask && s.started == 1 && s.authFail == 1 && s.accepted == 1);
  SrtpRx f = fresh();
  CHECK(feed(f, 9, false) == LKF_SRTP_RX_AUTH && f.started == 0);
  CHECK(feed(f, 9, true) == LKF_SRTP_RX_OK && f.sl == 9);
}
static void t_negative_index_falls_back() {
  SrtpRx s = fresh();
  feed(s, 3);
  u64 v;
  // SEQ 65530 is 9 behind index 3: s_l + (int16) = -6, so v = SEQ
  CHECK(feed(s, 65530, true, &v) == LKF_SRTP_RX_OK && v == 65530);
  CHECK(s.sl == 65530 && s.mask == 1);
}
static void t_malformed_counts() {
  SrtpRx s = fresh();
  u64 v = 99;
  CHECK(step(s, true, 5, true, v) == LKF_SRTP_RX_MALFORMED && v == 0);
  CHECK(s.malformed == 1 && s.started == 0);
}

// a datagram at `off` of a zeroed arena
static Parsed parse_of(const std::vector<u8> &d, u32 off, u32 tag, u64 arenaLen = 0) {
  std::vector<u8> arena(off + d.size() + 1, 0);
  if (!d.empty()) std::memcpy(arena.data() + off, d.data(), d.size());
  return parse(arena.data(), arenaLen ? arenaLen : off + d.size(), off, u32(d.size()), tag);
}
static std::vector<u8> pkt(u8 b0, u32 seq, size_t total) {
  std::vector<u8> d(total, 0);
  d[0] = b0;
  d[2] = u8(seq >> 8);
  d[3] = u8(seq);
  return d;
}
static void t_parse_plain() {
  const Parsed p = parse_of(pkt(0x80, 0xABCD, 22), 16, 10);
  CHECK(!p.malformed && p.seq == 0xABCD && p.h == 12);
}
static void t_parse_short() { CHECK(parse_of(pkt(0x80, 1, 11), 0, 10).malformed); }
static void t_parse_version() {
  CHECK(parse_of(pkt(0x40, 1, 40), 0, 10).malformed);
  CHECK(parse_of(pkt(0xC0, 1, 40), 0, 10).malformed);
}
static void t_parse_misaligned() { CHECK(parse_of(pkt(0x80, 1, 40), 8, 10).malformed); }
static void t_parse_csrc() {
  CHECK(parse_of(pkt(0x82, 1, 30), 0, 10).h == 20);
  CHECK(parse_of(pkt(0x82, 1, 29), 0, 10).malformed);
}
static void t_parse_ext() {
  std::vector<u8> d = pkt(0x90, 1, 12 + 4 + 8 + 16);
  d[12] = 0xBE, d[13] = 0xDE, d[15] = 2;  // one-byte profile, two words
  CHECK(parse_of(d, 0, 16).h == 24);
  d[12] = 0x10, d[13] = 0x00;  // two-byte profile
  CHECK(parse_of(d, 0, 16).h == 24);
  d[15] = 3;  // one word more than the datagram has room for before the tag
  CHECK(parse_of(d, 0, 16).malformed);
  CHECK(parse_of(pkt(0x90, 1, 14), 0, 0).malformed);  // no room for the extension header itself
}
static void t_parse_short_for_tag() {
  CHECK(!parse_of(pkt(0x80, 1, 22), 0, 10).malformed);
  CHECK(parse_of(pkt(0x80, 1, 21), 0, 10).malformed);
  CHECK(parse_of(pkt(0x80, 1, 27), 0, 16).malformed);
}
static void t_parse_outside_arena() { CHECK(parse_of(pkt(0x80, 1, 40), 16, 10, 55).malformed); }

struct Case {
  const char *name;
  void (*fn)();
};
static const Case kCases[] = {
    {"first_packet", t_first_packet},
    {"in_order", t_in_order},
    {"wrap_forward", t_wrap_forward},
    {"reorder_across_wrap", t_reorder_across_wrap},
    {"dup", t_dup},
    {"behind_63", t_behind_63},
    {"behind_64", t_behind_64},
    {"jump_shift_64", t_jump_shift_64},
    {"auth_no_state_change", t_auth_no_state_change},
    {"negative_index_falls_back", t_negative_index_falls_back},
    {"malformed_counts", t_malformed_counts},
    {"parse_plain", t_parse_plain},
    {"parse_short", t_parse_short},
    {"parse_version", t_parse_version},
    {"parse_misaligned", t_parse_misaligned},
    {"parse_csrc", t_parse_csrc},
    {"parse_ext", t_parse_ext},
    {"parse_short_for_tag", t_parse_short_for_tag},
    {"parse_outside_arena", t_parse_outside_arena},
};

static void print_state(const SrtpRx &s) {
  std::printf("state started=%u s_l=%" PRIu64 " mask=%" PRIu64 " accepted=%" PRIu64 " auth_failures=%" PRIu64
              " replays=%" PRIu64 " malformed=%" PRIu64 "\n",
              s.started, s.sl, s.mask, s.accepted, s.authFail, s.replay, s.malformed);
}

static int replay() {
  SrtpRx s = fresh();
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string op;
    if (!(in >> op)) continue;
    if (op == "p") {
      u32 seq = 0, mal = 0, auth = 0;
      in >> seq >> mal >> auth;
      u64 v = 0;
      const u32 st = step(s, mal != 0, seq & 0xffff, auth != 0, v);
      std::printf("p st=%u v=%" PRIu64 "\n", st, v);
    } else if (op == "d") {
      u32 tag = 0, off = 0;
      u64 alen = 0;
      std::string hex;
      in >> tag >> off >> alen >> hex;
      if (hex == "-") hex.clear();
      std::vector<u8> d(hex.size() / 2);
      for (size_t i = 0; i < d.size(); i++) d[i] = u8(std::stoul(hex.substr(2 * i, 2), nullptr, 16));
      const Parsed p = parse_of(d, off, tag, alen);
      std::printf("d malformed=%u seq=%u h=%u\n", p.malformed, p.malformed ? 0 : p.seq, p.malformed ? 0 : p.h);
    } else if (op == "state") {
      print_state(s);
    } else if (op == "reset") {
      print_state(s);
      s = fresh();
    } else {
      std::fprintf(stderr, "unknown op: %s\n", op.c_str());
      return 2;
    }
  }
  return 0;
}

int main(int argc, char **argv) {
  const std::string arg = argc > 1 ? argv[1] : "";
  if (arg == "--list") {
    for (const Case &c : kCases) std::printf("%s\n", c.name);
    return 0;
  }
  if (arg == "--replay") return replay();
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
