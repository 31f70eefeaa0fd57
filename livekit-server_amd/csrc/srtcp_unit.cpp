// srtcp_unit.cpp — CPU unit tests of the SRTCP receive steps (srtcp_device.h):
// the datagram parse for both tag lengths, the per-SSRC slot table of a
// transport, the 64-packet replay window over the explicit index and the
// commit.  The authentication outcome is an input.  Built with the host
// compiler alone (make srtcp_unit; address + undefined sanitizers).
//   srtcp_unit --list     the case names
//   srtcp_unit <name>     one case ("PASS <name>" / exit 1)
//   srtcp_unit            every case
//   srtcp_unit --replay   a script on stdin (below), results on stdout
//
// --replay script, one op per line, integers in decimal:
//   p <st> <ssrc> <index> <auth>      one datagram of the transport whose parse gave <st> (0, 1 or 5),
//                                     <ssrc> and <index>: prints "p st=<status>"
//   d <tag> <off> <arena_len> <hex>   parse of the datagram <hex> placed at <off> of an arena of
//                                     <arena_len> bytes: prints "d st=<st> ssrc=<ssrc> index=<index>"
//   state                             prints the counters and the 16 slots
//   reset                             prints them, then a fresh transport (the next script)
// Every datagram parsed ends at the end of a heap block, so a read past it is
// an AddressSanitizer report.
#define __host__
#define __device__
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "srtcp_device.h"

using namespace lkf::srtcp;

static_assert(sizeof(lkf_srtcp_raw) == 12, "lkf_srtcp_raw is 12 B");
static_assert(sizeof(lkf_srtcp_rx_result) == 16, "lkf_srtcp_rx_result is 16 B");
static_assert(sizeof(lkf_rtcp_entry) == 8, "lkf_rtcp_entry is 8 B");
static_assert(sizeof(lkf_transport_srtcp) == 368, "lkf_transport_srtcp is 368 B");
static_assert(sizeof(lkf_srtcp_tx_result) == 16, "lkf_srtcp_tx_result is 16 B");

static int g_fail = 0;
#define CHECK(c)                                                         \
  do {                                                                   \
    if (!(c)) {                                                          \
      std::printf("  check failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
      g_fail++;                                                          \
    }                                                                    \
  } while (0)

static lkf_transport_srtcp fresh() {
  lkf_transport_srtcp t;
  std::memset(&t, 0, sizeof(t));
  return t;
}
static u32 feed(lkf_transport_srtcp &t, u32 ssrc, u32 index, bool auth = true) {
  return step(t, Parsed{LKF_SRTCP_RX_OK, ssrc, index}, auth);
}

static void t_first_packet() {
  lkf_transport_srtcp t = fresh();
  CHECK(feed(t, 0xAABBCCDD, 1) == LKF_SRTCP_RX_OK);
  CHECK(t.in_use[0] == 1 && t.ssrc[0] == 0xAABBCCDD && t.latest[0] == 1 && t.mask[0] == 1 && t.accepted == 1);
  CHECK(t.in_use[1] == 0);
}
static void t_in_order() {
  lkf_transport_srtcp t = fresh();
  for (u32 q = 1; q <= 10; q++) CHECK(feed(t, 7, q) == LKF_SRTCP_RX_OK);
  CHECK(t.latest[0] == 10 && t.mask[0] == 0x3ff && t.accepted == 10);
}
static void t_index_zero_first() {
  lkf_transport_srtcp t = fresh();
  CHECK(feed(t, 7, 0) == LKF_SRTCP_RX_OK);
  CHECK(t.in_use[0] == 1 && t.latest[0] == 0 && t.mask[0] == 1);
  CHECK(feed(t, 7, 0) == LKF_SRTCP_RX_REPLAY_DUP);
}
static void t_dup() {
  lkf_transport_srtcp t = fresh();
  feed(t, 7, 100);
  feed(t, 7, 101);
  CHECK(feed(t, 7, 101) == LKF_SRTCP_RX_REPLAY_DUP);
  CHECK(feed(t, 7, 100) == LKF_SRTCP_RX_REPLAY_DUP);
  CHECK(t.replays == 2 && t.accepted == 2 && t.mask[0] == 3);
}
static void t_behind_63() {
  lkf_transport_srtcp t = fresh();
  feed(t, 7, 1000);
  feed(t, 7, 1100);
  CHECK(feed(t, 7, 1037) == LKF_SRTCP_RX_OK);
  CHECK(t.mask[0] == ((1ull << 63) | 1));
  CHECK(feed(t, 7, 1037) == LKF_SRTCP_RX_REPLAY_DUP);
}
static void t_behind_64() {
  lkf_transport_srtcp t = fresh();
  feed(t, 7, 1000);
  feed(t, 7, 1100);
  CHECK(feed(t, 7, 1036) == LKF_SRTCP_RX_REPLAY_OLD);
  CHECK(t.replays == 1 && t.mask[0] == 1);
}
static void t_jump_shift_64() {
  lkf_transport_srtcp t = fresh();
  feed(t, 7, 5);
  feed(t, 7, 5 + 63);
  CHECK(t.mask[0] == ((1ull << 63) | 1));
  feed(t, 7, 5 + 63 + 64);  // shift of exactly 64: the whole window leaves
  CHECK(t.mask[0] == 1);
  feed(t, 7, 5 + 63 + 64 + 300);
  CHECK(t.mask[0] == 1 && t.latest[0] == 5 + 63 + 64 + 300);
}
static void t_carry_and_top() {
  lkf_transport_srtcp t = fresh();
  CHECK(feed(t, 7, 0xffff) == LKF_SRTCP_RX_OK);
  CHECK(feed(t, 7, 0x10000) == LKF_SRTCP_RX_OK && t.mask[0] == 3);
  CHECK(feed(t, 7, 0x7fffffff) == LKF_SRTCP_RX_OK && t.latest[0] == 0x7fffffff && t.mask[0] == 1);
  CHECK(feed(t, 7, 0) == LKF_SRTCP_RX_REPLAY_OLD);  // no wrap handling: plain unsigned
}
static void t_auth_no_state_change() {
  lkf_transport_srtcp t = fresh();
  feed(t, 7, 3);
  const lkf_transport_srtcp before = t;
  CHECK(feed(t, 7, 30000, false) == LKF_SRTCP_RX_AUTH);  // far ahead: latest does not move
  CHECK(t.latest[0] == before.latest[0] && t.mask[0] == before.mask[0] && t.auth_failures == 1);
  CHECK(feed(t, 99, 1, false) == LKF_SRTCP_RX_AUTH);  // a new SSRC: no slot taken
  CHECK(t.in_use[1] == 0 && t.auth_failures == 2 && t.accepted == 1);
  CHECK(feed(t, 99, 1, true) == LKF_SRTCP_RX_OK && t.in_use[1] == 1 && t.ssrc[1] == 99);
}
static void t_two_ssrcs_independent() {
  lkf_transport_srtcp t = fresh();
  feed(t, 1, 10);
  feed(t, 2, 10);
  feed(t, 1, 11);
  CHECK(t.ssrc[0] == 1 && t.latest[0] == 11 && t.mask[0] == 3);
  CHECK(t.ssrc[1] == 2 && t.latest[1] == 10 && t.mask[1] == 1);
  CHECK(feed(t, 2, 10) == LKF_SRTCP_RX_REPLAY_DUP && feed(t, 2, 11) == LKF_SRTCP_RX_OK);
}
static void t_table_fills() {
  lkf_transport_srtcp t = fresh();
  for (u32 s = 0; s < kSlots; s++) CHECK(feed(t, 1000 + s, 1) == LKF_SRTCP_RX_OK);
  for (u32 s = 0; s < kSlots; s++) CHECK(t.in_use[s] == 1 && t.ssrc[s] == 1000 + s);
  CHECK(feed(t, 5000, 1) == LKF_SRTCP_RX_NO_SLOT && t.no_slot == 1);
  CHECK(feed(t, 5000, 1, false) == LKF_SRTCP_RX_NO_SLOT);  // step 4 precedes step 5
  CHECK(feed(t, 1003, 2) == LKF_SRTCP_RX_OK && t.latest[3] == 2);  // an old SSRC is still served
  CHECK(t.accepted == kSlots + 1 && t.no_slot == 2);
}
static void t_parse_status_counts() {
  lkf_transport_srtcp t = fresh();
  CHECK(step(t, Parsed{LKF_SRTCP_RX_MALFORMED, 0, 0}, true) == LKF_SRTCP_RX_MALFORMED);
  CHECK(step(t, Parsed{LKF_SRTCP_RX_UNENCRYPTED, 0, 0}, true) == LKF_SRTCP_RX_UNENCRYPTED);
  CHECK(t.malformed == 1 && t.unencrypted == 1 && t.in_use[0] == 0 && t.accepted == 0);
}

// the datagram at `off` of an arena that ends where the datagram does (a heap block of exactly that size)
static Parsed parse_of(const std::vector<u8> &d, u32 off, u32 tag, u64 arenaLen = ~0ull) {
  std::unique_ptr<u8[]> arena(new u8[off + d.size()]);
  std::memset(arena.get(), 0, off);
  if (!d.empty()) std::memcpy(arena.get() + off, d.data(), d.size());
  return parse(arena.get(), arenaLen == ~0ull ? off + d.size() : arenaLen, off, u32(d.size()), tag);
}
static std::vector<u8> pkt(u8 b0, u32 ssrc, u32 trailer, size_t total, u32 tag) {
  std::vector<u8> d(total, 0x5A);
  d[0] = b0;
  for (int k = 0; k < 4; k++) d[4 + k] = u8(ssrc >> (24 - 8 * k));
  const size_t tp = trailer_pos(u32(total), tag);
  for (int k = 0; k < 4; k++) d[tp + k] = u8(trailer >> (24 - 8 * k));
  return d;
}
static void t_parse_cm() {
  const Parsed p = parse_of(pkt(0x81, 0xCAFEBABE, 0x80000000u | 77, 8 + 24 + 14, 10), 16, 10);
  CHECK(p.st == LKF_SRTCP_RX_OK && p.ssrc == 0xCAFEBABE && p.index == 77);
}
static void t_parse_gcm() {
  const Parsed p = parse_of(pkt(0x80, 0x01020304, 0xFFFFFFFFu, 8 + 20, 16), 0, 16);
  CHECK(p.st == LKF_SRTCP_RX_OK && p.ssrc == 0x01020304 && p.index == 0x7fffffff);
}
static void t_parse_short() {
  CHECK(parse_of(pkt(0x80, 1, 0x80000001u, 22, 10), 0, 10).st == LKF_SRTCP_RX_OK);  // an empty body
  CHECK(parse_of(std::vector<u8>(21, 0x80), 0, 10).st == LKF_SRTCP_RX_MALFORMED);
  CHECK(parse_of(pkt(0x80, 1, 0x80000001u, 28, 16), 0, 16).st == LKF_SRTCP_RX_OK);
  CHECK(parse_of(std::vector<u8>(27, 0x80), 0, 16).st == LKF_SRTCP_RX_MALFORMED);
  CHECK(parse_of({}, 0, 10).st == LKF_SRTCP_RX_MALFORMED);
}
static void t_parse_version() {
  CHECK(parse_of(pkt(0x40, 1, 0x80000001u, 40, 10), 0, 10).st == LKF_SRTCP_RX_MALFORMED);
  CHECK(parse_of(pkt(0xC0, 1, 0x80000001u, 40, 10), 0, 10).st == LKF_SRTCP_RX_MALFORMED);
  CHECK(parse_of(pkt(0x00, 1, 0x80000001u, 40, 16), 0, 16).st == LKF_SRTCP_RX_MALFORMED);
}
static void t_parse_misaligned() { CHECK(parse_of(pkt(0x80, 1, 0x80000001u, 40, 10), 8, 10).st == LKF_SRTCP_RX_MALFORMED); }
static void t_parse_outside_arena() {
  CHECK(parse_of(pkt(0x80, 1, 0x80000001u, 40, 10), 16, 10, 55).st == LKF_SRTCP_RX_MALFORMED);
}
static void t_parse_unencrypted() {
  const Parsed p = parse_of(pkt(0x80, 9, 0x00000005u, 40, 10), 0, 10);
  CHECK(p.st == LKF_SRTCP_RX_UNENCRYPTED && p.ssrc == 0 && p.index == 0);
  CHECK(parse_of(pkt(0x80, 9, 0x7fffffffu, 40, 16), 0, 16).st == LKF_SRTCP_RX_UNENCRYPTED);
}
static void t_parse_odd_length() {  // a forged datagram need not be a multiple of 4 bytes long
  const Parsed p = parse_of(pkt(0x80, 3, 0x80000009u, 37, 10), 0, 10);
  CHECK(p.st == LKF_SRTCP_RX_OK && p.index == 9);
}

struct Case {
  const char *name;
  void (*fn)();
};
static const Case kCases[] = {
    {"first_packet", t_first_packet},
    {"in_order", t_in_order},
    {"index_zero_first", t_index_zero_first},
    {"dup", t_dup},
    {"behind_63", t_behind_63},
    {"behind_64", t_behind_64},
    {"jump_shift_64", t_jump_shift_64},
    {"carry_and_top", t_carry_and_top},
    {"auth_no_state_change", t_auth_no_state_change},
    {"two_ssrcs_independent", t_two_ssrcs_independent},
    {"table_fills", t_table_fills},
    {"parse_status_counts", t_parse_status_counts},
    {"parse_cm", t_parse_cm},
    {"parse_gcm", t_parse_gcm},
    {"parse_short", t_parse_short},
    {"parse_version", t_parse_version},
    {"parse_misaligned", t_parse_misaligned},
    {"parse_outside_arena", t_parse_outside_arena},
    {"parse_unencrypted", t_parse_unencrypted},
    {"parse_odd_length", t_parse_odd_length},
};

static void print_state(const lkf_transport_srtcp &t) {
  std::printf("state accepted=%" PRIu64 " auth_failures=%" PRIu64 " replays=%" PRIu64 " malformed=%" PRIu64
              " unencrypted=%" PRIu64 " no_slot=%" PRIu64 "\n",
              t.accepted, t.auth_failures, t.replays, t.malformed, t.unencrypted, t.no_slot);
  for (u32 k = 0; k < kSlots; k++)
    std::printf("slot i=%u in_use=%u ssrc=%u latest=%u mask=%" PRIu64 "\n", k, t.in_use[k], t.ssrc[k], t.latest[k],
                t.mask[k]);
}

static int replay() {
  lkf_transport_srtcp t = fresh();
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string op;
    if (!(in >> op)) continue;
    if (op == "p") {
      u32 st = 0, ssrc = 0, index = 0, auth = 0;
      in >> st >> ssrc >> index >> auth;
      std::printf("p st=%u\n", step(t, Parsed{st, ssrc, index}, auth != 0));
    } else if (op == "d") {
      u32 tag = 0, off = 0;
      u64 alen = 0;
      std::string hex;
      in >> tag >> off >> alen >> hex;
      if (hex == "-") hex.clear();
      std::vector<u8> d(hex.size() / 2);
      for (size_t i = 0; i < d.size(); i++) d[i] = u8(std::stoul(hex.substr(2 * i, 2), nullptr, 16));
      const Parsed p = parse_of(d, off, tag, alen);
      std::printf("d st=%u ssrc=%u index=%u\n", p.st, p.ssrc, p.index);
    } else if (op == "state") {
      print_state(t);
    } else if (op == "reset") {
      print_state(t);
      t = fresh();
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
