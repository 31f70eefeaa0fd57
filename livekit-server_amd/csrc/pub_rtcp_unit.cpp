// pub_rtcp_unit.cpp — CPU unit tests of the publisher RTCP loop's scalar
// semantics (pub_rtcp_device.h): the reception report's nil cases, clamps and
// conversions, the sender report's early returns, wrap, skew test and
// first-packet-time adjustment, the walk over a publisher's compound packet
// and the two marshallers.  Built with the host compiler alone (make
// pub_rtcp_unit; address + undefined sanitizers).
//   pub_rtcp_unit --list     the case names
//   pub_rtcp_unit <name>     one case ("PASS <name>" / exit 1)
//   pub_rtcp_unit            every case
//   pub_rtcp_unit --replay   a script on stdin (below), results and state on stdout
//
// --replay script, one op per line, integers in decimal:
//   stream <clock> <ssrc>                    DevStream (first line of a script)
//   init <t> <sn> <ts>                       the first packet: S_INIT, the starts, firstTime
//   adv <ext_highest_sn> <packets_lost> <jitter bits>      the counters the later packets moved
//   sr <now> <rtp> <ntp>                     SetSenderReportData
//   bytes <now> <hex | ->                    one compound packet (- : len 0), parsed in a heap
//                                            block of its exact length
//   rr <now> <proxy>                         GetRtcpReceptionReport and its 32 bytes
//   close                                    Buffer.Close
//   state                                    prints the state
//   reset                                    prints the state, then a fresh stream (the next script)
// Each sr / bytes / rr prints one line of name=value integers; the state is
// printed at the end as well.
#define __host__
#define __device__
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "pub_rtcp_device.h"

using namespace lkf;
using namespace lkf::pubrtcp;
using lkf::rtcp::ntp_from_unix;

static_assert(sizeof(lkf_stream_rtcp) == sizeof(StreamRtcp), "lkf_stream_rtcp is StreamRtcp's layout");

static int g_fail = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::printf("  check failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
      g_fail++;                                                    \
    }                                                              \
  } while (0)

struct St {
  StreamRtcp R;
  StreamHot H;
  DevStream D;
  St() {
    std::memset(&R, 0, sizeof(R));
    std::memset(&H, 0, sizeof(H));
    std::memset(&D, 0, sizeof(D));
    D.clockRate = 90000;
    D.ssrc = 0x11223344u;
  }
};
static const i64 T0 = 1700000000LL * 1000000000LL;
static const i64 SEC = 1000000000LL;
static const i64 MS = 1000000LL;

static void first_packet(St &s, i64 t, u16 sn, u32 ts) {
  s.H.flags |= S_INIT | S_SN_INIT | S_TS_INIT;
  s.H.snStart = s.H.snHighest = sn;
  s.H.snExtHighest = sn;
  s.H.tsStart = s.H.tsHighest = ts;
  s.H.tsExtHighest = ts;
  s.H.firstTime = s.H.highestTime = t;
}
static St started(u16 sn = 100, u32 ts = 5000) {
  St s;
  first_packet(s, T0, sn, ts);
  return s;
}
static lkf_stream_rr report(St &s, u32 proxy, i64 now) {
  lkf_stream_rr o;
  reception_report(s.R, s.H, s.D, 3, proxy, now, o);
  return o;
}
static lkf_stream_sr_result sender(St &s, u32 rtp, u64 ntp, i64 now) {
  lkf_stream_sr_result o;
  set_sender_report(s.R, s.H, s.D, rtp, ntp, now, o);
  return o;
}
// a compound packet parsed in a heap block of its exact length (the sanitizer sees every byte past it)
static lkf_stream_rtcp_in_result ingest(St &s, const std::vector<u8> &b, i64 now) {
  u8 *p = static_cast<u8 *>(std::malloc(b.size() ? b.size() : 1));
  if (!b.empty()) std::memcpy(p, b.data(), b.size());
  lkf_stream_rtcp_in_result r;
  ingest_entry(s.R, s.H, s.D, p, u32(b.size()), now, r);
  std::free(p);
  return r;
}
static void put32(std::vector<u8> &b, u32 v) {
  for (int k = 3; k >= 0; k--) b.push_back(u8(v >> (8 * k)));
}
static void hdr(std::vector<u8> &b, u32 count, u32 pt, u32 words) { put32(b, (2u << 30) | (count << 24) | (pt << 16) | words); }
static std::vector<u8> sr_pkt(u32 ssrc, u64 ntp, u32 rtp, u32 blocks = 0, int lengthDelta = 0) {
  std::vector<u8> b;
  hdr(b, blocks, 200, u32(int(6 + 6 * blocks) + lengthDelta));
  put32(b, ssrc);
  put32(b, u32(ntp >> 32));
  put32(b, u32(ntp));
  put32(b, rtp);
  put32(b, 10);
  put32(b, 1000);
  for (u32 k = 0; k < 6 * blocks; k++) put32(b, 0);
  for (int k = 0; k < lengthDelta; k++) put32(b, 0);
  if (lengthDelta < 0) b.resize(b.size() + 4 * lengthDelta);
  return b;
}
static std::vector<u8> sdes_pkt(u32 ssrc) {
  std::vector<u8> b;
  hdr(b, 1, 202, 3);
  put32(b, ssrc);
  const u8 item[8] = {1, 5, 'c', 'n', 'a', 'm', 'e', 0};
  b.insert(b.end(), item, item + 8);
  return b;
}
static std::vector<u8> rr_pkt(u32 ssrc) {
  std::vector<u8> b;
  hdr(b, 0, 201, 1);
  put32(b, ssrc);
  return b;
}
static std::vector<u8> cat(std::vector<u8> a, const std::vector<u8> &b) {
  a.insert(a.end(), b.begin(), b.end());
  return a;
}

// ---- reception reports ---------------------------------------------------------
static void rr_uninitialized() {
  St s;
  const StreamRtcp before = s.R;
  const lkf_stream_rr o = report(s, 9, T0);
  CHECK(o.flags == 0 && o.stream == 3 && o.fraction_lost == 0);
  CHECK(std::memcmp(&before, &s.R, sizeof(before)) == 0);
}
static void rr_first_from_start() {
  St s = started(100);
  s.H.snExtHighest = 109;  // 100 .. 109: 10 expected
  const lkf_stream_rr o = report(s, 0, T0 + SEC);
  CHECK(o.flags == LKF_SRR_VALID && o.ssrc == 0x11223344u);
  CHECK(o.fraction_lost == 0 && o.total_lost == 0 && o.last_sequence_number == 110);
  CHECK(s.R.started == 1 && s.R.startTime == T0);
  CHECK(s.R.snapIsValid == 1 && s.R.snapStartTime == T0 + SEC && s.R.snapExtStartSN == 110);
}
static void rr_nothing_expected() {
  St s = started(100);
  s.H.snExtHighest = 109;
  report(s, 0, T0 + SEC);
  const lkf_stream_rr o = report(s, 77, T0 + 2 * SEC);
  CHECK(o.flags == 0);
  CHECK(s.R.snapStartTime == T0 + 2 * SEC);  // replaced all the same
}
static void rr_3_of_20() {
  St s = started(100);
  s.H.snExtHighest = 119;
  s.H.packetsLost = 3;
  const lkf_stream_rr o = report(s, 0, T0 + SEC);
  CHECK(o.flags == LKF_SRR_VALID && o.fraction_lost == 38 && o.total_lost == 3);  // float32(3) / float32(20) * 256 = 38.4
}
static void rr_proxy() {
  St s = started(100);
  s.H.snExtHighest = 119;
  s.H.packetsLost = 3;
  CHECK(report(s, 39, T0 + SEC).fraction_lost == 39);  // above the computed 38
  s.H.snExtHighest = 139;
  s.H.packetsLost = 6;
  CHECK(report(s, 37, T0 + 2 * SEC).fraction_lost == 38);  // below it
  s.H.snExtHighest = 159;
  s.H.packetsLost = 9;
  CHECK(report(s, 0x100 | 40, T0 + 3 * SEC).fraction_lost == 40);  // a uint8 in the reference: the low 8 bits
}
static void rr_loss_rate_one() {
  St s = started(100);
  s.H.snExtHighest = 119;
  s.H.packetsLost = 20;
  const lkf_stream_rr o = report(s, 0, T0 + SEC);
  CHECK(o.flags == LKF_SRR_VALID && o.fraction_lost == 0 && o.total_lost == 20);  // uint8(256.0)
  CHECK(f32_to_u8(256.0f) == 0 && f32_to_u8(255.9f) == 255 && f32_to_u8(3.0e9f) == 0 && f32_to_u8(511.5f) == 255);
}
static void rr_negative_lost_clamped() {
  St s = started(100);
  s.H.snExtHighest = 119;
  s.H.packetsLost = 5;
  report(s, 0, T0 + SEC);
  s.H.snExtHighest = 139;
  s.H.packetsLost = 2;  // reordered packets filled three holes
  const lkf_stream_rr o = report(s, 0, T0 + 2 * SEC);
  CHECK(o.flags == LKF_SRR_VALID && o.fraction_lost == 0 && o.total_lost == 2);
}
static void rr_expected_65536() {
  St s = started(100);
  s.H.snExtHighest = 100 + 65535;
  const lkf_stream_rr o = report(s, 0, T0 + SEC);
  CHECK(o.flags == LKF_SRR_VALID && o.last_sequence_number == 100 + 65536);
}
static void rr_expected_65537() {
  St s = started(100);
  s.H.snExtHighest = 100 + 65536;
  const lkf_stream_rr o = report(s, 0, T0 + SEC);
  CHECK(o.flags == 0);
  CHECK(s.R.snapIsValid == 1 && s.R.snapExtStartSN == 100 + 65537 && s.R.snapStartTime == T0 + SEC);
  s.H.snExtHighest += 5;
  CHECK(report(s, 0, T0 + 2 * SEC).flags == LKF_SRR_VALID);
}
static void rr_total_lost_saturates() {
  St s = started(100);
  s.H.snExtHighest = 119;
  s.H.packetsLost = 0x1000000ull;
  CHECK(report(s, 0, T0 + SEC).total_lost == 0xffffffu);
  s.H.snExtHighest = 139;
  s.H.packetsLost = u64(0) - 1;  // more reordered than lost so far: the uint64 wrapped
  CHECK(report(s, 0, T0 + 2 * SEC).total_lost == 0xffffffu);
}
static void rr_sequence_wrap() {
  St s = started(65530);
  s.H.snExtHighest = 65536 + 4;  // wrapped: 65530 .. 65535, 0 .. 4
  const lkf_stream_rr o = report(s, 0, T0 + SEC);
  CHECK(o.flags == LKF_SRR_VALID && o.last_sequence_number == 65536 + 5);
  s.H.snExtHighest = 65536 + 24;
  s.H.packetsLost = 3;
  const lkf_stream_rr p = report(s, 0, T0 + 2 * SEC);
  CHECK(p.fraction_lost == 38 && p.last_sequence_number == 65536 + 25);
}
static void rr_no_sr() {
  St s = started(100);
  s.H.snExtHighest = 119;
  const lkf_stream_rr o = report(s, 0, T0 + SEC);
  CHECK(o.last_sender_report == 0 && o.delay == 0);
}
static void rr_dlsr() {
  St s = started(100);
  const u64 ntp = ntp_from_unix(T0 + 5 * MS);
  sender(s, 5450, ntp, T0 + 10 * MS);
  s.H.snExtHighest = 119;
  lkf_stream_rr o = report(s, 0, T0 + 10 * MS + 1000);  // 1 us: 65536 / 1e6 = 0
  CHECK(o.last_sender_report == u32(ntp >> 16) && o.delay == 0);
  s.H.snExtHighest = 139;
  o = report(s, 0, T0 + 10 * MS + SEC);
  CHECK(o.delay == 65536);
  s.H.snExtHighest = 159;
  o = report(s, 0, T0 + 10 * MS + 1234567899);  // 1234567 us * 65536 / 1e6 = 80908.58...
  CHECK(o.delay == 80908);
  s.H.snExtHighest = 179;
  o = report(s, 0, T0 + 10 * MS + 999);  // below 1 us
  CHECK(o.delay == 0);
}
static void rr_jitter_conversion() {
  St s = started(100);
  s.H.snExtHighest = 119;
  s.H.jitter = 1234.99;
  CHECK(report(s, 0, T0 + SEC).jitter == 1234);
  CHECK(f64_to_u32(4294967296.0 + 7.5) == 7 && f64_to_u32(1e30) == 0 && f64_to_u32(-1.0) == 0xffffffffu);
}
static void rr_wire() {
  St s = started(100);
  sender(s, 5450, ntp_from_unix(T0 + 5 * MS), T0 + 10 * MS);
  s.H.snExtHighest = 119;
  s.H.packetsLost = 3;
  s.H.jitter = 77.5;
  const lkf_stream_rr o = report(s, 0, T0 + SEC);
  u8 w[32];
  receiver_report_wire(o, w);
  const u8 head[12] = {0x81, 201, 0, 7, 0x11, 0x22, 0x33, 0x44, 0x11, 0x22, 0x33, 0x44};
  CHECK(std::memcmp(w, head, 12) == 0);
  CHECK(w[12] == o.fraction_lost && rtcpin::be24(w + 13) == o.total_lost);
  CHECK(rtcpin::be32(w + 16) == o.last_sequence_number && rtcpin::be32(w + 20) == o.jitter);
  CHECK(rtcpin::be32(w + 24) == o.last_sender_report && rtcpin::be32(w + 28) == o.delay);
  std::printf("wire");
  for (int i = 0; i < 32; i++) std::printf(" %02x", w[i]);
  std::printf("\nrecord %u %u %u %u %u %u %u\n", o.ssrc, o.fraction_lost, o.total_lost, o.last_sequence_number, o.jitter,
              o.last_sender_report, o.delay);
  lkf_stream_rr z = o;
  z.flags = 0;
  receiver_report_wire(z, w);
  for (int i = 0; i < 32; i++) CHECK(w[i] == 0);
}
static void rr_closed() {
  St s = started(100);
  s.H.snExtHighest = 119;
  s.D.closed = 1;
  const StreamRtcp before = s.R;
  CHECK(report(s, 0, T0 + SEC).flags == 0);
  CHECK(std::memcmp(&before, &s.R, sizeof(before)) == 0);
}
// TestFractionLostReport buffer_test.go:221-263: an Opus stream, 15 packets with
// SN = TS = i, one second slept after the first, proxy 55; doReports' gate is
// the caller's (buffer.go:688-700, lastReport starts as the zero time)
static void fraction_lost_report() {
  St s;
  s.D.clockRate = 48000;
  i64 now = T0, lastReport = 0;
  int reports = 0;
  for (int i = 0; i < 15; i++) {
    if (i == 1) now += SEC;
    if (i == 0) first_packet(s, now, 0, 0);
    s.H.snExtHighest = u64(i);
    s.H.tsExtHighest = u64(i);
    if (now - lastReport < SEC) continue;
    lastReport = now;
    const lkf_stream_rr o = report(s, 55, now);
    if (o.flags & LKF_SRR_VALID) {
      CHECK(o.fraction_lost == 55);
      reports++;
    }
    now += MS;
  }
  CHECK(reports == 2);
}

// ---- sender reports ------------------------------------------------------------
static void sr_before_init() {
  St s;
  const StreamRtcp before = s.R;
  const lkf_stream_sr_result o = sender(s, 1, ntp_from_unix(T0), T0);
  CHECK(o.flags == LKF_SSR_IGNORED_UNINIT && o.ntp == 0 && o.rtp_ext == 0);
  CHECK(std::memcmp(&before, &s.R, sizeof(before)) == 0);
}
static void sr_first() {
  St s = started(100, 5000);
  const u64 ntp = ntp_from_unix(T0 + 5 * MS);
  const lkf_stream_sr_result o = sender(s, 5450, ntp, T0 + 10 * MS);  // 450 ticks = 5 ms: firstTime + 5 ms, later
  CHECK(o.flags == 0 && o.ntp == ntp && o.rtp_ext == 5450);
  CHECK(s.R.srNewest.valid && s.R.srFirst.valid && std::memcmp(&s.R.srFirst, &s.R.srNewest, sizeof(RtcpSrData)) == 0);
  CHECK(s.R.srNewest.at == T0 + 10 * MS && s.R.srNewest.ntp == ntp && s.R.srNewest.rtpExt == 5450);
  CHECK(s.R.started == 1 && s.R.startTime == T0 && s.H.firstTime == T0);
}
static void sr_anachronous() {
  St s = started();
  sender(s, 5450, ntp_from_unix(T0 + SEC), T0 + SEC);
  const StreamRtcp before = s.R;
  const lkf_stream_sr_result o = sender(s, 95450, ntp_from_unix(T0 + SEC) - 1, T0 + 2 * SEC);
  CHECK(o.flags == LKF_SSR_ANACHRONOUS && o.ntp == 0);
  CHECK(std::memcmp(&before, &s.R, sizeof(before)) == 0);
}
static void sr_rtp_forward_wrap() {
  St s = started(100, 0xFFFF0000u);
  sender(s, 0xFFFFF000u, ntp_from_unix(T0 + SEC), T0 + SEC);
  const lkf_stream_sr_result o = sender(s, 0x00015000u, ntp_from_unix(T0 + 2 * SEC), T0 + 2 * SEC);
  CHECK(o.rtp_ext == 0x100015000ull && !(o.flags & LKF_SSR_RESET_FIRST));
  CHECK(s.R.srFirst.rtpExt == 0xFFFFF000ull && s.R.outOfOrderSenderReportCount == 0);
}
static void sr_backwards_resets_first() {
  St s = started();
  sender(s, 200000, ntp_from_unix(T0 + SEC), T0 + SEC);
  sender(s, 290000, ntp_from_unix(T0 + 2 * SEC), T0 + 2 * SEC);
  const lkf_stream_sr_result o = sender(s, 100000, ntp_from_unix(T0 + 3 * SEC), T0 + 3 * SEC);
  CHECK(o.flags & LKF_SSR_RESET_FIRST);
  CHECK(o.rtp_ext == 100000 && s.R.outOfOrderSenderReportCount == 1);
  CHECK(s.R.srFirst.rtpExt == 100000 && s.R.srFirst.at == T0 + 3 * SEC && s.R.srNewest.rtpExt == 100000);
}
static void sr_clock_skew() {
  {  // half the rate over the one interval there is: against both
    St s = started();
    sender(s, 100000, ntp_from_unix(T0 + SEC), T0 + SEC);
    sender(s, 100000 + 90000 / 2, ntp_from_unix(T0 + 2 * SEC), T0 + 2 * SEC);
    CHECK(s.R.clockSkewCount == 1);
    // against the last only: three right intervals, then 120000 ticks in 1 s
    St t = started();
    sender(t, 100000, ntp_from_unix(T0 + SEC), T0 + SEC);
    sender(t, 190000, ntp_from_unix(T0 + 2 * SEC), T0 + 2 * SEC);
    sender(t, 280000, ntp_from_unix(T0 + 3 * SEC), T0 + 3 * SEC);
    sender(t, 370000, ntp_from_unix(T0 + 4 * SEC), T0 + 4 * SEC);
    CHECK(t.R.clockSkewCount == 0);
    const lkf_stream_sr_result o = sender(t, 370000 + 120000, ntp_from_unix(T0 + 5 * SEC), T0 + 5 * SEC);
    CHECK((o.flags & LKF_SSR_CLOCK_SKEW) && t.R.clockSkewCount == 1);  // last: 120000 / s; first: 390000 / 4 s = 97500
  }
  {  // against the first only: the last interval is right, the sum is not
    St s = started();
    sender(s, 100000, ntp_from_unix(T0 + SEC), T0 + SEC);
    s.R.srNewest.rtpExt = 100000 + 200000;  // (the state a skewed middle report leaves)
    s.R.srNewest.ntp = ntp_from_unix(T0 + 2 * SEC);
    const lkf_stream_sr_result o = sender(s, 100000 + 290000, ntp_from_unix(T0 + 3 * SEC), T0 + 3 * SEC);
    CHECK((o.flags & LKF_SSR_CLOCK_SKEW) && s.R.clockSkewCount == 1);  // last: 90000 / s; first: 290000 / 2 s
  }
  {  // under the 0.2 s floor: 0.1 s with twice the ticks is not tested
    St s = started();
    sender(s, 100000, ntp_from_unix(T0 + SEC), T0 + SEC);
    const lkf_stream_sr_result o = sender(s, 100000 + 18000, ntp_from_unix(T0 + SEC + 100 * MS), T0 + SEC + 100 * MS);
    CHECK(!(o.flags & LKF_SSR_CLOCK_SKEW) && s.R.clockSkewCount == 0);
  }
}
static void sr_first_time_earlier() {
  St s = started(100, 5000);
  // 1 s after the first packet the report says 1.5 s of samples have passed: the first packet was 0.5 s late
  const lkf_stream_sr_result o = sender(s, 5000 + 135000, ntp_from_unix(T0 + SEC), T0 + SEC);
  CHECK(o.flags == LKF_SSR_FIRST_TIME_ADJUSTED);
  CHECK(s.H.firstTime == T0 - SEC / 2 && s.R.startTime == T0);
}
static void sr_first_time_not_later() {
  St s = started(100, 5000);
  const lkf_stream_sr_result o = sender(s, 5000 + 45000, ntp_from_unix(T0 + SEC), T0 + SEC);
  CHECK(o.flags == 0 && s.H.firstTime == T0);
}
static void sr_adjust_too_big() {
  St s = started(100, 5000);
  const lkf_stream_sr_result o = sender(s, 5000 + 90000 * 302, ntp_from_unix(T0 + SEC), T0 + SEC);  // 301 s earlier
  CHECK(o.flags == LKF_SSR_ADJUST_TOO_BIG && s.H.firstTime == T0);
  St t = started(100, 5000);
  CHECK(sender(t, 5000 + 90000 * 301, ntp_from_unix(T0 + SEC), T0 + SEC).flags == LKF_SSR_FIRST_TIME_ADJUSTED);  // exactly 5 min
  CHECK(t.H.firstTime == T0 - 300 * SEC);
}
static void sr_after_window() {
  St s = started(100, 5000);
  const i64 now = T0 + 120 * SEC + 1;
  const lkf_stream_sr_result o = sender(s, 5000 + 90000 * 130, ntp_from_unix(now), now);
  CHECK(o.flags == 0 && s.H.firstTime == T0);
  St t = started(100, 5000);
  CHECK(sender(t, 5000 + 90000 * 130, ntp_from_unix(now - 1), now - 1).flags == LKF_SSR_FIRST_TIME_ADJUSTED);  // at the window's edge
}
static void sr_samples_diff_negative() {
  St s = started(100, 5000);
  const lkf_stream_sr_result o = sender(s, 4000, ntp_from_unix(T0 + SEC), T0 + SEC);  // int32(4000 - 5000) < 0
  CHECK(o.flags == 0 && s.H.firstTime == T0 && o.rtp_ext == 4000);
}
static void sr_closed() {
  St s = started();
  s.D.closed = 1;
  const StreamRtcp before = s.R;
  CHECK(sender(s, 5450, ntp_from_unix(T0), T0).flags == LKF_SSR_CLOSED);
  CHECK(std::memcmp(&before, &s.R, sizeof(before)) == 0);
}

// ---- compounds -----------------------------------------------------------------
static void compound_sr_alone() {
  St s = started();
  const u64 ntp = ntp_from_unix(T0 + SEC);
  const lkf_stream_rtcp_in_result r = ingest(s, sr_pkt(0x11223344u, ntp, 95000), T0 + SEC);
  CHECK(r.status == LKF_RTCP_IN_OK && r.n_sr == 1 && r.flags == 0 && r.ntp == ntp && r.rtp_ext == 95000);
  CHECK(s.R.srNewest.valid && s.R.srNewest.ntp == ntp && s.R.srNewest.at == T0 + SEC);
}
static void compound_sr_sdes() {
  St s = started();
  const u64 ntp = ntp_from_unix(T0 + SEC);
  const lkf_stream_rtcp_in_result r = ingest(s, cat(sr_pkt(0x11223344u, ntp, 95000, 1), sdes_pkt(0x11223344u)), T0 + SEC);
  CHECK(r.status == LKF_RTCP_IN_OK && r.n_sr == 1 && r.ntp == ntp);
}
static void compound_two_srs() {
  St s = started();
  const u64 n1 = ntp_from_unix(T0 + SEC), n2 = ntp_from_unix(T0 + 2 * SEC);
  const lkf_stream_rtcp_in_result r = ingest(s, cat(sr_pkt(1, n1, 95000), sr_pkt(1, n2, 185000)), T0 + 2 * SEC);
  CHECK(r.status == LKF_RTCP_IN_OK && r.n_sr == 2 && r.ntp == n2 && r.rtp_ext == 185000);
  CHECK(s.R.srFirst.ntp == n1 && s.R.srNewest.ntp == n2);
  // in packet order: the other way round the second is anachronous
  St t = started();
  const lkf_stream_rtcp_in_result q = ingest(t, cat(sr_pkt(1, n2, 185000), sr_pkt(1, n1, 95000)), T0 + 2 * SEC);
  CHECK(q.n_sr == 2 && q.flags == LKF_SSR_ANACHRONOUS && q.ntp == n2 && t.R.srNewest.ntp == n2);
}
static void compound_rr_only() {
  St s = started();
  const StreamRtcp before = s.R;
  const lkf_stream_rtcp_in_result r = ingest(s, rr_pkt(7), T0 + SEC);
  CHECK(r.status == LKF_RTCP_IN_OK && r.n_sr == 0 && r.flags == 0 && r.ntp == 0);
  CHECK(std::memcmp(&before, &s.R, sizeof(before)) == 0);
}
static void compound_foreign_ssrc() {
  St s = started();
  const u64 ntp = ntp_from_unix(T0 + SEC);
  const lkf_stream_rtcp_in_result r = ingest(s, sr_pkt(0xdeadbeefu, ntp, 95000), T0 + SEC);
  CHECK(r.status == LKF_RTCP_IN_OK && r.n_sr == 1 && s.R.srNewest.ntp == ntp);  // mediatrack.go:204-205 does not compare
}
static void compound_truncated_sr() {
  St s = started();
  const StreamRtcp before = s.R;
  const StreamHot hot = s.H;
  // a valid SR, then one that claims a report block it has no room for (size 28 < 28 + 24)
  std::vector<u8> bad = sr_pkt(1, ntp_from_unix(T0 + 2 * SEC), 185000);
  bad[0] = 0x81;
  const lkf_stream_rtcp_in_result r = ingest(s, cat(sr_pkt(1, ntp_from_unix(T0 + SEC), 5000 + 135000), bad), T0 + SEC);
  CHECK(r.status == LKF_RTCP_IN_MALFORMED && r.n_sr == 0 && r.flags == 0 && r.ntp == 0);
  CHECK(std::memcmp(&before, &s.R, sizeof(before)) == 0 && std::memcmp(&hot, &s.H, sizeof(hot)) == 0);
  // and one shorter than the fixed part
  CHECK(ingest(s, sr_pkt(1, 5, 5, 0, -1), T0).status == LKF_RTCP_IN_MALFORMED);
}
static void compound_len_0() {
  St s = started();
  CHECK(ingest(s, {}, T0).status == LKF_RTCP_IN_MALFORMED);
}

// ---- NACK wire -------------------------------------------------------------------
static void nack_check(const std::vector<lkf_rtcp_nack> &recs, const std::vector<lkf_nack_pair> &pairs) {
  u64 total = 0;
  for (size_t i = 0; i < recs.size(); i++) {
    CHECK(nack_wire_off(u32(i), recs[i].pair_off) == total);  // packed: each packet follows the one before
    total += nack_wire_len(recs[i].n_pairs);
  }
  CHECK(total == 12 * recs.size() + 4 * pairs.size());
  for (size_t i = 0; i < recs.size(); i++) {
    const lkf_rtcp_nack &r = recs[i];
    CHECK(nack_wire_word(r, pairs.data() + r.pair_off, 0) == ((0x81u << 24) | (205u << 16) | (2u + r.n_pairs)));
    CHECK(nack_wire_word(r, pairs.data() + r.pair_off, 1) == r.media_ssrc);
    CHECK(nack_wire_word(r, pairs.data() + r.pair_off, 2) == r.media_ssrc);
    for (u32 k = 0; k < r.n_pairs; k++) {
      const lkf_nack_pair &p = pairs[r.pair_off + k];
      CHECK(nack_wire_word(r, pairs.data() + r.pair_off, 3 + k) == ((u32(p.packet_id) << 16) | p.lost_packets));
    }
  }
}
static std::vector<lkf_nack_pair> some_pairs(u32 n) {
  std::vector<lkf_nack_pair> p(n);
  for (u32 k = 0; k < n; k++) p[k] = lkf_nack_pair{u16(65530 + 20 * k), u16(0x8001u * (k + 1))};
  return p;
}
static void nack_wire_1() { nack_check({lkf_rtcp_nack{4, 1, 0xa1b2c3d4u, 0, 1, 3, 0}}, some_pairs(1)); }
static void nack_wire_17() { nack_check({lkf_rtcp_nack{0, 2, 0xa1b2c3d4u, 0, 17, 40, 0}}, some_pairs(17)); }
static void nack_wire_two_records() {
  nack_check({lkf_rtcp_nack{2, 0, 0x01020304u, 0, 3, 5, 0}, lkf_rtcp_nack{9, 1, 0x05060708u, 3, 2, 2, 0}}, some_pairs(5));
  CHECK(nack_wire_off(1, 3) == 24 && nack_wire_len(2) == 20);
}

struct Case {
  const char *name;
  void (*fn)();
};
static const Case kCases[] = {
    {"rr_uninitialized", rr_uninitialized},
    {"rr_first_from_start", rr_first_from_start},
    {"rr_nothing_expected", rr_nothing_expected},
    {"rr_3_of_20", rr_3_of_20},
    {"rr_proxy", rr_proxy},
    {"rr_loss_rate_one", rr_loss_rate_one},
    {"rr_negative_lost_clamped", rr_negative_lost_clamped},
    {"rr_expected_65536", rr_expected_65536},
    {"rr_expected_65537", rr_expected_65537},
    {"rr_total_lost_saturates", rr_total_lost_saturates},
    {"rr_sequence_wrap", rr_sequence_wrap},
    {"rr_no_sr", rr_no_sr},
    {"rr_dlsr", rr_dlsr},
    {"rr_jitter_conversion", rr_jitter_conversion},
    {"rr_wire", rr_wire},
    {"rr_closed", rr_closed},
    {"fraction_lost_report", fraction_lost_report},
    {"sr_before_init", sr_before_init},
    {"sr_first", sr_first},
    {"sr_anachronous", sr_anachronous},
    {"sr_rtp_forward_wrap", sr_rtp_forward_wrap},
    {"sr_backwards_resets_first", sr_backwards_resets_first},
    {"sr_clock_skew", sr_clock_skew},
    {"sr_first_time_earlier", sr_first_time_earlier},
    {"sr_first_time_not_later", sr_first_time_not_later},
    {"sr_adjust_too_big", sr_adjust_too_big},
    {"sr_after_window", sr_after_window},
    {"sr_samples_diff_negative", sr_samples_diff_negative},
    {"sr_closed", sr_closed},
    {"compound_sr_alone", compound_sr_alone},
    {"compound_sr_sdes", compound_sr_sdes},
    {"compound_two_srs", compound_two_srs},
    {"compound_rr_only", compound_rr_only},
    {"compound_foreign_ssrc", compound_foreign_ssrc},
    {"compound_truncated_sr", compound_truncated_sr},
    {"compound_len_0", compound_len_0},
    {"nack_wire_1", nack_wire_1},
    {"nack_wire_17", nack_wire_17},
    {"nack_wire_two_records", nack_wire_two_records},
};

// ---- --replay -------------------------------------------------------------------
static void print_state(const St &s) {
  const StreamRtcp &R = s.R;
  std::printf("state initialized=%u first_time=%" PRId64 " started=%u start_time=%" PRId64
              " snap_is_valid=%u snap_start_time=%" PRId64 " snap_ext_start_sn=%" PRIu64 " snap_packets_lost=%" PRIu64
              " clock_skew_count=%u out_of_order_sr_count=%u",
              (s.H.flags & S_INIT) ? 1u : 0u, s.H.firstTime, R.started, R.startTime, R.snapIsValid, R.snapStartTime,
              R.snapExtStartSN, R.snapPacketsLost, R.clockSkewCount, R.outOfOrderSenderReportCount);
  const RtcpSrData *sr[2] = {&R.srFirst, &R.srNewest};
  for (int i = 0; i < 2; i++)
    std::printf(" sr%d_valid=%u sr%d_ntp=%" PRIu64 " sr%d_rtp_ext=%" PRIu64 " sr%d_at=%" PRId64, i, sr[i]->valid, i,
                sr[i]->ntp, i, sr[i]->rtpExt, i, sr[i]->at);
  std::printf("\n");
}
static bool unhex(const std::string &h, std::vector<u8> &b) {
  b.clear();
  if (h == "-") return true;
  if (h.size() % 2) return false;
  for (size_t i = 0; i < h.size(); i += 2) {
    unsigned v;
    if (std::sscanf(h.c_str() + i, "%2x", &v) != 1) return false;
    b.push_back(u8(v));
  }
  return true;
}

static int replay() {
  St s;
  std::string op;
  while (std::cin >> op) {
    if (op == "stream") {
      u32 clock, ssrc;
      std::cin >> clock >> ssrc;
      s.D.clockRate = clock;
      s.D.ssrc = ssrc;
    } else if (op == "init") {
      i64 t;
      u32 sn, ts;
      std::cin >> t >> sn >> ts;
      first_packet(s, t, u16(sn), ts);
    } else if (op == "adv") {
      u64 high, lost, jb;
      std::cin >> high >> lost >> jb;
      s.H.snExtHighest = high;
      s.H.packetsLost = lost;
      std::memcpy(&s.H.jitter, &jb, 8);
    } else if (op == "sr") {
      i64 now;
      u32 rtp;
      u64 ntp;
      std::cin >> now >> rtp >> ntp;
      const lkf_stream_sr_result o = sender(s, rtp, ntp, now);
      std::printf("sr flags=%u ntp=%" PRIu64 " rtp_ext=%" PRIu64 "\n", o.flags, o.ntp, o.rtp_ext);
    } else if (op == "bytes") {
      i64 now;
      std::string h;
      std::cin >> now >> h;
      std::vector<u8> b;
      if (!unhex(h, b)) {
        std::fprintf(stderr, "bad hex\n");
        return 2;
      }
      const lkf_stream_rtcp_in_result r = ingest(s, b, now);
      std::printf("bytes status=%u n_sr=%u flags=%u ntp=%" PRIu64 " rtp_ext=%" PRIu64 "\n", r.status, r.n_sr, r.flags,
                  r.ntp, r.rtp_ext);
    } else if (op == "rr") {
      i64 now;
      u32 proxy;
      std::cin >> now >> proxy;
      const lkf_stream_rr o = report(s, proxy, now);
      u8 w[32];
      receiver_report_wire(o, w);
      std::printf("rr flags=%u ssrc=%u fraction_lost=%u total_lost=%u last_sequence_number=%u jitter=%u"
                  " last_sender_report=%u delay=%u wire=",
                  o.flags, o.ssrc, o.fraction_lost, o.total_lost, o.last_sequence_number, o.jitter, o.last_sender_report,
                  o.delay);
      for (int i = 0; i < 32; i++) std::printf("%02x", w[i]);
      std::printf("\n");
    } else if (op == "close") {
      s.D.closed = 1;
    } else if (op == "state") {
      print_state(s);
    } else if (op == "reset") {
      print_state(s);
      s = St();
    } else {
      std::fprintf(stderr, "unknown op %s\n", op.c_str());
      return 2;
    }
    if (!std::cin) {
      std::fprintf(stderr, "bad arguments of %s\n", op.c_str());
      return 2;
    }
  }
  print_state(s);
  return 0;
}

int main(int argc, char **argv) {
  if (argc > 1 && std::strcmp(argv[1], "--list") == 0) {
    for (const Case &c : kCases) std::printf("%s\n", c.name);
    return 0;
  }
  if (argc > 1 && std::strcmp(argv[1], "--replay") == 0) return replay();
  int ran = 0;
  for (const Case &c : kCases) {
    if (argc > 1 && std::strcmp(argv[1], c.name) != 0) continue;
    const int before = g_fail;
    c.fn();
    std::printf("%s %s\n", g_fail == before ? "PASS" : "FAIL", c.name);
    ran++;
  }
  if (!ran) {
    std::printf("no such case\n");
    return 1;
  }
  return g_fail ? 1 : 0;
}
