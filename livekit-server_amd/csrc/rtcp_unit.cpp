// rtcp_unit.cpp — CPU unit tests of the RTCP loop's scalar semantics
// (rtcp_device.h): the three mediatransportutil definitions, the receiver
// report's early returns and wrap-arounds, getIntervalStats' closed form
// against a brute-force loop, the sender report's branches and
// DeltaInfoSender's clamps.  Built with the host compiler alone (make
// rtcp_unit; address + undefined sanitizers).
//   rtcp_unit --list     the case names
//   rtcp_unit <name>     one case ("PASS <name>" / exit 1)
//   rtcp_unit            every case
//   rtcp_unit --replay   a script on stdin (below), results and state on stdout
//
// --replay script, one op per line, integers in decimal:
//   clock <rate>                             SenderStats.clockRate (first line)
//   ss <field> <value>                       a SenderStats field by name (initial state)
//   ring <slot> <value>                      an snInfo ring slot (initial state)
//   update <t> <esn> <ets> <marker> <hdr> <pay> <pad>      RTPStatsSender.Update
//   rr <now> <lsn> <total_lost> <jitter> <lsr> <dlsr>      UpdateFromReceiverReport
//   nack <nacks> <plis> <firs>                             UpdateNack / UpdatePli / UpdateFir
//   sr <now> <calculated_clock_rate>                       GetRtcpSenderReport (ssrc 0x11223344)
//   delta                                                  DeltaInfoSender
//   stop                                                   rtpStatsBase.Stop
//   state                                                  prints the state
//   reset                                                  prints the state, then a fresh DownTrack (the next script)
// Each rr / sr / delta prints one line of name=value integers (doubles as the
// 64 bits, in hex); the state is printed at the end as well.
#define __host__
#define __device__
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "rtcp_device.h"

using namespace lkf;
using namespace lkf::rtcp;

static_assert(sizeof(lkf_sender_rtcp) == sizeof(SenderRtcp), "lkf_sender_rtcp is SenderRtcp's layout");

static int g_fail = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::printf("  check failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
      g_fail++;                                                    \
    }                                                              \
  } while (0)

// ---- a copy of sender_device.h's scalar Update (that header is device code) --
static void ss_gap(u32 *gap, i64 g) {
  if (g < 2) return;
  const i64 missing = g - 1;
  gap[missing > kGapBins ? kGapBins - 1 : missing - 1]++;
}
static void ss_jitter(SenderStats &S, u64 ets, i64 t) {
  if (S.lastJitterExtTimestamp == ets) return;
  const i64 since = i64(u64(t) - u64(S.firstTime));
  const u64 rtp = u64(i64(u64(since) * u64(i64(S.clockRate))) / 1000000000LL);
  const u64 transit = rtp - ets;
  if (S.lastTransit != 0) {
    i64 d = i64(transit - S.lastTransit);
    if (d < 0) d = i64(0 - u64(d));
    S.jitter += (double(d) - S.jitter) / 16;
    if (S.jitter > S.maxJitter) S.maxJitter = S.jitter;
  }
  S.lastTransit = transit;
  S.lastJitterExtTimestamp = ets;
}
static void ss_update(SenderStats &S, u32 *ring, u32 *gap, i64 t, u64 esn, u64 ets, bool marker, u32 hdr, u32 pay,
                      u32 pad) {
  constexpr u64 kSnMask = kSnInfoSize - 1;
  if (!S.initialized) {
    if (pay == 0) return;
    S.initialized = 1;
    S.firstTime = t;
    S.highestTime = t;
    S.extStartSN = esn;
    S.extHighestSN = esn - 1;
    S.extStartTS = ets;
    S.extHighestTS = ets;
  }
  const u64 pkt = u64(hdr + pay + pad);
  const u32 info = u32(u16(pkt)) | (u32(u8(hdr)) << 16) | ((marker ? kInfoMarker : 0u) | (pay == 0 ? kInfoPadding : 0u))
                                                              << 24;
  bool dup = false;
  const i64 g = i64(esn - S.extHighestSN);
  if (g <= 0) {
    if (pay == 0 && esn < S.extStartSN) return;
    if (esn < S.extStartSN) {
      S.packetsLost += S.extStartSN - esn;
      S.extStartSN = esn;
    }
    if (g != 0) S.packetsOutOfOrder++;
    const i64 off = i64(S.extHighestSN - esn);
    const int slot = (off >= kSnInfoSize || off < 0) ? -1 : int(esn & kSnMask);
    if (!(slot >= 0 && (ring[slot] & 0xffffu) == 0)) {
      S.bytesDuplicate += pkt;
      S.headerBytesDuplicate += hdr;
      S.packetsDuplicate++;
      dup = true;
    } else {
      S.packetsLost--;
      ring[slot] = info | (kInfoOOO << 24);
    }
  } else {
    ss_gap(gap, g);
    const u64 nclr = u64(g - 1) < u64(kSnInfoSize) ? u64(g - 1) : u64(kSnInfoSize);
    for (u64 i = 0; i < nclr; i++) ring[(S.extHighestSN + 1 + i) & kSnMask] = 0;
    S.packetsLost += u64(g - 1);
    ring[esn & kSnMask] = info;
    S.extHighestSN = esn;
  }
  if (ets < S.extStartTS) S.extStartTS = ets;
  if (ets > S.extHighestTS) {
    if (pay > 0) S.highestTime = t;
    S.extHighestTS = ets;
  }
  if (!dup) {
    if (pay == 0) {
      S.packetsPadding++;
      S.bytesPadding += pkt;
      S.headerBytesPadding += hdr;
    } else {
      S.bytes += pkt;
      S.headerBytes += hdr;
      if (marker) S.frames++;
      ss_jitter(S, ets, t);
    }
  }
}

// ---- fixtures ---------------------------------------------------------------
struct Dt {
  SenderStats S;
  SenderRtcp R;
  std::vector<u32> ring, gap;
  Dt() : ring(kSnInfoSize, 0), gap(kGapWords, 0) {
    std::memset(&S, 0, sizeof(S));
    std::memset(&R, 0, sizeof(R));
  }
};
static const i64 T0 = 1700000000LL * 1000000000LL;
static const i64 SEC = 1000000000LL;

static u64 dbits(double d) {
  u64 b;
  std::memcpy(&b, &d, 8);
  return b;
}

// getIntervalStats as the Go loop runs it (rtpstats_sender.go:947-987), one esn at a time
static RtcpIntervalStats brute_interval(const std::vector<u32> &ring, u64 start, u64 endEx, u64 ehsn) {
  RtcpIntervalStats is;
  std::memset(&is, 0, sizeof(is));
  for (u64 esn = start; esn != endEx; esn++) {
    const i64 offset = i64(ehsn - esn);
    if (offset >= kSnInfoSize || offset < 0) {
      is.packetsNotFound++;
      continue;
    }
    const u32 info = ring[esn & (kSnInfoSize - 1)];
    const u32 pktSize = info & 0xffff, hdrSize = (info >> 16) & 0xff, flags = info >> 24;
    if (pktSize == 0) {
      is.packetsLost++;
    } else if (flags & kInfoPadding) {
      is.packetsPadding++;
      is.bytesPadding += pktSize;
      is.headerBytesPadding += hdrSize;
    } else {
      is.packets++;
      is.bytes += pktSize;
      is.headerBytes += hdrSize;
      if (flags & kInfoOOO) is.packetsOutOfOrder++;
    }
    if (flags & kInfoMarker) is.frames++;
  }
  return is;
}
static std::vector<u32> random_ring(u32 seed) {
  std::vector<u32> ring(kSnInfoSize);
  u32 x = seed * 2654435761u + 12345u;
  for (auto &w : ring) {
    x = x * 1664525u + 1013904223u;
    const u32 r = x >> 8;
    const u32 kind = r % 10;  // 2 in 10 lost, 1 padding, 1 out of order
    const u32 size = kind < 2 ? 0u : 40u + (r >> 4) % 1400u;
    const u32 flags = (kind == 2 ? kInfoPadding : 0u) | (kind == 3 ? kInfoOOO : 0u) | ((r >> 20) % 7 == 0 ? kInfoMarker : 0u);
    w = size | ((12u + (r >> 16) % 40u) << 16) | (size ? flags << 24 : 0u);
  }
  return ring;
}
static void interval_case(u64 len) {
  const std::vector<u32> ring = random_ring(u32(len));
  const u64 ehsn = 200000 + 37;  // (not 64-aligned; the longer intervals wrap slot 4095)
  // the interval ends at, ahead of and behind the highest sequence number; and starts at 1
  const i64 ends[] = {1, 6, -10, -4090, -5000, 3000};
  for (i64 de : ends) {
    const u64 endEx = u64(i64(ehsn) + de);
    const u64 start = endEx - len;
    const RtcpIntervalStats a = interval_stats(ring.data(), start, endEx, ehsn), b = brute_interval(ring, start, endEx, ehsn);
    CHECK(std::memcmp(&a, &b, sizeof(a)) == 0);
    CHECK(a.packets + a.packetsPadding + a.packetsLost + a.packetsNotFound == len);
    const IntervalPlan p = interval_plan(start, endEx, ehsn);
    CHECK(p.count <= u32(kSnInfoSize));
  }
}

// ---- cases --------------------------------------------------------------------
static void ntp_zero() { CHECK(ntp_from_unix(0) == (2208988800ull << 32)); }
static void ntp_half() { CHECK(ntp_from_unix(500000000) == ((2208988800ull << 32) | 0x80000000ull)); }
static void ntp_round_up() {
  // 1 ns: 2^32 / 1e9 = 4.29..., remainder below half: 4.  2 ns: 8.58...: rounds up to 9.
  CHECK((ntp_from_unix(1) & 0xffffffffull) == 4);
  CHECK((ntp_from_unix(2) & 0xffffffffull) == 9);
}
static void ntp_round_trip() {
  const i64 ts[] = {0, 1, 2, 999999999, T0, T0 + 123456789, 1700000000123456789LL, 2085978495LL * SEC + 999999999};  // (up to the end of NTP era 0)
  for (i64 t : ts) CHECK(ntp_to_unix(ntp_from_unix(t)) == t);
}
static RrIn rr_of(u32 lsn, u32 lost, u32 jitter, u32 lsr, u32 dlsr) { return RrIn{lsn, lost, jitter, lsr, dlsr}; }
static void rtt_no_lsr() {
  u32 rtt = 7;
  CHECK(!rtt_ms(rr_of(0, 0, 0, 0, 0), ntp_from_unix(T0), T0, T0 + SEC, rtt) && rtt == 0);
}
static void rtt_wrong_lsr() {
  const u64 ntp = ntp_from_unix(T0);
  u32 rtt = 7;
  CHECK(!rtt_ms(rr_of(0, 0, 0, u32(ntp >> 16) + 1, 0), ntp, T0, T0 + SEC, rtt) && rtt == 0);
}
static void rtt_before() {  // DLSR 2 s, 1.5 s elapsed
  const u64 ntp = ntp_from_unix(T0);
  u32 rtt = 7;
  CHECK(!rtt_ms(rr_of(0, 0, 0, u32(ntp >> 16), 0x20000), ntp, T0, T0 + SEC + SEC / 2, rtt) && rtt == 0);
}
static void rtt_value() {
  const u64 ntp = ntp_from_unix(T0);
  u32 rtt = 0;
  // 1.5 s elapsed, DLSR 1 s: 0.5 s = 32768 / 65536 -> 500 ms
  CHECK(rtt_ms(rr_of(0, 0, 0, u32(ntp >> 16), 0x10000), ntp, T0, T0 + SEC + SEC / 2, rtt) && rtt == 500);
  // 0.1 s elapsed, DLSR 0: frac = round(0.1 * 2^32) = 0x1999999A, >> 16 = 6553 -> 99.99 ms -> 100
  CHECK(rtt_ms(rr_of(0, 0, 0, u32(ntp >> 16), 0), ntp, T0, T0 + SEC / 10, rtt) && rtt == 100);
  // lastSRNTP 0 skips the LSR comparison; the NTP epoch itself is then before any LSR
  CHECK(!rtt_ms(rr_of(0, 0, 0, u32(ntp >> 16), 0), 0, T0, T0, rtt) && rtt == 0);
}
static Dt started(u64 startSN, u64 highSN) {
  Dt d;
  d.S.initialized = 1;
  d.S.clockRate = 90000;
  d.S.extStartSN = startSN;
  d.S.extHighestSN = highSN;
  d.S.firstTime = T0;
  d.S.highestTime = T0 + SEC;
  d.S.extStartTS = 1000;
  d.S.extHighestTS = 91000;
  return d;
}
static void rr_sn_wrap() {
  Dt d = started(100, 0x100000005ull);
  d.R.lastRRTime = T0;
  d.R.lastRRLastSequenceNumber = 0xFFFFFFF0u;
  d.R.extHighestSNFromRR = 0xFFFFFFF0ull;
  d.R.snap.extLastRRSN = 0xFFFFFFF0ull;
  u32 rtt;
  const u32 fl = update_from_receiver_report(d.R, d.S, d.ring.data(), rr_of(5, 0, 0, 0, 0), T0 + SEC, rtt);
  CHECK(!(fl & LKF_FB_IGNORED));
  CHECK(d.R.extHighestSNFromRR == 0x100000005ull);
  CHECK(d.R.snap.extLastRRSN == 0x100000005ull);
  CHECK(d.R.snap.intervalStats.packetsLost == 21);  // 0xFFFFFFF1 .. 0x100000005, an empty ring
  CHECK(d.R.lastRRTime == T0 + SEC && d.R.lastRRLastSequenceNumber == 5);
}
static void rr_lost_wrap() {
  Dt d = started(100, 200);
  d.R.lastRRTime = T0;
  d.R.lastRRLastSequenceNumber = 150;
  d.R.extHighestSNFromRR = 150;
  d.R.snap.extLastRRSN = 150;
  d.R.lastRRTotalLost = 0xFFFFFFFEu;
  d.R.packetsLostFromRR = 0x2FFFFFFFEull;
  u32 rtt;
  update_from_receiver_report(d.R, d.S, d.ring.data(), rr_of(160, 1, 0, 0, 0), T0 + SEC, rtt);
  CHECK(d.R.packetsLostFromRR == 0x300000001ull);
  CHECK(d.R.lastRRTotalLost == 1);
}
static void ignored_case(Dt &d, const RrIn &rr) {
  const SenderRtcp before = d.R;
  u32 rtt = 9;
  const u32 fl = update_from_receiver_report(d.R, d.S, d.ring.data(), rr, T0 + SEC, rtt);
  CHECK(fl == LKF_FB_IGNORED && rtt == 0);
  CHECK(std::memcmp(&before, &d.R, sizeof(before)) == 0);
}
static void rr_before_start() {  // extStartSN 70000: base 65536; 65536 + 100 < 70000
  Dt d = started(70000, 70100);
  ignored_case(d, rr_of(100, 0, 0, 0, 0));
}
static void rr_out_of_order() {
  Dt d = started(100, 600);
  d.R.lastRRTime = T0;
  d.R.lastRRLastSequenceNumber = 500;
  d.R.extHighestSNFromRR = 500;
  ignored_case(d, rr_of(400, 0, 0, 0, 0));
}
static void rr_uninitialized() {
  Dt d;
  d.S.clockRate = 90000;
  ignored_case(d, rr_of(400, 0, 0, 0, 0));
}
static void rr_closed() {
  Dt d = started(100, 600);
  d.R.endTime = 1;
  ignored_case(d, rr_of(400, 0, 0, 0, 0));
  update_counts(d.R, 3, 2, 1);  // skipped once endTime is set
  CHECK(d.R.nacks == 0 && d.R.plis == 0 && d.R.firs == 0);
  d.R.endTime = 0;
  update_counts(d.R, 3, 2, 1);
  CHECK(d.R.nacks == 3 && d.R.plis == 2 && d.R.firs == 1);
}
static void interval_0() { interval_case(0); }
static void interval_1() { interval_case(1); }
static void interval_63() { interval_case(63); }
static void interval_64() { interval_case(64); }
static void interval_65() { interval_case(65); }
static void interval_4096() { interval_case(4096); }
static void interval_4097() { interval_case(4097); }
static void interval_70000() {
  interval_case(70000);
  // the zero snapshot's first interval: from esn 1
  const std::vector<u32> ring = random_ring(9);
  const u64 ehsn = 70100;
  const RtcpIntervalStats a = interval_stats(ring.data(), 1, 70001, ehsn), b = brute_interval(ring, 1, 70001, ehsn);
  CHECK(std::memcmp(&a, &b, sizeof(a)) == 0);
  CHECK(a.packetsNotFound == 70100 - 4096);  // esn 1 .. ehsn - 4096
}
static void interval_empty_divergence() {  // endEx < start: about 2^64 iterations in Go, empty here
  const std::vector<u32> ring = random_ring(3);
  const RtcpIntervalStats a = interval_stats(ring.data(), 5000, 4000, 6000);
  RtcpIntervalStats z;
  std::memset(&z, 0, sizeof(z));
  CHECK(std::memcmp(&a, &z, sizeof(a)) == 0);
  const IntervalPlan p = interval_plan(5000, 4000, 6000);
  CHECK(p.count == 0 && p.notFound == 0);
}
static Dt sr_dt() {
  Dt d = started(10, 19);
  d.S.packetsLost = 1;
  d.S.packetsPadding = 2;
  d.S.packetsDuplicate = 3;
  d.S.bytes = 7000;
  d.S.bytesDuplicate = 300;
  d.S.bytesPadding = 200;
  return d;
}
static void sr_first() {
  Dt d = sr_dt();
  lkf_rtcp_sr o;
  sender_report(d.R, d.S, 4, 0, T0 + 2 * SEC, o);
  CHECK(o.flags == LKF_SR_VALID && o.dt == 4);
  CHECK(o.ntp == ntp_from_unix(T0 + 2 * SEC));
  CHECK(o.rtp_ext == 181000 && o.rtp == 181000);  // 91000 + 1 s at 90 kHz
  CHECK(o.packet_count == 12);                    // (10 - 1 - 2) primary + 3 duplicate + 2 padding
  CHECK(o.octet_count == 7500);
  CHECK(d.R.srNewest.valid && d.R.srFirst.valid && std::memcmp(&d.R.srFirst, &d.R.srNewest, sizeof(RtcpSrData)) == 0);
  CHECK(d.R.srNewest.at == T0 + 2 * SEC && d.R.srNewest.rtpExt == 181000);
  // the calculated clock rate wins when it is ahead: 1000 + 100000 * 2 s
  Dt e = sr_dt();
  sender_report(e.R, e.S, 4, 100000, T0 + 2 * SEC, o);
  CHECK(o.rtp_ext == 201000);
  // an uninitialized DownTrack: nil
  Dt u;
  sender_report(u.R, u.S, 4, 0, T0, o);
  CHECK(o.flags == 0 && !u.R.srNewest.valid);
}
static void sr_repair() {
  Dt d = sr_dt();
  d.R.srNewest.valid = d.R.srFirst.valid = 1;
  d.R.srNewest.ntp = ntp_from_unix(T0 + SEC);
  d.R.srNewest.rtpExt = 500000;
  d.R.srNewest.at = T0 + SEC;
  d.R.srFirst = d.R.srNewest;
  lkf_rtcp_sr o;
  sender_report(d.R, d.S, 4, 0, T0 + 2 * SEC, o);
  CHECK(o.flags == (LKF_SR_VALID | LKF_SR_REPAIRED));
  CHECK(o.rtp_ext == 590000);  // 500000 + 1 s at 90 kHz
  CHECK(d.R.outOfOrderSenderReportCount == 1 && d.R.clockSkewCount == 0);
  CHECK(d.R.srFirst.rtpExt == 500000 && d.R.srNewest.rtpExt == 590000);
}
static void sr_clock_skew() {
  Dt d = sr_dt();
  d.R.srNewest.valid = d.R.srFirst.valid = 1;
  d.R.srNewest.ntp = ntp_from_unix(T0 + SEC);
  d.R.srNewest.rtpExt = 1000;  // 180000 ticks in 1 s against 90 kHz
  d.R.srNewest.at = T0 + SEC;
  lkf_rtcp_sr o;
  sender_report(d.R, d.S, 4, 0, T0 + 2 * SEC, o);
  CHECK(o.flags == (LKF_SR_VALID | LKF_SR_CLOCK_SKEW) && d.R.clockSkewCount == 1);
  // within 20 %: no count
  d.R.srNewest.rtpExt = 181000;
  d.R.srNewest.ntp = ntp_from_unix(T0 + 2 * SEC);
  sender_report(d.R, d.S, 4, 0, T0 + 3 * SEC, o);
  CHECK(o.flags == LKF_SR_VALID && d.R.clockSkewCount == 1 && o.rtp_ext == 271000);
}
static void sr_primary_zero() {
  Dt d = sr_dt();
  d.S.packetsLost = 11;  // more lost than expected: primary 0
  CHECK(total_packets_primary(d.S) == 0);
  lkf_rtcp_sr o;
  sender_report(d.R, d.S, 4, 0, T0 + 2 * SEC, o);
  CHECK(o.packet_count == 5);
  d.S.packetsLost = 1;
  d.S.packetsPadding = 10;  // more padding than seen: primary 0
  CHECK(total_packets_primary(d.S) == 0);
  sender_report(d.R, d.S, 4, 0, T0 + 3 * SEC, o);
  CHECK(o.packet_count == 13);
}
static void sr_wire() {
  Dt d = sr_dt();
  lkf_rtcp_sr o;
  sender_report(d.R, d.S, 4, 0, T0 + 2 * SEC, o);
  u8 w[28];
  sender_report_wire(o, 0x11223344u, w);
  const u8 head[8] = {0x80, 200, 0, 6, 0x11, 0x22, 0x33, 0x44};
  CHECK(std::memcmp(w, head, 8) == 0);
  u64 ntp = 0;
  for (int i = 0; i < 8; i++) ntp = (ntp << 8) | w[8 + i];
  CHECK(ntp == o.ntp);
  auto be32 = [&](int off) { return (u32(w[off]) << 24) | (u32(w[off + 1]) << 16) | (u32(w[off + 2]) << 8) | w[off + 3]; };
  CHECK(be32(16) == o.rtp && be32(20) == o.packet_count && be32(24) == o.octet_count);
  std::printf("wire");
  for (int i = 0; i < 28; i++) std::printf(" %02x", w[i]);
  std::printf("\nrecord %" PRIu64 " %u %u %u\n", o.ntp, o.rtp, o.packet_count, o.octet_count);
}
static void delta_nil_before_rr() {
  Dt d = started(100, 200);
  const SenderRtcp before = d.R;
  lkf_rtp_delta_info o;
  delta_info_sender(d.R, d.S, o);
  CHECK(o.valid == 0 && std::memcmp(&before, &d.R, sizeof(before)) == 0);
}
static void delta_expected_zero() {  // the zero snapshot: initialized here, nothing expected yet
  Dt d = started(100, 200);
  d.R.lastRRTime = T0 + SEC;
  lkf_rtp_delta_info o;
  delta_info_sender(d.R, d.S, o);
  CHECK(o.valid == 0);
  CHECK(d.R.snap.isValid == 1 && d.R.snap.extStartSN == 100 && d.R.snap.extLastRRSN == 99);
  CHECK(d.R.snap.startTime == T0 + SEC);
}
static Dt delta_dt() {
  Dt d = started(100, 200);
  d.R.lastRRTime = T0 + 3 * SEC;
  d.R.snap = init_sender_snapshot(T0, 100);
  d.R.snap.extLastRRSN = 109;  // 10 expected
  d.R.snap.intervalStats.packets = 8;
  d.R.snap.intervalStats.bytes = 8000;
  d.R.snap.intervalStats.headerBytes = 96;
  d.R.snap.intervalStats.packetsPadding = 1;
  d.R.snap.intervalStats.bytesPadding = 100;
  d.R.snap.intervalStats.headerBytesPadding = 12;
  d.R.snap.intervalStats.packetsLost = 1;
  d.R.snap.intervalStats.packetsOutOfOrder = 2;
  d.R.snap.intervalStats.frames = 3;
  d.R.snap.maxRtt = 55;
  d.R.snap.maxJitter = 900.0;
  d.R.snap.maxJitterFeed = 450.0;
  d.R.nacks = 4;
  d.R.plis = 2;
  d.R.firs = 1;
  d.R.rtt = 40;
  return d;
}
static void delta_lost_clamped() {
  Dt d = delta_dt();
  d.R.snap.packetsLost = u64(0) - 100;  // now.packetsLost is 0: a delta of 100 against 10 expected
  lkf_rtp_delta_info o;
  delta_info_sender(d.R, d.S, o);
  CHECK(o.valid == 1 && o.packets_lost == 10);
  CHECK(o.packets == 9 && o.packets_padding == 1 && o.bytes == 8000 && o.header_bytes == 96);
  CHECK(o.bytes_padding == 100 && o.header_bytes_padding == 12 && o.packets_out_of_order == 2 && o.frames == 3);
  CHECK(o.start_time_ns == T0 && o.duration_ns == 3 * SEC && o.rtt_max == 55);
  CHECK(o.jitter_max == 450.0 / 90000.0 * 1e6);
  CHECK(o.nacks == 4 && o.plis == 2 && o.firs == 1);
  CHECK(d.R.snap.extStartSN == 110 && d.R.snap.maxRtt == 40 && d.R.snap.intervalStats.packets == 0);
  delta_info_sender(d.R, d.S, o);  // again with no report in between: nothing expected
  CHECK(o.valid == 0);
}
static void delta_negative_clamped() {
  Dt d = delta_dt();
  d.R.snap.packetsLost = 5;       // 0 - 5 < 0
  d.R.snap.packetsLostFeed = 10;  // 3 - 10 < 0
  d.S.packetsLost = 3;
  d.R.snap.maxJitterFeed = 1000.0;  // 900 - 1000 < 0
  lkf_rtp_delta_info o;
  delta_info_sender(d.R, d.S, o);
  CHECK(o.valid == 1 && o.packets_lost == 0 && o.packets_missing == 0 && o.jitter_max == 0.0);
}

struct Case {
  const char *name;
  void (*fn)();
};
static const Case kCases[] = {
    {"ntp_zero", ntp_zero},
    {"ntp_half", ntp_half},
    {"ntp_round_up", ntp_round_up},
    {"ntp_round_trip", ntp_round_trip},
    {"rtt_no_lsr", rtt_no_lsr},
    {"rtt_wrong_lsr", rtt_wrong_lsr},
    {"rtt_before", rtt_before},
    {"rtt_value", rtt_value},
    {"rr_sn_wrap", rr_sn_wrap},
    {"rr_lost_wrap", rr_lost_wrap},
    {"rr_before_start", rr_before_start},
    {"rr_out_of_order", rr_out_of_order},
    {"rr_uninitialized", rr_uninitialized},
    {"rr_closed", rr_closed},
    {"interval_0", interval_0},
    {"interval_1", interval_1},
    {"interval_63", interval_63},
    {"interval_64", interval_64},
    {"interval_65", interval_65},
    {"interval_4096", interval_4096},
    {"interval_4097", interval_4097},
    {"interval_70000", interval_70000},
    {"interval_empty_divergence", interval_empty_divergence},
    {"sr_first", sr_first},
    {"sr_repair", sr_repair},
    {"sr_clock_skew", sr_clock_skew},
    {"sr_primary_zero", sr_primary_zero},
    {"sr_wire", sr_wire},
    {"delta_nil_before_rr", delta_nil_before_rr},
    {"delta_expected_zero", delta_expected_zero},
    {"delta_lost_clamped", delta_lost_clamped},
    {"delta_negative_clamped", delta_negative_clamped},
};

// ---- --replay -------------------------------------------------------------------
static void print_state(const Dt &d) {
  const SenderStats &S = d.S;
  const SenderRtcp &R = d.R;
  const RtcpSnapshot &s = R.snap;
  const RtcpIntervalStats &is = s.intervalStats;
  std::printf("state initialized=%u ext_start_sn=%" PRIu64 " ext_highest_sn=%" PRIu64 " ext_start_ts=%" PRIu64
              " ext_highest_ts=%" PRIu64 " first_time=%" PRId64 " highest_time=%" PRId64 " packets_lost=%" PRIu64
              " packets_padding=%" PRIu64 " packets_duplicate=%" PRIu64 " packets_out_of_order=%" PRIu64
              " bytes=%" PRIu64 " bytes_duplicate=%" PRIu64 " bytes_padding=%" PRIu64 " frames=%u jitter=%" PRIx64,
              S.initialized, S.extStartSN, S.extHighestSN, S.extStartTS, S.extHighestTS, S.firstTime, S.highestTime,
              S.packetsLost, S.packetsPadding, S.packetsDuplicate, S.packetsOutOfOrder, S.bytes, S.bytesDuplicate,
              S.bytesPadding, S.frames, dbits(S.jitter));
  std::printf(" ext_highest_sn_from_rr=%" PRIu64 " last_rr_time=%" PRId64 " packets_lost_from_rr=%" PRIu64
              " jitter_from_rr=%" PRIx64 " max_jitter_from_rr=%" PRIx64 " end_time=%" PRId64
              " last_rr_lsn=%u last_rr_total_lost=%u rtt=%u max_rtt=%u nacks=%u plis=%u firs=%u clock_skew_count=%u"
              " out_of_order_sr_count=%u cache_overflow_count=%u",
              R.extHighestSNFromRR, R.lastRRTime, R.packetsLostFromRR, dbits(R.jitterFromRR),
              dbits(R.maxJitterFromRR), R.endTime, R.lastRRLastSequenceNumber, R.lastRRTotalLost, R.rtt, R.maxRtt,
              R.nacks, R.plis, R.firs, R.clockSkewCount, R.outOfOrderSenderReportCount,
              R.metadataCacheOverflowCount);
  const RtcpSrData *sr[2] = {&R.srFirst, &R.srNewest};
  for (int i = 0; i < 2; i++)
    std::printf(" sr%d_valid=%u sr%d_ntp=%" PRIu64 " sr%d_rtp_ext=%" PRIu64 " sr%d_at=%" PRId64, i, sr[i]->valid, i,
                sr[i]->ntp, i, sr[i]->rtpExt, i, sr[i]->at);
  std::printf(" s_is_valid=%u s_frames=%u s_start_time=%" PRId64 " s_ext_start_sn=%" PRIu64 " s_bytes=%" PRIu64
              " s_header_bytes=%" PRIu64 " s_packets_padding=%" PRIu64 " s_bytes_padding=%" PRIu64
              " s_header_bytes_padding=%" PRIu64 " s_packets_duplicate=%" PRIu64 " s_bytes_duplicate=%" PRIu64
              " s_header_bytes_duplicate=%" PRIu64 " s_packets_out_of_order=%" PRIu64 " s_packets_lost_feed=%" PRIu64
              " s_packets_lost=%" PRIu64 " s_nacks=%u s_plis=%u s_firs=%u s_max_rtt=%u s_max_jitter_feed=%" PRIx64
              " s_max_jitter=%" PRIx64 " s_ext_last_rr_sn=%" PRIu64,
              s.isValid, s.frames, s.startTime, s.extStartSN, s.bytes, s.headerBytes, s.packetsPadding, s.bytesPadding,
              s.headerBytesPadding, s.packetsDuplicate, s.bytesDuplicate, s.headerBytesDuplicate, s.packetsOutOfOrder,
              s.packetsLostFeed, s.packetsLost, s.nacks, s.plis, s.firs, s.maxRtt, dbits(s.maxJitterFeed),
              dbits(s.maxJitter), s.extLastRRSN);
  std::printf(" is_packets=%" PRIu64 " is_bytes=%" PRIu64 " is_header_bytes=%" PRIu64 " is_packets_padding=%" PRIu64
              " is_bytes_padding=%" PRIu64 " is_header_bytes_padding=%" PRIu64 " is_packets_lost=%" PRIu64
              " is_packets_out_of_order=%" PRIu64 " is_packets_not_found=%" PRIu64 " is_frames=%u\n",
              is.packets, is.bytes, is.headerBytes, is.packetsPadding, is.bytesPadding, is.headerBytesPadding,
              is.packetsLost, is.packetsOutOfOrder, is.packetsNotFound, is.frames);
}

static bool set_ss_field(SenderStats &S, const std::string &f, u64 v) {
  struct F {
    const char *name;
    u64 *p;
  };
  const F fs[] = {{"ext_start_sn", &S.extStartSN},   {"ext_highest_sn", &S.extHighestSN},
                  {"ext_start_ts", &S.extStartTS},   {"ext_highest_ts", &S.extHighestTS},
                  {"packets_lost", &S.packetsLost},  {"packets_padding", &S.packetsPadding},
                  {"packets_duplicate", &S.packetsDuplicate}, {"bytes", &S.bytes},
                  {"bytes_duplicate", &S.bytesDuplicate},     {"bytes_padding", &S.bytesPadding}};
  for (const F &x : fs)
    if (f == x.name) {
      *x.p = v;
      return true;
    }
  if (f == "initialized") S.initialized = u32(v);
  else if (f == "first_time") S.firstTime = i64(v);
  else if (f == "highest_time") S.highestTime = i64(v);
  else return false;
  return true;
}

static int replay() {
  Dt d;
  std::string op;
  while (std::cin >> op) {
    if (op == "clock") {
      u32 r;
      std::cin >> r;
      d.S.clockRate = r;
    } else if (op == "ss") {
      std::string f;
      u64 v;
      std::cin >> f >> v;
      if (!set_ss_field(d.S, f, v)) {
        std::fprintf(stderr, "unknown field %s\n", f.c_str());
        return 2;
      }
    } else if (op == "ring") {
      u32 slot, v;
      std::cin >> slot >> v;
      if (slot >= u32(kSnInfoSize)) return 2;
      d.ring[slot] = v;
    } else if (op == "update") {
      i64 t;
      u64 esn, ets;
      u32 marker, hdr, pay, pad;
      std::cin >> t >> esn >> ets >> marker >> hdr >> pay >> pad;
      if (d.R.endTime == 0) ss_update(d.S, d.ring.data(), d.gap.data(), t, esn, ets, marker != 0, hdr, pay, pad);
    } else if (op == "rr") {
      i64 now;
      RrIn rr;
      std::cin >> now >> rr.lastSequenceNumber >> rr.totalLost >> rr.jitter >> rr.lastSenderReport >> rr.delay;
      u32 rtt = 0;
      const u32 fl = update_from_receiver_report(d.R, d.S, d.ring.data(), rr, now, rtt);
      std::printf("rr rtt=%u flags=%u\n", rtt, fl);
    } else if (op == "nack") {
      u32 a, b, c;
      std::cin >> a >> b >> c;
      update_counts(d.R, a, b, c);
    } else if (op == "sr") {
      i64 now;
      u32 ccr;
      std::cin >> now >> ccr;
      lkf_rtcp_sr o;
      sender_report(d.R, d.S, 0, ccr, now, o);
      u8 w[28];
      sender_report_wire(o, 0x11223344u, w);
      std::printf("sr flags=%u ntp=%" PRIu64 " rtp=%u rtp_ext=%" PRIu64 " packet_count=%u octet_count=%u wire=", o.flags,
                  o.ntp, o.rtp, o.rtp_ext, o.packet_count, o.octet_count);
      for (int i = 0; i < 28; i++) std::printf("%02x", w[i]);
      std::printf("\n");
    } else if (op == "delta") {
      lkf_rtp_delta_info o;
      delta_info_sender(d.R, d.S, o);
      std::printf("delta valid=%u start_time=%" PRId64 " duration=%" PRId64 " packets=%u bytes=%" PRIu64
                  " header_bytes=%" PRIu64 " packets_duplicate=%u bytes_duplicate=%" PRIu64
                  " header_bytes_duplicate=%" PRIu64 " packets_padding=%u bytes_padding=%" PRIu64
                  " header_bytes_padding=%" PRIu64 " packets_lost=%u packets_missing=%u packets_out_of_order=%u"
                  " frames=%u rtt_max=%u jitter_max=%" PRIx64 " nacks=%u plis=%u firs=%u\n",
                  o.valid, o.start_time_ns, o.duration_ns, o.packets, o.bytes, o.header_bytes, o.packets_duplicate,
                  o.bytes_duplicate, o.header_bytes_duplicate, o.packets_padding, o.bytes_padding,
                  o.header_bytes_padding, o.packets_lost, o.packets_missing, o.packets_out_of_order, o.frames,
                  o.rtt_max, dbits(o.jitter_max), o.nacks, o.plis, o.firs);
    } else if (op == "stop") {
      d.R.endTime = 1;
    } else if (op == "state") {
      print_state(d);
    } else if (op == "reset") {
      print_state(d);
      d = Dt();
    } else {
      std::fprintf(stderr, "unknown op %s\n", op.c_str());
      return 2;
    }
    if (!std::cin) {
      std::fprintf(stderr, "bad arguments of %s\n", op.c_str());
      return 2;
    }
  }
  print_state(d);
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
