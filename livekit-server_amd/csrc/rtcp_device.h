// rtcp_device.h — the RTCP half of buffer.RTPStatsSender as scalar code for
// the host and the device: UpdateFromReceiverReport, GetRtcpSenderReport,
// DeltaInfoSender and the counter adds, restated statement by statement over
// SenderRtcp (fwd_state.h) and the per-packet SenderStats.  Shared by
// rtcp_kernels.hip (k_rr_update, k_sr_build, k_delta_sender) and the host
// unit program rtcp_unit.cpp.  Go's uint64 / int64 arithmetic wraps: sums and
// products are formed in u64.  No FMA contraction (built with
// -ffp-contract=off): the doubles are bit-exact against the tests' restatement.
//
// time.Now() is the call's now_ns, time.Since(x) is now_ns - x, the zero time
// is 0.  startTime is SenderStats.firstTime (fwd_state.h).
//
// mediatransportutil (v0.0.0-20231213075826-cccbf2b93d3f) is not part of the
// reference tree: ntp_from_unix, ntp_duration and rtt_ms below are the
// definitions of include/lkfwd.h (parity unpinned).
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include <math.h>

#include "../../include/lkfwd.h"
#include "fwd_state.h"

namespace lkf {
namespace rtcp {
using u8 = uint8_t;
using u16 = uint16_t;
using u32 = uint32_t;
using u64 = uint64_t;
using i64 = int64_t;

constexpr u64 kNtpEpochNs = 2208988800ull * 1000000000ull;  // 1900-01-01 -> 1970-01-01
constexpr u32 kNumSequenceNumbers = 65536;                  // cNumSequenceNumbers rtpstats_base.go:32
constexpr u32 kInfoMarker = 1, kInfoPadding = 2, kInfoOOO = 4;  // snInfoFlag rtpstats_sender.go:36-40

// Go's int64 division truncates toward zero, as C++'s does; the product wraps.
__host__ __device__ inline i64 mul_wrap(i64 a, i64 b) { return i64(u64(a) * u64(b)); }

// time.Duration.Seconds
__host__ __device__ inline double dur_seconds(i64 d) {
  const i64 sec = d / 1000000000LL, nsec = d % 1000000000LL;
  return double(sec) + double(nsec) / 1e9;
}

// uint64(float64) as amd64 Go converts it: truncation toward zero through
// int64 below 2^63, through the upper half above; the integer indefinite
// value for NaN and what is out of range.  (A plain C++ cast is undefined for
// negative values, and the device saturates.)
__host__ __device__ inline u64 f64_to_u64(double v) {
  if (!(v > -9223372036854775808.0 && v < 18446744073709551616.0)) return 0x8000000000000000ull;
  if (v < 9223372036854775808.0) return u64(i64(v));
  return u64(i64(v - 9223372036854775808.0)) ^ 0x8000000000000000ull;
}

// mediatransportutil.ToNtpTime of a Unix-ns time (include/lkfwd.h)
__host__ __device__ inline u64 ntp_from_unix(i64 unixNs) {
  const u64 n = u64(unixNs) + kNtpEpochNs;
  const u64 sec = n / 1000000000ull;
  const u64 f = (n - sec * 1000000000ull) << 32;
  u64 frac = f / 1000000000ull;
  if (f % 1000000000ull >= 500000000ull) frac++;
  return (sec << 32) | frac;
}
// NtpTime.Duration: ns since the NTP epoch (NtpTime.Time() = ntpEpoch.Add(Duration()))
__host__ __device__ inline i64 ntp_duration(u64 t) {
  const u64 sec = (t >> 32) * 1000000000ull;
  const u64 frac = (t & 0xFFFFFFFFull) * 1000000000ull;
  u64 nsec = frac >> 32;
  if (u32(frac) >= 0x80000000u) nsec++;
  return i64(sec + nsec);
}
// NtpTime.Time() as Unix ns
__host__ __device__ inline i64 ntp_to_unix(u64 t) { return i64(u64(ntp_duration(t)) - kNtpEpochNs); }

// the rtcp.ReceptionReport fields UpdateFromReceiverReport reads
struct RrIn {
  u32 lastSequenceNumber, totalLost, jitter, lastSenderReport, delay;
};

// mediatransportutil.GetRttMs (include/lkfwd.h); false: an error (no RTT, rtt 0)
__host__ __device__ inline bool rtt_ms(const RrIn &rr, u64 lastSRNTP, i64 lastSentAt, i64 now, u32 &rtt) {
  rtt = 0;
  if (rr.lastSenderReport == 0) return false;                                    // ErrRttNoLastSenderReport
  if (lastSRNTP != 0 && u32(lastSRNTP >> 16) != rr.lastSenderReport) return false;  // ErrRttNotLastSenderReport
  const u64 nowNTP = ntp_from_unix(i64(u64(ntp_to_unix(lastSRNTP)) + (u64(now) - u64(lastSentAt))));
  const u32 now32 = u32(nowNTP >> 16);
  if (now32 < u32(rr.lastSenderReport + rr.delay)) return false;
  rtt = u32(ceil(double(u32(now32 - rr.lastSenderReport - rr.delay)) * 1000.0 / 65536.0));
  return true;
}

// rtpStatsBase.getTotalPacketsPrimary rtpstats_base.go:517-530
__host__ __device__ inline u64 total_packets_primary(const SenderStats &S) {
  const u64 packetsExpected = S.extHighestSN - S.extStartSN + 1;
  if (S.packetsLost > packetsExpected) return 0;  // should not happen
  const u64 packetsSeen = packetsExpected - S.packetsLost;
  if (S.packetsPadding > packetsSeen) return 0;
  return packetsSeen - S.packetsPadding;
}

// UpdateNack / UpdatePli / UpdateFir rtpstats_base.go:315-324, :351-364,
// :407-416: skipped once endTime is set
__host__ __device__ inline void update_counts(SenderRtcp &R, u32 nacks, u32 plis, u32 firs) {
  if (R.endTime != 0) return;
  R.nacks += nacks;
  R.plis += plis;
  R.firs += firs;
}

// ---- getIntervalStats rtpstats_sender.go:947-987 ---------------------------
// The sequence numbers of [start, endEx) that getSnInfoOutOfOrderSlot
// (:889-897) finds are those with 0 <= ehsn - esn < 4096: at most 4096
// consecutive ones, first .. first + count - 1.  Every other one of the
// interval is packetsNotFound, counted in closed form.  Divergence: with
// endEx < start the Go loop runs about 2^64 times; here the interval is empty.
struct IntervalPlan {
  u64 first;
  u32 count;
  u64 notFound;
};
__host__ __device__ inline IntervalPlan interval_plan(u64 start, u64 endEx, u64 ehsn) {
  IntervalPlan p = {start, 0, 0};
  if (endEx <= start) return p;
  const u64 len = endEx - start;
  // esn = start + k has offset o0 - k (mod 2^64); k <= o0 keeps it from wrapping
  // (a wrapped offset is found only from k > o0 + 2^64 - 4096: no such k < len
  // once len <= 2^64 - 4096, which extended sequence numbers never reach)
  const u64 o0 = ehsn - start;
  const u64 kLo = o0 >= u64(kSnInfoSize) ? o0 - u64(kSnInfoSize - 1) : 0;
  const u64 kHi = o0 < len - 1 ? o0 : len - 1;
  if (i64(o0) >= 0 && kLo <= kHi) {  // (offset < 0: ahead of the highest from the start on)
    p.first = start + kLo;
    p.count = u32(kHi - kLo + 1);
  }
  p.notFound = len - p.count;
  return p;
}
// processESN's switch for one found slot, into 32-bit partial counters (a
// lane's share of at most 4096 slots cannot overflow them)
struct IntervalPart {
  u32 packets, bytes, headerBytes, packetsPadding, bytesPadding, headerBytesPadding, packetsLost, packetsOutOfOrder,
      frames;
};
__host__ __device__ inline void interval_classify(IntervalPart &a, u32 info) {
  const u32 pktSize = info & 0xffffu, hdrSize = (info >> 16) & 0xffu, flags = info >> 24;
  // the switch as three exclusive predicates (lanes of a wave take different cases)
  const u32 lost = pktSize == 0 ? 1u : 0u;                             // case snInfo.pktSize == 0
  const u32 padding = (!lost && (flags & kInfoPadding)) ? 1u : 0u;     // case flags & snInfoFlagPadding
  const u32 primary = (!lost && !padding) ? 1u : 0u;                   // default
  a.packetsLost += lost;
  a.packetsPadding += padding;
  a.bytesPadding += padding ? pktSize : 0u;
  a.headerBytesPadding += padding ? hdrSize : 0u;
  a.packets += primary;
  a.bytes += primary ? pktSize : 0u;
  a.headerBytes += primary ? hdrSize : 0u;
  a.packetsOutOfOrder += (primary && (flags & kInfoOOO)) ? 1u : 0u;
  a.frames += (flags & kInfoMarker) ? 1u : 0u;
}
__host__ __device__ inline RtcpIntervalStats interval_total(const IntervalPart &a, u64 notFound) {
  RtcpIntervalStats is;
  is.packets = a.packets;
  is.bytes = a.bytes;
  is.headerBytes = a.headerBytes;
  is.packetsPadding = a.packetsPadding;
  is.bytesPadding = a.bytesPadding;
  is.headerBytesPadding = a.headerBytesPadding;
  is.packetsLost = a.packetsLost;
  is.packetsOutOfOrder = a.packetsOutOfOrder;
  is.packetsNotFound = notFound;
  is.frames = a.frames;
  is.pad = 0;
  return is;
}
// one thread over the whole interval (the host unit; the kernel spreads the
// found slots over a wave)
__host__ __device__ inline RtcpIntervalStats interval_stats(const u32 *ring, u64 start, u64 endEx, u64 ehsn) {
  const IntervalPlan p = interval_plan(start, endEx, ehsn);
  IntervalPart a = {};
  for (u32 k = 0; k < p.count; k++) interval_classify(a, ring[(p.first + k) & u64(kSnInfoSize - 1)]);
  return interval_total(a, p.notFound);
}
// intervalStats.aggregate rtpstats_sender.go:63-78
__host__ __device__ inline void interval_aggregate(RtcpIntervalStats &is, const RtcpIntervalStats &o) {
  is.packets += o.packets;
  is.bytes += o.bytes;
  is.headerBytes += o.headerBytes;
  is.packetsPadding += o.packetsPadding;
  is.bytesPadding += o.bytesPadding;
  is.headerBytesPadding += o.headerBytesPadding;
  is.packetsLost += o.packetsLost;
  is.packetsOutOfOrder += o.packetsOutOfOrder;
  is.frames += o.frames;
  is.packetsNotFound += o.packetsNotFound;
}

// ---- UpdateFromReceiverReport rtpstats_sender.go:441-565 -------------------
// (minus the base-snapshot loop :506-511 and the logging), in two halves
// around getIntervalStats: rr_head up to :525's arguments, rr_tail from the
// aggregate on.  ignored: one of the early returns (:445, :455, :461).
struct RrHead {
  bool ignored, rttChanged;
  u32 rtt;
  u64 start, endEx;  // getIntervalStats(s.extLastRRSN + 1, extReceivedRRSN + 1, r.extHighestSN)
};
__host__ __device__ inline RrHead rr_head(SenderRtcp &R, const SenderStats &S, const RrIn &rr, i64 now) {
  RrHead h = {true, false, 0, 0, 0};
  if (!S.initialized || R.endTime != 0) return h;  // :445
  u64 extHighestSNFromRR = (R.extHighestSNFromRR & 0xFFFFFFFF00000000ull) + u64(rr.lastSequenceNumber);  // :449
  if (R.lastRRTime != 0) {
    if (u32(rr.lastSequenceNumber - R.lastRRLastSequenceNumber) < (1u << 31) &&
        rr.lastSequenceNumber < R.lastRRLastSequenceNumber)
      extHighestSNFromRR += 1ull << 32;
  }
  if (extHighestSNFromRR + (S.extStartSN & 0xFFFFFFFFFFFF0000ull) < S.extStartSN) return h;  // :455 before the start
  if (R.lastRRTime != 0 && R.extHighestSNFromRR > extHighestSNFromRR) return h;              // :461 out of order
  h.ignored = false;
  R.extHighestSNFromRR = extHighestSNFromRR;  // :472

  if (R.srNewest.valid) {  // :474-484
    if (rtt_ms(rr, R.srNewest.ntp, R.srNewest.at, now, h.rtt)) h.rttChanged = h.rtt != R.rtt;
  }

  // :487-491
  u64 packetsLostFromRR = (R.packetsLostFromRR & 0xFFFFFFFF00000000ull) + u64(rr.totalLost);
  if (u32(rr.totalLost - R.lastRRTotalLost) < (1u << 31) && rr.totalLost < R.lastRRTotalLost)
    packetsLostFromRR += 1ull << 32;
  R.packetsLostFromRR = packetsLostFromRR;

  if (h.rttChanged) {  // :493-498
    R.rtt = h.rtt;
    if (h.rtt > R.maxRtt) R.maxRtt = h.rtt;
  }

  R.jitterFromRR = double(rr.jitter);  // :500-503
  if (R.jitterFromRR > R.maxJitterFromRR) R.maxJitterFromRR = R.jitterFromRR;

  // :513-525, the one sender snapshot
  const u64 extReceivedRRSN = R.extHighestSNFromRR + (S.extStartSN & 0xFFFFFFFFFFFF0000ull);
  RtcpSnapshot &s = R.snap;
  if (h.rttChanged && h.rtt > s.maxRtt) s.maxRtt = h.rtt;
  if (R.jitterFromRR > s.maxJitter) s.maxJitter = R.jitterFromRR;
  h.start = s.extLastRRSN + 1;
  h.endEx = extReceivedRRSN + 1;
  return h;
}
__host__ __device__ inline void rr_tail(SenderRtcp &R, const RrHead &h, const RtcpIntervalStats &is, const RrIn &rr,
                                        i64 now) {
  interval_aggregate(R.snap.intervalStats, is);          // :526-527
  if (is.packetsNotFound != 0) R.metadataCacheOverflowCount++;  // :528-558
  R.snap.extLastRRSN = h.endEx - 1;                      // :559
  R.lastRRTime = now;                                    // :562-563
  R.lastRRLastSequenceNumber = rr.lastSequenceNumber;
  R.lastRRTotalLost = rr.totalLost;
}
// result flags of one report (LKF_FB_*)
__host__ __device__ inline u32 rr_flags(const RrHead &h, const RtcpIntervalStats &is) {
  if (h.ignored) return LKF_FB_IGNORED;
  return (h.rttChanged ? u32(LKF_FB_RTT_CHANGED) : 0u) | (is.packetsNotFound ? u32(LKF_FB_CACHE_OVERFLOW) : 0u);
}
// the whole function on one thread
__host__ __device__ inline u32 update_from_receiver_report(SenderRtcp &R, const SenderStats &S, const u32 *ring,
                                                           const RrIn &rr, i64 now, u32 &rtt) {
  const RrHead h = rr_head(R, S, rr, now);
  RtcpIntervalStats is = {};
  if (!h.ignored) {
    is = interval_stats(ring, h.start, h.endEx, S.extHighestSN);
    rr_tail(R, h, is, rr, now);
  }
  rtt = h.rtt;
  return rr_flags(h, is);
}

// ---- GetRtcpSenderReport rtpstats_sender.go:596-714 -------------------------
__host__ __device__ inline void sender_report(SenderRtcp &R, const SenderStats &S, int32_t dt,
                                              u32 calculatedClockRate, i64 nowNs, lkf_rtcp_sr &o) {
  o.dt = dt;
  o.flags = 0;
  o.ntp = o.rtp_ext = 0;
  o.rtp = o.packet_count = o.octet_count = o.reserved = 0;
  if (!S.initialized) return;  // :600

  // :605-612 (now = firstTime + time.Since(firstTime) = now_ns)
  const i64 timeSinceFirst = i64(u64(nowNs) - u64(S.firstTime));
  const i64 now = i64(u64(S.firstTime) + u64(timeSinceFirst));
  const u64 nowNTP = ntp_from_unix(now);
  const i64 timeSinceHighest = i64(u64(now) - u64(S.highestTime));
  u64 nowRTPExt = S.extHighestTS + u64(mul_wrap(timeSinceHighest, i64(S.clockRate)) / 1000000000LL);
  u32 nowRTP = u32(nowRTPExt);

  if (calculatedClockRate != 0) {  // :617-624
    const u64 nowRTPExtUsingRate = S.extStartTS + f64_to_u64(double(calculatedClockRate) * dur_seconds(timeSinceFirst));
    if (nowRTPExtUsingRate > nowRTPExt) {
      nowRTPExt = nowRTPExtUsingRate;
      nowRTP = u32(nowRTPExt);
    }
  }

  if (R.srNewest.valid && nowRTPExt >= R.srNewest.rtpExt) {  // :632-660
    const i64 timeSinceLastReport = i64(u64(ntp_duration(nowNTP)) - u64(ntp_duration(R.srNewest.ntp)));
    const u64 rtpDiffSinceLastReport = nowRTPExt - R.srNewest.rtpExt;
    const double windowClockRate = double(rtpDiffSinceLastReport) / dur_seconds(timeSinceLastReport);
    if (dur_seconds(timeSinceLastReport) > 0.2 &&
        fabs(double(S.clockRate) - windowClockRate) > 0.2 * double(S.clockRate)) {
      R.clockSkewCount++;
      o.flags |= LKF_SR_CLOCK_SKEW;
    }
  }

  if (R.srNewest.valid && nowRTPExt < R.srNewest.rtpExt) {  // :662-700 behind the last report: repair
    R.outOfOrderSenderReportCount++;
    const i64 ntpDiffSinceLast = i64(u64(ntp_duration(nowNTP)) - u64(ntp_duration(R.srNewest.ntp)));
    nowRTPExt = R.srNewest.rtpExt + f64_to_u64(dur_seconds(ntpDiffSinceLast) * double(S.clockRate));
    nowRTP = u32(nowRTPExt);
    o.flags |= LKF_SR_REPAIRED;
  }

  // :702-705
  R.srNewest.ntp = nowNTP;
  R.srNewest.rtpExt = nowRTPExt;
  R.srNewest.at = now;
  R.srNewest.valid = 1;
  R.srNewest.pad = 0;
  if (!R.srFirst.valid) R.srFirst = R.srNewest;

  // :707-713
  o.flags |= LKF_SR_VALID;
  o.ntp = nowNTP;
  o.rtp = nowRTP;
  o.rtp_ext = nowRTPExt;
  o.packet_count = u32(total_packets_primary(S) + S.packetsDuplicate + S.packetsPadding);
  o.octet_count = u32(S.bytes + S.bytesDuplicate + S.bytesPadding);
}
// rtcp.SenderReport.Marshal with no reception reports: 28 bytes, big-endian
// (word i is bytes 4i .. 4i + 3, most significant first; zeros when the report is not VALID)
__host__ __device__ inline u32 sender_report_word(const lkf_rtcp_sr &r, u32 ssrc, int i) {
  if (!(r.flags & LKF_SR_VALID)) return 0;
  switch (i) {
    case 0: return (2u << 30) | (200u << 16) | 6u;  // V=2 P=0 RC=0, PT=200, length 6
    case 1: return ssrc;
    case 2: return u32(r.ntp >> 32);
    case 3: return u32(r.ntp);
    case 4: return r.rtp;
    case 5: return r.packet_count;
    default: return r.octet_count;
  }
}
__host__ __device__ inline void sender_report_wire(const lkf_rtcp_sr &r, u32 ssrc, u8 *w) {
  for (int i = 0; i < 7; i++) {
    const u32 v = sender_report_word(r, ssrc, i);
    w[4 * i + 0] = u8(v >> 24);
    w[4 * i + 1] = u8(v >> 16);
    w[4 * i + 2] = u8(v >> 8);
    w[4 * i + 3] = u8(v);
  }
}

// ---- DeltaInfoSender rtpstats_sender.go:723-808 -----------------------------
// initSenderSnapshot :850-857
__host__ __device__ inline RtcpSnapshot init_sender_snapshot(i64 startTime, u64 extStartSN) {
  RtcpSnapshot s = {};
  s.isValid = 1;
  s.startTime = startTime;
  s.extStartSN = extStartSN;
  s.extLastRRSN = extStartSN - 1;
  return s;
}
// getSenderSnapshot :859-887
__host__ __device__ inline RtcpSnapshot get_sender_snapshot(const SenderRtcp &R, const SenderStats &S, i64 startTime,
                                                            const RtcpSnapshot &s) {
  RtcpSnapshot n = {};
  n.isValid = 1;
  n.startTime = startTime;
  n.extStartSN = s.extLastRRSN + 1;
  n.bytes = s.bytes + s.intervalStats.bytes;
  n.headerBytes = s.headerBytes + s.intervalStats.headerBytes;
  n.packetsPadding = s.packetsPadding + s.intervalStats.packetsPadding;
  n.bytesPadding = s.bytesPadding + s.intervalStats.bytesPadding;
  n.headerBytesPadding = s.headerBytesPadding + s.intervalStats.headerBytesPadding;
  n.packetsDuplicate = S.packetsDuplicate;
  n.bytesDuplicate = S.bytesDuplicate;
  n.headerBytesDuplicate = S.headerBytesDuplicate;
  n.packetsLostFeed = S.packetsLost;
  n.packetsOutOfOrder = s.packetsOutOfOrder + s.intervalStats.packetsOutOfOrder;
  n.frames = s.frames + s.intervalStats.frames;
  n.nacks = R.nacks;
  n.plis = R.plis;
  n.firs = R.firs;
  n.maxRtt = R.rtt;
  n.maxJitterFeed = S.jitter;
  n.maxJitter = R.jitterFromRR;
  n.extLastRRSN = s.extLastRRSN;
  return n;
}
__host__ __device__ inline void delta_info_sender(SenderRtcp &R, const SenderStats &S, lkf_rtp_delta_info &o) {
  lkf_rtp_delta_info z = {};
  o = z;
  if (R.lastRRTime == 0) return;  // :726
  // getAndResetSenderSnapshot :832-848
  if (!S.initialized) return;
  RtcpSnapshot then = R.snap;
  if (!then.isValid) then = init_sender_snapshot(S.firstTime, S.extStartSN);
  const RtcpSnapshot now = get_sender_snapshot(R, S, R.lastRRTime, then);
  R.snap = now;

  const u32 packetsExpected = u32(now.extStartSN - then.extStartSN);  // :738-754
  if (packetsExpected > kNumSequenceNumbers) return;
  if (packetsExpected == 0) return;

  u32 packetsLost = u32(now.packetsLost - then.packetsLost);  // :756-777
  if (int32_t(packetsLost) < 0) packetsLost = 0;
  u32 packetsLostFeed = u32(now.packetsLostFeed - then.packetsLostFeed);
  if (int32_t(packetsLostFeed) < 0) packetsLostFeed = 0;
  if (packetsLost > packetsExpected) packetsLost = packetsExpected;

  double maxJitter = then.maxJitter - then.maxJitterFeed;  // :780-784
  if (maxJitter < 0.0) maxJitter = 0.0;
  const double maxJitterTime = maxJitter / double(S.clockRate) * 1e6;

  o.valid = 1;  // :786-807
  o.start_time_ns = then.startTime;
  o.duration_ns = i64(u64(now.startTime) - u64(then.startTime));
  o.packets = packetsExpected - u32(now.packetsPadding - then.packetsPadding);
  o.bytes = now.bytes - then.bytes;
  o.header_bytes = now.headerBytes - then.headerBytes;
  o.packets_duplicate = u32(now.packetsDuplicate - then.packetsDuplicate);
  o.bytes_duplicate = now.bytesDuplicate - then.bytesDuplicate;
  o.header_bytes_duplicate = now.headerBytesDuplicate - then.headerBytesDuplicate;
  o.packets_padding = u32(now.packetsPadding - then.packetsPadding);
  o.bytes_padding = now.bytesPadding - then.bytesPadding;
  o.header_bytes_padding = now.headerBytesPadding - then.headerBytesPadding;
  o.packets_lost = packetsLost;
  o.packets_missing = packetsLostFeed;
  o.packets_out_of_order = u32(now.packetsOutOfOrder - then.packetsOutOfOrder);
  o.frames = now.frames - then.frames;
  o.rtt_max = then.maxRtt;
  o.jitter_max = maxJitterTime;
  o.nacks = now.nacks - then.nacks;
  o.plis = now.plis - then.plis;
  o.firs = now.firs - then.firs;
}

}  // namespace rtcp
}  // namespace lkf
