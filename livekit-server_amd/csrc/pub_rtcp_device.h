// pub_rtcp_device.h — the RTCP half of buffer.RTPStatsReceiver as scalar code
// for the host and the device: SetRtcpSenderReportData with
// maybeAdjustFirstPacketTime, GetRtcpReceptionReport with getAndResetSnapshot,
// the walk over a publisher's compound packet and the two marshallers
// (rtcp.ReceiverReport with one block, rtcp.TransportLayerNack), restated
// statement by statement over StreamRtcp, StreamHot and DevStream
// (fwd_state.h).  Shared by rtcp_kernels.hip (k_pub_rtcp_check, k_pub_sr_apply,
// k_pub_rr_build, k_nack_wire) and the host unit program pub_rtcp_unit.cpp.
// Go's uint64 / int64 arithmetic wraps: sums and differences are formed in u64.
// No FMA contraction (built with -ffp-contract=off): the doubles are bit-exact
// against the tests' restatement.
//
// time.Now() is the call's now_ns, time.Since(x) is now_ns - x, the zero time
// is 0.  startTime is StreamRtcp.startTime (fwd_state.h says where it comes
// from).  NtpTime.Time() is rtcp_device.h's ntp_to_unix; the two float to
// integer conversions below are include/lkfwd.h's (parity unpinned).
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include <math.h>

#include "../../include/lkfwd.h"
#include "fwd_state.h"
#include "rtcp_device.h"
#include "rtcp_in_device.h"

namespace lkf {
namespace pubrtcp {
using u8 = uint8_t;
using u16 = uint16_t;
using u32 = uint32_t;
using u64 = uint64_t;
using i64 = int64_t;

constexpr i64 kFirstPacketTimeAdjustWindow = 2 * 60 * 1000000000LL;     // rtpstats_base.go:35
constexpr i64 kFirstPacketTimeAdjustThreshold = 5 * 60 * 1000000000LL;  // rtpstats_base.go:36

// int64(float64) as amd64 Go converts it: truncation toward zero, the integer
// indefinite value for NaN and what int64 does not hold.  (A plain C++ cast is
// undefined there, and the device saturates.)
__host__ __device__ inline i64 f64_to_i64(double v) {
  if (!(v >= -9223372036854775808.0 && v < 9223372036854775808.0)) return i64(0x8000000000000000ull);
  return i64(v);
}
// uint32(float64): the low 32 bits of that
__host__ __device__ inline u32 f64_to_u32(double v) { return u32(u64(f64_to_i64(v))); }
// uint8(float32): the low 8 bits of the value truncated to int32
__host__ __device__ inline u32 f32_to_u8(float v) {
  if (!(v >= -2147483648.0f && v < 2147483648.0f)) return 0;  // 0x80000000
  return u32(int32_t(v)) & 0xffu;
}

// the first of the publisher calls that finds the stream initialized keeps
// the first packet's time as startTime
__host__ __device__ inline void capture_start(StreamRtcp &R, const StreamHot &H) {
  if (!R.started && (H.flags & S_INIT)) {
    R.started = 1;
    R.startTime = H.firstTime;
  }
}

// ---- maybeAdjustFirstPacketTime rtpstats_base.go:469-515 --------------------
// -> LKF_SSR_FIRST_TIME_ADJUSTED / LKF_SSR_ADJUST_TOO_BIG / 0; writes H.firstTime
__host__ __device__ inline u32 maybe_adjust_first_packet_time(const StreamRtcp &R, StreamHot &H, u32 clockRate, u32 ts,
                                                              u32 startTS, i64 nowNs) {
  if (i64(u64(nowNs) - u64(R.startTime)) > kFirstPacketTimeAdjustWindow) return 0;  // :470
  const int32_t samplesDiff = int32_t(ts - startTS);                                   // :480
  if (samplesDiff < 0) return 0;  // out-of-order, skip
  const i64 samplesDuration = f64_to_i64(double(samplesDiff) / double(clockRate) * 1e9);  // :486
  const i64 timeSinceFirst = i64(u64(nowNs) - u64(H.firstTime));
  const i64 now = i64(u64(H.firstTime) + u64(timeSinceFirst));
  const i64 firstTime = i64(u64(now) - u64(samplesDuration));
  if (firstTime < H.firstTime) {                                                          // :490
    if (i64(u64(H.firstTime) - u64(firstTime)) > kFirstPacketTimeAdjustThreshold) return LKF_SSR_ADJUST_TOO_BIG;
    H.firstTime = firstTime;
    return LKF_SSR_FIRST_TIME_ADJUSTED;
  }
  return 0;
}

// ---- SetRtcpSenderReportData rtpstats_receiver.go:243-322 -------------------
// srData = {rtp, ntp, At: nowNs}.  o: the result record (ntp / rtp_ext: what
// was stored, 0 when nothing was).
__host__ __device__ inline void set_sender_report(StreamRtcp &R, StreamHot &H, const DevStream &D, u32 rtp, u64 ntp,
                                                  i64 nowNs, lkf_stream_sr_result &o) {
  o.ntp = o.rtp_ext = 0;
  o.flags = o.reserved = 0;
  if (D.closed) {  // Buffer.Close: no reader is left to call it
    o.flags = LKF_SSR_CLOSED;
    return;
  }
  if (!(H.flags & S_INIT)) {  // :247
    o.flags = LKF_SSR_IGNORED_UNINIT;
    return;
  }
  capture_start(R, H);
  if (R.srNewest.valid && R.srNewest.ntp > ntp) {  // :252 anachronous
    o.flags = LKF_SSR_ANACHRONOUS;
    return;
  }

  u64 tsCycles = 0;  // :261-267
  if (R.srNewest.valid) {
    const u32 newestRtp = u32(R.srNewest.rtpExt);
    tsCycles = R.srNewest.rtpExt & 0xFFFFFFFF00000000ull;
    if (u32(rtp - newestRtp) < (1u << 31) && rtp < newestRtp) tsCycles += 1ull << 32;
  }
  const u64 rtpExt = u64(rtp) + tsCycles;  // :270

  o.flags |= maybe_adjust_first_packet_time(R, H, D.clockRate, rtp, H.tsStart, nowNs);  // :272

  if (R.srNewest.valid) {  // :274-298
    const i64 t = rtcp::ntp_to_unix(ntp);
    const double timeSinceLast = rtcp::dur_seconds(i64(u64(t) - u64(rtcp::ntp_to_unix(R.srNewest.ntp))));
    const u64 rtpDiffSinceLast = rtpExt - R.srNewest.rtpExt;
    const double fromLast = double(rtpDiffSinceLast) / timeSinceLast;
    const double timeSinceFirst = rtcp::dur_seconds(i64(u64(t) - u64(rtcp::ntp_to_unix(R.srFirst.ntp))));
    const u64 rtpDiffSinceFirst = rtpExt - R.srFirst.rtpExt;
    const double fromFirst = double(rtpDiffSinceFirst) / timeSinceFirst;
    const double clock = double(D.clockRate);
    if ((timeSinceLast > 0.2 && fabs(clock - fromLast) > 0.2 * clock) ||
        (timeSinceFirst > 0.2 && fabs(clock - fromFirst) > 0.2 * clock)) {
      R.clockSkewCount++;
      o.flags |= LKF_SSR_CLOCK_SKEW;
    }
  }

  if (R.srNewest.valid && rtpExt < R.srNewest.rtpExt) {  // :300-316
    R.outOfOrderSenderReportCount++;
    R.srFirst.valid = 0;
    o.flags |= LKF_SSR_RESET_FIRST;
  }

  R.srNewest.ntp = ntp;  // :318-321
  R.srNewest.rtpExt = rtpExt;
  R.srNewest.at = nowNs;
  R.srNewest.valid = 1;
  R.srNewest.pad = 0;
  if (!R.srFirst.valid) R.srFirst = R.srNewest;
  o.ntp = ntp;
  o.rtp_ext = rtpExt;
}

// ---- GetRtcpReceptionReport rtpstats_receiver.go:340-396 --------------------
// (getAndResetSnapshot rtpstats_base.go:812-828 with the fields this reads)
__host__ __device__ inline void reception_report(StreamRtcp &R, const StreamHot &H, const DevStream &D, int32_t stream,
                                                 u32 proxyFracLost, i64 nowNs, lkf_stream_rr &o) {
  o.stream = stream;
  o.flags = 0;
  o.ssrc = o.fraction_lost = o.total_lost = o.last_sequence_number = o.jitter = o.last_sender_report = o.delay = 0;
  o.reserved = 0;
  if (D.closed) return;
  if (!(H.flags & S_INIT)) return;  // :813
  capture_start(R, H);
  const u64 extStartSN = u64(H.snStart), extHighestSN = H.snExtHighest;
  // then: the kept snapshot, or initSnapshot(startTime, extStartSN)
  const u64 thenExtStartSN = R.snapIsValid ? R.snapExtStartSN : extStartSN;
  const u64 thenPacketsLost = R.snapIsValid ? R.snapPacketsLost : 0;
  // now: getSnapshot(time.Now(), extHighestSN + 1); it replaces the kept one whatever follows
  R.snapIsValid = 1;
  R.snapStartTime = nowNs;
  R.snapExtStartSN = extHighestSN + 1;
  R.snapPacketsLost = H.packetsLost;

  const u64 packetsExpected = R.snapExtStartSN - thenExtStartSN;  // :350
  if (packetsExpected > rtcp::kNumSequenceNumbers) return;
  if (packetsExpected == 0) return;

  u32 packetsLost = u32(R.snapPacketsLost - thenPacketsLost);  // :362-370
  if (int32_t(packetsLost) < 0) packetsLost = 0;
  const float lossRate = float(packetsLost) / float(packetsExpected);
  u32 fracLost = f32_to_u8(lossRate * 256.0f);
  const u32 proxy = proxyFracLost & 0xffu;
  if (proxy > fracLost) fracLost = proxy;

  u64 totalLost = H.packetsLost;  // :372-375
  if (totalLost > 0xffffffull) totalLost = 0xffffffull;

  u32 lastSR = 0, dlsr = 0;  // :377-385
  if (R.srNewest.valid) {
    lastSR = u32(R.srNewest.ntp >> 16);
    if (R.srNewest.at != 0) {
      const i64 delayUS = i64(u64(nowNs) - u64(R.srNewest.at)) / 1000;
      dlsr = u32(u64(rtcp::mul_wrap(delayUS, 65536) / 1000000));
    }
  }

  o.flags = LKF_SRR_VALID;  // :387-395
  o.ssrc = D.ssrc;
  o.fraction_lost = fracLost;
  o.total_lost = u32(totalLost);
  o.last_sequence_number = u32(R.snapExtStartSN);
  o.jitter = f64_to_u32(H.jitter);
  o.last_sender_report = lastSR;
  o.delay = dlsr;
}
// rtcp.ReceiverReport{SSRC, Reports: [1]}.Marshal: 32 bytes, big-endian (word i
// is bytes 4i .. 4i + 3, most significant first; zeros when the record is not VALID)
__host__ __device__ inline u32 receiver_report_word(const lkf_stream_rr &r, int i) {
  if (!(r.flags & LKF_SRR_VALID)) return 0;
  switch (i) {
    case 0: return (2u << 30) | (1u << 24) | (201u << 16) | 7u;  // V=2 P=0 RC=1, PT=201, length 7
    case 1: return r.ssrc;                                        // the sender: the Buffer's mediaSSRC
    case 2: return r.ssrc;                                        // the block's source
    case 3: return ((r.fraction_lost & 0xffu) << 24) | (r.total_lost & 0xffffffu);
    case 4: return r.last_sequence_number;
    case 5: return r.jitter;
    case 6: return r.last_sender_report;
    default: return r.delay;
  }
}
__host__ __device__ inline void put_be32(u8 *w, u32 v) {
  w[0] = u8(v >> 24);
  w[1] = u8(v >> 16);
  w[2] = u8(v >> 8);
  w[3] = u8(v);
}
__host__ __device__ inline void receiver_report_wire(const lkf_stream_rr &r, u8 *w) {
  for (int i = 0; i < 8; i++) put_be32(w + 4 * i, receiver_report_word(r, i));
}

// ---- the publisher's compound packet (mediatrack.go:193-208) ----------------
// rtcp_in_device.h's framing and size checks; the sink sees sr(q) for every
// PT 200 packet (q: its first byte, at least 28 bytes), in packet order.
// -> LKF_RTCP_IN_OK / LKF_RTCP_IN_MALFORMED.  A malformed packet may follow
// packets the sink has seen: the caller voids the whole entry then (the
// kernels walk twice: count and check first, apply behind it).
template <class Sink>
__host__ __device__ inline u32 walk(const u8 *p, u32 len, Sink &s) {
  if (len == 0) return LKF_RTCP_IN_MALFORMED;
  for (u32 at = 0; at < len;) {
    rtcpin::Pkt k;
    if (!rtcpin::frame(p, len, at, k)) return LKF_RTCP_IN_MALFORMED;
    const u8 *q = p + at;
    if (rtcpin::classify(q, k) == rtcpin::K_BAD) return LKF_RTCP_IN_MALFORMED;
    if (k.pt == 200) s.sr(q);
    at += k.size;
  }
  return LKF_RTCP_IN_OK;
}
struct CountSr {
  u32 n = 0;
  __host__ __device__ void sr(const u8 *) { n++; }
};
__host__ __device__ inline u64 sr_ntp(const u8 *q) { return (u64(rtcpin::be32(q + 8)) << 32) | rtcpin::be32(q + 12); }
__host__ __device__ inline u32 sr_rtp(const u8 *q) { return rtcpin::be32(q + 16); }
// the apply pass's sink: SetSenderReportData for each, the entry's result folded
struct ApplySr {
  StreamRtcp &R;
  StreamHot &H;
  const DevStream &D;
  i64 now;
  lkf_stream_rtcp_in_result &res;
  __host__ __device__ void sr(const u8 *q) {
    lkf_stream_sr_result o;
    set_sender_report(R, H, D, sr_rtp(q), sr_ntp(q), now, o);
    res.flags |= o.flags;
    if (o.ntp | o.rtp_ext) {
      res.ntp = o.ntp;
      res.rtp_ext = o.rtp_ext;
    }
  }
};
// one entry, both passes on one thread (the host unit)
__host__ __device__ inline void ingest_entry(StreamRtcp &R, StreamHot &H, const DevStream &D, const u8 *p, u32 len,
                                             i64 now, lkf_stream_rtcp_in_result &res) {
  res.status = LKF_RTCP_IN_MALFORMED;
  res.n_sr = res.flags = res.reserved = 0;
  res.ntp = res.rtp_ext = 0;
  CountSr c;
  if (walk(p, len, c) != LKF_RTCP_IN_OK) return;
  res.status = LKF_RTCP_IN_OK;
  res.n_sr = c.n;
  ApplySr a{R, H, D, now, res};
  walk(p, len, a);
}

// ---- rtcp.TransportLayerNack.Marshal (buffer.go:702-712) ---------------------
// record i of lkf_ingest_nacks's list lies at 12 * i + 4 * pair_off[i]: the
// list's own prefix gives every offset
__host__ __device__ inline u64 nack_wire_off(u32 i, u32 pairOff) { return 12ull * i + 4ull * pairOff; }
__host__ __device__ inline u32 nack_wire_len(u32 nPairs) { return 12 + 4 * nPairs; }
// word w of the packet (w < 3 + nPairs), pairs = the record's pairs
__host__ __device__ inline u32 nack_wire_word(const lkf_rtcp_nack &r, const lkf_nack_pair *pairs, u32 w) {
  switch (w) {
    case 0: return (2u << 30) | (1u << 24) | (205u << 16) | (2u + r.n_pairs);  // V=2 P=0 FMT=1, PT=205
    case 1: return r.media_ssrc;                                               // SenderSSRC
    case 2: return r.media_ssrc;                                               // MediaSSRC
    default: return (u32(pairs[w - 3].packet_id) << 16) | pairs[w - 3].lost_packets;
  }
}

}  // namespace pubrtcp
}  // namespace lkf
