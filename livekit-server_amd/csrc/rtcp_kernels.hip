// rtcp_kernels.hip — the DownTrack RTCP loop on the GPU (gfx950): the RTCP
// half of buffer.RTPStatsSender over the snInfo ring the decide wave keeps.
//
//   k_rr_update     one wave per DownTrack that has entries in the call:
//                   UpdateFromReceiverReport (rtpstats_sender.go:441-565) and
//                   UpdateNack / UpdatePli / UpdateFir for each entry in list
//                   order.  The scalar head runs on wave-uniform state (every
//                   lane the same registers); getIntervalStats (:947-987) is
//                   lane-parallel: packetsNotFound in closed form, the at most
//                   4096 found sequence numbers as consecutive ring slots (one
//                   256-B row per step, the start not aligned, wrapping at slot
//                   4095), nine counters per lane, one cross-lane reduction.
//                   No atomics, no LDS.  Lane 0 writes the state back.
//   k_sr_build      one thread per request: GetRtcpSenderReport (:596-714), the
//                   lkf_rtcp_sr record and, when asked, the 28-byte packet.
//   k_delta_sender  one thread per DownTrack: DeltaInfoSender (:723-808).
//   k_rtcp_in_*     RTCP ingress (lkf_rtcp_ingest), one lane per compound
//                   packet: count what the entry yields, write its fb records,
//                   NACKed sequence numbers and pass-through records at the
//                   scanned offsets (input order, no cursors), fold the
//                   reports' results into the entry's rtt_ms.
//   k_rtcp_dmx_*    RTCP demultiplexing (lkf_rtcp_demux): one lane per datagram
//                   marks the routing-table rows its destination SSRCs find in
//                   a bitmap row of its own; one lane per DownTrack of the
//                   table then counts and, behind a scan, writes its {dt,
//                   dgram} entries in datagram order.  No atomics, no sort.
//   k_pub_*        the publisher RTCP loop (lkf_stream_*): one lane per compound
//                   checks its framing and counts its sender reports; one lane
//                   per stream group then applies the group's sender reports
//                   in list order (SetRtcpSenderReportData, rtpstats_receiver.go
//                   :243-322, with maybeAdjustFirstPacketTime), a byte entry's
//                   as the second walk meets them; one thread per request
//                   builds a reception report (:340-396) and its 32 bytes.
//   k_nack_wire     one lane per record of the last ingest's NACK list: its
//                   rtcp.TransportLayerNack at 12 * i + 4 * pair_off (the
//                   list's own prefix: no scan, no atomics).
//
// The semantics are rtcp_device.h's, rtcp_in_device.h's, rtcp_dmx_device.h's
// and pub_rtcp_device.h's (shared with the host unit programs).
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "rtcp_device.h"
#include "rtcp_in_device.h"
#include "rtcp_dmx_device.h"
#include "pub_rtcp_device.h"

namespace lkf {
namespace {
using u8 = uint8_t;
using u32 = uint32_t;
using u64 = uint64_t;
using i64 = int64_t;
using namespace rtcp;

// Checked builds (-DLKF_CHECKED=1, liblkfwd_checked.so): as forward_kernels.hip's
// CHK, with this file's own record (read_check_rtcp).
#ifndef LKF_CHECKED
#define LKF_CHECKED 0
#endif
enum : u32 {
  CK_RTCP_DT = 101,
  CK_RTCP_SLOT = 102,
  CK_RTCP_ENTRY = 103,
  CK_RTCP_ARENA = 104,
  CK_RTCP_FB = 105,
  CK_RTCP_NACK = 106,
  CK_RTCP_REF = 107,
  CK_DMX_ROW = 108,
  CK_DMX_TRANSPORT = 109,
  CK_DMX_WORD = 110,
  CK_DMX_DGRAM = 111,
  CK_DMX_ENTRY = 112,
  CK_PUB_STREAM = 113,
  CK_NACK_PAIR = 114
};
#if LKF_CHECKED
__device__ unsigned long long g_chk_rtcp[4];
__device__ __noinline__ void chk_fail(u32 site, u64 idx, u64 cap) {
  if (atomicAdd(&g_chk_rtcp[0], 1ull) == 0) {
    g_chk_rtcp[1] = site;
    g_chk_rtcp[2] = idx;
    g_chk_rtcp[3] = cap;
  }
}
#define CHK(cond, site, idx, cap)                   \
  do {                                              \
    if (!(cond)) chk_fail(site, u64(idx), u64(cap)); \
  } while (0)
#else
#define CHK(cond, site, idx, cap) \
  do {                            \
  } while (0)
#endif

__device__ __forceinline__ u32 wave_sum(u32 v) {
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

__global__ __launch_bounds__(64) void k_rr_update(RrUpdateLaunch A) {
  const u32 g = blockIdx.x, lane = threadIdx.x;
  if (g >= A.ngroups) return;
  const u32 b = A.gBegin[g], e = A.gBegin[g + 1];
  CHK(e <= A.n, CK_RTCP_ENTRY, e, A.n);
  if (b >= e || e > A.n) return;
  const u32 d = u32(A.in[b].dt);
  CHK(d < A.ndts, CK_RTCP_DT, d, A.ndts);
  if (d >= A.ndts) return;
  SenderRtcp R = A.rtcp[d];
  const SenderStats S = A.ss[d];
  const u32 *ring = A.ring + size_t(d) * kSnInfoSize;
  for (u32 i = b; i < e; i++) {
    const lkf_rtcp_fb &f = A.in[i];
    u32 rtt = 0, flags = 0;
    if (f.flags & LKF_FB_HAS_RR) {
      const RrIn rr = {f.last_sequence_number, f.total_lost, f.jitter, f.last_sender_report, f.delay};
      const RrHead h = rr_head(R, S, rr, A.now);
      rtt = h.rtt;
      flags = LKF_FB_IGNORED;
      if (!h.ignored) {
        const IntervalPlan p = interval_plan(h.start, h.endEx, S.extHighestSN);
        IntervalPart a = {};
        for (u32 k = lane; k < p.count; k += 64) {
          const u32 slot = u32((p.first + k) & u64(kSnInfoSize - 1));
          CHK(slot < u32(kSnInfoSize), CK_RTCP_SLOT, slot, kSnInfoSize);
          interval_classify(a, ring[slot]);
        }
        a.packets = wave_sum(a.packets);
        a.bytes = wave_sum(a.bytes);
        a.headerBytes = wave_sum(a.headerBytes);
        a.packetsPadding = wave_sum(a.packetsPadding);
        a.bytesPadding = wave_sum(a.bytesPadding);
        a.headerBytesPadding = wave_sum(a.headerBytesPadding);
        a.packetsLost = wave_sum(a.packetsLost);
        a.packetsOutOfOrder = wave_sum(a.packetsOutOfOrder);
        a.frames = wave_sum(a.frames);
        const RtcpIntervalStats is = interval_total(a, p.notFound);
        rr_tail(R, h, is, rr, A.now);
        flags = rr_flags(h, is);
      }
    }
    update_counts(R, f.nacks, f.plis, f.firs);  // after the report, as handleRTCP (downtrack.go:1565-1567)
    if (lane == 0) {
      lkf_rtcp_fb_result r;
      r.rtt_ms = rtt;
      r.flags = flags;
      A.out[i] = r;
    }
  }
  if (lane == 0) {
    // what UpdateFromReceiverReport and the counter adds write: the scalars
    // ahead of srFirst and four members of the snapshot (a whole-struct store
    // would carry the untouched 160 B through scratch)
    SenderRtcp &o = A.rtcp[d];
    o.extHighestSNFromRR = R.extHighestSNFromRR;
    o.lastRRTime = R.lastRRTime;
    o.packetsLostFromRR = R.packetsLostFromRR;
    o.jitterFromRR = R.jitterFromRR;
    o.maxJitterFromRR = R.maxJitterFromRR;
    o.lastRRLastSequenceNumber = R.lastRRLastSequenceNumber;
    o.lastRRTotalLost = R.lastRRTotalLost;
    o.rtt = R.rtt;
    o.maxRtt = R.maxRtt;
    o.nacks = R.nacks;
    o.plis = R.plis;
    o.firs = R.firs;
    o.metadataCacheOverflowCount = R.metadataCacheOverflowCount;
    o.snap.maxRtt = R.snap.maxRtt;
    o.snap.maxJitter = R.snap.maxJitter;
    o.snap.extLastRRSN = R.snap.extLastRRSN;
    o.snap.intervalStats = R.snap.intervalStats;
  }
}

__global__ void k_sr_build(SrBuildLaunch A) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  const lkf_rtcp_sr_req q = A.req[i];
  const u32 d = u32(q.dt);
  CHK(d < A.ndts, CK_RTCP_DT, d, A.ndts);
  if (d >= A.ndts) return;
  SenderRtcp R = A.rtcp[d];
  const SenderStats S = A.ss[d];
  lkf_rtcp_sr o;
  sender_report(R, S, q.dt, q.calculated_clock_rate, A.now, o);
  if (o.flags & LKF_SR_VALID) A.rtcp[d] = R;
  A.out[i] = o;
  if (A.wire) {  // 28 B per request: 4-B aligned, big-endian words
    const u32 ssrc = A.dts[d].ssrc;
    u32 *w = reinterpret_cast<u32 *>(A.wire + size_t(i) * 28);
    for (int k = 0; k < 7; k++) w[k] = __builtin_bswap32(sender_report_word(o, ssrc, k));
  }
}

__global__ void k_delta_sender(DeltaSenderLaunch A) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  const u32 d = u32(A.dts[i]);
  CHK(d < A.ndts, CK_RTCP_DT, d, A.ndts);
  if (d >= A.ndts) return;
  SenderRtcp R = A.rtcp[d];
  const SenderStats S = A.ss[d];
  lkf_rtp_delta_info o;
  delta_info_sender(R, S, o);
  A.rtcp[d].snap = R.snap;
  A.out[i] = o;
}

// ---- RTCP ingress (lkf_rtcp_ingest): rtcp_in_device.h's walk, one lane per entry
__global__ void k_rtcp_in_count(RtcpInLaunch A) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  const lkf_rtcp_raw r = A.in[i];
  const u32 d = u32(r.dt);
  CHK(d < A.ndts, CK_RTCP_DT, d, A.ndts);
  CHK(u64(r.off) + r.len <= A.arenaLen, CK_RTCP_ARENA, u64(r.off) + r.len, A.arenaLen);
  lkf_rtcp_in_result o = {};
  o.status = LKF_RTCP_IN_MALFORMED;
  o.pli_layer = -1;
  if (d < A.ndts && u64(r.off) + r.len <= A.arenaLen) {
    rtcpin::Counts c;
    if (rtcpin::walk(A.arena + r.off, r.len, A.dts[d].ssrc, c) == LKF_RTCP_IN_OK) {
      o.status = LKF_RTCP_IN_OK;
      o.fb_count = c.reports ? c.reports : 1;
      o.reports = c.reports;
      o.nacks = c.nacks;
      o.plis = c.plis;
      o.firs = c.firs;
      o.ref_count = c.refs;
    }
  }
  A.res[i] = o;
  A.fbCnt[i] = o.fb_count;
  A.nackCnt[i] = o.nacks;
  A.refCnt[i] = o.ref_count;
}

// the write pass's sink: each list's cursor and end (the entry's share, from the scans)
struct RtcpInWriter {
  lkf_rtcp_fb *fb, *fbEnd;
  lkf_nack *nk, *nkEnd;
  lkf_rtcp_ref *rf, *rfEnd;
  int32_t dt;
  u32 entry, off;
  __device__ void report(const u8 *b) {
    if (fb >= fbEnd) return;
    lkf_rtcp_fb f = {};
    f.dt = dt;
    f.flags = LKF_FB_HAS_RR;
    rtcpin::read_report(b, f);
    *fb++ = f;
  }
  __device__ void pair(u32 pid, u32 blp) {
    rtcpin::pair_expand(pid, blp, [&](uint16_t sn) {
      if (nk >= nkEnd) return;
      lkf_nack x;
      x.dt = dt;
      x.sn = sn;
      x.reserved = 0;
      *nk++ = x;
    });
  }
  __device__ void pli() {}
  __device__ void fir() {}
  __device__ void ref(u32 kind, u32 at, u32 size) {
    if (rf >= rfEnd) return;
    lkf_rtcp_ref x;
    x.entry = entry;
    x.kind = kind;
    x.off = off + at;
    x.len = size;
    *rf++ = x;
  }
};

__global__ void k_rtcp_in_write(RtcpInLaunch A) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= A.ngroups)  // the fb list's DownTrack group bounds
    A.fbG[i] = i < A.ngroups ? u32(A.fbOff[A.gEntry[i]]) : u32(A.totals[0]);
  if (i >= A.n) return;
  const lkf_rtcp_raw r = A.in[i];
  const u32 d = u32(r.dt);
  const u64 f0 = A.fbOff[i], n0 = A.nackOff[i], r0 = A.refOff[i];
  lkf_rtcp_in_result &o = A.res[i];
  const u32 fbc = o.fb_count, reports = o.reports, nacks = o.nacks, plis = o.plis, firs = o.firs, refc = o.ref_count;
  o.fb_first = u32(f0);
  o.nack_first = u32(n0);
  o.ref_first = u32(r0);
  if (o.status != LKF_RTCP_IN_OK || d >= A.ndts) return;
  CHK(f0 + fbc <= A.fbCap, CK_RTCP_FB, f0 + fbc, A.fbCap);
  CHK(n0 + nacks <= A.nackCap, CK_RTCP_NACK, n0 + nacks, A.nackCap);
  CHK(r0 + refc <= A.refCap, CK_RTCP_REF, r0 + refc, A.refCap);
  if (f0 + fbc > A.fbCap || n0 + nacks > A.nackCap || r0 + refc > A.refCap) return;
  if (plis + firs) {  // sendPliOnce: CheckSync's layer, the request spatial layer
    const int32_t req = A.hot[d].reqS;
    o.pli_layer = req >= 0 ? req : -1;
  }
  lkf_rtcp_fb *fb = A.fb + f0;
  if (!reports) {
    lkf_rtcp_fb f = {};
    f.dt = r.dt;
    *fb = f;
  }
  RtcpInWriter w;
  w.fb = fb, w.fbEnd = fb + reports;
  w.nk = A.nacks + n0, w.nkEnd = w.nk + nacks;
  w.rf = A.refs + r0, w.rfEnd = w.rf + refc;
  w.dt = r.dt, w.entry = i, w.off = r.off;
  rtcpin::walk(A.arena + r.off, r.len, A.dts[d].ssrc, w);
  lkf_rtcp_fb &last = fb[fbc - 1];  // the counts ride on the entry's last record
  last.nacks = nacks;
  last.plis = plis;
  last.firs = firs;
}

__global__ void k_rtcp_in_fold(RtcpInLaunch A) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  const u32 b = A.res[i].fb_first, c = A.res[i].fb_count;
  u32 rtt = 0;
  if (u64(b) + c <= A.fbCap)
    for (u32 k = b; k < b + c; k++)
      if (A.fbOut[k].flags & LKF_FB_RTT_CHANGED) rtt = A.fbOut[k].rtt_ms;  // rttToReport (downtrack.go:1529-1531)
  A.res[i].rtt_ms = rtt;
}

// ---- RTCP demultiplexing (lkf_rtcp_demux): rtcp_dmx_device.h's walk and lookup
static_assert(sizeof(RtcpDmxRow) == sizeof(rtcpdmx::Row) && sizeof(RtcpDmxRow) == 12, "routing-table row");

__global__ void k_rtcp_dmx_mark(RtcpDmxLaunch A) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  const lkf_srtcp_raw r = A.in[i];
  const u32 len = A.rx ? A.rx[i].len : r.len;
  lkf_rtcp_dmx_result o = {};
  o.status = LKF_RTCP_DMX_EMPTY;
  if (len) {
    o.status = LKF_RTCP_DMX_MALFORMED;
    const u32 t = u32(r.transport);
    const u32 w0 = A.bmOff[i], w1 = A.bmOff[i + 1];
    CHK(t < A.ntransports, CK_DMX_TRANSPORT, t, A.ntransports);
    CHK(u64(r.off) + len <= A.arenaLen, CK_RTCP_ARENA, u64(r.off) + len, A.arenaLen);
    CHK(w0 <= w1 && w1 <= A.bmWords, CK_DMX_WORD, w1, A.bmWords);
    if (t < A.ntransports && u64(r.off) + len <= A.arenaLen && w0 <= w1 && w1 <= A.bmWords) {
      const u32 lo = A.tFirst[t], hi = A.tFirst[t + 1];
      CHK(lo <= hi && hi <= A.nrows, CK_DMX_ROW, hi, A.nrows);
      if (lo <= hi && hi <= A.nrows) {
        CHK(w1 - w0 == rtcpdmx::row_words(hi - lo), CK_DMX_WORD, w1 - w0, rtcpdmx::row_words(hi - lo));
        u32 *bits = A.bits + w0;
        rtcpdmx::Mark m{reinterpret_cast<const rtcpdmx::Row *>(A.rows), lo, hi, bits, w1 - w0};
        if (rtcpdmx::walk(A.arena + r.off, len, m) == LKF_RTCP_DMX_OK) {
          o.status = LKF_RTCP_DMX_OK;
          o.dests = m.dests;
          o.unrouted = m.unrouted;
          for (u32 w = 0; w < w1 - w0; w++) o.entries += u32(__popc(bits[w]));
        } else {  // a malformed packet behind marked ones: the datagram routes to nobody
          for (u32 w = 0; w < w1 - w0; w++) bits[w] = 0;
        }
      }
    }
  }
  A.res[i] = o;
}

// position k of the ascending-DownTrack order: its row's datagrams, in call order
template <bool Write>
__device__ __forceinline__ void dmx_gather(const RtcpDmxLaunch &A, u32 k) {
  const u32 r = A.byDt[k];
  CHK(r < A.nrows, CK_DMX_ROW, r, A.nrows);
  u32 c = 0;
  if (r < A.nrows) {
    const RtcpDmxRow row = A.rows[r];
    const u32 t = row.transport;
    CHK(t < A.ntransports, CK_DMX_TRANSPORT, t, A.ntransports);
    if (t < A.ntransports) {
      const u32 lo = A.tFirst[t], j0 = A.tdFirst[t], j1 = A.tdFirst[t + 1];
      CHK(lo <= r, CK_DMX_ROW, lo, r);
      CHK(j0 <= j1 && j1 <= A.n, CK_DMX_DGRAM, j1, A.n);
      if (lo <= r && j0 <= j1 && j1 <= A.n) {
        const u32 bit = r - lo;
        const u64 o = Write ? A.off[k] : 0;
        for (u32 j = j0; j < j1; j++) {
          const u32 i = A.tdList[j];
          CHK(i < A.n, CK_DMX_DGRAM, i, A.n);
          if (i >= A.n) continue;
          const u64 w = u64(A.bmOff[i]) + (bit >> 5);
          CHK(w < A.bmOff[i + 1] && w < A.bmWords, CK_DMX_WORD, w, A.bmWords);
          if (w >= A.bmOff[i + 1] || w >= A.bmWords) continue;
          if (!((A.bits[w] >> (bit & 31)) & 1)) continue;
          if (Write) {
            CHK(o + c < A.entryCap, CK_DMX_ENTRY, o + c, A.entryCap);
            if (o + c < A.entryCap) {
              lkf_rtcp_entry x;
              x.dt = row.dt;
              x.dgram = i;
              A.entries[o + c] = x;
            }
          }
          c++;
        }
      }
    }
  }
  if (!Write) A.cnt[k] = c;
}

__global__ void k_rtcp_dmx_count(RtcpDmxLaunch A) {
  const u32 k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < A.nrows) dmx_gather<false>(A, k);
}

__global__ void k_rtcp_dmx_write(RtcpDmxLaunch A) {
  const u32 k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < A.nrows) dmx_gather<true>(A, k);
}

// ---- the publisher RTCP loop (lkf_stream_*): pub_rtcp_device.h's semantics ----
__global__ void k_pub_rtcp_check(PubSrLaunch A) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  const lkf_stream_rtcp_raw r = A.raw[i];
  CHK(u64(r.off) + r.len <= A.arenaLen, CK_RTCP_ARENA, u64(r.off) + r.len, A.arenaLen);
  lkf_stream_rtcp_in_result o = {};
  o.status = LKF_RTCP_IN_MALFORMED;
  if (u64(r.off) + r.len <= A.arenaLen) {
    pubrtcp::CountSr c;
    if (pubrtcp::walk(A.arena + r.off, r.len, c) == LKF_RTCP_IN_OK) {
      o.status = LKF_RTCP_IN_OK;
      o.n_sr = c.n;
    }
  }
  A.res[i] = o;
}

__global__ void k_pub_sr_apply(PubSrLaunch A) {
  const u32 g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= A.ngroups) return;
  const u32 b = A.gBegin[g], e = A.gBegin[g + 1];
  CHK(e <= A.n, CK_RTCP_ENTRY, e, A.n);
  if (b >= e || e > A.n) return;
  const u32 sid = u32(A.sr ? A.sr[b].stream : A.raw[b].stream);
  CHK(sid < A.nstreams, CK_PUB_STREAM, sid, A.nstreams);
  if (sid >= A.nstreams) return;
  StreamRtcp R = A.rtcp[sid];
  StreamHot &hot = A.hot[sid];
  // the four members the semantics read, and the one they write
  StreamHot H;
  H.flags = hot.flags;
  H.tsStart = hot.tsStart;
  H.firstTime = hot.firstTime;
  const i64 firstTime0 = H.firstTime;
  const DevStream D = A.streams[sid];
  for (u32 i = b; i < e; i++) {
    if (A.sr) {
      lkf_stream_sr_result o;
      pubrtcp::set_sender_report(R, H, D, A.sr[i].rtp, A.sr[i].ntp, A.now, o);
      A.srOut[i] = o;
    } else {
      lkf_stream_rtcp_in_result o = A.res[i];
      const lkf_stream_rtcp_raw r = A.raw[i];
      if (o.status == LKF_RTCP_IN_OK && u64(r.off) + r.len <= A.arenaLen) {
        pubrtcp::ApplySr ap{R, H, D, A.now, o};
        pubrtcp::walk(A.arena + r.off, r.len, ap);
        A.res[i] = o;
      }
    }
  }
  A.rtcp[sid] = R;
  if (H.firstTime != firstTime0) hot.firstTime = H.firstTime;
}

__global__ void k_pub_rr_build(PubRrLaunch A) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  const lkf_stream_rr_req q = A.req[i];
  const u32 sid = u32(q.stream);
  CHK(sid < A.nstreams, CK_PUB_STREAM, sid, A.nstreams);
  if (sid >= A.nstreams) return;
  StreamRtcp R = A.rtcp[sid];
  const StreamHot &hot = A.hot[sid];
  StreamHot H;
  H.flags = hot.flags;
  H.firstTime = hot.firstTime;
  H.snStart = hot.snStart;
  H.snExtHighest = hot.snExtHighest;
  H.packetsLost = hot.packetsLost;
  H.jitter = hot.jitter;
  lkf_stream_rr o;
  pubrtcp::reception_report(R, H, A.streams[sid], q.stream, q.proxy_fraction_lost, A.now, o);
  A.rtcp[sid] = R;
  A.out[i] = o;
  if (A.wire) {  // 32 B per request: 4-B aligned, big-endian words
    u32 *w = reinterpret_cast<u32 *>(A.wire + size_t(i) * 32);
    for (int k = 0; k < 8; k++) w[k] = __builtin_bswap32(pubrtcp::receiver_report_word(o, k));
  }
}

__global__ void k_nack_wire(NackWireLaunch A) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  const lkf_rtcp_nack r = A.recs[i];
  const u64 off = pubrtcp::nack_wire_off(i, r.pair_off);
  const u32 len = pubrtcp::nack_wire_len(r.n_pairs);
  lkf_stream_rtcp_pkt p;
  p.datagram = r.datagram;
  p.stream = r.stream;
  p.off = u32(off);
  p.len = len;
  A.pkts[i] = p;
  CHK(off + len <= A.arenaCap, CK_RTCP_ARENA, off + len, A.arenaCap);
  CHK(u64(r.pair_off) + r.n_pairs <= A.npairs, CK_NACK_PAIR, u64(r.pair_off) + r.n_pairs, A.npairs);
  if (off + len > A.arenaCap || u64(r.pair_off) + r.n_pairs > A.npairs) return;
  u32 *w = reinterpret_cast<u32 *>(A.arena + off);  // (every offset is a multiple of 4)
  const lkf_nack_pair *pairs = A.pairs + r.pair_off;
  for (u32 k = 0; k < 3u + r.n_pairs; k++) w[k] = __builtin_bswap32(pubrtcp::nack_wire_word(r, pairs, k));
}
}  // namespace

hipError_t launch_rr_update(hipStream_t s, const RrUpdateLaunch &a) {
  if (!a.ngroups) return hipSuccess;
  hipLaunchKernelGGL(k_rr_update, dim3(a.ngroups), dim3(64), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_sr_build(hipStream_t s, const SrBuildLaunch &a) {
  if (!a.n) return hipSuccess;
  hipLaunchKernelGGL(k_sr_build, dim3((a.n + 63) / 64), dim3(64), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_delta_sender(hipStream_t s, const DeltaSenderLaunch &a) {
  if (!a.n) return hipSuccess;
  hipLaunchKernelGGL(k_delta_sender, dim3((a.n + 63) / 64), dim3(64), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_rtcp_in_count(hipStream_t s, const RtcpInLaunch &a) {
  if (!a.n) return hipSuccess;
  hipLaunchKernelGGL(k_rtcp_in_count, dim3((a.n + 63) / 64), dim3(64), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_rtcp_in_write(hipStream_t s, const RtcpInLaunch &a) {
  if (!a.n) return hipSuccess;
  hipLaunchKernelGGL(k_rtcp_in_write, dim3((a.n + 64) / 64), dim3(64), 0, s, a);  // n + 1 lanes: the group bounds
  return hipGetLastError();
}

hipError_t launch_rtcp_in_fold(hipStream_t s, const RtcpInLaunch &a) {
  if (!a.n) return hipSuccess;
  hipLaunchKernelGGL(k_rtcp_in_fold, dim3((a.n + 63) / 64), dim3(64), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_rtcp_dmx_mark(hipStream_t s, const RtcpDmxLaunch &a) {
  if (!a.n) return hipSuccess;
  hipLaunchKernelGGL(k_rtcp_dmx_mark, dim3((a.n + 63) / 64), dim3(64), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_rtcp_dmx_count(hipStream_t s, const RtcpDmxLaunch &a) {
  if (!a.nrows) return hipSuccess;
  hipLaunchKernelGGL(k_rtcp_dmx_count, dim3((a.nrows + 63) / 64), dim3(64), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_rtcp_dmx_write(hipStream_t s, const RtcpDmxLaunch &a) {
  if (!a.nrows) return hipSuccess;
  hipLaunchKernelGGL(k_rtcp_dmx_write, dim3((a.nrows + 63) / 64), dim3(64), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_pub_rtcp_check(hipStream_t s, const PubSrLaunch &a) {
  if (!a.n || !a.raw) return hipSuccess;
  hipLaunchKernelGGL(k_pub_rtcp_check, dim3((a.n + 63) / 64), dim3(64), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_pub_sr_apply(hipStream_t s, const PubSrLaunch &a) {
  if (!a.ngroups) return hipSuccess;
  hipLaunchKernelGGL(k_pub_sr_apply, dim3((a.ngroups + 63) / 64), dim3(64), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_pub_rr_build(hipStream_t s, const PubRrLaunch &a) {
  if (!a.n) return hipSuccess;
  hipLaunchKernelGGL(k_pub_rr_build, dim3((a.n + 63) / 64), dim3(64), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_nack_wire(hipStream_t s, const NackWireLaunch &a) {
  if (!a.n) return hipSuccess;
  hipLaunchKernelGGL(k_nack_wire, dim3((a.n + 63) / 64), dim3(64), 0, s, a);
  return hipGetLastError();
}

hipError_t read_check_rtcp(unsigned long long out[4], int reset) {
#if LKF_CHECKED
  hipError_t r = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_chk_rtcp), sizeof(unsigned long long) * 4);
  if (r == hipSuccess && reset) {
    unsigned long long z[4] = {};
    r = hipMemcpyToSymbol(HIP_SYMBOL(g_chk_rtcp), z, sizeof(z));
  }
  return r;
#else
  (void)reset;
  for (int i = 0; i < 4; i++) out[i] = 0;
  return hipErrorNotSupported;
#endif
}

}  // namespace lkf
