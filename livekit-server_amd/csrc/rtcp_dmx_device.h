// rtcp_dmx_device.h — which DownTracks a subscriber's compound RTCP packet
// addresses, as scalar code for the host and the device: the destination SSRCs
// of every packet (pion/rtcp DestinationSSRC as include/lkfwd.h tabulates it;
// pion/rtcp is not part of the reference tree, parity unpinned)
// and the lookup of an SSRC in a transport's slice of the routing table.
// Framing and size checks are rtcp_in_device.h's frame / classify, so a
// compound routes exactly when lkf_rtcp_ingest would call it OK.  Shared by
// rtcp_kernels.hip (k_rtcp_dmx_mark) and the host unit program rtcp_dmx_unit.cpp.
//
// Every byte the walk reads lies in [p, p + len): a packet is looked at only
// after its framing put its `size` bytes inside the datagram, and every
// destination is read below the size classify demanded of its type (for the
// two types classify does not size, RRR and SLI, below an explicit size >= 12).
#pragma once
#include "rtcp_in_device.h"

namespace lkf {
namespace rtcpdmx {
using rtcpin::be32;
using rtcpin::u32;
using rtcpin::u8;

struct Row {  // one routing-table row; the table is sorted by (transport, ssrc)
  u32 transport, ssrc;
  int32_t dt;
};

// The walk over one datagram (len > 0 bytes at p).  The sink is called once
// per destination SSRC, in packet order, repeats included.
// -> LKF_RTCP_DMX_OK / LKF_RTCP_DMX_MALFORMED.  A malformed packet may follow
// packets whose destinations the sink has seen: the caller voids them then.
template <class Sink>
__host__ __device__ inline u32 walk(const u8 *p, u32 len, Sink &s) {
  if (len == 0) return LKF_RTCP_DMX_MALFORMED;
  for (u32 at = 0; at < len;) {
    rtcpin::Pkt k;
    if (!rtcpin::frame(p, len, at, k)) return LKF_RTCP_DMX_MALFORMED;
    const u8 *q = p + at;
    if (rtcpin::classify(q, k) == rtcpin::K_BAD) return LKF_RTCP_DMX_MALFORMED;
    if (k.pt == 201) {  // size >= 8 + 24 * fmt
      for (u32 r = 0; r < k.fmt; r++) s.dest(be32(q + 8 + 24 * r));
    } else if (k.pt == 200) {  // size >= 28 + 24 * fmt
      for (u32 r = 0; r < k.fmt; r++) s.dest(be32(q + 28 + 24 * r));
      s.dest(be32(q + 4));
    } else if (k.pt == 205) {
      if (k.fmt == 1 || k.fmt == 15) s.dest(be32(q + 8));  // size >= 12 / 20
      else if (k.fmt == 5 && k.size >= 12) s.dest(be32(q + 8));
    } else if (k.pt == 206) {
      if (k.fmt == 1) s.dest(be32(q + 8));  // size >= 12
      else if (k.fmt == 2 && k.size >= 12) s.dest(be32(q + 8));
      else if (k.fmt == 4)  // size = 12 + 8 * entries
        for (u32 o = 12; o + 8 <= k.size; o += 8) s.dest(be32(q + o));
      else if (k.fmt == 15)  // size >= 20 + 4 * numSSRC
        for (u32 i = 0, n = q[16]; i < n; i++) s.dest(be32(q + 20 + 4 * i));
    }
    at += k.size;
  }
  return LKF_RTCP_DMX_OK;
}

// The row of `ssrc` among rows[lo, hi) (one transport's slice, SSRCs ascending
// and distinct); ~0u: none.
__host__ __device__ inline u32 find(const Row *rows, u32 lo, u32 hi, u32 ssrc) {
  while (lo < hi) {
    const u32 mid = lo + (hi - lo) / 2;
    const u32 v = rows[mid].ssrc;
    if (v == ssrc) return mid;
    if (v < ssrc) lo = mid + 1;
    else hi = mid;
  }
  return ~0u;
}

// words of a datagram's bitmap row: one bit per DownTrack of its transport
__host__ __device__ inline u32 row_words(u32 rows) { return (rows + 31) / 32; }

// The mark pass's sink (and the host unit's): sets bit (row - lo) of the
// datagram's private bitmap row `bits` (nwords words, zeroed) for every
// destination found, counts the others.
struct Mark {
  const Row *rows;
  u32 lo, hi;
  u32 *bits;
  u32 nwords;
  u32 dests = 0, unrouted = 0;
  __host__ __device__ void dest(u32 ssrc) {
    dests++;
    const u32 r = find(rows, lo, hi, ssrc);
    const u32 b = r - lo;
    if (r == ~0u || (b >> 5) >= nwords) {
      unrouted++;
      return;
    }
    bits[b >> 5] |= 1u << (b & 31);
  }
};

}  // namespace rtcpdmx
}  // namespace lkf
