// rtcp_in_device.h — the parse of one subscriber's compound RTCP packet as
// scalar code for the host and the device: rtcp.Unmarshal and the switch of
// DownTrack.handleRTCP (downtrack.go:1474-1563) as include/lkfwd.h defines them
// (pion/rtcp is not part of the reference tree; parity unpinned).
// The framing walk, the per-type size checks, the NACK pair expansion and the
// big-endian readers, nothing else.  Shared by rtcp_kernels.hip (k_rtcp_in_count,
// k_rtcp_in_write) and the host unit program rtcp_in_unit.cpp.
//
// Every byte the walk reads lies in [p, p + len): a packet is looked at only
// after its framing put its `size` bytes inside the entry, and each type reads
// only below the size its check demanded.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#include "../../include/lkfwd.h"

namespace lkf {
namespace rtcpin {
using u8 = uint8_t;
using u16 = uint16_t;
using u32 = uint32_t;

__host__ __device__ inline u32 be16(const u8 *p) { return (u32(p[0]) << 8) | u32(p[1]); }
__host__ __device__ inline u32 be24(const u8 *p) { return (u32(p[0]) << 16) | (u32(p[1]) << 8) | u32(p[2]); }
__host__ __device__ inline u32 be32(const u8 *p) {
  return (u32(p[0]) << 24) | (u32(p[1]) << 16) | (u32(p[2]) << 8) | u32(p[3]);
}

// what handleRTCP does with a packet; K_BAD: a size check failed (malformed)
enum Kind : u32 { K_SKIP = 0, K_RR, K_NACK, K_TWCC, K_PLI, K_FIR, K_REMB, K_BAD };

struct Pkt {
  u32 pt, fmt;  // packet type, the header's five count / format bits
  u32 size;     // bytes with the header: 4 * (length + 1)
};

// The common header of the packet at p[at ..): false = malformed (fewer than
// four bytes left, version != 2, or a size beyond the bytes left).  The P bit
// is ignored: pad bytes belong to the packet body.
__host__ __device__ inline bool frame(const u8 *p, u32 len, u32 at, Pkt &k) {
  if (len - at < 4) return false;
  const u32 b0 = p[at];
  if ((b0 >> 6) != 2) return false;
  k.fmt = b0 & 31;
  k.pt = p[at + 1];
  k.size = 4 * (be16(p + at + 2) + 1);
  return k.size <= len - at;
}

// The per-type size checks; q = the packet's first byte, k.size bytes readable.
__host__ __device__ inline Kind classify(const u8 *q, const Pkt &k) {
  switch (k.pt) {
    case 201: return k.size >= 8 + 24 * k.fmt ? K_RR : K_BAD;
    case 200: return k.size >= 28 + 24 * k.fmt ? K_SKIP : K_BAD;  // handleRTCP has no case for a sender report
    case 205:
      if (k.fmt == 1) return k.size >= 12 ? K_NACK : K_BAD;
      if (k.fmt == 15) return k.size >= 20 ? K_TWCC : K_BAD;
      return K_SKIP;
    case 206:
      if (k.fmt == 1) return k.size >= 12 ? K_PLI : K_BAD;
      if (k.fmt == 4) return (k.size >= 12 && (k.size - 12) % 8 == 0) ? K_FIR : K_BAD;
      if (k.fmt == 15) {
        if (k.size < 20 || q[12] != 'R' || q[13] != 'E' || q[14] != 'M' || q[15] != 'B') return K_BAD;
        return k.size >= 20 + 4 * u32(q[16]) ? K_REMB : K_BAD;
      }
      return K_SKIP;
    default: return K_SKIP;
  }
}

// rtcp.NackPair.PacketList: the PID, then PID + i + 1 (u16 wrap) for each set
// BLP bit i, ascending
__host__ __device__ inline u32 pair_count(u32 blp) { return 1 + u32(__builtin_popcount(blp & 0xffffu)); }
template <class F>
__host__ __device__ inline void pair_expand(u32 pid, u32 blp, F &&f) {
  f(u16(pid));
  for (u32 i = 0; i < 16; i++)
    if ((blp >> i) & 1) f(u16(pid + i + 1));
}

// one reception report block (24 B at b) into the lkf_rtcp_fb fields
__host__ __device__ inline void read_report(const u8 *b, lkf_rtcp_fb &f) {
  f.fraction_lost = b[4];
  f.total_lost = be24(b + 5);
  f.last_sequence_number = be32(b + 8);
  f.jitter = be32(b + 12);
  f.last_sender_report = be32(b + 16);
  f.delay = be32(b + 20);
}

// The walk over one entry (len bytes at p, a DownTrack whose SSRC is ssrc).
// The sink sees, in packet order:
//   report(b)            a reception report block for ssrc (24 B at b)
//   pair(pid, blp)       one NACK pair
//   pli() / fir()        one PictureLossIndication / FullIntraRequest packet
//   ref(kind, at, size)  a pass-through packet at entry offset `at`
// -> LKF_RTCP_IN_OK / LKF_RTCP_IN_MALFORMED.  A malformed packet may follow
// packets the sink has seen: the caller voids the whole entry then.
template <class Sink>
__host__ __device__ inline u32 walk(const u8 *p, u32 len, u32 ssrc, Sink &s) {
  if (len == 0) return LKF_RTCP_IN_MALFORMED;
  for (u32 at = 0; at < len;) {
    Pkt k;
    if (!frame(p, len, at, k)) return LKF_RTCP_IN_MALFORMED;
    const u8 *q = p + at;
    switch (classify(q, k)) {
      case K_BAD: return LKF_RTCP_IN_MALFORMED;
      case K_RR:
        for (u32 r = 0; r < k.fmt; r++) {
          const u8 *b = q + 8 + 24 * r;
          if (be32(b) == ssrc) s.report(b);
        }
        break;
      case K_NACK:
        for (u32 o = 12; o + 4 <= k.size; o += 4) s.pair(be16(q + o), be16(q + o + 2));
        break;
      case K_TWCC:
        if (be32(q + 8) == ssrc) s.ref(u32(LKF_RTCP_REF_TWCC), at, k.size);
        break;
      case K_PLI: s.pli(); break;
      case K_FIR: s.fir(); break;
      case K_REMB: s.ref(u32(LKF_RTCP_REF_REMB), at, k.size); break;
      default: break;
    }
    at += k.size;
  }
  return LKF_RTCP_IN_OK;
}

// the count pass's sink (and the host unit's): what an entry needs of each list
// (32 bits hold them: len <= LKF_RTCP_MAX_LEN gives at most 17 * len / 4 sequence numbers)
struct Counts {
  u32 reports = 0, nacks = 0, plis = 0, firs = 0, refs = 0;
  __host__ __device__ void report(const u8 *) { reports++; }
  __host__ __device__ void pair(u32, u32 blp) { nacks += pair_count(blp); }
  __host__ __device__ void pli() { plis++; }
  __host__ __device__ void fir() { firs++; }
  __host__ __device__ void ref(u32, u32, u32) { refs++; }
};

}  // namespace rtcpin
}  // namespace lkf
