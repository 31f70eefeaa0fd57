// srtp_rx_device.h — the receive side's scalar recurrence as code for the host
// and the device: datagram parse, packet-index estimate (RFC 3711 §3.3.1 in the
// u64 form of include/lkfwd.h), the 64-packet replay window and its commit.
// Shared by srtp_kernels.hip (k_srtp_rx_index, k_srtp_unprotect,
// k_srtp_rx_commit) and the host unit program srtp_rx_unit.cpp: both run this
// text.  pion/srtp is not part of the reference tree; the definitions are
// those of include/lkfwd.h (parity unpinned).
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

#include "../../include/lkfwd.h"

namespace lkf {

// One received stream's SRTP state (64 B; lkf_stream_srtp_get copies it out).
struct SrtpRx {
  uint64_t sl;    // ROC << 16 | SEQ of the highest authenticated packet
  uint64_t mask;  // bit k: index sl - k was accepted
  uint32_t started;
  uint32_t tp1;   // transport + 1 (0: unbound, the stream passes through)
  uint64_t accepted, authFail, replay, malformed;
  uint64_t pad;
};
static_assert(sizeof(SrtpRx) == 64, "SrtpRx is 64 B");

namespace srtprx {
using u8 = uint8_t;
using u16 = uint16_t;
using u32 = uint32_t;
using u64 = uint64_t;
using i64 = int64_t;

constexpr u32 kWindow = 64;  // pion/webrtc's default replay protection window

struct Parsed {
  u32 malformed;
  u32 seq;
  u32 h;  // header length: fixed part, CSRCs, extension block
};

// Step 1.  `tag` is the profile's tag length.  A datagram that does not lie
// inside the arena is malformed as well (no byte of it is read).
__host__ __device__ inline Parsed parse(const u8 *arena, u64 arenaLen, u32 off, u32 len, u32 tag) {
  Parsed p{1, 0, 0};
  if (off & 15) return p;
  if (u64(off) + len > arenaLen) return p;
  if (len < 12) return p;
  const u8 *d = arena + off;
  if ((d[0] >> 6) != 2) return p;
  u64 h = 12 + 4 * u64(d[0] & 15);
  if (d[0] & 0x10) {
    if (h + 4 > len) return p;
    h += 4 + 4 * ((u64(d[h + 2]) << 8) | d[h + 3]);
  }
  if (h + tag > len) return p;
  p.malformed = 0;
  p.seq = (u32(d[2]) << 8) | d[3];
  p.h = u32(h);
  return p;
}

// Steps 2 and 3: the packet index v of SEQ against the state, and the replay
// verdict (LKF_SRTP_RX_OK: go on to authenticate with ROC = v >> 16).
__host__ __device__ inline u32 check(const SrtpRx &s, u32 seq, u64 &v) {
  if (!s.started) {
    v = seq;
    return LKF_SRTP_RX_OK;
  }
  const i64 c = i64(s.sl) + i64(int16_t(u16(seq - u32(s.sl & 0xffff))));
  v = c < 0 ? u64(seq) : u64(c);
  if (v <= s.sl) {
    const u64 k = s.sl - v;
    if (k >= kWindow) return LKF_SRTP_RX_REPLAY_OLD;
    if ((s.mask >> k) & 1) return LKF_SRTP_RX_REPLAY_DUP;
  }
  return LKF_SRTP_RX_OK;
}

// Step 5, for an authenticated packet.
__host__ __device__ inline void accept(SrtpRx &s, u64 v) {
  if (!s.started) {
    s.started = 1;
    s.sl = v;
    s.mask = 1;
  } else if (v > s.sl) {
    const u64 sh = v - s.sl;
    s.mask = (sh >= 64 ? 0 : s.mask << sh) | 1;
    s.sl = v;
  } else {
    s.mask |= 1ull << (s.sl - v);
  }
  s.accepted++;
}

__host__ __device__ inline void count_reject(SrtpRx &s, u32 status) {
  if (status == LKF_SRTP_RX_MALFORMED) s.malformed++;
  if (status == LKF_SRTP_RX_REPLAY_OLD || status == LKF_SRTP_RX_REPLAY_DUP) s.replay++;
  if (status == LKF_SRTP_RX_AUTH) s.authFail++;
}

// One datagram of the serial definition, the authentication outcome given:
// `auth` is consulted only when the datagram reaches step 4.
__host__ __device__ inline u32 step(SrtpRx &s, bool malformed, u32 seq, bool auth, u64 &v) {
  v = 0;
  u32 st = LKF_SRTP_RX_MALFORMED;
  if (!malformed) {
    st = check(s, seq, v);
    if (st == LKF_SRTP_RX_OK && !auth) st = LKF_SRTP_RX_AUTH;
  }
  if (st == LKF_SRTP_RX_OK)
    accept(s, v);
  else
    count_reject(s, st);
  return st;
}

}  // namespace srtprx
}  // namespace lkf
