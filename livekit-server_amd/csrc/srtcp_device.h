// srtcp_device.h — the SRTCP receive side's scalar steps as code for the host
// and the device (include/lkfwd.h "SRTCP"): datagram parse, the per-SSRC slot
// table of a transport, the replay verdict against a slot's explicit 31-bit
// index, and the commit.  Shared by srtp_kernels.hip (k_srtcp_rx_index,
// k_srtcp_unprotect, k_srtcp_rx_commit) and the host unit program
// srtcp_unit.cpp: both run this text.  The kernels keep a transport's table one
// slot per lane and find the slot with a ballot; check, accept and counter_of
// are the same for both forms, find_slot and step are the scalar form.
// pion/srtp is not part of the reference tree; the definitions are those of
// include/lkfwd.h (parity unpinned).
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

#include "../../include/lkfwd.h"

namespace lkf {
namespace srtcp {
using u8 = uint8_t;
using u32 = uint32_t;
using u64 = uint64_t;

constexpr u32 kWindow = 64;  // pion/webrtc's default replay protection window
constexpr u32 kSlots = LKF_SRTCP_SSRCS;

struct Parsed {
  u32 st;  // LKF_SRTCP_RX_OK (go on to step 4), _MALFORMED or _UNENCRYPTED
  u32 ssrc, index;
};

__host__ __device__ inline u32 be32(const u8 *p) {
  return (u32(p[0]) << 24) | (u32(p[1]) << 16) | (u32(p[2]) << 8) | p[3];
}

// Where the E || index word sits: before the tag for AES-CM (tag 10), after it for GCM (tag 16).
__host__ __device__ inline u32 trailer_pos(u32 len, u32 tag) { return tag == 16 ? len - 4 : len - 4 - tag; }

// Steps 1 to 3.  `tag` is the profile's tag length.  A datagram that does not
// lie inside the arena is malformed as well (no byte of it is read).
__host__ __device__ inline Parsed parse(const u8 *arena, u64 arenaLen, u32 off, u32 len, u32 tag) {
  Parsed p{LKF_SRTCP_RX_MALFORMED, 0, 0};
  if (off & 15) return p;
  if (u64(off) + len > arenaLen) return p;
  if (len < 8 + 4 + tag) return p;
  const u8 *d = arena + off;
  if ((d[0] >> 6) != 2) return p;
  const u32 w = be32(d + trailer_pos(len, tag));
  if (!(w >> 31)) {
    p.st = LKF_SRTCP_RX_UNENCRYPTED;
    return p;
  }
  p.st = LKF_SRTCP_RX_OK;
  p.ssrc = be32(d + 4);
  p.index = w & 0x7fffffffu;
  return p;
}

struct Slot {
  u32 inUse, ssrc, latest;
  u64 mask;
};

// Step 4: the verdict before authentication.  found: an in-use slot holds the
// SSRC (latest, mask are its); anyFree: a free slot exists.
__host__ __device__ inline u32 check(bool found, bool anyFree, u32 latest, u64 mask, u32 index) {
  if (!found) return anyFree ? LKF_SRTCP_RX_OK : LKF_SRTCP_RX_NO_SLOT;
  if (index <= latest) {
    const u32 k = latest - index;
    if (k >= kWindow) return LKF_SRTCP_RX_REPLAY_OLD;
    if ((mask >> k) & 1) return LKF_SRTCP_RX_REPLAY_DUP;
  }
  return LKF_SRTCP_RX_OK;
}

// Step 6, for an authenticated packet: `s` is the SSRC's slot, or the lowest free one.
__host__ __device__ inline void accept(Slot &s, bool found, u32 ssrc, u32 index) {
  if (!found) {
    s.inUse = 1;
    s.ssrc = ssrc;
    s.latest = index;
    s.mask = 1;
  } else if (index > s.latest) {
    const u32 sh = index - s.latest;
    s.mask = (sh >= 64 ? 0 : s.mask << sh) | 1;
    s.latest = index;
  } else {
    s.mask |= 1ull << (s.latest - index);
  }
}

// The counter a verdict adds to, as an index into lkf_transport_srtcp's six
// (accepted, auth_failures, replays, malformed, unencrypted, no_slot).
__host__ __device__ inline u32 counter_of(u32 status) {
  switch (status) {
    case LKF_SRTCP_RX_OK: return 0;
    case LKF_SRTCP_RX_AUTH: return 1;
    case LKF_SRTCP_RX_REPLAY_OLD:
    case LKF_SRTCP_RX_REPLAY_DUP: return 2;
    case LKF_SRTCP_RX_MALFORMED: return 3;
    case LKF_SRTCP_RX_UNENCRYPTED: return 4;
    default: return 5;
  }
}
__host__ __device__ inline void count_reject(lkf_transport_srtcp &t, u32 status) {
  const u32 c = counter_of(status);
  if (c == 1) t.auth_failures++;
  if (c == 2) t.replays++;
  if (c == 3) t.malformed++;
  if (c == 4) t.unencrypted++;
  if (c == 5) t.no_slot++;
}

// The in-use slot holding `ssrc`, else kSlots; `free`: the lowest free slot, else kSlots.
__host__ __device__ inline u32 find_slot(const lkf_transport_srtcp &t, u32 ssrc, u32 &free) {
  u32 hit = kSlots;
  free = kSlots;
  for (u32 k = kSlots; k-- > 0;) {
    if (t.in_use[k] && t.ssrc[k] == ssrc) hit = k;
    if (!t.in_use[k]) free = k;
  }
  return hit;
}

// One datagram of the serial definition, the authentication outcome given:
// `auth` is consulted only when the datagram reaches step 5.
__host__ __device__ inline u32 step(lkf_transport_srtcp &t, const Parsed &p, bool auth) {
  u32 st = p.st;
  if (st == LKF_SRTCP_RX_OK) {
    u32 free;
    const u32 hit = find_slot(t, p.ssrc, free);
    const bool found = hit < kSlots;
    const u32 k = found ? hit : free;
    Slot s{0, 0, 0, 0};
    if (k < kSlots) s = Slot{t.in_use[k], t.ssrc[k], t.latest[k], t.mask[k]};
    st = check(found, free < kSlots, s.latest, s.mask, p.index);
    if (st == LKF_SRTCP_RX_OK && !auth) st = LKF_SRTCP_RX_AUTH;
    if (st == LKF_SRTCP_RX_OK) {
      accept(s, found, p.ssrc, p.index);
      t.in_use[k] = s.inUse;
      t.ssrc[k] = s.ssrc;
      t.latest[k] = s.latest;
      t.mask[k] = s.mask;
      t.accepted++;
    }
  }
  if (st != LKF_SRTCP_RX_OK) count_reject(t, st);
  return st;
}

}  // namespace srtcp
}  // namespace lkf
