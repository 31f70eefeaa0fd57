// fps_dd_device.h — the dependency-descriptor frame-rate calculator of a
// received stream (buffer/fps.go:319-570: FrameRateCalculatorDD with
// RecvPacket, calc, SetMaxLayer, close and the reset on a frame number that is
// not continuous) as Buffer.doFpsCalc drives it (buffer.go:191-201, :518-543).
// State and step, host and device, split as fps_device.h splits the PictureID
// calculators: k_ing_fps_dd (ingress_kernels.hip) runs it one wave per enabled
// stream, fps_dd_unit.cpp on the host compiler under the sanitizers,
// tests/fps_dd_lib.PyFpsDD restates the Go with its lists and frame records.
//
// The window.  fnReceived[256] (fps.go:326): slot k is the frame
// uint16(baseFn + k) and holds ts, spatial and temporal (seq and the stored
// frameDiff are never read again).  A wave holds four slots per lane (slot k in
// lane k % 64, word k / 64), so a mask over the window is four 64-bit words.
// The presence set, the rates, firstFrames / secondFrames (slot numbers) and
// the max layer are wave-uniform (Head).  The base frame is slot 0 and keeps
// spatial 0, temporal 0 whatever its packet said (fps.go:376), and it also
// becomes firstFrames and secondFrames of its own layer.
//
// The per-layer chain is a set.  targetFrames[s][t] (fps.go:331) is only ever
// inserted into in sorted position, duplicates skipped (fps.go:435-449), and
// walked front to back (fps.go:477): it is the set of its frame numbers in
// PLAIN uint16 order (`val < dependFrame` is not wrap-aware).
//   INVARIANT: every member lies inside the window.  A dependency is kept only
//   if uint16(dependFrame - secondFrames[s][t].fn) <= 0x8000 (fps.go:431), the
//   second frame is in the window, the packet's frame is at slot 1..255 and a
//   diff on the wire is 1..4096 (12 bits + 1), so a member is in
//   [second.fn, fn), or it is fn itself, pushed when the chain is empty
//   (fps.go:425).  recv() checks it (LKF_FPSDD_ASSERT: the host program aborts;
//   the device drops such a member, which calc() would skip anyway, fps.go:479).
// So a chain is 256 membership bits (12 bits per slot, lane-held), and the walk
// order is slot order rotated to start at slot 65536 - baseFn when that is
// below 256 (the frames past the 16-bit wrap come first in plain order),
// otherwise plain slot order.
//
// calc() (fps.go:454-526), carried over literally where it is odd:
//   - the last decodable frame is the last member, in walk order, before the
//     first member whose slot is empty;
//   - it replaces secondFrames[s][t] only under the plain compare
//     lastFrame.fn > second.fn, otherwise the layer is skipped this round;
//   - frameCount runs over the slots first..last (empty if first > last) and
//     counts frames with spatial == s && temporal <= t;
//   - a rate needs frameCount >= minFrames[t] and the plain compare
//     lastFrame.ts > firstFrame.ts; it is fps::rate_of (two separately rounded
//     binary32 operations);
//   - "a lower temporal of this spatial is calculated and this one was never
//     seen: count it" (fps.go:467) stays, and so does the counter it keys on
//     (rates found in earlier rounds only);
//   - complete when rateCounter == (maxSpatial + 1) * (maxTemporal + 1); then
//     close() clears everything but the rates.
//
// Divergences, both where the reference panics.  minFramesForCalculation has 3
// entries (fps.go:24): the reference indexes it with temporal 3 as soon as a
// temporal-3 chain advances; here the second frame advances and no rate is ever
// computed for temporal 3 (the one fps_device.h documents).  And SetMaxLayer
// takes a structure's layers unchecked, while frameRates is [3][4]: with a max
// layer beyond (2, 3) the reference indexes out of range; here the loops stop
// at the array and the completion product keeps the values as set, so such a
// calculator never completes.
#pragma once
#include <stdint.h>

#include "fps_device.h"

#ifndef LKF_FPSDD_ASSERT
#define LKF_FPSDD_ASSERT(c) ((void)0)
#endif

namespace lkf {
namespace fpsdd {

constexpr uint32_t kWin = 256;  // len(fnReceived) fps.go:326
constexpr int kWords = 4;       // 64-bit words of a mask over the window
constexpr int kSpatial = 3, kTemporal = 4, kLayers = kSpatial * kTemporal;
constexpr uint32_t KIND_DD = 3;  // (= LKF_FPS_DD)

struct M256 {
  uint64_t w[kWords];
};
// bits [0, n), n <= 256
__host__ __device__ inline M256 below256(uint32_t n) {
  M256 m;
#if defined(__clang__)
#pragma unroll
#endif
  for (int j = 0; j < kWords; j++) m.w[j] = n <= 64u * j ? 0ull : fps::below(n - 64u * j);
  return m;
}
__host__ __device__ inline bool any256(const M256 &m) { return (m.w[0] | m.w[1] | m.w[2] | m.w[3]) != 0; }
__host__ __device__ inline uint32_t ctz256(const M256 &m) {  // m != 0
  return m.w[0] ? fps::ctz64(m.w[0]) : m.w[1] ? 64 + fps::ctz64(m.w[1]) : m.w[2] ? 128 + fps::ctz64(m.w[2])
                                                                                  : 192 + fps::ctz64(m.w[3]);
}
__host__ __device__ inline uint32_t top256(const M256 &m) {  // m != 0
  return m.w[3] ? 192 + fps::top64(m.w[3]) : m.w[2] ? 128 + fps::top64(m.w[2]) : m.w[1] ? 64 + fps::top64(m.w[1])
                                                                                        : fps::top64(m.w[0]);
}
// a word of a four-word array by a run-time index (no indexed access: the head stays in registers)
__host__ __device__ inline uint64_t word_of(const uint64_t w[kWords], uint32_t j) {
  const uint64_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3];
  return j == 0 ? w0 : j == 1 ? w1 : j == 2 ? w2 : w3;
}

// The calculator without its window: wave-uniform, 128 B.  All zero but for
// the max layer is the state NewFrameRateCalculatorDD leaves.
struct alignas(16) Head {
  uint64_t present[kWords];         // bit k: fnReceived[k] != nil
  float rate[kSpatial][kTemporal];  // frameRates
  uint32_t first[kSpatial];         // byte t: firstFrames[s][t]'s slot (valid with its bit of `has`)
  uint32_t second[kSpatial];        // byte t: secondFrames[s][t]'s slot
  uint16_t has;       // bit 4 s + t: firstFrames / secondFrames[s][t] != nil (set and cleared together)
  uint16_t chainAny;  // bit 4 s + t: targetFrames[s][t].Len() != 0
  uint16_t baseFn;    // baseFrame.fn
  uint8_t hasBase, completed;
  uint8_t maxSpatial, maxTemporal;  // SetMaxLayer (defaults 2, 3)
  uint16_t dirty;  // bit 4 s + t: the chain, or the presence of one of its members, changed since calc()
                   // last walked it (not the reference's state: see calc())
  uint32_t resets;  // resets on a frame number that is not continuous, and close()
  uint32_t pad[2];
};
static_assert(sizeof(Head) == 128, "Head is 128 B");

// One enabled stream as it rests in device memory between ingests; written by
// k_ing_fps_dd alone after the enable.  Its structure pair (the one in force
// for the datagram being read, and the one an attached structure is read
// into) lies beside it, two DDStruct per entry, `cur` naming the one in force.
struct alignas(16) State {
  uint32_t kind;        // KIND_DD
  uint32_t calculated;  // Buffer.frameRateCalculated
  uint32_t clockRate;
  uint32_t stream;     // the handle (for the reader)
  uint32_t vp8;        // a VP8 track: ep.Spatial is invalid and becomes 0 (buffer.go:640, fps.go:365)
  uint32_t cur;        // the private structure slot in force
  uint32_t hasStruct;  // ... once one was read
  uint32_t pad;
  Head h;
  uint32_t ts[kWin];     // fnReceived[k].ts
  uint16_t chain[kWin];  // bit 4 s + t: frame baseFn + k is in targetFrames[s][t]
  uint8_t layer[kWin];   // fnReceived[k].spatial << 2 | .temporal
};
static_assert(sizeof(State) == 32 + 128 + 1024 + 512 + 256, "State is 1952 B");

__host__ __device__ inline uint32_t byte_of(uint32_t packed, int t) { return (packed >> (8 * t)) & 0xffu; }
__host__ __device__ inline uint32_t with_byte(uint32_t packed, int t, uint32_t v) {
  return (packed & ~(0xffu << (8 * t))) | (v << (8 * t));
}
// a word of a three-word array by a run-time index: by value (a select between the elements' addresses
// would keep the head in memory)
__host__ __device__ inline uint32_t sel3(const uint32_t a[kSpatial], int s) {
  const uint32_t a0 = a[0], a1 = a[1], a2 = a[2];
  return s == 0 ? a0 : s == 1 ? a1 : a2;
}
__host__ __device__ inline void put3(uint32_t a[kSpatial], int s, uint32_t v) {
  a[0] = s == 0 ? v : a[0];
  a[1] = s == 1 ? v : a[1];
  a[2] = s == 2 ? v : a[2];
}
__host__ __device__ inline void set_present(Head &h, uint32_t slot) {
  const uint64_t b = 1ull << (slot & 63);
  h.present[0] |= (slot >> 6) == 0 ? b : 0;
  h.present[1] |= (slot >> 6) == 1 ? b : 0;
  h.present[2] |= (slot >> 6) == 2 ? b : 0;
  h.present[3] |= (slot >> 6) == 3 ? b : 0;
}

// The window type W (HostWin below: 256 scalar entries; WaveWin: the wave):
//   W::chain_word(l, j)     bits of word j: the slot is in chain l = 4 s + t
//   W::count_word(s, t, j)  bits of word j: the slot's spatial == s && temporal <= t (set slots only matter)
//   W::ts_at(slot)
//   W::set(slot, ts, s, t)  fnReceived[slot] = frame
//   W::chain_add(l, slot)
//   W::chains_of(slot)      bit l: the slot is in chain l
//   W::clear()              every slot and chain empty
struct HostWin {
  uint32_t *ts;
  uint16_t *chain;
  uint8_t *layer;
  __host__ __device__ uint64_t chain_word(int l, int j) const {
    uint64_t m = 0;
    for (uint32_t k = 0; k < 64; k++) m |= uint64_t((chain[64 * j + k] >> l) & 1u) << k;
    return m;
  }
  __host__ __device__ uint64_t count_word(int s, int t, int j) const {
    uint64_t m = 0;
    for (uint32_t k = 0; k < 64; k++) {
      const int v = layer[64 * j + k];
      m |= uint64_t((v >> 2) == s && (v & 3) <= t) << k;
    }
    return m;
  }
  __host__ __device__ uint32_t ts_at(uint32_t slot) const { return ts[slot]; }
  __host__ __device__ void set(uint32_t slot, uint32_t t, uint32_t sp, uint32_t tmp) {
    ts[slot] = t;
    layer[slot] = uint8_t(sp << 2 | tmp);
  }
  __host__ __device__ void chain_add(int l, uint32_t slot) { chain[slot] |= uint16_t(1u << l); }
  __host__ __device__ uint32_t chains_of(uint32_t slot) const { return chain[slot]; }
  __host__ __device__ void clear() {
    for (uint32_t k = 0; k < kWin; k++) ts[k] = 0, chain[k] = 0, layer[k] = 0;
  }
};

#if defined(__HIPCC__)
// the wave: lane i holds slots i, 64 + i, 128 + i, 192 + i (all 64 lanes active at every call)
struct WaveWin {
  uint32_t ts0, ts1, ts2, ts3;
  uint32_t layer;  // byte j: slot 64 j + lane
  uint64_t chain;  // bits 16 j + l: slot 64 j + lane is in chain l
  uint32_t lane;
  __device__ uint64_t chain_word(int l, int j) const { return __ballot(int((chain >> (16 * j + l)) & 1ull)); }
  __device__ uint64_t count_word(int s, int t, int j) const {
    const uint32_t v = (layer >> (8 * j)) & 0xffu;
    return __ballot(int(v >> 2) == s && int(v & 3) <= t);
  }
  __device__ uint32_t ts_at(uint32_t slot) const {
    const uint32_t j = slot >> 6;
    const uint32_t v = j == 0 ? ts0 : j == 1 ? ts1 : j == 2 ? ts2 : ts3;
    return uint32_t(__builtin_amdgcn_readlane(int(v), int(slot & 63)));
  }
  __device__ void set(uint32_t slot, uint32_t t, uint32_t sp, uint32_t tmp) {
    if (lane == (slot & 63)) {
      const uint32_t j = slot >> 6;
      ts0 = j == 0 ? t : ts0;
      ts1 = j == 1 ? t : ts1;
      ts2 = j == 2 ? t : ts2;
      ts3 = j == 3 ? t : ts3;
      layer = (layer & ~(0xffu << (8 * j))) | ((sp << 2 | tmp) << (8 * j));
    }
  }
  __device__ void chain_add(int l, uint32_t slot) {
    if (lane == (slot & 63)) chain |= 1ull << (16 * (slot >> 6) + uint32_t(l));
  }
  __device__ uint32_t chains_of(uint32_t slot) const {
    const uint32_t v = uint32_t(chain >> (16 * (slot >> 6))) & 0xffffu;
    return uint32_t(__builtin_amdgcn_readlane(int(v), int(slot & 63)));
  }
  __device__ void clear() {
    ts0 = ts1 = ts2 = ts3 = 0;
    layer = 0;
    chain = 0;
  }
};
#endif

// What the reset on a frame number that is not continuous (fps.go:388-402) and
// close() (fps.go:535-552) both do: the rates and the max layer stay
template <class W>
__host__ __device__ inline void reset(Head &h, W &w) {
  h.present[0] = h.present[1] = h.present[2] = h.present[3] = 0;
  h.first[0] = h.first[1] = h.first[2] = 0;
  h.second[0] = h.second[1] = h.second[2] = 0;
  h.has = h.chainAny = h.dirty = 0;
  h.baseFn = 0;
  h.hasBase = 0;
  h.resets++;
  w.clear();
}

// SetMaxLayer fps.go:349
__host__ __device__ inline void set_max_layer(Head &h, uint32_t spatial, uint32_t temporal) {
  h.maxSpatial = uint8_t(spatial);
  h.maxTemporal = uint8_t(temporal);
}

// The value DependencyDescriptorParser.Parse hands onMaxLayerChanged
// (dependencydescriptorparser.go:143-155): the maximum layer over the decode
// targets present in `mask`, a target's layer being the one
// ProcessFrameDependencyStructure gave it (:178-193: the maximum sid / tid over
// the templates whose DTI for it is not NotPresent).  target / dtS / dtT: the
// structure's n decode targets in any order.  -> spatial | temporal << 8
__host__ __device__ inline uint32_t max_layer_of(uint32_t mask, uint32_t n, const uint8_t *target, const uint8_t *dtS,
                                                 const uint8_t *dtT) {
  uint32_t ms = 0, mt = 0;
  for (uint32_t i = 0; i < n; i++)
    if ((mask >> target[i]) & 1u) {
      ms = dtS[i] > ms ? dtS[i] : ms;
      mt = dtT[i] > mt ? dtT[i] : mt;
    }
  return ms | mt << 8;
}

// calc() fps.go:454-526.  The reference walks every layer's chain at every
// call.  A walk whose chain and whose members' presence are what they were at
// the layer's last walk finds the same last frame, and that walk left
// lastFrame.fn > second.fn false (it either was, or second became lastFrame),
// so it ends at the `continue` of fps.go:497 with nothing changed: Head.dirty
// names the layers for which that is not known, and only those are walked.
template <class W>
__host__ __device__ inline bool calc(Head &h, W &w, uint32_t clockRate) {
  int rateCounter = 0;
  // walk order of a chain: from slot rot to 255, then 0 to rot - 1
  const uint32_t wrapAt = 65536u - h.baseFn;
  const M256 lo = below256(wrapAt < kWin ? wrapAt : 0);  // the slots walked second
#if defined(__clang__)
#pragma unroll
#endif
  for (int s = 0; s < kSpatial; s++) {
    int spatialCounter = 0;
#if defined(__clang__)
#pragma unroll
#endif
    for (int t = 0; t < kTemporal; t++) {
      if (s > int(h.maxSpatial) || t > int(h.maxTemporal)) continue;
      const int l = 4 * s + t;
      if (h.rate[s][t] > 0) {
        rateCounter++;
        spatialCounter++;
        continue;
      }
      const bool seen = (h.has >> l) & 1;
      // lower temporal layer calculated, this one never seen: it does not exist (fps.go:466-471)
      if (spatialCounter > 0 && !seen) {
        spatialCounter++;
        rateCounter++;
        continue;
      }
      if (!((h.chainAny >> l) & 1)) continue;  // an empty chain has no last frame
      if (!((h.dirty >> l) & 1)) continue;     // nothing of this chain changed since its last walk
      h.dirty &= uint16_t(~(1u << l));
      // the last decodable frame (fps.go:475-492)
      M256 hiMiss, loMiss, hiC, loC;
#if defined(__clang__)
#pragma unroll
#endif
      for (int j = 0; j < kWords; j++) {
        const uint64_t c = w.chain_word(l, j);
        hiC.w[j] = c & ~lo.w[j];
        loC.w[j] = c & lo.w[j];
        hiMiss.w[j] = hiC.w[j] & ~h.present[j];
        loMiss.w[j] = loC.w[j] & ~h.present[j];
      }
      if (any256(hiMiss)) {  // the walk ends in its first part
        const M256 b = below256(ctz256(hiMiss));
        for (int j = 0; j < kWords; j++) hiC.w[j] &= b.w[j], loC.w[j] = 0;
      } else if (any256(loMiss)) {
        const M256 b = below256(ctz256(loMiss));
        for (int j = 0; j < kWords; j++) loC.w[j] &= b.w[j];
      }
      if (!any256(hiC) && !any256(loC)) continue;
      const uint32_t last = any256(loC) ? top256(loC) : top256(hiC);
      const uint32_t fst = byte_of(h.first[s], t), sec = byte_of(h.second[s], t);
      if (!(uint16_t(h.baseFn + last) > uint16_t(h.baseFn + sec))) continue;  // (plain compare, fps.go:494)
      h.second[s] = with_byte(h.second[s], t, last);
      if (t == 3) continue;  // (the reference panics here: the header's divergence)
      uint32_t frameCount = 0;
      if (fst <= last) {
        const M256 a = below256(fst), b = below256(last + 1);
#if defined(__clang__)
#pragma unroll
#endif
        for (int j = 0; j < kWords; j++)
          frameCount += uint32_t(fps::popc64(w.count_word(s, t, j) & h.present[j] & b.w[j] & ~a.w[j]));
      }
      const uint32_t lastTs = w.ts_at(last), firstTs = w.ts_at(fst);
      if (frameCount >= fps::min_frames(t) && lastTs > firstTs) {
        h.rate[s][t] = fps::rate_of(clockRate, lastTs, firstTs, frameCount);
        rateCounter++;
      }
    }
  }
  if (rateCounter == (int(h.maxSpatial) + 1) * (int(h.maxTemporal) + 1)) {
    h.completed = 1;
    reset(h, w);  // close()
    return true;
  }
  return false;
}

// RecvPacket would return false and change nothing (fps.go:369, :384, :404; not
// the completed case, which returns true): a caller that has to fetch the
// frame's diffs need not
__host__ __device__ inline bool recv_ignores(const Head &h, uint16_t fn, int32_t spatial, int32_t temporal) {
  if (spatial < 0) spatial = 0;
  if (temporal < 0 || temporal >= kTemporal || spatial >= kSpatial) return true;
  if (h.completed || !h.hasBase) return false;
  const uint16_t baseDiff = uint16_t(fn - h.baseFn);
  if (baseDiff == 0 || baseDiff > 0x8000) return true;
  if (baseDiff >= kWin) return false;
  return (word_of(h.present, baseDiff >> 6) >> (baseDiff & 63)) & 1;
}

// RecvPacket fps.go:353-452 for a packet with a descriptor.  D gives the
// frame's FrameDiffs in order: D::size(), then D::next() that many times.
template <class W, class D>
__host__ __device__ inline bool recv(Head &h, W &w, uint16_t fn, uint32_t ts, int32_t spatial, int32_t temporal, D &d,
                                     uint32_t clockRate) {
  if (h.completed) return true;
  if (spatial < 0) spatial = 0;  // non-SVC codec
  if (temporal < 0 || temporal >= kTemporal || spatial >= kSpatial) return false;
  const int l = 4 * spatial + temporal;
  if (!h.hasBase) {  // (the base frame's record keeps spatial 0, temporal 0, fps.go:376)
    h.hasBase = 1;
    h.baseFn = fn;
    h.present[0] = 1;
    w.set(0, ts, 0, 0);
    put3(h.first, spatial, with_byte(sel3(h.first, spatial), temporal, 0));
    put3(h.second, spatial, with_byte(sel3(h.second, spatial), temporal, 0));
    h.has |= uint16_t(1u << l);
    return false;
  }
  const uint16_t baseDiff = uint16_t(fn - h.baseFn);
  if (baseDiff == 0 || baseDiff > 0x8000) return false;
  if (baseDiff >= kWin) {  // frame number is not continuous
    reset(h, w);
    return false;
  }
  if ((word_of(h.present, baseDiff >> 6) >> (baseDiff & 63)) & 1) return false;
  set_present(h, baseDiff);
  w.set(baseDiff, ts, uint32_t(spatial), uint32_t(temporal));
  h.dirty |= uint16_t(w.chains_of(baseDiff));  // the chains that waited for this frame
  if (!((h.has >> l) & 1)) {
    put3(h.first, spatial, with_byte(sel3(h.first, spatial), temporal, baseDiff));
    put3(h.second, spatial, with_byte(sel3(h.second, spatial), temporal, baseDiff));
    h.has |= uint16_t(1u << l);
    return false;
  }
  if (!((h.chainAny >> l) & 1)) {
    h.chainAny |= uint16_t(1u << l);
    w.chain_add(l, baseDiff);
  }
  h.dirty |= uint16_t(1u << l);  // (members may be added below)
  const uint16_t secondFn = uint16_t(h.baseFn + byte_of(sel3(h.second, spatial), temporal));
  const uint32_t n = d.size();
  for (uint32_t i = 0; i < n; i++) {
    const uint16_t dependFrame = uint16_t(fn - uint16_t(d.next()));
    if (uint16_t(dependFrame - secondFn) > 0x8000) continue;  // frame too old
    const uint16_t slot = uint16_t(dependFrame - h.baseFn);
    LKF_FPSDD_ASSERT(slot < kWin);  // the header's invariant
    if (slot < kWin) w.chain_add(l, slot);
  }
  return calc(h, w, clockRate);
}

}  // namespace fpsdd
}  // namespace lkf
