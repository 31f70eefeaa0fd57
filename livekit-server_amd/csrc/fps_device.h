// fps_device.h — the PictureID frame-rate calculators of a received stream
// (buffer/fps.go:24-315: frameRateCalculatorVPx, FrameRateCalculatorVP8,
// FrameRateCalculatorVP9) as Buffer.doFpsCalc drives them (buffer.go:518-543).
// State and step, host and device: k_ing_fps (ingress_kernels.hip) runs it one
// wave per enabled stream, fps_unit.cpp runs it on the host compiler under the
// sanitizers, tests/fps_lib.PyFps restates it on Python ints.
//
// The window is the wave.  fnReceived[64] (fps.go:50) is slot j = lane j: a
// lane holds the timestamp and temporal layer of its slot, the presence set is
// one 64-bit mask, firstFrames / secondFrames (fps.go:48-49) are slot numbers
// (every frame they point to is in the window; the base frame is slot 0) and a
// slot's frame number is uint16(baseFn + slot).  calc() (fps.go:126-173) then
// needs no loop over frames: per temporal layer the range (first, second] is a
// lane mask, the first missing slot a count-trailing-zeros, frameCount a
// popcount of ballot(temporal <= t) and lastTs one readlane.  The step itself
// is wave-uniform code over a window type W:
//   W::le_mask(t)     bit j: slot j's temporal <= t     (device: one ballot)
//   W::ts_at(slot)    slot's timestamp                  (device: one readlane)
//   W::set(slot, ts, temporal)                          (device: the slot's lane writes)
// HostWin below is the 64-entry scalar stand-in, WaveWin the wave.
//
// Which packets reach the step (doFpsCalc, buffer.go:519): those that produced
// an ExtPacket with a non-empty payload, on a stream that is neither closed nor
// already calculated.  Buffer.paused has no counterpart in the engine: a host
// that pauses a Buffer stops ingesting its datagrams.
//
// One divergence.  minFramesForCalculation has 3 entries, frameRates 4
// (fps.go:24, :45): a stream that delivers two distinct frames at temporal 3
// makes the reference index out of range and panic (fps.go:155).  Here no rate
// is ever computed for temporal 3, so a calculator whose window holds two
// temporal-3 frames does not complete: a stream that keeps sending them never
// does (temporal 3 can still count as "lower layer calculated, never seen",
// fps.go:137-140, in a window without one).
//
// Not here: FrameRateCalculatorDD (fps.go:319-570), the calculator of a stream
// with a dependency descriptor.  It is fps_dd_device.h, run by k_ing_fps_dd,
// and uses min_frames, rate_of and the 64-bit mask helpers of this header.
#pragma once
#include <stdint.h>

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

namespace lkf {
namespace fps {

constexpr uint32_t kWin = 64;      // len(fnReceived) fps.go:50
constexpr int kTemporal = 4;       // DefaultMaxLayerTemporal + 1
constexpr int kSpatial = 3;        // DefaultMaxLayerSpatial + 1 (FrameRateCalculatorVP9, fps.go:234)
enum : uint32_t { KIND_NONE = 0, KIND_VP8 = 1, KIND_VP9 = 2 };  // (= LKF_FPS_*)

// minFramesForCalculation fps.go:24 (a function: no device-side table)
__host__ __device__ inline uint32_t min_frames(int t) { return t == 0 ? 8u : t == 1 ? 15u : 40u; }

// One frameRateCalculatorVPx without its window: wave-uniform, 48 B.  All zero
// is the state newFrameRateCalculatorVPx leaves.
struct alignas(16) Head {
  uint64_t present;     // bit j: fnReceived[j] != nil
  float rate[kTemporal];  // frameRates
  uint32_t first;       // byte t: firstFrames[t]'s slot + 1 (0: nil)
  uint32_t second;      // byte t: secondFrames[t]'s slot + 1 (0: nil)
  uint16_t baseFn;      // baseFrame.fn
  uint8_t hasBase, completed;
  uint32_t resets;      // reset() calls (fps.go:175), the one on completion included
  uint32_t pad[2];
};
static_assert(sizeof(Head) == 48, "Head is 48 B");

// ... and with its window, as it rests in device memory between ingests
struct alignas(16) Calc {
  Head h;
  uint32_t ts[kWin];       // fnReceived[j].ts
  uint8_t temporal[kWin];  // fnReceived[j].temporal
};
static_assert(sizeof(Calc) == 368, "Calc is 368 B");

// One enabled stream.  Zeroed at enable but for kind / clockRate / stream;
// written by k_ing_fps alone.
struct alignas(16) State {
  uint32_t kind;        // KIND_*
  uint32_t calculated;  // Buffer.frameRateCalculated
  uint32_t clockRate;
  uint32_t stream;      // the handle (for the reader)
  Calc c[kSpatial];     // VP8: c[0] alone
};
static_assert(sizeof(State) % 16 == 0 && sizeof(State) == 1120, "State is 16-B granular");

__host__ __device__ inline uint32_t slot_of(uint32_t packed, int t) { return (packed >> (8 * t)) & 0xffu; }
__host__ __device__ inline uint32_t with_slot(uint32_t packed, int t, uint32_t slot) {
  return (packed & ~(0xffu << (8 * t))) | ((slot + 1) << (8 * t));
}

// the 64-entry scalar stand-in for the wave
struct HostWin {
  uint32_t *ts;
  uint8_t *temporal;
  __host__ __device__ uint64_t le_mask(int t) const {
    uint64_t m = 0;
    for (uint32_t j = 0; j < kWin; j++) m |= uint64_t(int(temporal[j]) <= t) << j;
    return m;
  }
  __host__ __device__ uint32_t ts_at(uint32_t slot) const { return ts[slot]; }
  __host__ __device__ void set(uint32_t slot, uint32_t t, uint32_t tmp) {
    ts[slot] = t;
    temporal[slot] = uint8_t(tmp);
  }
};

#if defined(__HIPCC__)
// the wave: lane j holds slot j (all 64 lanes active at every call)
struct WaveWin {
  uint32_t ts, temporal, lane;
  __device__ uint64_t le_mask(int t) const { return __ballot(int(temporal) <= t); }
  __device__ uint32_t ts_at(uint32_t slot) const { return uint32_t(__builtin_amdgcn_readlane(int(ts), int(slot))); }
  __device__ void set(uint32_t slot, uint32_t t, uint32_t tmp) {
    if (lane == slot) {
      ts = t;
      temporal = tmp;
    }
  }
};
#endif

__host__ __device__ inline int popc64(uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popcll(v);
#else
  return __builtin_popcountll(v);
#endif
}
__host__ __device__ inline uint32_t ctz64(uint64_t v) {  // v != 0
#if defined(__HIP_DEVICE_COMPILE__)
  return uint32_t(__ffsll((long long)v) - 1);
#else
  return uint32_t(__builtin_ctzll(v));
#endif
}
__host__ __device__ inline uint32_t top64(uint64_t v) {  // v != 0: its highest set bit
#if defined(__HIP_DEVICE_COMPILE__)
  return 63u - uint32_t(__clzll((long long)v));
#else
  return 63u - uint32_t(__builtin_clzll(v));
#endif
}
// bits [0, n), n <= 64
__host__ __device__ inline uint64_t below(uint32_t n) { return n >= 64 ? ~0ull : (1ull << n) - 1; }

// reset() fps.go:175-185 (the rates stay)
__host__ __device__ inline void reset(Head &h) {
  h.first = h.second = 0;
  h.present = 0;
  h.hasBase = 0;
  h.baseFn = 0;
  h.resets++;
}

// The rate of fps.go:156: two separately rounded binary32 operations on a
// uint32 timestamp difference; a zero difference gives +Inf, which counts as
// calculated (> 0).  The device division is the plain operator: the project
// builds without fast-math, where hipcc keeps binary32 division correctly
// rounded (tests/test_fps_gpu.py compares the bits with the host's).
__host__ __device__ inline float rate_of(uint32_t clockRate, uint32_t lastTs, uint32_t firstTs, uint32_t frames) {
  const float q = float(clockRate) / float(uint32_t(lastTs - firstTs));
  return q * float(frames);
}

// calc() fps.go:126-173
template <class W>
__host__ __device__ inline bool calc(Head &h, const W &w, uint32_t clockRate) {
  int rateCounter = 0;
#if defined(__clang__)  // (constant indices into rate[]: the head stays in registers)
#pragma unroll
#endif
  for (int t = 0; t < kTemporal; t++) {
    if (h.rate[t] > 0) {
      rateCounter++;
      continue;
    }
    const uint32_t f = slot_of(h.first, t), s = slot_of(h.second, t);
    // lower layer calculated, this one never seen: it does not exist (fps.go:136-140)
    if (rateCounter > 0 && !f) {
      rateCounter++;
      continue;
    }
    if (!f || !s) continue;
    if (t == 3) continue;  // (the reference panics here: the header's divergence)
    const uint32_t a = f - 1, b = s - 1;
    // slots (a, b] (fps.go:147), up to the first one that is missing
    const uint64_t range = below(b + 1) & ~below(a + 1);
    const uint64_t miss = ~h.present & range;
    const uint64_t counted = w.le_mask(t) & range & (miss ? below(ctz64(miss)) : ~0ull);
    const uint32_t frameCount = uint32_t(popc64(counted));
    if (frameCount >= min_frames(t)) {
      const uint32_t firstTs = w.ts_at(a);
      const uint32_t lastTs = w.ts_at(top64(counted));  // (frameCount >= 8: not empty)
      h.rate[t] = rate_of(clockRate, lastTs, firstTs, frameCount);
      rateCounter++;
    }
  }
  if (rateCounter == kTemporal) {
    h.completed = 1;
    // Edge's middle layer: a fixed 1:2 of the highest (fps.go:164-168)
    if (h.rate[2] > 0 && h.rate[2] > h.rate[1] * 3) h.rate[1] = h.rate[2] / 2;
    reset(h);
    return true;
  }
  return false;
}

// frameRateCalculatorVPx.RecvPacket fps.go:66-124; every frame-number
// operation is uint16, the compare with the second frame included (not
// wrap-aware: a 15-bit PictureID that wraps 32767 -> 0 gives baseDiff > 0x4000
// and the calculator stalls, as in the reference)
template <class W>
__host__ __device__ inline bool recv(Head &h, W &w, uint16_t fn, uint32_t ts, int32_t temporal, uint32_t clockRate) {
  if (h.completed) return true;
  if (temporal >= kTemporal) return false;
  if (temporal < 0) temporal = 0;
  if (!h.hasBase) {  // (the base frame keeps temporal 0, fps.go:82)
    h.hasBase = 1;
    h.baseFn = fn;
    h.present = 1;
    w.set(0, ts, 0);
    h.first = with_slot(h.first, temporal, 0);
    return false;
  }
  const uint16_t baseDiff = uint16_t(fn - h.baseFn);
  if (baseDiff == 0 || baseDiff > 0x4000) return false;
  if (baseDiff >= kWin) {  // frame number is not continuous
    reset(h);
    return false;
  }
  if ((h.present >> baseDiff) & 1) return false;
  h.present |= 1ull << baseDiff;
  w.set(baseDiff, ts, uint32_t(temporal));
  const uint32_t f = slot_of(h.first, temporal), s = slot_of(h.second, temporal);
  if (!f) {
    h.first = with_slot(h.first, temporal, baseDiff);
  } else {
    const uint16_t firstFn = uint16_t(h.baseFn + (f - 1)), secondFn = uint16_t(h.baseFn + (s - 1));
    if ((!s || secondFn < fn) && fn != firstFn && uint16_t(fn - firstFn) < 0x4000)
      h.second = with_slot(h.second, temporal, baseDiff);
  }
  return calc(h, w, clockRate);
}

// FrameRateCalculatorVP8 / VP9.RecvPacket under doFpsCalc (fps.go:206-223,
// :253-290; buffer.go:522-541) for one packet that reaches it: h / w are the
// calculator the packet selects (VP9: ep.Spatial < 3, the caller drops the
// others, fps.go:264), done[] every calculator's completed flag after the
// step.  True: the stream became calculated (onFpsChanged).
__host__ __device__ inline bool stream_done(uint32_t kind, bool ret, const uint8_t done[kSpatial]) {
  if (!ret) return false;
  if (kind == KIND_VP8) return done[0] != 0;
  return done[0] && done[1] && done[2];  // all three spatial calculators (fps.go:271-280)
}

// codecs.VP9Packet.PictureID from the payload's first bytes (pion/rtp v1.8.3
// vp9_packet.go parsePictureID; parity unpinned like vp9_parse): b0 the
// descriptor's first byte, b1 / b2 the two after it (0 beyond the payload)
__host__ __device__ inline uint16_t vp9_picture_id(uint8_t b0, uint8_t b1, uint8_t b2) {
  if (!(b0 & 0x80)) return 0;                                  // I clear
  if (b1 & 0x80) return uint16_t((uint16_t(b1 & 0x7f) << 8) | b2);  // M: 15 bits
  return uint16_t(b1 & 0x7f);
}

}  // namespace fps
}  // namespace lkf
