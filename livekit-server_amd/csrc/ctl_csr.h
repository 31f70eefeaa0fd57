// ctl_csr.h — the queued control ops of a run as a per-lane CSR (host only).
//
// Stable order: by lane, inside a lane by key, ops with equal keys in queue
// order.  The key of an lkf_ctl op is its at_pkt (0 below every keyed op,
// 0xffffffff above); a keyed op (lkf_ctl_key*) sorts by the datagram index or
// arrival time it was queued with.  Only the ops are sorted: an LSD radix sort
// on the lane (8-bit digits, as many passes as the lane count needs), then,
// while the ops are written out, a stable insertion by key inside a lane whose
// ops were queued out of key order.  Ops of a DownTrack without a lane (removed) are dropped.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <utility>
#include <vector>

#include "../../include/lkfwd.h"
#include "fwd_state.h"

namespace lkf {

struct CtlPend {  // one queued op (64 B)
  uint32_t dt;
  int32_t kind;  // lkf_at_kind (ev.at holds the position of an LKF_AT_PKT op)
  DevEvent ev;
  int64_t key;  // kind != LKF_AT_PKT: the datagram index or arrival time
};
static_assert(sizeof(CtlPend) == 64, "CtlPend is one cache line");

// The key an op sorts by within its lane.
inline int64_t ctl_sort_key(const CtlPend &p) {
  if (p.kind != LKF_AT_PKT) return p.key;
  if (p.ev.at == 0) return INT64_MIN;
  if (p.ev.at == 0xffffffffu) return INT64_MAX;
  return int64_t(p.ev.at);
}

// An op that names a position inside the batch in the space of its kind:
// every keyed op, and an lkf_ctl op neither at the batch start nor at its end.
inline bool ctl_in_batch(const CtlPend &p) {
  return p.kind != LKF_AT_PKT || (p.ev.at != 0 && p.ev.at != 0xffffffffu);
}

struct CtlCsr {
  std::vector<std::pair<uint32_t, uint32_t>> a, b;  // (lane, pending index); reused from run to run
  std::vector<uint8_t> kinds;                       // mixed(): per DownTrack, the in-batch kinds seen
  std::vector<int64_t> sk;                          // emit(): the sort key of each op written so far

  // The first DownTrack with a lane whose in-batch ops are of two different
  // kinds (one run resolves a DownTrack's positions in one space), or -1.
  int64_t mixed(const CtlPend *pend, size_t n, const int32_t *dtLane, size_t ndt) {
    kinds.assign(ndt, 0);
    for (size_t i = 0; i < n; i++) {
      const CtlPend &p = pend[i];
      if (dtLane[p.dt] < 0 || !ctl_in_batch(p)) continue;
      kinds[p.dt] |= uint8_t(1u << p.kind);
      if (kinds[p.dt] & (kinds[p.dt] - 1)) return int64_t(p.dt);
    }
    return -1;
  }

  // Sorts the ops that have a lane (dtLane[dt] >= 0; nl lanes); returns how many.
  size_t sort(const CtlPend *pend, size_t n, const int32_t *dtLane, uint32_t nl) {
    a.clear();
    for (uint32_t i = 0; i < uint32_t(n); i++) {
      const int l = dtLane[pend[i].dt];
      if (l >= 0) a.push_back({uint32_t(l), i});
    }
    b.resize(a.size());
    for (uint32_t shift = 0; shift < 32 && (nl >> shift) > 0; shift += 8) {  // stable LSD passes
      uint32_t cnt[257] = {0};
      for (auto &k : a) cnt[((k.first >> shift) & 0xff) + 1]++;
      for (int d = 0; d < 256; d++) cnt[d + 1] += cnt[d];
      for (auto &k : a) b[cnt[(k.first >> shift) & 0xff]++] = k;
      a.swap(b);
    }
    return a.size();
  }

  // Writes the sorted ops and their lanes (room for sort()'s count each), and
  // with keys their position keys (dtp: the DownTracks' parameters, for the track).
  void emit(const CtlPend *pend, DevEvent *evs, uint32_t *lanes, DevKey *keys = nullptr,
            const lkf_downtrack_params *dtp = nullptr) {
    sk.resize(a.size());
    for (size_t i = 0; i < a.size(); i++) {
      const CtlPend &p = pend[a[i].second];
      const int64_t k = ctl_sort_key(p);
      evs[i] = p.ev;
      lanes[i] = a[i].first;
      sk[i] = k;
      if (keys) {
        keys[i].key = p.key;
        keys[i].kind = p.kind;
        keys[i].track = dtp ? uint32_t(dtp[p.dt].track) : 0u;
      }
      if (i && a[i - 1].first == a[i].first && k < sk[i - 1]) {
        const DevEvent v = evs[i];  // queued out of key order: stable insertion within the lane
        const DevKey vk = keys ? keys[i] : DevKey{};
        size_t j = i;
        while (j > 0 && lanes[j - 1] == a[i].first && sk[j - 1] > k) {
          evs[j] = evs[j - 1];
          sk[j] = sk[j - 1];
          if (keys) keys[j] = keys[j - 1];
          j--;
        }
        evs[j] = v;
        sk[j] = k;
        if (keys) keys[j] = vk;
      }
    }
  }
};

}  // namespace lkf
