// ctl_csr.h — the queued control ops of a run as a per-lane CSR (host only).
//
// Stable order: by lane, inside a lane by at_pkt, ops with equal at_pkt in
// queue order.  Only the ops are sorted: an LSD radix sort on the lane (8-bit
// digits, as many passes as the lane count needs), then a stable insertion by
// at_pkt inside a lane whose ops were queued out of at_pkt order.  Ops of a
// DownTrack without a lane (removed) are dropped.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <utility>
#include <vector>

#include "../../include/lkfwd.h"
#include "fwd_state.h"

namespace lkf {

struct CtlPend {  // one queued op
  uint32_t dt;
  DevEvent ev;
};

struct CtlCsr {
  std::vector<std::pair<uint32_t, uint32_t>> a, b;  // (lane, pending index); reused from run to run

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

  // Writes the sorted ops and their lanes (room for sort()'s count each).
  void emit(const CtlPend *pend, DevEvent *evs, uint32_t *lanes) const {
    for (size_t i = 0; i < a.size(); i++) {
      evs[i] = pend[a[i].second].ev;
      lanes[i] = a[i].first;
      if (i && a[i - 1].first == a[i].first && evs[i].at < evs[i - 1].at) {
        const DevEvent v = evs[i];  // queued out of at_pkt order: stable insertion within the lane
        size_t j = i;
        while (j > 0 && lanes[j - 1] == a[i].first && evs[j - 1].at > v.at) {
          evs[j] = evs[j - 1];
          j--;
        }
        evs[j] = v;
      }
    }
  }
};

}  // namespace lkf
