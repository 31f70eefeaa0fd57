// handles.h — validation and grouping of the handle lists the control calls
// take (DownTracks, trackers): one pass over a strided list of int32_t handles
// that answers a bad list the way every call did by hand.  Host only, no HIP
// header; tested by host_unit.cpp.
//
// The first offending entry in list order decides the code.  For one entry:
// out of range (LKF_EINVAL), then the caller's own per-entry test
// (LKF_EINVAL), then "reappears" (the policy's code), then "inactive".
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/lkfwd.h"

namespace lkf {

enum class Repeat {
  Any,             // only the range (and the caller's test) is checked
  DistinctEinval,  // every handle at most once; a second occurrence is LKF_EINVAL
  DistinctEorder,  // every handle at most once; a second occurrence is LKF_EORDER
  Groups,          // contiguous runs of one handle; a handle that reappears after a gap is LKF_EORDER
};
enum class Inactive {
  Refuse,  // a handle whose active byte is 0 is LKF_EINVAL
  Skip,    // ... is accepted, but its group is left out of the group list
};
enum class HandleFault { None, Range, Entry, Repeat, Inactive };  // why a list was refused

struct HandlePolicy {
  Repeat repeat = Repeat::Any;
  // group starts: entry i opens a group when its handle differs from entry
  // i - 1's (every entry, under the two distinct policies); with `end`, n is
  // appended as the last group's end bound
  std::vector<uint32_t> *groups = nullptr;
  bool end = false;
  const uint8_t *active = nullptr;  // per handle, `limit` bytes; null: every handle counts as active
  Inactive inactive = Inactive::Refuse;
  HandleFault *why = nullptr;
};

// n handles, the i-th at first + i * stride bytes, each in [0, limit).
// entryOk(i) is the caller's test of entry i (a byte range, say).
template <typename EntryOk>
int check_handles(const void *first, size_t stride, uint32_t n, size_t limit, const HandlePolicy &p, EntryOk entryOk) {
  auto refuse = [&](HandleFault f, int rc) {
    if (p.why) *p.why = f;
    return rc;
  };
  if (p.why) *p.why = HandleFault::None;
  if (p.groups) p.groups->clear();
  std::vector<uint8_t> seen(p.repeat == Repeat::Any ? 0 : limit, 0);
  const bool runs = p.repeat == Repeat::Any || p.repeat == Repeat::Groups;
  int32_t prev = -1;
  for (uint32_t i = 0; i < n; i++) {
    int32_t h;
    memcpy(&h, static_cast<const uint8_t *>(first) + size_t(i) * stride, sizeof(h));
    if (h < 0 || size_t(h) >= limit) return refuse(HandleFault::Range, LKF_EINVAL);
    if (!entryOk(i)) return refuse(HandleFault::Entry, LKF_EINVAL);
    if (!runs || i == 0 || h != prev) {
      if (p.repeat != Repeat::Any) {
        if (seen[h]) return refuse(HandleFault::Repeat, p.repeat == Repeat::DistinctEinval ? LKF_EINVAL : LKF_EORDER);
        seen[h] = 1;
      }
      if (p.active && !p.active[h]) {
        if (p.inactive == Inactive::Refuse) return refuse(HandleFault::Inactive, LKF_EINVAL);
      } else if (p.groups) {
        p.groups->push_back(i);
      }
    }
    prev = h;
  }
  if (p.groups && p.end) p.groups->push_back(n);
  return LKF_OK;
}

inline int check_handles(const void *first, size_t stride, uint32_t n, size_t limit, const HandlePolicy &p) {
  return check_handles(first, stride, n, limit, p, [](uint32_t) { return true; });
}

}  // namespace lkf
