// host_unit.cpp — CPU unit tests of the engine's pure host pieces: DevBuf
// (dev_buf.h) over a malloc-backed fake of its two allocation functions, the
// control-op CSR (ctl_csr.h) against std::stable_sort, and the control calls'
// handle lists (handles.h) against a naive restatement.  Built with the
// host compiler alone (make host_unit; address + undefined sanitizers).
//   host_unit --list     the case names
//   host_unit <name>     one case ("PASS <name>" / exit 1)
//   host_unit            every case
#define __host__
#define __device__
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "ctl_csr.h"
#include "dev_buf.h"
#include "handles.h"

using namespace lkf;

// ---- the fake allocator -----------------------------------------------------
static std::map<void *, size_t> g_live;  // pointer -> bytes
static int g_allocs = 0, g_frees = 0, g_bad_frees = 0;
static bool g_fail_next = false;
static std::vector<void *> g_freed;  // in order

int lkf::dev_alloc(void **p, size_t bytes) {
  *p = nullptr;
  if (g_fail_next) {
    g_fail_next = false;
    return 2;  // hipErrorOutOfMemory
  }
  *p = std::malloc(bytes);
  g_live[*p] = bytes;
  g_allocs++;
  return 0;
}
int lkf::dev_free(void *p) {
  auto it = g_live.find(p);
  if (it == g_live.end()) {
    g_bad_frees++;  // a double free, or a pointer the fake never handed out
    return 1;
  }
  g_live.erase(it);
  g_freed.push_back(p);
  g_frees++;
  std::free(p);
  return 0;
}

static int g_fail = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::printf("  %s:%d: CHECK(%s)\n", __FILE__, __LINE__, #c); \
      g_fail++;                                                   \
    }                                                             \
  } while (0)

// ---- DevBuf -----------------------------------------------------------------
static void devbuf_reserve_floor() {
  DevBuf<uint32_t> b;
  CHECK(b.get() == nullptr && b.cap() == 0);
  CHECK(b.reserve(0, 256) == 0 && b.get() == nullptr);  // nothing asked: nothing allocated
  CHECK(b.reserve(10, 256) == 0 && b.cap() == 256);     // below the floor
  CHECK(g_live.at(b.get()) == 256 * sizeof(uint32_t));
  DevBuf<uint32_t> c;
  CHECK(c.reserve(256, 256) == 0 && c.cap() == 256);  // at the floor
  DevBuf<uint64_t> d;
  CHECK(d.reserve(257, 256) == 0 && d.cap() == 257);  // above it
  CHECK(g_live.at(d.get()) == 257 * sizeof(uint64_t));
  uint64_t *raw = d;  // converts to T*
  CHECK(raw == d.get());
}

static void devbuf_no_realloc() {
  DevBuf<uint16_t> b;
  CHECK(b.reserve(40, 256) == 0);
  uint16_t *p = b;
  const int a0 = g_allocs, f0 = g_frees;
  CHECK(b.reserve(40, 256) == 0 && b.reserve(256, 256) == 0 && b.reserve(1, 1 << 20) == 0);
  CHECK(b.get() == p && b.cap() == 256 && g_allocs == a0 && g_frees == f0);
  CHECK(b.reserve(257, 256) == 0 && b.cap() == 257);  // grows: the old buffer is freed first
  CHECK(g_allocs == a0 + 1 && g_frees == f0 + 1 && g_freed.back() == p);
  CHECK(b.reserve(40, 256) == 0 && b.cap() == 257);  // never shrinks
}

static void devbuf_failed_grow() {
  DevBuf<uint8_t> b;
  CHECK(b.reserve(100, 1024) == 0 && b.cap() == 1024);
  g_fail_next = true;
  CHECK(b.reserve(5000, 1024) != 0);
  CHECK(b.get() == nullptr && b.cap() == 0);  // empty, not "large and null"
  CHECK(b.reserve(100, 1024) == 0 && b.get() != nullptr && b.cap() == 1024);  // a smaller n retries
  g_fail_next = true;
  DevBuf<uint8_t> c;
  CHECK(c.alloc(7) != 0 && c.get() == nullptr && c.cap() == 0);
  CHECK(c.alloc(7) == 0 && c.cap() == 7);
}

static void devbuf_alloc_fixed() {
  DevBuf<uint32_t> b;
  CHECK(b.alloc(0) == 0 && b.get() != nullptr && b.cap() == 0);  // an empty table still has an address
  CHECK(g_live.at(b.get()) == sizeof(uint32_t));
  uint32_t *p = b;
  CHECK(b.alloc(12) == 0 && b.cap() == 12 && g_freed.back() == p);
  const int f0 = g_frees;
  CHECK(b.reset() == 0 && b.get() == nullptr && b.cap() == 0 && g_frees == f0 + 1);
  CHECK(b.reset() == 0 && g_frees == f0 + 1);  // idempotent
}

static void devbuf_move() {
  DevBuf<uint32_t> a, b;
  CHECK(a.alloc(8) == 0 && b.alloc(16) == 0);
  uint32_t *pa = a, *pb = b;
  const int f0 = g_frees;
  a = std::move(b);  // a's old buffer is freed exactly once; b is left empty
  CHECK(g_frees == f0 + 1 && g_freed.back() == pa && g_bad_frees == 0);
  CHECK(a.get() == pb && a.cap() == 16 && b.get() == nullptr && b.cap() == 0);
  DevBuf<uint32_t> c(std::move(a));
  CHECK(c.get() == pb && c.cap() == 16 && a.get() == nullptr && g_frees == f0 + 1);
  DevBuf<uint32_t> x, y;
  CHECK(x.alloc(1) == 0 && y.alloc(1) == 0);
  const int f1 = g_frees;
  release_all(x, y);
  CHECK(g_frees == f1 + 2 && !x.get() && !y.get());
}

// two calls with opposite shapes share a family (as feedback and sender reports do)
static void devbuf_family_settles() {
  DevBuf<uint8_t> in, out;
  DevBuf<uint32_t> g;
  auto call = [&](uint64_t nin, uint64_t ng, uint64_t nout) {
    if (!family_short(want(in, nin, 64), want(g, ng, 8), want(out, nout, 64))) return 0;
    CHECK(regrow_family(want(in, nin, 64, 2 * nin), want(g, ng, 8, 2 * ng), want(out, nout, 64, 2 * nout)) == 0);
    return 1;
  };
  CHECK(call(10, 0, 10) == 1 && in.cap() == 64 && g.cap() == 8 && out.cap() == 64);  // the floors
  CHECK(call(64, 8, 64) == 0);
  CHECK(call(300, 3, 20) == 1 && in.cap() == 600 && out.cap() == 64);   // input-heavy
  CHECK(call(20, 0, 100) == 1 && in.cap() == 600 && out.cap() == 200);  // output-heavy: the input side keeps its size
  const int a0 = g_allocs;
  for (int tick = 0; tick < 5; tick++) CHECK(call(300, 3, 20) == 0 && call(20, 0, 100) == 0);
  CHECK(g_allocs == a0 && in.cap() == 600 && g.cap() == 8 && out.cap() == 200);
  // a failed regrow: the buffers from the failure on are empty, the next call retries
  g_fail_next = true;
  CHECK(regrow_family(want(in, 700, 64), want(g, 1, 8), want(out, 1, 64)) != 0);
  CHECK(in.get() == nullptr && in.cap() == 0 && g.cap() == 0 && out.cap() == 0);
  CHECK(call(20, 0, 100) == 1 && in.cap() == 64 && out.cap() == 200);
}

// ---- control-op CSR ---------------------------------------------------------
struct Ref {
  uint32_t lane, at;
  int64_t id;
};

// pend[i].ev.a[0] = i identifies an op
static void csr_check(const std::vector<CtlPend> &pend, const std::vector<int32_t> &dtLane, uint32_t nl) {
  std::vector<Ref> ref;
  for (size_t i = 0; i < pend.size(); i++)
    if (dtLane[pend[i].dt] >= 0) ref.push_back({uint32_t(dtLane[pend[i].dt]), pend[i].ev.at, int64_t(i)});
  std::stable_sort(ref.begin(), ref.end(),
                   [](const Ref &a, const Ref &b) { return a.lane != b.lane ? a.lane < b.lane : a.at < b.at; });
  CtlCsr csr;
  const size_t nev = csr.sort(pend.data(), pend.size(), dtLane.data(), nl);
  CHECK(nev == ref.size());
  std::vector<DevEvent> evs(nev + 1);
  std::vector<uint32_t> lanes(nev + 1, 0xdeadbeefu);
  std::memset(evs.data(), 0x5a, evs.size() * sizeof(DevEvent));
  csr.emit(pend.data(), evs.data(), lanes.data());
  bool same = nev == ref.size();
  for (size_t i = 0; same && i < nev; i++)
    same = lanes[i] == ref[i].lane && evs[i].at == ref[i].at && evs[i].a[0] == ref[i].id &&
           std::memcmp(&evs[i], &pend[size_t(ref[i].id)].ev, sizeof(DevEvent)) == 0;
  CHECK(same);
  CHECK(lanes[nev] == 0xdeadbeefu);  // nothing past the count
}

static CtlPend op(uint32_t dt, uint32_t at, size_t id) {
  CtlPend p;
  std::memset(&p, 0, sizeof(p));
  p.dt = dt;
  p.ev.at = at;
  p.ev.op = int32_t(id % 7);
  p.ev.a[0] = int64_t(id);
  p.ev.a[3] = -int64_t(id);
  return p;
}

static void csr_empty() {
  csr_check({}, {0, 1, 2}, 3);
  csr_check({}, {}, 0);
}

static void csr_one_lane_out_of_order() {
  std::vector<CtlPend> p;
  const uint32_t at[] = {9, 3, 7, 0, 8, 1, 1, 4};
  for (size_t i = 0; i < 8; i++) p.push_back(op(2, at[i], i));
  csr_check(p, {-1, 0, 5, 1}, 6);
}

static void csr_equal_at_keeps_queue_order() {
  std::vector<CtlPend> p;
  for (size_t i = 0; i < 12; i++) p.push_back(op(uint32_t(i % 2), i < 6 ? 5 : 2, i));
  csr_check(p, {1, 0}, 2);
}

static void csr_removed_dropped() {
  std::vector<CtlPend> p;
  for (size_t i = 0; i < 20; i++) p.push_back(op(uint32_t(i % 4), uint32_t(20 - i), i));
  csr_check(p, {3, -1, 0, -1}, 4);
  csr_check(p, {-1, -1, -1, -1}, 4);  // every op dropped
}

static void csr_random(uint32_t nl, size_t nops) {
  uint64_t s = 0x9e3779b97f4a7c15ull ^ nl;
  auto rnd = [&]() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return uint32_t(s >> 33);
  };
  // one DownTrack per lane, lanes permuted; every 9th DownTrack has none
  std::vector<int32_t> dtLane(nl);
  for (uint32_t d = 0; d < nl; d++) dtLane[d] = int32_t(d);
  for (uint32_t d = nl; d > 1; d--) std::swap(dtLane[d - 1], dtLane[rnd() % d]);
  for (uint32_t d = 0; d < nl; d += 9) dtLane[d] = -1;
  std::vector<uint32_t> hot;  // a few DownTracks get many ops, so lanes repeat
  for (int i = 0; i < 12; i++) hot.push_back(rnd() % nl);
  hot.push_back(nl - 1);
  std::vector<CtlPend> p;
  for (size_t i = 0; i < nops; i++)
    p.push_back(op((rnd() & 1) ? hot[rnd() % hot.size()] : rnd() % nl, rnd() % 6, i));
  csr_check(p, dtLane, nl);
}
static void csr_nl_200() { csr_random(200, 300); }      // one radix pass
static void csr_nl_300() { csr_random(300, 400); }      // two
static void csr_nl_70000() { csr_random(70000, 500); }  // three

// ---- handle lists (handles.h) --------------------------------------------------
using H = std::vector<int32_t>;
using G = std::vector<uint32_t>;
static const Repeat kPolicies[] = {Repeat::DistinctEinval, Repeat::DistinctEorder, Repeat::Groups};

static int hcheck(const H &h, size_t limit, Repeat rep, G *groups = nullptr, const uint8_t *active = nullptr,
                  Inactive ina = Inactive::Refuse, HandleFault *why = nullptr) {
  HandlePolicy p;
  p.repeat = rep;
  p.groups = groups;
  p.end = true;
  p.active = active;
  p.inactive = ina;
  p.why = why;
  return check_handles(h.data(), sizeof(int32_t), uint32_t(h.size()), limit, p);
}

static void handles_empty() {
  for (Repeat rep : kPolicies) {
    G g = {7, 7};
    CHECK(hcheck({}, 4, rep, &g) == LKF_OK && g == G({0}));
    CHECK(hcheck({}, 0, rep) == LKF_OK);
  }
  CHECK(hcheck({}, 4, Repeat::Any) == LKF_OK);
}

static void handles_range() {
  for (Repeat rep : {Repeat::Any, Repeat::DistinctEinval, Repeat::DistinctEorder, Repeat::Groups}) {
    HandleFault why = HandleFault::None;
    CHECK(hcheck({0, -1}, 4, rep, nullptr, nullptr, Inactive::Refuse, &why) == LKF_EINVAL && why == HandleFault::Range);
    CHECK(hcheck({4}, 4, rep) == LKF_EINVAL);
    CHECK(hcheck({3, 0}, 4, rep) == LKF_OK);
    CHECK(hcheck({0}, 0, rep) == LKF_EINVAL);
    CHECK(hcheck({INT32_MIN}, 4, rep) == LKF_EINVAL && hcheck({INT32_MAX}, 4, rep) == LKF_EINVAL);
  }
}

static void handles_adjacent_repeat() {
  G g;
  HandleFault why = HandleFault::None;
  CHECK(hcheck({1, 2, 2, 3}, 4, Repeat::DistinctEinval, &g, nullptr, Inactive::Refuse, &why) == LKF_EINVAL &&
        why == HandleFault::Repeat);
  CHECK(hcheck({1, 2, 2, 3}, 4, Repeat::DistinctEorder, &g, nullptr, Inactive::Refuse, &why) == LKF_EORDER &&
        why == HandleFault::Repeat);
  CHECK(hcheck({1, 2, 2, 3}, 4, Repeat::Groups, &g, nullptr, Inactive::Refuse, &why) == LKF_OK &&
        why == HandleFault::None && g == G({0, 1, 3, 4}));
  CHECK(hcheck({1, 2, 2, 3}, 4, Repeat::Any, &g) == LKF_OK && g == G({0, 1, 3, 4}));
  CHECK(hcheck({0, 1, 2, 3}, 4, Repeat::DistinctEinval, &g) == LKF_OK && g == G({0, 1, 2, 3, 4}));
}

static void handles_split_repeat() {
  CHECK(hcheck({1, 2, 1}, 4, Repeat::DistinctEinval) == LKF_EINVAL);
  CHECK(hcheck({1, 2, 1}, 4, Repeat::DistinctEorder) == LKF_EORDER);
  CHECK(hcheck({1, 2, 1}, 4, Repeat::Groups) == LKF_EORDER);
  CHECK(hcheck({1, 1, 2, 2, 1}, 4, Repeat::Groups) == LKF_EORDER);
  CHECK(hcheck({1, 2, 1}, 4, Repeat::Any) == LKF_OK);
}

static void handles_first_offender_wins() {
  for (Repeat rep : {Repeat::DistinctEorder, Repeat::Groups}) {
    CHECK(hcheck({9, 1, 2, 1}, 4, rep) == LKF_EINVAL);  // [bad range, repeat]
    CHECK(hcheck({1, 2, 1, 9}, 4, rep) == LKF_EORDER);  // [repeat, bad range]
    CHECK(hcheck({1, 2, -1, 1}, 4, rep) == LKF_EINVAL);
  }
  // one entry: its range before the caller's test, the caller's test before "reappears"
  const H h = {1, 2, 1, 9};
  HandlePolicy p;
  p.repeat = Repeat::Groups;
  HandleFault why = HandleFault::None;
  p.why = &why;
  uint32_t asked = 0;
  CHECK(check_handles(h.data(), 4, 4, 4, p, [&](uint32_t i) { return asked = i, i != 2; }) == LKF_EINVAL);
  CHECK(why == HandleFault::Entry && asked == 2);
  CHECK(check_handles(h.data(), 4, 4, 4, p, [&](uint32_t i) { return i != 3; }) == LKF_EORDER && why == HandleFault::Repeat);
  const H r = {9, 0};
  asked = 77;
  CHECK(check_handles(r.data(), 4, 2, 4, p, [&](uint32_t i) { return asked = i, false; }) == LKF_EINVAL);
  CHECK(why == HandleFault::Range && asked == 77);  // the test is not asked about an entry out of range
}

static void handles_stride() {
  struct Rec {
    uint8_t pad[3];  // (the handle is not 4-byte aligned)
    uint8_t h[4];
    uint8_t tail[6];
  };
  static_assert(sizeof(Rec) == 13, "an odd stride");
  auto list = [](const H &h) {
    std::vector<Rec> v(h.size());
    for (size_t i = 0; i < h.size(); i++) {
      std::memset(&v[i], 0xee, sizeof(Rec));
      std::memcpy(v[i].h, &h[i], 4);
    }
    return v;
  };
  HandlePolicy p;
  G g;
  p.repeat = Repeat::Groups;
  p.groups = &g;
  p.end = true;
  auto a = list({3, 3, 0, 2, 2, 2});
  CHECK(check_handles(a[0].h, sizeof(Rec), 6, 4, p) == LKF_OK && g == G({0, 2, 3, 6}));
  auto b = list({3, 0, 3});
  CHECK(check_handles(b[0].h, sizeof(Rec), 3, 4, p) == LKF_EORDER);
  auto c = list({3, 0, 4});
  CHECK(check_handles(c[0].h, sizeof(Rec), 3, 4, p) == LKF_EINVAL);
  CHECK(check_handles(c[0].h, sizeof(Rec), 2, 4, p) == LKF_OK && g == G({0, 1, 2}));  // n bounds the reads
}

static void handles_inactive_refused() {
  const uint8_t active[4] = {1, 0, 1, 1};
  HandleFault why = HandleFault::None;
  for (Repeat rep : kPolicies) {
    CHECK(hcheck({0, 1, 2}, 4, rep, nullptr, active, Inactive::Refuse, &why) == LKF_EINVAL && why == HandleFault::Inactive);
    CHECK(hcheck({0, 2, 3}, 4, rep, nullptr, active, Inactive::Refuse, &why) == LKF_OK);
    CHECK(hcheck({0, 5, 1}, 4, rep, nullptr, active, Inactive::Refuse, &why) == LKF_EINVAL && why == HandleFault::Range);
  }
  // a repeat earlier in the list is met first
  CHECK(hcheck({0, 0, 1}, 4, Repeat::DistinctEorder, nullptr, active, Inactive::Refuse, &why) == LKF_EORDER);
  CHECK(hcheck({1, 1}, 4, Repeat::DistinctEorder, nullptr, active, Inactive::Refuse, &why) == LKF_EINVAL &&
        why == HandleFault::Inactive);
}

static void handles_inactive_skipped() {
  const uint8_t active[4] = {1, 0, 1, 0};
  G g;
  CHECK(hcheck({0, 0, 1, 1, 2, 3}, 4, Repeat::Groups, &g, active, Inactive::Skip) == LKF_OK && g == G({0, 4, 6}));
  CHECK(hcheck({1, 3}, 4, Repeat::Groups, &g, active, Inactive::Skip) == LKF_OK && g == G({2}));
  CHECK(hcheck({0, 1, 2}, 4, Repeat::DistinctEinval, &g, active, Inactive::Skip) == LKF_OK && g == G({0, 2, 3}));
  // a skipped handle still counts as seen
  CHECK(hcheck({1, 0, 1}, 4, Repeat::Groups, &g, active, Inactive::Skip) == LKF_EORDER);
  HandlePolicy p;  // without the end bound: the starts alone
  p.repeat = Repeat::Groups;
  p.groups = &g;
  p.active = active;
  p.inactive = Inactive::Skip;
  const H h = {2, 2, 3, 0};
  CHECK(check_handles(h.data(), 4, 4, 4, p) == LKF_OK && g == G({0, 3}));
}

// the rules restated entry by entry, every earlier entry rescanned
static int handles_naive(const H &h, const std::vector<uint8_t> &entryBad, size_t limit, Repeat rep,
                         const uint8_t *active, Inactive ina, G &groups) {
  groups.clear();
  for (size_t i = 0; i < h.size(); i++) {
    if (h[i] < 0 || h[i] >= int64_t(limit)) return LKF_EINVAL;
    if (entryBad[i]) return LKF_EINVAL;
    const bool run = rep == Repeat::Groups || rep == Repeat::Any;
    if (run && i > 0 && h[i - 1] == h[i]) continue;
    if (rep != Repeat::Any)
      for (size_t j = 0; j < i; j++)
        if (h[j] == h[i]) return rep == Repeat::DistinctEinval ? LKF_EINVAL : LKF_EORDER;
    if (active && !active[h[i]]) {
      if (ina == Inactive::Refuse) return LKF_EINVAL;
      continue;
    }
    groups.push_back(uint32_t(i));
  }
  groups.push_back(uint32_t(h.size()));
  return LKF_OK;
}

static void handles_random() {
  uint64_t s = 0x2545f4914f6cdd1dull;
  auto rnd = [&]() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return uint32_t(s >> 33);
  };
  int ok = 0, einval = 0, eorder = 0;
  for (int it = 0; it < 600; it++) {
    const size_t limit = 4, n = rnd() % 9;
    H h(n);
    std::vector<uint8_t> bad(n, 0);
    int32_t cur = int32_t(rnd() % limit);
    for (size_t i = 0; i < n; i++) {
      if (rnd() % 3) cur = int32_t(rnd() % limit);          // else: the run goes on
      h[i] = rnd() % 40 == 0 ? int32_t(rnd() % 7) - 2 : cur;  // now and then out of range
      bad[i] = rnd() % 50 == 0;
    }
    uint8_t active[4];
    for (auto &a : active) a = rnd() % 5 != 0;
    const Repeat rep = Repeat(rnd() % 4);
    const Inactive ina = rnd() & 1 ? Inactive::Refuse : Inactive::Skip;
    const uint8_t *act = rnd() & 1 ? active : nullptr;
    G want, got;
    const int rc = handles_naive(h, bad, limit, rep, act, ina, want);
    HandlePolicy p;
    p.repeat = rep;
    p.groups = &got;
    p.end = true;
    p.active = act;
    p.inactive = ina;
    CHECK(check_handles(h.data(), 4, uint32_t(n), limit, p, [&](uint32_t i) { return !bad[i]; }) == rc);
    if (rc == LKF_OK) CHECK(got == want);
    (rc == LKF_OK ? ok : rc == LKF_EINVAL ? einval : eorder)++;
  }
  CHECK(ok > 50 && einval > 50 && eorder > 50);  // every outcome is exercised
}

static const struct {
  const char *name;
  void (*fn)();
} kCases[] = {
    {"handles_empty", handles_empty},
    {"handles_range", handles_range},
    {"handles_adjacent_repeat", handles_adjacent_repeat},
    {"handles_split_repeat", handles_split_repeat},
    {"handles_first_offender_wins", handles_first_offender_wins},
    {"handles_stride", handles_stride},
    {"handles_inactive_refused", handles_inactive_refused},
    {"handles_inactive_skipped", handles_inactive_skipped},
    {"handles_random", handles_random},
    {"devbuf_reserve_floor", devbuf_reserve_floor},
    {"devbuf_no_realloc", devbuf_no_realloc},
    {"devbuf_failed_grow", devbuf_failed_grow},
    {"devbuf_alloc_fixed", devbuf_alloc_fixed},
    {"devbuf_move", devbuf_move},
    {"devbuf_family_settles", devbuf_family_settles},
    {"csr_empty", csr_empty},
    {"csr_one_lane_out_of_order", csr_one_lane_out_of_order},
    {"csr_equal_at_keeps_queue_order", csr_equal_at_keeps_queue_order},
    {"csr_removed_dropped", csr_removed_dropped},
    {"csr_nl_200", csr_nl_200},
    {"csr_nl_300", csr_nl_300},
    {"csr_nl_70000", csr_nl_70000},
};

int main(int argc, char **argv) {
  if (argc > 1 && !std::strcmp(argv[1], "--list")) {
    for (auto &c : kCases) std::printf("%s\n", c.name);
    return 0;
  }
  int ran = 0;
  for (auto &c : kCases) {
    if (argc > 1 && std::strcmp(argv[1], c.name)) continue;
    const int before = g_fail;
    c.fn();
    // every case ends balanced: each allocation freed once, nothing freed twice
    CHECK(g_live.empty() && g_allocs == g_frees && g_bad_frees == 0);
    std::printf("%s %s\n", g_fail == before ? "PASS" : "FAIL", c.name);
    ran++;
  }
  if (!ran) {
    std::printf("no such case\n");
    return 2;
  }
  return g_fail ? 1 : 0;
}
