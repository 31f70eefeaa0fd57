// ctl_key_unit.cpp — CPU unit tests of the keyed control ops' host side
// (ctl_csr.h): the CSR order by (lane, key) with stable ties, where lkf_ctl
// ops at the batch start and end sort among keyed ops, the detection of a
// DownTrack whose in-batch ops are of two kinds, and the keys staged beside
// the ops.  Built with the host compiler alone (make ctl_key_unit; address +
// undefined sanitizers).
//   ctl_key_unit --list     the case names
//   ctl_key_unit <name>     one case ("PASS <name>" / exit 1)
//   ctl_key_unit            every case
#define __host__
#define __device__
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ctl_csr.h"

using namespace lkf;

static_assert(sizeof(lkf_ctl_event_key) == 56, "lkf_ctl_event_key is 56 B");
static_assert(sizeof(lkf_ctl_event) == 48, "lkf_ctl_event is 48 B");
static_assert(sizeof(DevKey) == 16, "DevKey is 16 B");

static int g_fail = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::printf("  check failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
      g_fail++;                                                    \
    }                                                              \
  } while (0)

// pend[i].ev.a[0] = i identifies an op
static CtlPend keyed(uint32_t dt, int32_t kind, int64_t key, size_t id) {
  CtlPend p;
  std::memset(&p, 0, sizeof(p));
  p.dt = dt;
  p.kind = kind;
  if (kind == LKF_AT_PKT)
    p.ev.at = uint32_t(key);
  else
    p.key = key;
  p.ev.op = LKF_CTL_MUTE;
  p.ev.a[0] = int64_t(id);
  return p;
}

static std::vector<lkf_downtrack_params> dtp_of(size_t ndt) {
  std::vector<lkf_downtrack_params> d(ndt);
  std::memset(d.data(), 0, ndt * sizeof(lkf_downtrack_params));
  for (size_t i = 0; i < ndt; i++) d[i].track = int32_t(100 + i);
  return d;
}

// The CSR against std::stable_sort by (lane, sort key); returns the op ids in CSR order.
static std::vector<int64_t> csr_check(const std::vector<CtlPend> &pend, const std::vector<int32_t> &dtLane,
                                      uint32_t nl) {
  struct Ref {
    uint32_t lane;
    int64_t key;
    size_t i;
  };
  std::vector<Ref> ref;
  for (size_t i = 0; i < pend.size(); i++)
    if (dtLane[pend[i].dt] >= 0) ref.push_back({uint32_t(dtLane[pend[i].dt]), ctl_sort_key(pend[i]), i});
  std::stable_sort(ref.begin(), ref.end(),
                   [](const Ref &a, const Ref &b) { return a.lane != b.lane ? a.lane < b.lane : a.key < b.key; });
  CtlCsr csr;
  const size_t nev = csr.sort(pend.data(), pend.size(), dtLane.data(), nl);
  CHECK(nev == ref.size());
  std::vector<DevEvent> evs(nev + 1);
  std::vector<uint32_t> lanes(nev + 1, 0xdeadbeefu);
  std::vector<DevKey> keys(nev + 1);
  std::memset(evs.data(), 0x5a, evs.size() * sizeof(DevEvent));
  std::memset(keys.data(), 0x5a, keys.size() * sizeof(DevKey));
  const std::vector<lkf_downtrack_params> dtp = dtp_of(dtLane.size());
  csr.emit(pend.data(), evs.data(), lanes.data(), keys.data(), dtp.data());
  std::vector<int64_t> ids;
  bool same = nev == ref.size();
  for (size_t i = 0; same && i < nev; i++) {
    const CtlPend &p = pend[ref[i].i];
    same = lanes[i] == ref[i].lane && evs[i].a[0] == int64_t(ref[i].i) && evs[i].at == p.ev.at &&
           keys[i].key == p.key && keys[i].kind == p.kind && keys[i].track == uint32_t(100 + p.dt);
    ids.push_back(evs[i].a[0]);
  }
  CHECK(same);
  CHECK(lanes[nev] == 0xdeadbeefu);  // nothing past the count
  CHECK(keys[nev].kind == 0x5a5a5a5a);
  return ids;
}

static void key_order_stable_ties() {
  // one lane, arrival keys queued out of order, equal keys in queue order
  std::vector<CtlPend> p;
  const int64_t k[] = {900, 100, 500, 100, 900, INT64_MIN, 500, INT64_MAX, INT64_MIN, 100};
  for (size_t i = 0; i < 10; i++) p.push_back(keyed(1, LKF_AT_ARRIVAL_NS, k[i], i));
  const std::vector<int64_t> ids = csr_check(p, {-1, 0}, 1);
  const std::vector<int64_t> want = {5, 8, 1, 3, 9, 2, 6, 0, 4, 7};
  CHECK(ids == want);
}

static void key_order_two_lanes_datagram() {
  std::vector<CtlPend> p;
  for (size_t i = 0; i < 40; i++) p.push_back(keyed(uint32_t(i % 3), LKF_AT_DATAGRAM, int64_t((i * 7) % 11), i));
  csr_check(p, {2, 0, 1}, 3);
  csr_check(p, {0, 0x1234, 300}, 0x1235);  // two radix passes
}

static void key_large_keys_not_truncated() {
  // keys that differ only above bit 32, and negative arrival times
  std::vector<CtlPend> p;
  p.push_back(keyed(0, LKF_AT_ARRIVAL_NS, (int64_t(5) << 32) + 1, 0));
  p.push_back(keyed(0, LKF_AT_ARRIVAL_NS, (int64_t(2) << 32) + 9, 1));
  p.push_back(keyed(0, LKF_AT_ARRIVAL_NS, -7, 2));
  p.push_back(keyed(0, LKF_AT_ARRIVAL_NS, int64_t(1700000000) * 1000000000, 3));
  const std::vector<int64_t> want = {2, 1, 0, 3};
  CHECK(csr_check(p, {0}, 1) == want);
}

static void pkt_start_and_end_placement() {
  // lkf_ctl ops at 0 sort below every key and at 0xffffffff above, also beside
  // the extreme arrival keys (equal sort keys: queue order)
  std::vector<CtlPend> p;
  p.push_back(keyed(0, LKF_AT_ARRIVAL_NS, 50, 0));
  p.push_back(keyed(0, LKF_AT_PKT, 0xffffffffu, 1));
  p.push_back(keyed(0, LKF_AT_ARRIVAL_NS, INT64_MAX, 2));
  p.push_back(keyed(0, LKF_AT_PKT, 0, 3));
  p.push_back(keyed(0, LKF_AT_ARRIVAL_NS, INT64_MIN, 4));
  p.push_back(keyed(0, LKF_AT_ARRIVAL_NS, -5, 5));
  p.push_back(keyed(0, LKF_AT_PKT, 0, 6));
  const std::vector<int64_t> want = {3, 4, 6, 5, 0, 1, 2};
  CHECK(csr_check(p, {0}, 1) == want);
  CtlCsr csr;
  const std::vector<int32_t> dtLane = {0};
  CHECK(csr.mixed(p.data(), p.size(), dtLane.data(), 1) < 0);  // batch start / end ops mix with any kind
  // the same with datagram keys: datagram 0 is a key of its own, above the at_pkt 0 ops
  std::vector<CtlPend> q;
  q.push_back(keyed(0, LKF_AT_DATAGRAM, 0, 0));
  q.push_back(keyed(0, LKF_AT_PKT, 0, 1));
  q.push_back(keyed(0, LKF_AT_PKT, 0xffffffffu, 2));
  q.push_back(keyed(0, LKF_AT_DATAGRAM, int64_t(1) << 40, 3));
  const std::vector<int64_t> wantq = {1, 0, 3, 2};
  CHECK(csr_check(q, {0}, 1) == wantq);
}

static void pkt_only_order_unchanged() {
  // lkf_ctl ops alone: by at_pkt, stable (what the CSR did before keys)
  std::vector<CtlPend> p;
  const uint32_t at[] = {9, 3, 7, 0, 8, 1, 1, 4, 0xffffffffu, 0, 3};
  for (size_t i = 0; i < 11; i++) p.push_back(keyed(2, LKF_AT_PKT, at[i], i));
  const std::vector<int64_t> want = {3, 9, 5, 6, 1, 10, 7, 2, 4, 0, 8};
  CHECK(csr_check(p, {-1, 0, 5, 1}, 6) == want);
}

static void mixed_kinds_detected() {
  CtlCsr csr;
  const std::vector<int32_t> dtLane = {0, 1, -1, 2};
  std::vector<CtlPend> p;
  p.push_back(keyed(0, LKF_AT_DATAGRAM, 4, 0));
  p.push_back(keyed(1, LKF_AT_ARRIVAL_NS, 4, 1));
  p.push_back(keyed(3, LKF_AT_PKT, 4, 2));
  p.push_back(keyed(0, LKF_AT_DATAGRAM, 9, 3));
  p.push_back(keyed(1, LKF_AT_PKT, 0, 4));
  p.push_back(keyed(1, LKF_AT_PKT, 0xffffffffu, 5));
  CHECK(csr.mixed(p.data(), p.size(), dtLane.data(), 4) < 0);  // one kind per DownTrack
  p.push_back(keyed(3, LKF_AT_DATAGRAM, 1, 6));  // in-batch at_pkt + datagram
  CHECK(csr.mixed(p.data(), p.size(), dtLane.data(), 4) == 3);
  p.pop_back();
  p.push_back(keyed(1, LKF_AT_DATAGRAM, 1, 6));  // arrival + datagram
  CHECK(csr.mixed(p.data(), p.size(), dtLane.data(), 4) == 1);
  p.pop_back();
  p.push_back(keyed(0, LKF_AT_PKT, 0xfffffffeu, 6));  // past any batch, but not the end marker: in-batch
  CHECK(csr.mixed(p.data(), p.size(), dtLane.data(), 4) == 0);
  p.pop_back();
  // a removed DownTrack's ops are dropped, so they do not count
  p.push_back(keyed(2, LKF_AT_DATAGRAM, 1, 6));
  p.push_back(keyed(2, LKF_AT_ARRIVAL_NS, 1, 7));
  CHECK(csr.mixed(p.data(), p.size(), dtLane.data(), 4) < 0);
  CHECK(csr.mixed(nullptr, 0, dtLane.data(), 4) < 0);
}

static void removed_dropped() {
  std::vector<CtlPend> p;
  for (size_t i = 0; i < 20; i++) p.push_back(keyed(uint32_t(i % 4), LKF_AT_ARRIVAL_NS, int64_t(20 - i), i));
  const std::vector<int64_t> ids = csr_check(p, {3, -1, 0, -1}, 4);
  CHECK(ids.size() == 10);
  for (int64_t id : ids) CHECK(id % 4 == 0 || id % 4 == 2);
  CHECK(csr_check(p, {-1, -1, -1, -1}, 4).empty());  // every op dropped
}

static void random_against_stable_sort() {
  uint32_t st = 12345;
  auto rnd = [&]() { return st = st * 1664525u + 1013904223u, st >> 8; };
  for (uint32_t nl : {7u, 300u, 70000u}) {
    std::vector<int32_t> dtLane(nl);
    for (uint32_t d = 0; d < nl; d++) dtLane[d] = (d % 9 == 4) ? -1 : int32_t(nl - 1 - d);
    std::vector<CtlPend> p;
    for (size_t i = 0; i < 600; i++) {
      const uint32_t dt = (rnd() & 1) ? rnd() % 5 : rnd() % nl;
      const uint32_t r = rnd() % 10;
      if (r == 0)
        p.push_back(keyed(dt, LKF_AT_PKT, 0, i));
      else if (r == 1)
        p.push_back(keyed(dt, LKF_AT_PKT, 0xffffffffu, i));
      else
        p.push_back(keyed(dt, LKF_AT_ARRIVAL_NS, int64_t(rnd() % 8) * 1000000007 - 3000000000, i));
    }
    csr_check(p, dtLane, nl);
  }
}

static const struct {
  const char *name;
  void (*fn)();
} kCases[] = {
    {"key_order_stable_ties", key_order_stable_ties},
    {"key_order_two_lanes_datagram", key_order_two_lanes_datagram},
    {"key_large_keys_not_truncated", key_large_keys_not_truncated},
    {"pkt_start_and_end_placement", pkt_start_and_end_placement},
    {"pkt_only_order_unchanged", pkt_only_order_unchanged},
    {"mixed_kinds_detected", mixed_kinds_detected},
    {"removed_dropped", removed_dropped},
    {"random_against_stable_sort", random_against_stable_sort},
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
    std::printf("%s %s\n", g_fail == before ? "PASS" : "FAIL", c.name);
    ran++;
  }
  if (!ran) {
    std::printf("no such case\n");
    return 2;
  }
  return g_fail ? 1 : 0;
}
