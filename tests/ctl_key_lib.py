"""Shared pieces of the keyed control-op tests (tests/test_ctl_key_gpu.py).

A raw batch with repeated datagrams (every datagram i % 5 == 2 sent twice:
the copy is a duplicate that yields no ExtPacket), the op lists keyed on it,
and the oracle side: the oracle has no keyed entry points, so each key is
translated on the host — through orc_ingest_flows' flow.pkt per datagram — to
the ExtPacket index the engine must resolve it to, and fed to orc_ctl_batch.
"""
import ctypes as C

import numpy as np

END = 0xFFFFFFFF
I64MIN, I64MAX = -(1 << 63), (1 << 63) - 1
MUTE = 1  # LKF_CTL_MUTE


class RawBatch:
    """Batch b of `tr` as raw datagrams, with every datagram i % 5 == 2
    repeated right after itself when `repeats`."""

    def __init__(self, tr, abi, b, repeats=True):
        rp, n, self.ar, self.alen = tr.batch_raw(b)
        rows, self.newidx, self.copies = [], [], []
        for i in range(n):
            self.newidx.append(len(rows))
            rows.append(i)
            if repeats and i % 5 == 2:
                self.copies.append(len(rows))
                rows.append(i)
        self.n0, self.n = n, len(rows)
        self.raws = (abi.lkf_raw_pkt * max(1, self.n))()
        for j, i in enumerate(rows):
            r = self.raws[j]
            r.arrival_ns, r.stream, r.off, r.len = rp[i].arrival_ns, rp[i].stream, rp[i].off, rp[i].len
        self.arrival = np.array([self.raws[j].arrival_ns for j in range(self.n)], dtype=np.int64)
        self.track = np.array([tr.streams[self.raws[j].stream].track for j in range(self.n)], dtype=np.int64)
        self.ranges = {}  # track -> [lo, hi) of its datagrams (grouped by track)
        for j in range(self.n):
            t = int(self.track[j])
            if t not in self.ranges:
                self.ranges[t] = [j, j + 1]
            else:
                assert self.ranges[t][1] == j, "raw batch not grouped by track"
                self.ranges[t][1] = j + 1
        for lo, hi in self.ranges.values():  # the batch contract the arrival key relies on
            assert np.all(np.diff(self.arrival[lo:hi]) >= 0), "arrivals decrease within a track"

    def remap(self, at_pkt):
        """A scripted at_pkt (index into the trace's own batch) as a datagram index here."""
        return self.newidx[at_pkt] if at_pkt < self.n0 else min(END, self.n + (at_pkt - self.n0))


def scripted_ops(tr, rb, b):
    """Batch b's scripted events, positions remapped through the insertion: (dt, op, a, datagram)."""
    return [(e.dt, e.op, tuple(e.a), rb.remap(e.at_pkt)) for e in tr.events(b)]


def strictly_inside(tr, rb, ops):
    n = 0
    for dt, _, _, d in ops:
        lo, hi = rb.ranges.get(tr.downtracks[dt].track, (0, 0))
        n += int(lo < d < hi)
    return n


def extra_mutes(tr, rb):
    """Every seventh DownTrack: MUTE(1,1) keyed on a repeated copy about a third
    into its track's range and MUTE(0,1) on one about two thirds in."""
    out = []
    copies = np.array(rb.copies, dtype=np.int64)
    for dt in range(0, tr.ndts, 7):
        lo, hi = rb.ranges.get(tr.downtracks[dt].track, (0, 0))
        mine = copies[(copies >= lo) & (copies < hi)]
        if len(mine) < 2:
            continue
        c1 = int(mine[np.searchsorted(mine, lo + (hi - lo) // 3).clip(0, len(mine) - 1)])
        c2 = int(mine[np.searchsorted(mine, lo + 2 * (hi - lo) // 3).clip(0, len(mine) - 1)])
        out.append((dt, MUTE, (1, 1, 0, 0), c1))
        out.append((dt, MUTE, (0, 1, 0, 0), c2))
    return out


def reversed_pair(tr, rb, dt):
    """Two ops queued in reversed key order whose keys — the datagram after a
    copy, then the copy — resolve to the same ExtPacket: in key order the
    DownTrack ends up muted, in queue order it would not."""
    lo, hi = rb.ranges.get(tr.downtracks[dt].track, (0, 0))
    mine = [c for c in rb.copies if lo < c < hi - 2]
    if not mine:
        return []
    c = mine[len(mine) // 2]
    return [(dt, MUTE, (1, 1, 0, 0), c + 1), (dt, MUTE, (0, 1, 0, 0), c)]


def to_arrival(rb, ops):
    """(dt, op, a, datagram) -> (dt, op, a, T): the datagram's arrival time, INT64_MAX past the batch."""
    return [(dt, op, a, int(rb.arrival[d]) if d < rb.n else I64MAX) for dt, op, a, d in ops]


def key_array(abi, ops, kind):
    arr = (abi.lkf_ctl_event_key * max(1, len(ops)))()
    for i, (dt, op, a, key) in enumerate(ops):
        arr[i].dt, arr[i].op, arr[i].kind, arr[i].key = dt, op, kind, key
        for j in range(4):
            arr[i].a[j] = a[j]
    return arr


def queue_keyed(eng, abi, ops, kind):
    if ops:
        assert eng.api["ctl_batch_key"](eng.h, C.cast(key_array(abi, ops, kind), C.c_void_p), len(ops)) == 0


def scan_of(flows):
    """Per datagram: the number of earlier datagrams that produced an ExtPacket."""
    has = (flows["pkt"] != END).astype(np.int64)
    return np.concatenate([[0], np.cumsum(has)])[:len(has)]


def resolve_datagram(scan, n, key):
    return int(scan[key]) if key < n else END


def resolve_arrival(arrival, rng, scan, T):
    """First datagram of the track's range [lo, hi) with arrival >= T, then the scan (scan None: the
    datagrams are the ExtPackets)."""
    lo, hi = rng
    j = lo + int(np.searchsorted(arrival[lo:hi], T, side="left"))
    if j >= hi:
        return END
    return j if scan is None else int(scan[j])


def queue_oracle(o, oh, abi, ops, resolve):
    """The oracle's form of a keyed op list: stable-sorted by key (the oracle
    orders equal at_pkt by queue order), each key resolved to its index."""
    ops = sorted(ops, key=lambda x: x[3])
    arr = (abi.lkfs_event * max(1, len(ops)))()
    for i, (dt, op, a, key) in enumerate(ops):
        arr[i].dt, arr[i].op, arr[i].at_pkt = dt, op, resolve(dt, key)
        for j in range(4):
            arr[i].a[j] = a[j]
    if ops:
        assert o.api["ctl_batch"](oh, C.cast(arr, C.c_void_p), len(ops)) == 0
    return [arr[i].at_pkt for i in range(len(ops))]


def oracle_ingest(o, oh, abi, pkg, rb):
    """orc_ingest of the raw batch -> (flows, ExtPacket array, count)."""
    assert o.api["ingest"](oh, rb.raws, rb.n, rb.ar, rb.alen) == 0
    flows = pkg.flows_array(o.api, oh)
    k = C.c_uint32()
    assert o.api["ingested"](oh, None, 0, C.byref(k)) in (0, -28)
    pk = (abi.lkf_pkt * max(1, k.value))()
    assert o.api["ingested"](oh, pk, k.value, C.byref(k)) == 0
    return flows, pk, k.value


def oracle_result(o, oh, abi, pkg):
    st = abi.lkf_stats()
    assert o.api["get_stats"](oh, C.byref(st)) == 0
    rec, ar = pkg.drain_arrays(o.api, oh)
    return st.as_dict(), rec, ar


def assert_same(abi, b, got, want):
    (gs, grec, gar), (os_, orec, oar) = got, want
    if gs is not None:
        assert gs == os_, (b, gs, os_)
    assert len(grec) == len(orec), (b, len(grec), len(orec))
    for f in abi.OUT_DTYPE.names:
        if not np.array_equal(grec[f], orec[f]):
            bad = np.nonzero(grec[f] != orec[f])[0][:5]
            raise AssertionError("batch %d field %s differs at %s: gpu %s orc %s" % (b, f, bad, grec[bad], orec[bad]))
    assert np.array_equal(gar, oar), b
