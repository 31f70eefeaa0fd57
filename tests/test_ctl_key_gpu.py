"""Control ops keyed by datagram index or arrival time (lkf_ctl_key*), engine vs oracle.

On the ingest path (lkf_ingest* + lkf_run) the ExtPacket batch is made on the
GPU, so a caller names the point a control call preceded as a datagram index
of its raw batch or as a time on the arrival clock; the engine resolves either
to an ExtPacket index on the device (k_ev_resolve).  The oracle has no such
entry points: each test translates the keys on the host, through the oracle's
own per-datagram flow records, and feeds orc_ctl_batch the indices.  Stats,
every lkf_out field, every arena byte and the exported Forwarder state of
every DownTrack must be identical.

The raw batches carry a repeated copy of every datagram i % 5 == 2 (about 330
duplicates per batch, none of which yields an ExtPacket), so that a datagram
index and an ExtPacket index differ by hundreds at the end of a batch.
"""
import ctypes as C

import numpy as np
import pytest

from tests import ctl_key_lib as K
from tests.oracle_lib import load as load_oracle
from tests.test_parity_gpu import _state_tuple

pytestmark = pytest.mark.gpu

DROP_MUTED = 0  # lkf_drop: muted || pubMuted
SHAPE = dict(duration_s=2.0, batch_s=0.5, rooms=1, loss=0.05, reorder=0.03, seed=21)


@pytest.fixture(scope="module")
def trace(workload):
    tr = workload.Trace(2, **SHAPE)
    assert (tr.ntracks, tr.ndts, tr.nstreams) == (20, 180, 40)
    yield tr
    tr.close()


@pytest.fixture(scope="module")
def batches(trace, abi):
    return [K.RawBatch(trace, abi, b) for b in range(trace.nbatches)]


def _ops_datagram(tr, rb, b):
    """Batch b's ops as (dt, op, a, datagram), in queue order."""
    return K.scripted_ops(tr, rb, b) + K.extra_mutes(tr, rb) + K.reversed_pair(tr, rb, 1)


def _ops_arrival(tr, rb, b):
    """The same ops keyed by the arrival time of their datagram, plus ops at
    -infinity, +infinity and at an arrival a datagram shares with its copy."""
    ops = K.to_arrival(rb, _ops_datagram(tr, rb, b))
    for dt in range(3, tr.ndts, 11):
        lo, hi = rb.ranges.get(tr.downtracks[dt].track, (0, 0))
        mine = [c for c in rb.copies if lo <= c < hi]
        ops.append((dt, K.MUTE, (1, 1, 0, 0), K.I64MIN))
        if mine:
            ops.append((dt, K.MUTE, (0, 1, 0, 0), int(rb.arrival[mine[len(mine) // 2]])))
        ops.append((dt, K.MUTE, (dt % 2, 1, 0, 0), K.I64MAX))
    return ops


def _new(pkg, workload, o, tr, norc=1, streams=True):
    eng = pkg.Engine.for_trace(tr, headroom=1.5)
    ohs = [o.create(500) for _ in range(norc)]
    for api, h in [(eng.api, eng.h)] + [(o.api, oh) for oh in ohs]:
        workload.load_topology(api, h, tr)
        if streams:
            workload.load_streams(api, h, tr)
    return eng, ohs


def _oracle_batch(o, oh, abi, pkg, tr, rb, ops, kind, check_copies=True):
    """The oracle's ingest + run of one raw batch with `ops` (keys of `kind`) -> (stats, records, arena)."""
    flows, pk, k = K.oracle_ingest(o, oh, abi, pkg, rb)
    if check_copies:  # the condition the tests stand on: every inserted copy is a duplicate without an ExtPacket
        assert np.all(flows["pkt"][np.array(rb.copies, dtype=np.int64)] == K.END)
        assert len(rb.copies) >= 300 or rb.n0 < 1500, len(rb.copies)
    scan = K.scan_of(flows)
    if kind == abi.LKF_AT_DATAGRAM:
        at = K.queue_oracle(o, oh, abi, ops, lambda dt, key: K.resolve_datagram(scan, rb.n, key))
    else:
        at = K.queue_oracle(o, oh, abi, ops, lambda dt, key: K.resolve_arrival(
            rb.arrival, rb.ranges.get(tr.downtracks[dt].track, (0, 0)), scan, key))
    o.run(oh, pk if k else None, k, rb.ar, rb.alen)
    return K.oracle_result(o, oh, abi, pkg), at


def _at_zero(o, oh, abi, pkg, rb, ops):
    """The same ops all at index 0 (what a caller without keys had to do) -> forwarded."""
    _, pk, k = K.oracle_ingest(o, oh, abi, pkg, rb)
    K.queue_oracle(o, oh, abi, ops, lambda dt, key: 0)
    o.run(oh, pk if k else None, k, rb.ar, rb.alen)
    return K.oracle_result(o, oh, abi, pkg)[0]["forwarded"]


def _states_equal(eng, o, oh, abi, tr):
    for d in range(tr.ndts):
        assert _state_tuple(eng.api, eng.h, d, abi) == _state_tuple(o.api, oh, d, abi), d


@pytest.mark.parametrize("queue_first", [True, False], ids=["ops_before_ingest", "ops_after_ingest"])
def test_datagram_keys_host_ingest(pkg, workload, abi, trace, batches, queue_first):
    tr, o = trace, load_oracle()
    eng, (oh, oh0) = _new(pkg, workload, o, tr, norc=2)
    try:
        fwd = fwd0 = inside = 0
        resolved_gap = 0
        for b, rb in enumerate(batches):
            ops = _ops_datagram(tr, rb, b)
            inside += K.strictly_inside(tr, rb, K.scripted_ops(tr, rb, b))
            if queue_first:
                K.queue_keyed(eng, abi, ops, abi.LKF_AT_DATAGRAM)
            eng.ingest(rb.raws, rb.n, rb.ar, rb.alen)
            if not queue_first:
                K.queue_keyed(eng, abi, ops, abi.LKF_AT_DATAGRAM)
            eng.run()
            eng.sync()
            want, at = _oracle_batch(o, oh, abi, pkg, tr, rb, ops, abi.LKF_AT_DATAGRAM)
            keys = sorted(k for _, _, _, k in ops)
            resolved_gap = max([resolved_gap] + [k - a for k, a in zip(keys, at) if k < rb.n])
            K.assert_same(abi, b, (eng.stats(),) + eng.drain(), want)
            fwd += want[0]["forwarded"]
            fwd0 += _at_zero(o, oh0, abi, pkg, rb, ops)
        assert inside == 95  # scripted ops strictly inside their track's range
        assert resolved_gap > 100  # a datagram index and its ExtPacket index are far apart
        assert fwd > 0 and fwd != fwd0, "the ops' positions did not matter"
        _states_equal(eng, o, oh, abi, tr)
    finally:
        eng.close()
        o.destroy(oh)
        o.destroy(oh0)


def test_arrival_keys_host_ingest(pkg, workload, abi, trace, batches):
    tr, o = trace, load_oracle()
    eng, (oh,) = _new(pkg, workload, o, tr)
    try:
        fwd = 0
        for b, rb in enumerate(batches):
            ops = _ops_arrival(tr, rb, b)
            K.queue_keyed(eng, abi, ops, abi.LKF_AT_ARRIVAL_NS)
            eng.ingest(rb.raws, rb.n, rb.ar, rb.alen)
            eng.run()
            eng.sync()
            want, _ = _oracle_batch(o, oh, abi, pkg, tr, rb, ops, abi.LKF_AT_ARRIVAL_NS)
            K.assert_same(abi, b, (eng.stats(),) + eng.drain(), want)
            fwd += want[0]["forwarded"]
        assert fwd > 0
        _states_equal(eng, o, oh, abi, tr)
    finally:
        eng.close()
        o.destroy(oh)


def test_datagram_keys_pipelined_ingest_device(pkg, workload, abi, trace, batches):
    """lkf_ingest_device, lkf_run, lkf_ingest_device, ... with no sync: the
    next ingest overwrites the scan the previous run's resolver reads."""
    import torch

    tr, o = trace, load_oracle()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    eng, (oh,) = _new(pkg, workload, o, tr)
    try:
        nb = 3
        rsz = C.sizeof(abi.lkf_raw_pkt)
        dpk, dar = [], []
        for rb in batches[:nb]:
            dpk.append(torch.frombuffer(bytearray(C.string_at(rb.raws, rb.n * rsz)), dtype=torch.uint8).to(dev))
            ta = torch.zeros(rb.alen + 64, dtype=torch.uint8, device=dev)
            ta[:rb.alen].copy_(torch.frombuffer(bytearray(C.string_at(rb.ar, rb.alen)), dtype=torch.uint8))
            dar.append(ta)
        torch.cuda.synchronize(dev)
        sp = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        allops = [_ops_datagram(tr, rb, b) for b, rb in enumerate(batches[:nb])]
        for b, rb in enumerate(batches[:nb]):
            K.queue_keyed(eng, abi, allops[b], abi.LKF_AT_DATAGRAM)
            eng.ingest_device(C.c_void_p(dpk[b].data_ptr()), rb.n, C.c_void_p(dar[b].data_ptr()), rb.alen)
            eng.run(sp)
        want = [_oracle_batch(o, oh, abi, pkg, tr, rb, allops[b], abi.LKF_AT_DATAGRAM)[0]
                for b, rb in enumerate(batches[:nb])]
        eng.sync()
        cap = int(tr.max_batch_tuples * 1.5) + 1024
        acap = int(tr.max_batch_out_bytes * 1.5) + (1 << 20)
        for age in range(nb):
            b = nb - 1 - age
            out = np.zeros(cap, dtype=abi.OUT_DTYPE)
            ar = np.zeros(acap, dtype=np.uint8)
            n, nbytes = eng.drain_run_into(age, C.c_void_p(out.ctypes.data), cap, C.c_void_p(ar.ctypes.data), acap)
            K.assert_same(abi, b, (None, out[:n], ar[:nbytes]), want[b])
        _states_equal(eng, o, oh, abi, tr)
    finally:
        eng.close()
        o.destroy(oh)


def test_empty_ingest_applies_keyed_ops_at_batch_end(pkg, workload, abi, trace, batches):
    tr, o = trace, load_oracle()
    eng, (oh,) = _new(pkg, workload, o, tr)
    try:
        rb0, rb1 = batches[0], batches[1]
        # batch 0 as usual
        ops = _ops_datagram(tr, rb0, 0)
        K.queue_keyed(eng, abi, ops, abi.LKF_AT_DATAGRAM)
        eng.ingest(rb0.raws, rb0.n, rb0.ar, rb0.alen)
        eng.run()
        eng.sync()
        K.assert_same(abi, 0, (eng.stats(),) + eng.drain(),
                      _oracle_batch(o, oh, abi, pkg, tr, rb0, ops, abi.LKF_AT_DATAGRAM)[0])
        # an empty ingest with keyed ops queued (datagram 0 is already past it): they apply at batch end
        mutes = [(dt, K.MUTE, (1, 1, 0, 0), 0) for dt in range(2, tr.ndts, 5)]
        mutes += [(dt, K.MUTE, (0, 1, 0, 0), 7) for dt in range(2, tr.ndts, 10)]
        K.queue_keyed(eng, abi, mutes, abi.LKF_AT_DATAGRAM)
        eng.ingest(rb0.raws, 0, rb0.ar, 0)
        eng.run()
        eng.sync()
        assert o.api["ingest"](oh, rb0.raws, 0, rb0.ar, 0) == 0
        K.queue_oracle(o, oh, abi, mutes, lambda dt, key: K.END)
        o.run(oh, None, 0, rb0.ar, rb0.alen)
        assert len(eng.drain()[0]) == 0
        # the next batch sees their effect
        ops = _ops_datagram(tr, rb1, 1)
        K.queue_keyed(eng, abi, ops, abi.LKF_AT_DATAGRAM)
        eng.ingest(rb1.raws, rb1.n, rb1.ar, rb1.alen)
        eng.run()
        eng.sync()
        want, _ = _oracle_batch(o, oh, abi, pkg, tr, rb1, ops, abi.LKF_AT_DATAGRAM)
        K.assert_same(abi, 1, (eng.stats(),) + eng.drain(), want)
        assert want[0]["drops"][DROP_MUTED] > 0
        _states_equal(eng, o, oh, abi, tr)
    finally:
        eng.close()
        o.destroy(oh)


def test_submitted_batch(pkg, workload, abi, trace):
    """lkf_submit of the trace's own ExtPacket batches: arrival keys against
    the index computed from the packets' arrival_ns, and in one batch datagram
    keys, which on a submitted batch are the ExtPacket indices themselves."""
    tr, o = trace, load_oracle()
    eng, (oh,) = _new(pkg, workload, o, tr, streams=False)
    try:
        fwd = 0
        for b in range(tr.nbatches):
            pk, n, ar, alen = tr.batch(b)
            arrival = np.array([pk[i].arrival_ns for i in range(n)], dtype=np.int64)
            ranges = {}
            for i in range(n):
                ranges.setdefault(pk[i].track, [i, i])[1] = i + 1
            script = [(e.dt, e.op, tuple(e.a), e.at_pkt) for e in tr.events(b)]
            if b == 1:
                kind = abi.LKF_AT_DATAGRAM
                ops = script
                resolve = lambda dt, key: key  # noqa: E731
            else:
                kind = abi.LKF_AT_ARRIVAL_NS
                ops = [(dt, op, a, int(arrival[d]) if d < n else K.I64MAX) for dt, op, a, d in script]
                ops += [(dt, K.MUTE, (1, 1, 0, 0), K.I64MIN) for dt in range(4, tr.ndts, 13)]
                ops += [(dt, K.MUTE, (0, 1, 0, 0), int(arrival[n // 2])) for dt in range(4, tr.ndts, 13)]
                resolve = lambda dt, key: K.resolve_arrival(  # noqa: E731
                    arrival, ranges.get(tr.downtracks[dt].track, (0, 0)), None, key)
            K.queue_keyed(eng, abi, ops, kind)
            eng.submit(pk, n, ar, alen)
            eng.run()
            eng.sync()
            K.queue_oracle(o, oh, abi, ops, resolve)
            o.run(oh, pk, n, ar, alen)
            want = K.oracle_result(o, oh, abi, pkg)
            K.assert_same(abi, b, (eng.stats(),) + eng.drain(), want)
            fwd += want[0]["forwarded"]
        assert fwd > 0
        _states_equal(eng, o, oh, abi, tr)
    finally:
        eng.close()
        o.destroy(oh)


@pytest.mark.parametrize("kind_name", ["datagram", "arrival"])
def test_svc_decide(pkg, workload, abi, kind_name):
    """Config 5 (VP9 / AV1 SVC with dependency descriptors, k_decide_dt<true>).
    Its raw batch is not the packet list one to one, so every scripted op is
    placed at offset at_pkt mod L into its track's L datagrams."""
    kind = abi.LKF_AT_DATAGRAM if kind_name == "datagram" else abi.LKF_AT_ARRIVAL_NS
    tr = workload.Trace(5, duration_s=2.0, batch_s=0.5, rooms=2, loss=0.05, reorder=0.03, seed=43)
    o = load_oracle()
    eng, (oh,) = _new(pkg, workload, o, tr)
    try:
        fwd = nops = 0
        for b in range(tr.nbatches):
            rb = K.RawBatch(tr, abi, b)
            ops = []
            for e in tr.events(b):
                lo, hi = rb.ranges.get(tr.downtracks[e.dt].track, (0, 0))
                ops.append((e.dt, e.op, tuple(e.a), lo + e.at_pkt % (hi - lo) if hi > lo else rb.n))
            if kind == abi.LKF_AT_ARRIVAL_NS:
                ops = K.to_arrival(rb, ops)
            nops += len(ops)
            K.queue_keyed(eng, abi, ops, kind)
            eng.ingest(rb.raws, rb.n, rb.ar, rb.alen)
            eng.run()
            eng.sync()
            want, _ = _oracle_batch(o, oh, abi, pkg, tr, rb, ops, kind, check_copies=False)
            K.assert_same(abi, b, (eng.stats(),) + eng.drain(), want)
            fwd += want[0]["forwarded"]
        assert fwd > 0 and nops > 0
        _states_equal(eng, o, oh, abi, tr)
    finally:
        eng.close()
        o.destroy(oh)
        tr.close()


@pytest.mark.parametrize("kind_name", ["datagram", "arrival"])
def test_workload_queue_events_keyed(pkg, workload, abi, trace, kind_name):
    """workload.queue_events_keyed on the trace as generated (raw batch = packet
    list one to one, no repeats): the scripted ops by datagram index or by
    arrival time, against the oracle at the index each key stands for."""
    kind = abi.LKF_AT_DATAGRAM if kind_name == "datagram" else abi.LKF_AT_ARRIVAL_NS
    tr, o = trace, load_oracle()
    eng, (oh,) = _new(pkg, workload, o, tr)
    try:
        fwd = 0
        for b in range(tr.nbatches):
            rb = K.RawBatch(tr, abi, b, repeats=False)
            workload.queue_events_keyed(eng.api, eng.h, tr, b, kind)
            eng.ingest(rb.raws, rb.n, rb.ar, rb.alen)
            eng.run()
            eng.sync()
            ev, n = workload.events_keyed(tr, b, kind)
            ops = [(ev[i].dt, ev[i].op, tuple(ev[i].a), ev[i].key) for i in range(n)]
            want, _ = _oracle_batch(o, oh, abi, pkg, tr, rb, ops, kind, check_copies=False)
            K.assert_same(abi, b, (eng.stats(),) + eng.drain(), want)
            fwd += want[0]["forwarded"]
        assert fwd > 0
        _states_equal(eng, o, oh, abi, tr)
    finally:
        eng.close()
        o.destroy(oh)


def _reports(tr, b, pk, n, rng):
    """(track, layer, ntp, rtp, at) for batch b: at inside the track's own packets."""
    ranges = {}
    for i in range(n):
        ranges.setdefault(pk[i].track, [i, i])[1] = i + 1
    out = []
    for t in range(tr.ntracks):
        p = tr.tracks[t]
        if p.kind != 1 or not p.has_ref_ts or t not in ranges:
            continue
        base = ((3_900_000_000 + b) << 32) + int(rng.integers(0, 1 << 31))
        x = int(rng.integers(0, 1 << 32))
        for layer in range(3):
            if rng.random() < 0.3:
                continue
            frac = int(rng.integers(0, 1 << 30))
            rtp = (x - int(p.layer_offsets[0][layer]) + frac * 90000 // (1 << 32) +
                   int(rng.integers(-400, 400))) & 0xFFFFFFFF
            out.append((t, layer, base + frac, rtp, int(rng.integers(ranges[t][0], ranges[t][1]))))
    return out, ranges


def test_sender_reports_by_arrival(pkg, workload, abi):
    """tests/test_layer_offsets_gpu.py's set-up with the reports keyed by
    arrival time (lkf_sender_report_key) and one lkf_set_layer_offsets_key."""
    tr = workload.Trace(2, duration_s=3.0, batch_s=1.0, rooms=2, seed=77)
    o = load_oracle()
    eng, (oh, oh0) = _new(pkg, workload, o, tr, norc=2, streams=False)
    try:
        rng = np.random.default_rng(9)
        differs = nrep = 0
        for b in range(tr.nbatches):
            pk, n, ar, alen = tr.batch(b)
            arrival = np.array([pk[i].arrival_ns for i in range(n)], dtype=np.int64)
            reps, ranges = _reports(tr, b, pk, n, rng)
            nrep += len(reps)

            def resolve_t(t, T):
                return K.resolve_arrival(arrival, ranges.get(t, (0, 0)), None, T)

            # scripted ops by arrival time too: one DownTrack holds one kind of in-batch position per run
            script = [(e.dt, e.op, tuple(e.a), int(arrival[e.at_pkt]) if e.at_pkt < n else K.I64MAX)
                      for e in tr.events(b)]
            K.queue_keyed(eng, abi, script, abi.LKF_AT_ARRIVAL_NS)
            for h in (oh, oh0):
                K.queue_oracle(o, h, abi, script, lambda dt, T: resolve_t(tr.downtracks[dt].track, T))
            for t, layer, ntp, rtp, at in sorted(reps, key=lambda r: int(arrival[r[4]])):  # (stable, by key)
                T = int(arrival[at])
                assert eng.api["sender_report_key"](eng.h, t, layer, ntp, rtp, abi.LKF_AT_ARRIVAL_NS, T) == 0
                assert o.api["sender_report"](oh, t, layer, ntp, rtp, resolve_t(t, T)) == 0
            if b == 1:  # a whole table from a time inside the batch
                t = next(t for t in range(tr.ntracks) if tr.tracks[t].kind == 1 and t in ranges)
                tab = (C.c_uint32 * 9)(*[(int(tr.tracks[t].layer_offsets[r][l]) + 7 * (r - l)) & 0xFFFFFFFF
                                         for r in range(3) for l in range(3)])
                T = int(arrival[(ranges[t][0] + ranges[t][1]) // 2])
                assert eng.api["set_layer_offsets_key"](eng.h, t, tab, abi.LKF_AT_ARRIVAL_NS, T) == 0
                assert o.api["set_layer_offsets_at"](oh, t, tab, resolve_t(t, T)) == 0
            eng.submit(pk, n, ar, alen)
            eng.run()
            eng.sync()
            o.run(oh, pk, n, ar, alen)
            o.run(oh0, pk, n, ar, alen)
            want = K.oracle_result(o, oh, abi, pkg)
            _, zrec, _ = K.oracle_result(o, oh0, abi, pkg)
            K.assert_same(abi, b, (eng.stats(),) + eng.drain(), want)
            differs += int(len(zrec) != len(want[1]) or not np.array_equal(zrec["ext_ts"], want[1]["ext_ts"]))
        assert nrep > 0
        assert differs > 0, "the reports changed nothing: no switch read the new offsets"
        _states_equal(eng, o, oh, abi, tr)
    finally:
        eng.close()
        o.destroy(oh)
        o.destroy(oh0)


def test_mixed_kinds_refused_and_batch_kept(pkg, workload, abi, trace, batches):
    tr, o = trace, load_oracle()
    eng, (oh,) = _new(pkg, workload, o, tr)
    try:
        rb = batches[0]
        lo, hi = rb.ranges[tr.downtracks[5].track]
        eng.ingest(rb.raws, rb.n, rb.ar, rb.alen)
        assert eng.api["ctl_key"](eng.h, 5, K.MUTE, 1, 1, 0, 0, abi.LKF_AT_DATAGRAM, (lo + hi) // 2) == 0
        assert eng.api["ctl"](eng.h, 5, K.MUTE, 0, 1, 0, 0, 3) == 0  # in-batch at_pkt on the same DownTrack
        assert eng.api["ctl_key"](eng.h, 9, K.MUTE, 1, 1, 0, 0, abi.LKF_AT_DATAGRAM, 0) == 0
        assert eng.lib.lkf_run(eng.h, None) == -22  # LKF_EINVAL, nothing enqueued
        msg = eng.lib.lkf_last_error(eng.h).decode()
        assert msg and "5" in msg, msg
        # the ops are dropped, the batch is still there: a second run forwards it without them
        eng.run()
        eng.sync()
        want, _ = _oracle_batch(o, oh, abi, pkg, tr, rb, [], abi.LKF_AT_DATAGRAM)
        K.assert_same(abi, 0, (eng.stats(),) + eng.drain(), want)
        assert want[0]["forwarded"] > 0
        # keyed ops beside at_pkt 0 and 0xffffffff ops on the same DownTracks are no mix
        rb = batches[1]
        lo, hi = rb.ranges[tr.downtracks[5].track]
        mid = (lo + hi) // 2
        eng.ingest(rb.raws, rb.n, rb.ar, rb.alen)
        assert eng.api["ctl"](eng.h, 5, K.MUTE, 0, 1, 0, 0, K.END) == 0
        assert eng.api["ctl_key"](eng.h, 5, K.MUTE, 1, 1, 0, 0, abi.LKF_AT_DATAGRAM, mid) == 0
        assert eng.api["ctl"](eng.h, 5, K.MUTE, 0, 1, 0, 0, 0) == 0
        assert eng.api["ctl"](eng.h, 6, K.MUTE, 1, 1, 0, 0, 0) == 0
        lo6, hi6 = rb.ranges[tr.downtracks[6].track]
        t6 = int(rb.arrival[(lo6 + hi6) // 2])
        assert eng.api["ctl_key"](eng.h, 6, K.MUTE, 0, 1, 0, 0, abi.LKF_AT_ARRIVAL_NS, t6) == 0
        eng.run()
        eng.sync()
        flows, pk, k = K.oracle_ingest(o, oh, abi, pkg, rb)
        scan = K.scan_of(flows)
        r = K.resolve_datagram(scan, rb.n, mid)
        for dt, muted, at in ((5, 0, 0), (5, 1, r), (5, 0, K.END), (6, 1, 0),
                              (6, 0, K.resolve_arrival(rb.arrival, (lo6, hi6), scan, t6))):
            assert o.api["ctl"](oh, dt, K.MUTE, muted, 1, 0, 0, at) == 0
        o.run(oh, pk, k, rb.ar, rb.alen)
        want = K.oracle_result(o, oh, abi, pkg)
        K.assert_same(abi, 1, (eng.stats(),) + eng.drain(), want)
        assert want[0]["drops"][DROP_MUTED] > 0
        _states_equal(eng, o, oh, abi, tr)
    finally:
        eng.close()
        o.destroy(oh)


def test_bad_arguments_refused_at_the_call(pkg, workload, abi, trace):
    tr, o = trace, load_oracle()
    eng, ohs = _new(pkg, workload, o, tr, norc=0, streams=False)
    try:
        ck = eng.api["ctl_key"]
        assert ck(eng.h, 0, K.MUTE, 1, 1, 0, 0, 3, 0) == -22  # unknown kind
        assert ck(eng.h, 0, K.MUTE, 1, 1, 0, 0, -1, 0) == -22
        assert ck(eng.h, tr.ndts, K.MUTE, 1, 1, 0, 0, abi.LKF_AT_DATAGRAM, 0) == -22  # bad DownTrack
        assert ck(eng.h, 0, 99, 1, 1, 0, 0, abi.LKF_AT_DATAGRAM, 0) == -22  # bad op
        assert ck(eng.h, 0, K.MUTE, 1, 1, 0, 0, abi.LKF_AT_DATAGRAM, -1) == -22  # negative datagram key
        assert ck(eng.h, 0, K.MUTE, 1, 1, 0, 0, abi.LKF_AT_ARRIVAL_NS, -1) == 0  # (a time may be negative)
        bad = K.key_array(abi, [(0, K.MUTE, (1, 1, 0, 0), 4), (0, K.MUTE, (1, 1, 0, 0), -4)], abi.LKF_AT_DATAGRAM)
        assert eng.api["ctl_batch_key"](eng.h, C.cast(bad, C.c_void_p), 2) == -22
        tab = (C.c_uint32 * 9)(*range(9))
        assert eng.api["sender_report_key"](eng.h, tr.ntracks, 0, 1, 1, abi.LKF_AT_ARRIVAL_NS, 0) == -22
        assert eng.api["sender_report_key"](eng.h, 0, 0, 1, 1, 5, 0) == -22
        assert eng.api["set_layer_offsets_key"](eng.h, 0, tab, abi.LKF_AT_DATAGRAM, -2) == -22
        eng.run()  # the one valid op, on an empty batch
        eng.sync()
    finally:
        eng.close()
