"""Prefix egress (lkf_set_egress(LKF_EGRESS_PREFIX)) on the MI355X against the
CPU oracle.  Engine and oracle get identical inputs; the oracle's wire output
gives, through tests/prefix_lib.py, the lkf_pre records and the prefix arena
the engine must produce, and "prefix ++ input slice" must rebuild the oracle's
wire arena.  Counters and every piece of state must not depend on the mode."""
import ctypes as C

import numpy as np
import pytest

from tests import prefix_lib
from tests.oracle_lib import load as load_oracle
from tests.test_parity_gpu import _state_tuple, check_sender_stats

pytestmark = pytest.mark.gpu

EINVAL, ENOSPC = -22, -28


def _oracle_stats(o, oh, abi):
    st = abi.lkf_stats()
    assert o.api["get_stats"](oh, C.byref(st)) == 0
    return st.as_dict()


def _prefix_batch(pkg, abi, tr, eng, o, oh, pkts, inp, what):
    """After both sides ran the batch (engine in prefix mode, synced): stats,
    records, prefix arena and reassembled wire against the oracle.  -> records."""
    gs = eng.stats()
    os_ = _oracle_stats(o, oh, abi)
    assert gs == os_, "%s stats differ:\n gpu %s\n orc %s" % (what, gs, os_)
    grec, gar = eng.drain_prefix()
    orec, owire = pkg.drain_arrays(o.api, oh)
    prefix_lib.check_prefix(abi, tr, pkts, inp, grec, gar, orec, owire, what)
    return len(grec)


def _wire_batch(pkg, abi, eng, o, oh, what):
    assert eng.stats() == _oracle_stats(o, oh, abi), what
    grec, gar = eng.drain()
    orec, oar = pkg.drain_arrays(o.api, oh)
    assert len(grec) == len(orec), what
    for f in abi.OUT_DTYPE.names:
        assert np.array_equal(grec[f], orec[f]), (what, f)
    assert np.array_equal(gar, oar), what
    return len(grec)


def _final_state(pkg, abi, tr, eng, o, oh, forwarded):
    """Forwarder state, sender stats, DownTrack summaries and a sequencer probe."""
    gsum = pkg.downtrack_summaries(eng.api, eng.h)
    osum = pkg.downtrack_summaries(o.api, oh)
    assert len(gsum) == len(osum) == tr.ndts
    for f in abi.DT_SUMMARY_DTYPE.names:
        assert np.array_equal(gsum[f], osum[f]), ("summary field", f)
    assert int(gsum["packets_sent"].sum()) == forwarded
    for dt in range(tr.ndts):
        assert _state_tuple(eng.api, eng.h, dt, abi) == _state_tuple(o.api, oh, dt, abi), dt
    check_sender_stats(pkg, eng.api, eng.h, o.api, oh, range(tr.ndts))
    now = 1700000000 * 10**9 + int(tr.nbatches * 1.5e9)
    for dt in range(0, tr.ndts, max(1, tr.ndts // 7)):
        gm, om = (abi.lkf_seq_meta * 64)(), (abi.lkf_seq_meta * 64)()
        gn, on = C.c_uint32(), C.c_uint32()
        st = abi.lkf_fwd_state()
        eng.api["get_state"](eng.h, dt, C.byref(st))
        base = st.ext_last_sn & 0xFFFF
        sns = (C.c_uint16 * 40)(*[(base - i * 3) & 0xFFFF for i in range(40)])
        assert eng.api["seq_lookup"](eng.h, dt, sns, 40, now, gm, C.byref(gn)) == 0
        assert o.api["seq_lookup"](oh, dt, sns, 40, now, om, C.byref(on)) == 0
        assert gn.value == on.value, (dt, gn.value, on.value)
        for i in range(gn.value):
            assert bytes(gm[i]) == bytes(om[i]), (dt, i)


def run_prefix_parity(pkg, workload, abi, tr, mode_of=lambda b: 1, extra_ops=None, empty_after=None, final=True):
    """Submit path.  mode_of(b): the egress mode of batch b.  -> records per batch."""
    o = load_oracle()
    eng = pkg.Engine.for_trace(tr)
    oh = o.create(500)
    counts = []
    try:
        workload.load_topology(eng.api, eng.h, tr)
        workload.load_topology(o.api, oh, tr)
        for b in range(tr.nbatches):
            workload.queue_events(eng.api, eng.h, tr, b)
            workload.queue_events(o.api, oh, tr, b)
            for (dt, op, a0, a1, a2, a3, at) in (extra_ops or {}).get(b, ()):
                assert eng.api["ctl"](eng.h, dt, op, a0, a1, a2, a3, at) == 0
                assert o.api["ctl"](oh, dt, op, a0, a1, a2, a3, at) == 0
            pk, n, ar, alen = tr.batch(b)
            dd = tr.batch_dd(b)[0] if tr.has_dd() else None
            mode = mode_of(b)
            eng.set_egress(mode)
            eng.submit(pk, n, ar, alen, dd)
            eng.run()
            eng.sync()
            o.run(oh, pk, n, ar, alen, dd)
            if mode == abi.LKF_EGRESS_PREFIX:
                counts.append(_prefix_batch(pkg, abi, tr, eng, o, oh, prefix_lib.pkts_array(pk, n),
                                            prefix_lib.arena_array(ar, alen), "batch %d" % b))
            else:
                counts.append(_wire_batch(pkg, abi, eng, o, oh, "batch %d" % b))
            if empty_after == b:  # an empty batch: no records, no bytes, LKF_OK
                eng.set_egress(abi.LKF_EGRESS_PREFIX)
                eng.submit(pk, 0, ar, 0)
                eng.run()
                eng.sync()
                st = eng.stats()
                assert st["tuples"] == 0 and st["forwarded"] == 0
                n_, len_ = C.c_uint64(7), C.c_uint64(7)
                assert eng.api["drain_prefix"](eng.h, None, 0, None, 0, C.byref(n_), C.byref(len_)) == 0
                assert (n_.value, len_.value) == (0, 0)
                rec, ar_ = eng.drain_prefix()
                assert len(rec) == 0 and len(ar_) == 0
                assert eng.output_prefix_device()[1::2] == (0, 0)
        if final:
            _final_state(pkg, abi, tr, eng, o, oh, sum(counts))
        return counts
    finally:
        eng.close()
        o.destroy(oh)


# ---- 1. submit path: codecs and extension profiles --------------------------
SUBMIT_TRACES = {
    "vp8_twcc": ((2,), dict(duration_s=3, batch_s=1, rooms=3, seed=8, twcc=1)),
    "config1": ((1,), dict(duration_s=1, batch_s=1)),
    "dd": ((5,), dict(duration_s=2, batch_s=0.5, rooms=3, seed=9, twcc=2)),
    "dd_wide": ((5,), dict(duration_s=2, batch_s=0.5, rooms=3, svc_dd=2, seed=61)),
    "vp9": ((5,), dict(duration_s=2, batch_s=0.5, rooms=3, svc_dd=0, seed=5)),
}


@pytest.mark.parametrize("name", list(SUBMIT_TRACES))
def test_prefix_submit(pkg, workload, abi, name):
    args, kw = SUBMIT_TRACES[name]
    tr = workload.Trace(*args, **kw)
    counts = run_prefix_parity(pkg, workload, abi, tr)
    assert sum(counts) > 0
    if name == "config1":
        # 1,793 records: the 1-s batch has 1,783 of them = 28 groups of 64 records, the last one
        # partial (the multi-group, non-multiple-of-64 case), the arrival tail the other 10
        assert counts == [1783, 10], counts
        assert (counts[0] + 63) // 64 == 28 and counts[0] % 64 != 0


# ---- 2. group edges ----------------------------------------------------------
def test_prefix_group_edges(pkg, workload, abi):
    """About 18 records per batch (less than one 64-record group, some batches
    with none) and an empty batch."""
    tr = workload.Trace(1, duration_s=0.2, batch_s=0.01)
    counts = run_prefix_parity(pkg, workload, abi, tr, empty_after=3)
    assert max(counts) < 64 and sum(counts) > 0, counts


# ---- 3. both modes on one engine ----------------------------------------------
def test_prefix_mode_alternation(pkg, workload, abi):
    tr = workload.Trace(2, duration_s=4, batch_s=0.5, rooms=3)
    counts = run_prefix_parity(pkg, workload, abi, tr, mode_of=lambda b: b & 1)
    assert len(counts) >= 8 and min(counts) > 0


def test_prefix_cross_mode_accessors(pkg, workload, abi):
    tr = workload.Trace(1, duration_s=2, batch_s=1)
    eng = pkg.Engine.for_trace(tr)
    lib = eng.lib
    n_, len_ = C.c_uint64(), C.c_uint64()
    p0, p1 = C.c_void_p(), C.c_void_p()
    drain_sig = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                 C.POINTER(C.c_uint64)]
    lib.lkf_drain_run.restype = lib.lkf_drain_run_async.restype = C.c_int
    lib.lkf_drain_run.argtypes = lib.lkf_drain_run_async.argtypes = drain_sig

    def refused(rc):
        assert rc == EINVAL, rc
        assert b"egress mode" in lib.lkf_last_error(eng.h)

    try:
        workload.load_topology(eng.api, eng.h, tr)
        assert eng.api["set_egress"](eng.h, 2) == EINVAL
        assert eng.api["set_egress"](eng.h, -1) == EINVAL
        pk, n, ar, alen = tr.batch(0)
        eng.set_egress(abi.LKF_EGRESS_PREFIX)
        eng.submit(pk, n, ar, alen)
        eng.run()
        eng.sync()
        refused(eng.api["drain"](eng.h, None, 0, None, 0, C.byref(n_), C.byref(len_)))
        refused(lib.lkf_output_device(eng.h, C.byref(p0), C.byref(n_), C.byref(p1), C.byref(len_)))
        refused(lib.lkf_drain_run(eng.h, 0, None, 0, None, 0, C.byref(n_), C.byref(len_)))
        refused(lib.lkf_drain_run_async(eng.h, 0, None, 0, None, 0, C.byref(n_), C.byref(len_)))
        refused(eng.api["protect"](eng.h, 1700000000 * 10**9))
        assert len(eng.drain_prefix()[0]) > 0
        pk, n, ar, alen = tr.batch(1)
        eng.set_egress(abi.LKF_EGRESS_WIRE)
        eng.submit(pk, n, ar, alen)
        eng.run()
        eng.sync()
        refused(eng.api["drain_prefix"](eng.h, None, 0, None, 0, C.byref(n_), C.byref(len_)))
        refused(eng.api["drain_prefix_run"](eng.h, 0, None, 0, None, 0, C.byref(n_), C.byref(len_)))
        refused(eng.api["output_prefix_device"](eng.h, C.byref(p0), C.byref(n_), C.byref(p1), C.byref(len_)))
        # the run before it is still a prefix run
        refused(lib.lkf_drain_run(eng.h, 1, None, 0, None, 0, C.byref(n_), C.byref(len_)))
        assert eng.api["drain_prefix_run"](eng.h, 1, None, 0, None, 0, C.byref(n_), C.byref(len_)) == ENOSPC
        assert n_.value > 0 and len_.value > 0  # (the size probe)
        assert len(eng.drain()[0]) > 0
    finally:
        eng.close()


# ---- 4. ingest path -----------------------------------------------------------
def test_prefix_ingest(pkg, workload, abi):
    """tail_src indexes the raw arena of lkf_ingest."""
    tr = workload.Trace(2, duration_s=3.0, batch_s=0.5, rooms=3, loss=0.05, reorder=0.03, seed=21)
    o = load_oracle()
    eng = pkg.Engine.for_trace(tr)
    oh = o.create(500)
    total = 0
    try:
        for api, h in ((eng.api, eng.h), (o.api, oh)):
            workload.load_topology(api, h, tr)
            workload.load_streams(api, h, tr)
        eng.set_egress(abi.LKF_EGRESS_PREFIX)
        for b in range(tr.nbatches):
            workload.queue_events(eng.api, eng.h, tr, b)
            workload.queue_events(o.api, oh, tr, b)
            rp, n, ar, alen = tr.batch_raw(b)
            eng.ingest(rp, n, ar, alen)
            assert o.api["ingest"](oh, rp, n, ar, alen) == 0
            m = C.c_uint32()
            assert o.api["ingested"](oh, None, 0, C.byref(m)) in (0, ENOSPC)
            ext = (abi.lkf_pkt * max(1, m.value))()
            assert o.api["ingested"](oh, ext, m.value, C.byref(m)) == 0
            eng.run()
            eng.sync()
            o.run(oh, ext if m.value else None, m.value, ar, alen)
            total += _prefix_batch(pkg, abi, tr, eng, o, oh, prefix_lib.pkts_array(ext, m.value),
                                   prefix_lib.arena_array(ar, alen), "ingest batch %d" % b)
        assert total > 0
        for dt in range(tr.ndts):
            assert _state_tuple(eng.api, eng.h, dt, abi) == _state_tuple(o.api, oh, dt, abi), dt
    finally:
        eng.close()
        o.destroy(oh)


# ---- 5. pipelined drain ---------------------------------------------------------
def test_prefix_pipelined_drain(pkg, workload, abi):
    """Three runs queued with no sync: lkf_drain_prefix_run at ages 2, 1, 0
    equals an engine drained after every batch."""
    tr = workload.Trace(2, duration_s=1.5, batch_s=0.5, rooms=3)
    assert tr.nbatches >= 3  # (the engine keeps three batch contexts: ages 0..2)
    a, b_ = pkg.Engine.for_trace(tr), pkg.Engine.for_trace(tr)
    try:
        ref = []
        for eng in (b_, a):
            workload.load_topology(eng.api, eng.h, tr)
            eng.set_egress(abi.LKF_EGRESS_PREFIX)
        for b in range(3):
            pk, n, ar, alen = tr.batch(b)
            for eng in (b_, a):
                workload.queue_events(eng.api, eng.h, tr, b)
                eng.submit(pk, n, ar, alen)
                eng.run()
            b_.sync()
            ref.append(b_.drain_prefix())
        for age in (2, 1, 0):
            rrec, rar = ref[2 - age]
            assert len(rrec) > 0
            recs = np.zeros(len(rrec), dtype=abi.PRE_DTYPE)  # (exact-fit capacities)
            arena = np.zeros(len(rar), dtype=np.uint8)
            got = a.drain_prefix_run_into(age, recs.ctypes.data, len(recs), arena.ctypes.data, len(arena))
            assert got == (len(rrec), len(rar)), (age, got)
            assert recs.tobytes() == rrec.tobytes(), age
            assert np.array_equal(arena, rar), age
        a.sync()
    finally:
        a.close()
        b_.close()


# ---- 6. capacity -----------------------------------------------------------------
def test_prefix_capacity(pkg, workload, abi):
    """max_out_pkts below the batch's records: the run writes nothing and
    reports LKF_ENOSPC, the drains hand out nothing."""
    tr = workload.Trace(1, duration_s=1.0, batch_s=1.0)
    eng = pkg.Engine(max_tracks=tr.ntracks + 8, max_downtracks=tr.ndts + 8, max_batch_pkts=tr.max_batch_pkts + 64,
                     max_batch_arena=tr.max_batch_arena + 4096, max_batch_tuples=tr.max_batch_tuples + 1024,
                     max_out_pkts=1024, max_out_bytes=64 << 20)
    n_, len_ = C.c_uint64(), C.c_uint64()
    p0, p1 = C.c_void_p(), C.c_void_p()
    try:
        workload.load_topology(eng.api, eng.h, tr)
        eng.set_egress(abi.LKF_EGRESS_PREFIX)
        workload.queue_events(eng.api, eng.h, tr, 0)  # (the initial allocations: 1,783 records, 490 without)
        pk, n, ar, alen = tr.batch(0)
        eng.submit(pk, n, ar, alen)
        eng.run()
        assert eng.lib.lkf_sync(eng.h) == ENOSPC
        assert eng.lib.lkf_sync(eng.h) == 0
        recs = np.zeros(4096, dtype=abi.PRE_DTYPE)
        arena = np.zeros(1 << 20, dtype=np.uint8)
        assert eng.api["drain_prefix"](eng.h, recs.ctypes.data, len(recs), arena.ctypes.data, len(arena),
                                       C.byref(n_), C.byref(len_)) == ENOSPC
        assert n_.value == 1783 > 1024 and len_.value == 0
        assert eng.api["drain_prefix_run"](eng.h, 0, recs.ctypes.data, len(recs), arena.ctypes.data, len(arena),
                                           C.byref(n_), C.byref(len_)) == ENOSPC
        assert eng.api["output_prefix_device"](eng.h, C.byref(p0), C.byref(n_), C.byref(p1), C.byref(len_)) == ENOSPC
        assert not recs.view(np.uint8).any() and not arena.any()
    finally:
        eng.close()


# ---- 7. playout delay -------------------------------------------------------------
def test_prefix_playout_delay(pkg, workload, abi):
    """DownTracks with the playout-delay extension (until LKF_CTL_PLAYOUT_ACKED)
    beside abs-send-time / transport-cc: 16-B extension blocks in the prefix."""
    tr = workload.Trace(2, duration_s=2, batch_s=0.5, rooms=2, seed=12, twcc=1)
    with_ext = list(range(0, tr.ndts, 2))
    for d in with_ext:
        tr.downtracks[d].ext_playout = 6
        tr.downtracks[d].playout_delay[0] = 0x12
        tr.downtracks[d].playout_delay[1] = 0x34
        tr.downtracks[d].playout_delay[2] = 0x56
    acked = {2: [(d, abi.LKF_CTL_PLAYOUT_ACKED, 1, 0, 0, 0, 0) for d in with_ext[::2]]}
    counts = run_prefix_parity(pkg, workload, abi, tr, extra_ops=acked)
    assert min(counts) > 0
