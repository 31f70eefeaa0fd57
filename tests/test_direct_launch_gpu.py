"""The direct-launch path (LKF_GRAPH=0), engine vs oracle.

With LKF_GRAPH=0 lkf_run enqueues the control-op pull, the prep stage and the
decide stage's scan tail as plain kernel launches instead of replaying the
graphs captured from the same launches.  Both paths go through one helper
(engine.cpp run_stage) and share their bodies; every other GPU test runs the
captured one.  Here each batch's output records, wire bytes and every
Forwarder state are compared with the CPU oracle on identical input.
"""
import numpy as np
import pytest

from tests import ctl_key_lib as K
from tests.test_regrow_gpu import _pair, _run_batch, _states

pytestmark = pytest.mark.gpu


def test_smoke_trace_ingest_then_submit(pkg, workload, abi, monkeypatch):
    """smoke()'s trace: batch 0 goes through lkf_ingest with its scripted ops
    and one more mute keyed by datagram index (the resolver, always launched
    directly, on the same path), the later batches are submitted."""
    monkeypatch.setenv("LKF_GRAPH", "0")  # read by lkf_create
    tr = workload.Trace(1, duration_s=2.0, batch_s=1.0)
    assert tr.nbatches >= 2
    o, eng, oh = _pair(pkg, workload, tr)
    try:
        workload.load_streams(eng.api, eng.h, tr)
        workload.load_streams(o.api, oh, tr)
        rb = K.RawBatch(tr, abi, 0, repeats=False)
        ev, n = workload.events_keyed(tr, 0, abi.LKF_AT_DATAGRAM)
        ops = [(ev[i].dt, ev[i].op, tuple(ev[i].a), ev[i].key) for i in range(n)]
        dt = tr.ndts // 2 + 1  # (no scripted op of batch 0 names it)
        assert all(op[0] != dt for op in ops)
        lo, hi = rb.ranges[tr.downtracks[dt].track]
        assert hi - lo > 2
        mute = (dt, K.MUTE, (1, 1, 0, 0), (lo + hi) // 2)
        workload.queue_events_keyed(eng.api, eng.h, tr, 0, abi.LKF_AT_DATAGRAM)
        eng.ingest(rb.raws, rb.n, rb.ar, rb.alen)
        eng.ctl_key(dt, K.MUTE, *mute[2], kind=abi.LKF_AT_DATAGRAM, key=mute[3])
        eng.run()
        eng.sync()
        flows, pk, k = K.oracle_ingest(o, oh, abi, pkg, rb)
        scan = K.scan_of(flows)
        at = K.queue_oracle(o, oh, abi, ops + [mute], lambda d, key: K.resolve_datagram(scan, rb.n, key))
        assert any(0 < a < k for a in at)  # an op inside the batch
        o.run(oh, pk if k else None, k, rb.ar, rb.alen)
        want = K.oracle_result(o, oh, abi, pkg)
        K.assert_same(abi, 0, (eng.stats(),) + eng.drain(), want)
        assert want[0]["forwarded"] > 0
        assert _states(abi, eng.api, eng.h, tr.ndts) == _states(abi, o.api, oh, tr.ndts)
        fwd = 0
        for b in range(1, tr.nbatches):
            fwd += _run_batch(pkg, workload, tr, o, eng, oh, b)
            assert _states(abi, eng.api, eng.h, tr.ndts) == _states(abi, o.api, oh, tr.ndts), b
        assert fwd > 0
    finally:
        eng.close()
        o.destroy(oh)
        tr.close()


def test_dependency_descriptor_batches(pkg, workload, abi, monkeypatch):
    """configs[4] (AV1 / VP9 with dependency descriptors), submitted with its
    lkf_pkt_dd side arrays: the DD decode of the prep stage and the DD
    instantiation of decide."""
    monkeypatch.setenv("LKF_GRAPH", "0")
    tr = workload.Trace(5, duration_s=1.0, batch_s=0.5, rooms=4)
    assert tr.has_dd()
    o, eng, oh = _pair(pkg, workload, tr)
    try:
        fwd = 0
        for b in range(tr.nbatches):
            workload.queue_events(eng.api, eng.h, tr, b)
            workload.queue_events(o.api, oh, tr, b)
            pk, n, ar, alen = tr.batch(b)
            dd = tr.batch_dd(b)[0]
            eng.submit(pk, n, ar, alen, dd)
            eng.run()
            eng.sync()
            o.run(oh, pk, n, ar, alen, dd)
            grec, gar = eng.drain()
            orec, oar = pkg.drain_arrays(o.api, oh)
            assert np.array_equal(grec, orec), "batch %d: output records differ from oracle" % b
            assert np.array_equal(gar, oar), "batch %d: wire bytes differ from oracle" % b
            assert _states(abi, eng.api, eng.h, tr.ndts) == _states(abi, o.api, oh, tr.ndts), b
            fwd += len(grec)
        assert fwd > 0
    finally:
        eng.close()
        o.destroy(oh)
        tr.close()
