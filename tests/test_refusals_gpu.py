"""Bad handle lists on the engine, against the CPU oracle (tests/refusals_lib).

Every control call that takes a list of DownTrack or tracker handles gets the
seven lists of refusals_lib.LISTS after the 2-second configs[0] trace has run
and one DownTrack has been removed.  The engine's return code and count
outputs must be the oracle's (for the four RTCP calls, which the oracle does
not export, the code include/lkfwd.h documents); a refused call must change
nothing; and afterwards one valid call per entry point must still equal the
oracle (the RTCP calls: tests/rtcp_lib.PyRtcp and the parse's restatement)
field for field."""
import ctypes as C

import numpy as np
import pytest

from tests import pad_lib, prov_lib, rtcp_lib, rtx_lib
from tests import refusals_lib as R
from tests import rtcp_wire_lib as W
from tests.rtcp_lib import ingest as checked_ingest
from tests.rtcp_lib import rr_lsn

pytestmark = pytest.mark.gpu


def _states(abi, api, h, ndts):
    out = []
    for d in range(ndts):
        st = abi.lkf_fwd_state()
        assert api["get_state"](h, d, C.byref(st)) == 0
        out.append(st.as_tuple())
    return out


def _same(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for f in want.dtype.names:
        if not f.startswith("reserved"):
            assert np.array_equal(got[f], want[f]), (what, f)


def _both(rig, name, arr, out_dtype, *extra):
    outs = []
    for api, h in ((rig.eng.api, rig.eng.h), (rig.o.api, rig.oh)):
        out = np.zeros(max(1, len(arr)), dtype=out_dtype)
        assert api[name](h, arr.ctypes.data, len(arr), *extra, out.ctypes.data) == 0, name
        outs.append(out[:len(arr)])
    _same(outs[0], outs[1], name)
    return outs[1]


def _valid_rtcp_list(rig, name, hs):
    """A valid list of an RTCP call, through the model so that it keeps step (empty entries: nothing changes)."""
    if name == "rtcp_feedback":
        assert rig.feedback([(d, False, 0, 0, 0, 0, 0, 0, 0, 0) for d in hs], R.NOW) == [(0, 0)] * len(hs)
    elif name == "rtcp_sender_reports":
        rig.sender_reports([(d, 0) for d in hs], R.NOW)
    elif name == "sender_delta_info":
        rig.delta(hs)
    else:
        out, _, nacks = checked_ingest(rig, [(d, R.SDES) for d in hs], R.NOW)
        assert nacks == [] and not out["reports"].any()


def test_refused_lists(pkg, workload, abi):
    tr = workload.Trace(1, duration_s=2.0, batch_s=1.0)
    rig = rtcp_lib.Rig(pkg, workload, tr, pkg.Engine.for_trace(tr))
    eng, o, oh = rig.eng, rig.o, rig.oh
    try:
        rig.forward(tr.nbatches)
        handles = R.prepare(eng.api, eng.h, tr)
        assert R.prepare(o.api, oh, tr) == handles
        a, b, gone, ndts = handles["dt"]
        rig.models[gone].stop()
        before = _states(abi, o.api, oh, ndts)
        assert _states(abi, eng.api, eng.h, ndts) == before
        rtcp_before = eng.sender_rtcp(range(ndts)).tobytes()
        want = R.oracle_answers(o, oh, handles)

        # the refusals
        refused = 0
        for name, which, hs in R.cases(handles):
            code = R.contract_code(name, which)
            if code == R.OK:
                continue
            rc, counts, _ = R.send(eng.api, eng.h, name, hs)
            print("engine", name, which, rc, counts, want.get((name, which), ("-", ()))[:2])
            refused += 1
            if name in R.NO_ORACLE:
                assert rc == code, (name, which, rc)
                if name == "rtcp_ingest":
                    assert counts == R.RTCP_INGEST_REFUSED_COUNTS, (which, counts)
                continue
            if (name, which) in R.PINNED_CODES:
                assert rc == R.PINNED_CODES[(name, which)], (name, which, rc)
                continue
            orc, ocounts, _ = want[(name, which)]
            assert rc == orc == code, (name, which, rc, orc)
            assert counts == R.PINNED_COUNTS.get((name, which), ocounts), (name, which, counts, ocounts)
        assert refused == 80  # of 91: eleven lists are valid for their call
        # ... changed nothing
        assert _states(abi, eng.api, eng.h, ndts) == before
        assert eng.sender_rtcp(range(ndts)).tobytes() == rtcp_before

        # the lists that are valid for their call: answered as the oracle answers them
        for name, which, hs in R.cases(handles):
            if R.contract_code(name, which) != R.OK:
                continue
            if name in R.NO_ORACLE:
                _valid_rtcp_list(rig, name, hs)
                continue
            rc, counts, out = R.send(eng.api, eng.h, name, hs)
            assert (rc, counts) == want[(name, which)][:2] and rc == R.OK, (name, which, rc, counts)
            assert out == want[(name, which)][2], (name, which)
        assert _states(abi, eng.api, eng.h, ndts) == _states(abi, o.api, oh, ndts)

        # one valid call per entry point
        now = R.NOW + 10**9
        live = [d for d, m in enumerate(rig.models) if m.s.init and d != gone]
        assert len(live) > 4
        rig.sender_reports([(d, 0) for d in live], now)
        rig.feedback([(d, True, rr_lsn(rig.models[d].s.high_sn, rig.models[d].s.start_sn), 1, 7, 0, 0, 1, 0, 1)
                      for d in live], now)
        rig.delta(live)
        entries = [(d, W.compound(W.rr(1, [W.report_block(int(tr.downtracks[d].ssrc), 0, 2,
                                                          rr_lsn(rig.models[d].s.high_sn, rig.models[d].s.start_sn),
                                                          9, 0, 0)]), W.sdes(1), W.pli(1, int(tr.downtracks[d].ssrc))))
                   for d in live[:5]]
        checked_ingest(rig, entries, now + 10**8)
        rig.check_state()
        nacks = rtx_lib.make_nacks(o.api, oh, tr, seed=3)
        r = rtx_lib.rtx_lookup(o.api, oh, nacks, now)
        assert len(r) > 0
        _same(rtx_lib.rtx_lookup(eng.api, eng.h, nacks, now), r, "rtx_lookup")
        rng = np.random.default_rng(4)
        vd = np.array([d for d in prov_lib.video_dts(tr) if d != gone], dtype=np.int32)
        reqs = prov_lib.alloc_reqs(rng, vd)
        _both(rig, "allocate_optimal", reqs, abi.ALLOCATION_DTYPE)
        for api, h in ((eng.api, eng.h), (o.api, oh)):
            assert api["provisional_prepare"](h, reqs.ctypes.data, len(reqs)) == 0
            assert api["provisional_reset"](h, vd.ctypes.data, len(vd)) == 0
        q = np.zeros(len(vd), dtype=abi.PROV_REQ_DTYPE)
        q["dt"], q["spatial"], q["temporal"], q["capacity"], q["allow_pause"] = vd, 1, 1, 1_500_000, 1
        _both(rig, "provisional_allocate", q, abi.PROV_RESULT_DTYPE)
        g = np.zeros(1, dtype=abi.ALLOC_GROUP_DTYPE)
        g["count"], g["capacity"], g["allow_pause"] = len(reqs), 2_000_000, 1
        outs = []
        for api, h in ((eng.api, eng.h), (o.api, oh)):
            out = np.zeros(len(reqs), dtype=abi.ALLOCATION_DTYPE)
            assert api["allocate_all"](h, g.ctypes.data, 1, reqs.ctypes.data, len(reqs), out.ctypes.data) == 0
            outs.append(out)
        _same(outs[0], outs[1], "allocate_all")
        preq = pad_lib.make_reqs(ndts, seed=2, frac=0.3)
        go, gw, gs = pad_lib.pad(eng.api, eng.h, preq, now)
        oo, ow, os_ = pad_lib.pad(o.api, oh, preq, now)
        assert len(oo) > 0
        _same(go, oo, "padding")
        assert np.array_equal(gw, ow) and np.array_equal(gs, os_)
        ids = np.array([0, 1, 2], dtype=np.int32)
        _both(rig, "dd_trackers_tick", ids, abi.DD_TRACKER_STATUS_DTYPE, 10**9)
        _both(rig, "stream_trackers_tick_at", ids, abi.TRACKER_STATUS_DTYPE, 1, 10**9, now)
        assert _states(abi, eng.api, eng.h, ndts) == _states(abi, o.api, oh, ndts)
    finally:
        rig.close()
