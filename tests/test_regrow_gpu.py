"""On-demand buffer growth of the engine's control calls, engine vs oracle.

Each case crosses the floor of a grown-on-demand device buffer family and then
keeps using the regrown buffers: the sequencer lookup scratch (floor 256), the
NACK -> RTX scratch (floor 1,024), a batch context's control-op staging and
event buffers (floor 4,096, which drains the engine and re-captures the
context's stage graphs), the RTCP calls' input / group / result buffers (floor
65,536 bytes; one call past it, and the three calls in turn with their
opposite shapes) and the RTCP ingress's per-entry buffers (floor 4,096 entries).
Every result is compared with the CPU oracle on identical input (the RTCP
calls: with tests/rtcp_lib.PyRtcp, replayed over the oracle's records), on the
2-second configs[0] trace smoke() uses.

The padding and allocation scratch families grow only past 1,024 distinct
DownTracks; a topology that large does not belong in a seconds-long test, and
they grow through the same code as the two RTCP families here."""
import ctypes as C

import numpy as np
import pytest

from tests import rtcp_lib, rtx_lib
from tests import rtcp_wire_lib as W
from tests.oracle_lib import load as load_oracle
from tests.rtcp_lib import ingest as checked_ingest
from tests.rtcp_lib import rr_lsn

pytestmark = pytest.mark.gpu
EPOCH = 1700000000 * 10**9


def _trace(workload):
    return workload.Trace(1, duration_s=2.0, batch_s=1.0)


def _pair(pkg, workload, tr):
    o = load_oracle()
    eng = pkg.Engine.for_trace(tr)
    oh = o.create(500)
    workload.load_topology(eng.api, eng.h, tr)
    workload.load_topology(o.api, oh, tr)
    return o, eng, oh


def _run_batch(pkg, workload, tr, o, eng, oh, b):
    """Batch b on both; the output records and wire bytes must be equal."""
    workload.queue_events(eng.api, eng.h, tr, b)
    workload.queue_events(o.api, oh, tr, b)
    pk, n, ar, alen = tr.batch(b)
    eng.submit(pk, n, ar, alen)
    eng.run()
    eng.sync()
    o.run(oh, pk, n, ar, alen)
    grec, gar = eng.drain()
    orec, oar = pkg.drain_arrays(o.api, oh)
    assert np.array_equal(grec, orec), "batch %d: output records differ from oracle" % b
    assert np.array_equal(gar, oar), "batch %d: wire bytes differ from oracle" % b
    return len(grec)


def _states(abi, api, h, ndts):
    out = []
    for d in range(ndts):
        st = abi.lkf_fwd_state()
        assert api["get_state"](h, d, C.byref(st)) == 0
        out.append(st.as_tuple())
    return out


def _busiest_dt(pkg, o, oh):
    return int(np.argmax(pkg.downtrack_summaries(o.api, oh)["packets_sent"]))


def test_seq_lookup_regrow(pkg, workload, abi):
    """lkf_seq_lookup with 40, 257 and 40 sequence numbers of one DownTrack:
    below the scratch's floor, above it (a regrow), and below again."""
    tr = _trace(workload)
    o, eng, oh = _pair(pkg, workload, tr)
    try:
        for b in range(tr.nbatches):
            _run_batch(pkg, workload, tr, o, eng, oh, b)
        dt = _busiest_dt(pkg, o, oh)
        st = abi.lkf_fwd_state()
        assert o.api["get_state"](oh, dt, C.byref(st)) == 0 and st.started
        base = st.ext_last_sn & 0xFFFF
        found = []
        for step, n in enumerate((40, 257, 40)):
            now = EPOCH + (3 + 2 * step) * 10**9
            sns = (C.c_uint16 * n)(*[(base - i) & 0xFFFF for i in range(n)])
            gm, om = (abi.lkf_seq_meta * n)(), (abi.lkf_seq_meta * n)()
            gn, on = C.c_uint32(), C.c_uint32()
            assert eng.api["seq_lookup"](eng.h, dt, sns, n, now, gm, C.byref(gn)) == 0
            assert o.api["seq_lookup"](oh, dt, sns, n, now, om, C.byref(on)) == 0
            assert gn.value == on.value, (step, gn.value, on.value)
            assert bytes(gm)[:gn.value * C.sizeof(abi.lkf_seq_meta)] == bytes(om)[:on.value * C.sizeof(abi.lkf_seq_meta)], step
            found.append(on.value)
        assert found[1] > found[0] > 0, found  # the long list reaches records the short one does not
    finally:
        eng.close()
        o.destroy(oh)
        tr.close()


def _nacks(abi, api, h, ndts, total):
    """`total` NACK entries, grouped per DownTrack, downwards from each one's last SN."""
    lasts = []
    for d in range(ndts):
        st = abi.lkf_fwd_state()
        assert api["get_state"](h, d, C.byref(st)) == 0
        if st.started:
            lasts.append((d, st.ext_last_sn & 0xFFFF))
    per = -(-total // len(lasts))
    rows = [(d, (last - k) & 0xFFFF, 0) for d, last in lasts for k in range(per)]
    return np.array(rows[:total], dtype=abi.NACK_DTYPE)


def test_rtx_lookup_regrow(pkg, workload, abi):
    """lkf_rtx_lookup with about 100 NACK entries, then 1,025 (past the floor of
    the seven NACK -> RTX buffers: all of them regrow)."""
    tr = _trace(workload)
    o, eng, oh = _pair(pkg, workload, tr)
    try:
        for b in range(tr.nbatches):
            _run_batch(pkg, workload, tr, o, eng, oh, b)
        for step, total in enumerate((100, 1025)):
            nacks = _nacks(abi, o.api, oh, tr.ndts, total)
            assert len(nacks) == total
            now = EPOCH + (3 + 2 * step) * 10**9
            g = rtx_lib.rtx_lookup(eng.api, eng.h, nacks, now)
            r = rtx_lib.rtx_lookup(o.api, oh, nacks, now)
            assert len(g) == len(r) > 0, (step, len(g), len(r))
            for f in r.dtype.names:
                assert np.array_equal(g[f], r[f]), (step, f)
        assert _states(abi, eng.api, eng.h, tr.ndts) == _states(abi, o.api, oh, tr.ndts)
    finally:
        eng.close()
        o.destroy(oh)
        tr.close()


def _mutes(abi, dts, count):
    ev = (abi.lkfs_event * count)()
    for i in range(count):
        ev[i].dt = dts[i % len(dts)]
        ev[i].op = abi.LKF_CTL_MUTE
        ev[i].a[0] = 1 - (i // len(dts)) % 2  # mute, unmute, mute, ... per DownTrack
        ev[i].at_pkt = 0
    return ev


def test_ctl_batch_regrow_and_recapture(pkg, workload, abi):
    """4,097 mute / unmute ops on five DownTracks before the fourth run: the
    second use of batch context 0, which by then holds a live staging buffer of
    the floor size (4,096 ops) and the stage graphs it captured and launched
    in run 0.  One op more than the floor, so that run
    drains the engine, frees and regrows the staging and event buffers, and
    re-captures the context's graphs in place of the old ones.  Runs 4 and 6
    carry three ops each; run 6 is context 0 again and replays the re-captured
    graphs over the regrown buffers."""
    tr = workload.Trace(1, duration_s=2.0, batch_s=0.25)  # (nine runs: context 0 at runs 0, 3 and 6)
    o, eng, oh = _pair(pkg, workload, tr)
    try:
        dts = list(range(0, tr.ndts, max(1, tr.ndts // 5)))[:5]
        fwd = 0
        assert tr.nbatches >= 7
        for b in range(tr.nbatches):
            count = {3: 4097, 4: 3, 6: 3}.get(b, 0)
            if count:
                ev = _mutes(abi, dts, count)
                assert eng.api["ctl_batch"](eng.h, C.cast(ev, C.c_void_p), count) == 0
                assert o.api["ctl_batch"](oh, C.cast(ev, C.c_void_p), count) == 0
            fwd += _run_batch(pkg, workload, tr, o, eng, oh, b)
            assert _states(abi, eng.api, eng.h, tr.ndts) == _states(abi, o.api, oh, tr.ndts), b
        assert fwd > 0
    finally:
        eng.close()
        o.destroy(oh)
        tr.close()


def _rtcp_rig(pkg, workload):
    tr = _trace(workload)
    rig = rtcp_lib.Rig(pkg, workload, tr, pkg.Engine.for_trace(tr))
    rig.forward(tr.nbatches)
    live = [d for d, m in enumerate(rig.models) if m.s.init]
    assert len(live) > 4
    return rig, live


def test_rtcp_feedback_regrow(pkg, workload):
    """lkf_rtcp_feedback with 100, 1,400 and 100 entries of 48 bytes: below the 65,536-byte floor of the call's
    input buffer, past it (the input, group and result buffers regrow), and below again.  Each DownTrack's
    entries are contiguous: a report first, then entries that only carry counts."""
    rig, live = _rtcp_rig(pkg, workload)
    try:
        for step, total in enumerate((100, 1400, 100)):
            per = -(-total // len(live))
            ent = []
            for d in live:
                m = rig.models[d]
                ent.append((d, True, rr_lsn(m.s.high_sn - 2 + step, m.s.start_sn), step, 10 * step + d % 7, 0, 0,
                            1, 0, 0))
                ent += [(d, False, 0, 0, 0, 0, 0, k % 3, k % 2, 1) for k in range(per - 1)]
            ent = ent[:total]
            assert len(ent) == total and total * 48 > (65536 if step == 1 else 0)
            rig.feedback(ent, EPOCH + (3 + step) * 10**9)
            rig.check_state()
    finally:
        rig.close()


def test_rtcp_ingest_regrow(pkg, workload):
    """lkf_rtcp_ingest with 64, 4,097 and 64 entries: below the 4,096-entry floor of the per-entry buffers,
    past it (all twelve regrow and the scan state is zeroed again), and below again.  A DownTrack's entries
    name the same few bytes, so the whole arena is a few hundred bytes."""
    rig, live = _rtcp_rig(pkg, workload)
    try:
        for step, total in enumerate((64, 4097, 64)):
            per = -(-total // len(live))
            entries = []
            for d in live:
                m, ssrc = rig.models[d], int(rig.tr.downtracks[d].ssrc)
                c = W.compound(W.rr(1, [W.report_block(ssrc, 0, step, rr_lsn(m.s.high_sn - 2 + step, m.s.start_sn),
                                                       5 + step, 0, 0)]), W.sdes(1), W.pli(1, ssrc))
                entries += [(d, c)] * per
            entries = entries[:total]
            assert len(entries) == total
            out, _, _ = checked_ingest(rig, entries, EPOCH + (3 + step) * 10**9)
            assert int(out["reports"].sum()) == total and int(out["plis"].sum()) == total
            rig.check_state()
    finally:
        rig.close()


def test_rtcp_calls_alternate_past_the_floor(pkg, workload):
    """The three RTCP calls share one scratch family and need opposite shapes: feedback is input-heavy (48 bytes
    in, 8 out per entry), sender reports and delta info are output-heavy (8 or 4 in, 68 or 120 out).  Over 1,080
    DownTracks a tick of the three crosses the 65,536-byte floor on the input side (2 x 1,076 x 48), then on the
    output side (1,076 x 68, then x 120); two ticks, every result and the whole state against the model."""
    tr = workload.Trace(2, rooms=6, duration_s=1.0, batch_s=1.0, seed=1)
    rig = rtcp_lib.Rig(pkg, workload, tr, pkg.Engine.for_trace(tr))
    try:
        rig.forward(tr.nbatches)
        live = [d for d, m in enumerate(rig.models) if m.s.init]
        assert len(live) * 2 * 48 > 65536 and len(live) * 68 > 65536 > len(live) * 2 * 8
        for tick in range(2):
            now = EPOCH + (2 + tick) * 10**9
            rig.sender_reports([(d, 0) for d in live], now)
            ent = []
            for d in live:
                m = rig.models[d]
                ent += [(d, True, rr_lsn(m.s.high_sn - 1 + tick, m.s.start_sn), tick, d % 5, 0, 0, 1, 0, 0),
                        (d, False, 0, 0, 0, 0, 0, 0, 1, tick)]
            rig.feedback(ent, now + 10**8)
            rig.delta(live)
            rig.check_state()
    finally:
        rig.close()
