"""The DownTrack RTCP loop on the GPU (lkf_rtcp_feedback, lkf_rtcp_sender_reports,
lkf_sender_delta_info; rtcp_kernels.hip) against tests/rtcp_lib.PyRtcp:
every result and the whole lkf_sender_rtcp_get state, bit-exact.

The model stands on a PySender replayed over the CPU oracle's records of the
same trace (tests/rtcp_lib.Rig), so the ring and the counters it reads are not
the engine's.  Each test runs one small engine: one room, four 1-s batches.
"""
import copy
import ctypes as C

import numpy as np
import pytest

from tests import pad_lib, rtcp_lib, rtx_lib
from tests.rtcp_lib import FB_CACHE_OVERFLOW, FB_IGNORED, FB_RTT_CHANGED, SR_REPAIRED, SR_VALID, rr_lsn

pytestmark = pytest.mark.gpu
EPOCH = 1700000000 * 10**9
SEC = 10**9


def _rig(pkg, workload, config, extra_dts=0):
    kw = dict(loss=0.08) if config == 2 else {}
    tr = workload.Trace(config, rooms=1, duration_s=4, batch_s=1.0, seed=1, **kw)
    return rtcp_lib.Rig(pkg, workload, tr, pkg.Engine.for_trace(tr, extra_dts=extra_dts))


def _ack(rig, dt, esn, now_lost=0, jitter=0, lsr=0, dlsr=0, counts=(0, 0, 0)):
    """A feedback entry whose report acknowledges the DownTrack's sent extended SN `esn`."""
    m = rig.models[dt]
    return (dt, True, rr_lsn(esn, m.s.start_sn), now_lost, jitter, lsr, dlsr) + tuple(counts)


def _add_downtrack_like(rig, dt):
    """One more DownTrack with dt's parameters on both sides -> its handle (it has forwarded nothing)."""
    p = rig.tr.downtracks[dt]
    h = rig.eng.api["add_downtrack"](rig.eng.h, C.byref(p))
    assert h == rig.o.api["add_downtrack"](rig.oh, C.byref(p)) == len(rig.models)
    rig.models.append(rtcp_lib.PyRtcp(rtcp_lib.PySender(int(rig.tr.tracks[p.track].clock_rate))))
    return h


@pytest.mark.parametrize("config", [2, 5])
def test_first_report_on_the_zero_snapshot(pkg, workload, config):
    """The first interval starts at esn 1: packetsNotFound in closed form plus at most 4096 ring reads."""
    rig = _rig(pkg, workload, config)
    try:
        rig.forward(2)
        dts = [d for d, m in enumerate(rig.models) if m.s.init]
        # precondition, from the model alone: a first interval far longer than the ring's reach
        assert any(rig.models[d].s.start_sn > 4096 for d in dts)
        want = rig.feedback([_ack(rig, d, rig.models[d].s.high_sn, jitter=d) for d in dts], EPOCH + 2 * SEC)
        assert any(f & FB_CACHE_OVERFLOW for _, f in want)
        assert all(not f & FB_IGNORED for _, f in want)
        rig.check_state()
        assert sum(m.snap["interval_stats"]["packets_not_found"] for m in rig.models) > 4096
    finally:
        rig.close()


@pytest.mark.parametrize("config", [2, 5])
def test_feedback_after_each_batch(pkg, workload, config):
    """One call per batch for every DownTrack; padding and retransmissions in between put padding,
    out-of-order and lost slots into the intervals."""
    rig = _rig(pkg, workload, config)
    try:
        for b in range(4):
            rig.forward(1)
            now = EPOCH + (b + 1) * SEC
            if b == 1:
                assert rig.padding(pad_lib.make_reqs(rig.tr.ndts, seed=3, frac=0.7), now - 10**6) > 0
                nacks = rtx_lib.make_nacks(rig.o.api, rig.oh, rig.tr, seed=5)
                assert rig.rtx(nacks, now - 10**5) > 0
            ent = [_ack(rig, d, m.s.high_sn if m.s.init else 0, now_lost=b + d % 3, jitter=100 * b + d,
                        counts=(d % 4, b % 2, d % 2)) for d, m in enumerate(rig.models)]
            rig.feedback(ent, now)
            rig.check_state()
        tot = {k: sum(m.snap["interval_stats"][k] for m in rig.models) for k in rtcp_lib.IS_FIELDS}
        for k in ("packets_lost", "packets_padding", "packets_out_of_order", "frames"):
            assert tot[k] > 0, (k, tot)  # otherwise vacuous
    finally:
        rig.close()


def test_interval_edges_in_one_grouped_call(pkg, workload):
    """Successive reports of one DownTrack acknowledge +0, +1, +63, +64, +65 packets, then a span that wraps
    ring slot 4095, then one ahead of extHighestSN: one grouped call, with other DownTracks' reports."""
    rig = _rig(pkg, workload, 2)
    try:
        rig.forward(4)
        pick = None
        for d, m in enumerate(rig.models):
            if not m.s.init:
                continue
            edge = (m.s.start_sn + 194 + 4095) & ~4095  # the first multiple of 4096 above start + 193
            if edge + 10 <= m.s.high_sn:
                pick = (d, edge)
                break
        assert pick is not None, "no DownTrack's sequence numbers cross a ring wrap late enough"
        w, edge = pick
        m = rig.models[w]
        a = max(m.s.start_sn, edge - 250)
        acks = [a]
        for step in (0, 1, 63, 64, 65):
            acks.append(acks[-1] + step)
        assert acks[-1] < edge
        acks += [edge + 10, m.s.high_sn + 7]
        others = [d for d, x in enumerate(rig.models) if x.s.init and d != w][:12]
        ent = [_ack(rig, d, rig.models[d].s.high_sn) for d in others[:6]]
        ent += [_ack(rig, w, e, jitter=i) for i, e in enumerate(acks)]
        ent += [_ack(rig, d, rig.models[d].s.high_sn - 3) for d in others[6:]]
        want = rig.feedback(ent, EPOCH + 4 * SEC)
        assert all(not f & FB_IGNORED for _, f in want)
        rig.check_state([w] + others)
        assert m.snap["ext_last_rr_sn"] == m.s.high_sn + 7
    finally:
        rig.close()


def test_ignored_reports_and_order_error(pkg, workload):
    rig = _rig(pkg, workload, 2, extra_dts=1)
    try:
        rig.forward(2)
        now = EPOCH + 2 * SEC
        d0 = next(d for d, m in enumerate(rig.models) if m.s.init and m.s.start_sn & 0xFFFF and
                  m.s.high_sn - m.s.start_sn > 100)
        m = rig.models[d0]
        never = _add_downtrack_like(rig, d0)
        gone = d0 + 1
        assert rig.models[gone].s.init
        assert rig.eng.api["remove_downtrack"](rig.eng.h, gone) == 0
        rig.models[gone].stop()
        assert rig.feedback([_ack(rig, d0, m.s.high_sn - 5)], now)[0][1] & FB_IGNORED == 0
        rig.check_state([d0, never, gone])
        before = rig.eng.sender_rtcp([d0, never, gone]).tobytes()
        cases = [_ack(rig, d0, m.s.high_sn - 60),           # stale: behind the last report
                 (d0, True, 0, 0, 0, 0, 0, 0, 0, 0),        # before the start SN (its low 16 bits are not 0)
                 (never, True, 500, 0, 0, 0, 0, 0, 0, 0),   # never forwarded
                 (gone, True, rr_lsn(rig.models[gone].s.high_sn, rig.models[gone].s.start_sn), 0, 0, 0, 0, 4, 1, 1)]
        want = rig.feedback(cases, now + SEC)
        assert [f for _, f in want] == [FB_IGNORED] * 4
        assert rig.eng.sender_rtcp([d0, never, gone]).tobytes() == before
        rig.check_state([d0, never, gone])
        # an ungrouped list
        ent = np.zeros(3, dtype=pkg.abi.RTCP_FB_DTYPE)
        ent["dt"] = [d0, gone, d0]
        out = np.zeros(3, dtype=pkg.abi.RTCP_FB_RESULT_DTYPE)
        assert rig.eng.api["rtcp_feedback"](rig.eng.h, ent.ctypes.data, 3, now, out.ctypes.data) == -34  # LKF_EORDER
        assert rig.eng.sender_rtcp([d0, never, gone]).tobytes() == before
    finally:
        rig.close()


def test_rtt(pkg, workload):
    rig = _rig(pkg, workload, 2)
    try:
        rig.forward(2)
        d = next(d for d, m in enumerate(rig.models) if m.s.init)
        m = rig.models[d]
        t0 = EPOCH + 2 * SEC
        rep = rig.sender_reports([(d, 0)], t0)[0]
        lsr = (rep["ntp"] >> 16) & 0xFFFFFFFF
        hi = m.s.high_sn
        # 1.5 s later, 1 s held at the receiver: 0.5 s
        rtt, fl = rig.feedback([_ack(rig, d, hi, lsr=lsr, dlsr=0x10000)], t0 + 3 * SEC // 2)[0]
        assert rtt == 500 and fl & FB_RTT_CHANGED  # (the first interval may also overflow the cache)
        # no LSR, and an LSR that is not the last report's: no RTT
        assert rig.feedback([_ack(rig, d, hi, lsr=0, dlsr=0x10000)], t0 + 2 * SEC)[0][0] == 0
        assert rig.feedback([_ack(rig, d, hi, lsr=lsr + 1, dlsr=0)], t0 + 2 * SEC)[0][0] == 0
        assert (m.rtt, m.max_rtt, m.snap["max_rtt"]) == (500, 500, 500)
        assert rig.feedback([_ack(rig, d, hi, lsr=lsr, dlsr=0)], t0 + 3 * SEC) == [(3000, FB_RTT_CHANGED)]
        assert rig.feedback([_ack(rig, d, hi, lsr=lsr, dlsr=0x38000)], t0 + 4 * SEC) == [(500, FB_RTT_CHANGED)]
        assert rig.feedback([_ack(rig, d, hi, lsr=lsr, dlsr=0x40000)], t0 + 4 * SEC + SEC // 2)[0] == (500, 0)
        assert (m.rtt, m.max_rtt, m.snap["max_rtt"]) == (500, 3000, 3000)
        rig.check_state([d])
    finally:
        rig.close()


def test_sender_reports(pkg, workload):
    rig = _rig(pkg, workload, 2, extra_dts=1)
    try:
        rig.forward(2)
        dts = [d for d, m in enumerate(rig.models) if m.s.init]
        never = _add_downtrack_like(rig, dts[0])
        t = EPOCH + 2 * SEC + 12345678
        first = rig.sender_reports([(never, 0)] + [(d, 0) for d in dts], t)
        assert first[0]["flags"] == 0
        assert all(r["flags"] & SR_VALID for r in first[1:])
        # packet and octet counts against the per-packet statistics
        ss = pkg.sender_stats(rig.eng.api, rig.eng.h, dts)
        for s, r in zip(ss, first[1:]):
            expected = int(s["ext_highest_sn"]) - int(s["ext_start_sn"]) + 1
            primary = expected - int(s["packets_lost"]) - int(s["packets_padding"])
            assert r["packet_count"] == (primary + int(s["packets_duplicate"]) + int(s["packets_padding"])) & 0xFFFFFFFF
            assert r["octet_count"] == (int(s["bytes"]) + int(s["bytes_duplicate"]) + int(s["bytes_padding"])) \
                & 0xFFFFFFFF
        rig.forward(1)
        second = rig.sender_reports([(d, 90000 if i % 2 else 0) for i, d in enumerate(dts)], t + SEC)
        assert all(r["flags"] & SR_VALID for r in second)
        # a report from a large calculated clock rate, then one without shortly after: behind, repaired
        a, b = dts[0], dts[2]
        before = rig.models[a].out_of_order_sr_count
        rig.sender_reports([(a, 10000000), (b, 0)], t + 2 * SEC)
        rep = rig.sender_reports([(b, 0), (a, 0)], t + 2 * SEC + 10**7)
        assert rep[1]["flags"] & SR_REPAIRED
        assert rig.models[a].out_of_order_sr_count == before + 1
        rig.check_state(dts + [never])
        # a DownTrack listed twice
        rq = np.array([(a, 0), (b, 0), (a, 0)], dtype=pkg.abi.RTCP_SR_REQ_DTYPE)
        out = np.zeros(3, dtype=pkg.abi.RTCP_SR_DTYPE)
        assert rig.eng.api["rtcp_sender_reports"](rig.eng.h, rq.ctypes.data, 3, t, out.ctypes.data, None) == -34
    finally:
        rig.close()


def test_sender_delta_info(pkg, workload):
    rig = _rig(pkg, workload, 2)
    try:
        rig.forward(2)
        dts = [d for d, m in enumerate(rig.models) if m.s.init][:40]
        assert rig.delta(dts) == [None] * len(dts)  # before any report
        rig.check_state(dts)
        rig.feedback([_ack(rig, d, rig.models[d].s.high_sn - 20, jitter=300 + d, counts=(2, 1, 0)) for d in dts],
                     EPOCH + 2 * SEC)
        # the zero snapshot is initialized here: nothing expected yet (rtpstats_sender.go:839-842, :751)
        assert rig.delta(dts) == [None] * len(dts)
        rig.check_state(dts)
        rig.forward(1)
        rig.feedback([_ack(rig, d, rig.models[d].s.high_sn, jitter=900 + d, counts=(3, 0, 1)) for d in dts],
                     EPOCH + 3 * SEC)
        got = rig.delta(dts)
        assert all(g is not None and g["packets"] > 0 for g in got)
        assert sum(g["bytes"] for g in got) > 0 and sum(g["frames"] for g in got) > 0
        rig.check_state(dts)
        assert rig.delta(dts) == [None] * len(dts)  # twice with no report in between
        rig.check_state(dts)
    finally:
        rig.close()


def test_seed_copies_the_rtcp_state(pkg, workload):
    rig = _rig(pkg, workload, 2, extra_dts=1)
    try:
        rig.forward(2)
        d = next(d for d, m in enumerate(rig.models) if m.s.init)
        m = rig.models[d]
        now = EPOCH + 2 * SEC
        rep = rig.sender_reports([(d, 0)], now)[0]
        rig.feedback([_ack(rig, d, m.s.high_sn - 9, now_lost=3, jitter=77, lsr=(rep["ntp"] >> 16) & 0xFFFFFFFF,
                           dlsr=100, counts=(5, 1, 1))], now + SEC // 4)
        rig.delta([d])
        rig.feedback([_ack(rig, d, m.s.high_sn - 4, now_lost=4, jitter=99)], now + SEC // 2)
        new = _add_downtrack_like(rig, d)
        for api, h in ((rig.eng.api, rig.eng.h), (rig.o.api, rig.oh)):
            assert api["sender_stats_seed"](h, new, d) == 0
        n = rig.models[new]
        n.s = copy.deepcopy(m.s)
        n.seed_from(m)
        rig.check_state([d, new])
        rows = rig.eng.sender_rtcp([d, new])
        not_seeded = ("end_time_ns", "clock_skew_count", "out_of_order_sender_report_count",
                      "metadata_cache_overflow_count")
        for k in rows.dtype.names:
            if k not in not_seeded:
                assert rows[0][k].tobytes() == rows[1][k].tobytes(), k
        assert int(rows[1]["snapshot"]["is_valid"]) == 1 and int(rows[1]["sr_newest"]["valid"]) == 1
        rig.feedback([_ack(rig, new, n.s.high_sn, now_lost=5, jitter=120)], now + SEC)
        rig.check_state([d, new])
    finally:
        rig.close()


def test_feedback_behind_queued_batches(pkg, workload):
    """lkf_rtcp_feedback with two batches still queued and no lkf_sync in between: the same as after a sync
    (the model has every packet of the queued batches)."""
    rig = _rig(pkg, workload, 2)
    try:
        rig.forward(2)
        rig.forward(2, sync=False)
        ent = [_ack(rig, d, m.s.high_sn, jitter=d) for d, m in enumerate(rig.models) if m.s.init]
        rig.feedback(ent, EPOCH + 4 * SEC)
        rig.check_state()
    finally:
        rig.close()
