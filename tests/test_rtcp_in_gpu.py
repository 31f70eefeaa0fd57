"""RTCP ingress on the GPU (lkf_rtcp_ingest, lkf_rtcp_ingested_nacks,
lkf_rtx_lookup_ingested; rtcp_kernels.hip k_rtcp_in_*): the compound packets
of tests/rtcp_wire_lib's marshaller through the engine, against

  - tests/rtcp_wire_lib.PyRtcpIn, the restatement of the parse (every result
    field, the fb records, the NACK list, the pass-through records),
  - tests/rtcp_lib.PyRtcp, the model of the RTCP state the reports update,
  - a twin engine driven through the struct calls lkf_rtcp_feedback /
    lkf_rtx_lookup, and the CPU oracle's lkf_rtx_lookup.

Each test runs small engines: one room, a few 1-s batches.
"""
import numpy as np
import pytest

from tests import pad_lib, rtcp_lib, rtx_lib
from tests import rtcp_wire_lib as W
from tests.rtcp_lib import ingest, pack, rr_lsn
from tests.rtcp_lib import ssrc as _ssrc

pytestmark = pytest.mark.gpu
EPOCH = 1700000000 * 10**9
SEC = 10**9


def _rig(pkg, workload, config, extra_dts=0, nb=4):
    kw = dict(loss=0.08) if config == 2 else {}
    tr = workload.Trace(config, rooms=1, duration_s=nb, batch_s=1.0, seed=1, **kw)
    return rtcp_lib.Rig(pkg, workload, tr, pkg.Engine.for_trace(tr, extra_dts=extra_dts))


def _block(rig, dt, esn, lost=0, jitter=0, lsr=0, dlsr=0):
    """A report block that acknowledges the DownTrack's sent extended SN `esn`."""
    return W.report_block(_ssrc(rig, dt), lost & 0xFF, lost, rr_lsn(esn, rig.models[dt].s.start_sn), jitter, lsr, dlsr)


def _compound_like_struct_entry(rig, ent):
    """The compound that carries one Rig.feedback tuple: its report, `nacks` sequence numbers, PLIs, FIRs."""
    dt, has_rr, lsn, lost, jit, lsr, dlsr, nacks, plis, firs = ent
    ssrc = _ssrc(rig, dt)
    pk = []
    if has_rr:
        pk.append(W.rr(1, [W.report_block(ssrc ^ 1), W.report_block(ssrc, 0, lost, lsn, jit, lsr, dlsr)]))
    pk.append(W.sdes(1))
    if nacks:
        pk.append(W.nack(1, ssrc, [(100 + 40 * k, 0) for k in range(nacks)]))
    pk += [W.pli(1, ssrc)] * plis + [W.fir(1, ssrc, [(ssrc, 3)])] * firs
    return W.compound(*pk)


@pytest.mark.parametrize("config", [2, 5])
def test_equals_the_struct_call(pkg, workload, config):
    """The same reports and counts as compounds through lkf_rtcp_ingest on one engine and as structs through
    lkf_rtcp_feedback on a twin: every DownTrack's lkf_sender_rtcp equal bit for bit, both equal to PyRtcp."""
    a, b = _rig(pkg, workload, config), _rig(pkg, workload, config)
    try:
        for k in range(3):
            now = EPOCH + (k + 1) * SEC
            for rig in (a, b):
                rig.forward(1)
                if k == 1:
                    assert rig.padding(pad_lib.make_reqs(rig.tr.ndts, seed=3, frac=0.7), now - 10**6) > 0
                    nacks = rtx_lib.make_nacks(rig.o.api, rig.oh, rig.tr, seed=5)
                    assert rig.rtx(nacks, now - 10**5) > 0
            lsr = 0
            if k == 2:  # a sender report first, so that the reports carry an RTT
                rep = [r.sender_reports([(d, 0) for d in range(r.tr.ndts)], now - SEC // 2) for r in (a, b)][0]
                lsr = [(x["ntp"] >> 16) & 0xFFFFFFFF for x in rep]
            ent = [(d, True, rr_lsn(m.s.high_sn if m.s.init else 0, m.s.start_sn), k + d % 3, 100 * k + d,
                    lsr[d] if lsr else 0, 0x4000 if lsr else 0, d % 4, k % 2, d % 2) for d, m in enumerate(a.models)]
            out, _, _ = ingest(a, [(e[0], _compound_like_struct_entry(a, e)) for e in ent], now)
            b.feedback(ent, now)
            if k == 2:
                assert any(int(x) for x in out["rtt_ms"])  # otherwise vacuous
            a.check_state()
            b.check_state()
            dts = list(range(a.tr.ndts))
            assert a.eng.sender_rtcp(dts).tobytes() == b.eng.sender_rtcp(dts).tobytes()
    finally:
        a.close()
        b.close()


def _nack_compounds(rig, nacks, split=True):
    """One entry per DownTrack of a NACK list (abi.NACK_DTYPE, grouped): its sequence numbers as NACK pairs, in
    two packets when there are enough."""
    entries, i = [], 0
    while i < len(nacks):
        d = int(nacks[i]["dt"])
        j = i
        while j < len(nacks) and int(nacks[j]["dt"]) == d:
            j += 1
        pairs = W.nack_pairs([int(x) for x in nacks["sn"][i:j]])
        h = len(pairs) // 2 if split else 0
        pk = [W.nack(1, _ssrc(rig, d), pairs[:h])] if h else []
        pk += [W.sdes(1), W.nack(1, _ssrc(rig, d), pairs[h:])]
        entries.append((d, W.compound(*pk)))
        i = j
    return entries


@pytest.mark.parametrize("config", [2, 5])
def test_nacks_to_rtx(pkg, workload, config):
    """The device-resident NACK list equals the restatement's, its lookup equals lkf_rtx_lookup of that list on
    a twin engine and on the oracle, the retransmissions' wire bytes are equal; a second round carries the NACK
    counts and the RTT suppression over."""
    a, b = _rig(pkg, workload, config), _rig(pkg, workload, config)
    try:
        for rig in (a, b):
            rig.forward(2)
        nacks = rtx_lib.make_nacks(a.o.api, a.oh, a.tr, seed=5)
        entries = _nack_compounds(a, nacks)
        idx = rtx_lib.packet_index(a.tr, a.b)
        names = [n for n in pkg.abi.RTX_DTYPE.names if n != "reserved"]
        total = 0
        for rnd, now in enumerate((EPOCH + 2 * SEC, EPOCH + 2 * SEC + 30 * 10**6, EPOCH + 2 * SEC + 400 * 10**6)):
            _, _, listed = ingest(a, entries, now)
            assert listed == [(int(x["dt"]), int(x["sn"])) for x in nacks]
            ga = a.eng.rtx_lookup_ingested(now)
            gb = rtx_lib.rtx_lookup(b.eng.api, b.eng.h, nacks, now)
            go = rtx_lib.rtx_lookup(a.o.api, a.oh, nacks, now)
            rtx_lib.rtx_lookup(b.o.api, b.oh, nacks, now)  # (the twin's oracle keeps step)
            assert ga.tobytes() == gb.tobytes(), rnd
            assert len(ga) == len(go) and all(np.array_equal(ga[n], go[n]) for n in names), rnd
            keys = set(zip(ga["dt"].tolist(), ga["target_sn"].tolist()))
            if rnd == 0:
                first = keys
            if rnd == 1:  # 30 ms after the first round: what it answered is suppressed
                assert len(first) > 0 and not (keys & first)
            total += len(ga)
            wa = rtx_lib.rtx_emit(a.eng.api, a.eng.h, a.tr, ga, idx)
            wb = rtx_lib.rtx_emit(b.eng.api, b.eng.h, b.tr, gb, idx)
            assert wa[0].tobytes() == wb[0].tobytes() and wa[1].tobytes() == wb[1].tobytes()
        assert total > 0 and int(ga["nacked"].max()) == 2
        # a DownTrack removed after the ingest answers nothing (the others' shares are packed on the device)
        gone = int(nacks[len(nacks) // 2]["dt"])
        now = EPOCH + 3 * SEC
        ingest(a, entries, now)
        for e in (a.eng, b.eng):
            assert e.api["remove_downtrack"](e.h, gone) == 0
        ga = a.eng.rtx_lookup_ingested(now)
        gb = rtx_lib.rtx_lookup(b.eng.api, b.eng.h, nacks, now)
        assert len(ga) > 0 and ga.tobytes() == gb.tobytes() and gone not in ga["dt"]
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("config", [2, 5])
def test_shared_bytes(pkg, workload, config):
    """One compound delivered to three DownTracks: an RR with blocks for two of them, a NACK for the third's
    SSRC and a PLI.  Each applies only its own block; all three count every sequence number and the PLI."""
    rig = _rig(pkg, workload, config, nb=2)
    try:
        rig.forward(2)
        d0, d1, d2 = [d for d, m in enumerate(rig.models) if m.s.init][:3]
        one = W.compound(W.rr(9, [_block(rig, d0, rig.models[d0].s.high_sn, jitter=11),
                                  _block(rig, d1, rig.models[d1].s.high_sn - 1, jitter=22)]),
                         W.nack(9, _ssrc(rig, d2), [(700, 0x0101), (900, 0)]), W.pli(9, _ssrc(rig, d2)))
        raws, arena, _ = pack(pkg, [(d0, one), (d1, one), (d2, one)])
        assert len(arena) == len(one) and len(set(raws["off"])) == 1
        before = rig.eng.sender_rtcp([d0, d1, d2])
        out, _, nacks = ingest(rig, [(d0, one), (d1, one), (d2, one)], EPOCH + 2 * SEC)
        assert [int(x) for x in out["reports"]] == [1, 1, 0]
        assert [int(x) for x in out["nacks"]] == [4, 4, 4] and [int(x) for x in out["plis"]] == [1, 1, 1]
        assert nacks == [(d, s) for d in (d0, d1, d2) for s in (700, 701, 709, 900)]
        after = rig.eng.sender_rtcp([d0, d1, d2])
        assert [int(x) for x in after["nacks"] - before["nacks"]] == [4, 4, 4]
        assert [int(x) for x in after["plis"] - before["plis"]] == [1, 1, 1]
        assert [float(x) for x in after["jitter_from_rr"]] == [11.0, 22.0, float(before["jitter_from_rr"][2])]
        rig.check_state([d0, d1, d2])
    finally:
        rig.close()


@pytest.mark.parametrize("config", [2, 5])
def test_malformed_between_good(pkg, workload, config):
    rig = _rig(pkg, workload, config, nb=2)
    try:
        rig.forward(2)
        dts = [d for d, m in enumerate(rig.models) if m.s.init][:6]
        good = lambda d: W.compound(W.rr(9, [_block(rig, d, rig.models[d].s.high_sn, jitter=5 + d)]),  # noqa: E731
                                    W.nack(9, 0, [(d, 3)]), W.pli(9, 0), W.remb(9, ssrcs=[1]))
        bad = [good(dts[1])[:-2],                                # truncated inside the last packet
               good(dts[3]) + W._hdr(4, 206, b"\0" * 12),        # a FIR of 16 bytes after valid packets
               good(dts[4]) + b"\x40\xc9\0\0"]                  # version 1
        entries = [(dts[0], good(dts[0])), (dts[1], bad[0]), (dts[2], good(dts[2])), (dts[3], bad[1]),
                   (dts[4], bad[2]), (dts[5], good(dts[5]))]
        void = [dts[1], dts[3], dts[4]]
        before = rig.eng.sender_rtcp(void).tobytes()
        out, res, nacks = ingest(rig, entries, EPOCH + 2 * SEC)
        assert [int(x) for x in out["status"]] == [0, 1, 0, 1, 1, 0]
        assert all(int(out[i]["pli_layer"]) == -1 and int(out[i]["rtt_ms"]) == 0 for i in (1, 3, 4))
        assert rig.eng.sender_rtcp(void).tobytes() == before
        assert sorted(set(d for d, _ in nacks)) == [dts[0], dts[2], dts[5]]
        assert [int(x) for x in rig.eng.sender_rtcp([dts[0], dts[2], dts[5]])["plis"]] == [1, 1, 1]
        rig.check_state(dts)
    finally:
        rig.close()


@pytest.mark.parametrize("config", [2, 5])
def test_shapes(pkg, workload, config):
    """0, 1, 63, 64, 65 and 129 entries: three per DownTrack for the first 22 (the 22nd group straddles index
    64), seven for the rest, with 0, 1 and 3 reports; the last entry ends exactly at arena_len; every other call
    starts the arena at an odd offset."""
    rig = _rig(pkg, workload, config, nb=2)
    try:
        rig.forward(2)
        live = [d for d, m in enumerate(rig.models) if m.s.init and m.s.high_sn - m.s.start_sn > 64]
        assert len(live) >= 10
        # (a small trace has fewer: the others' reports are ignored, which the model restates too)
        dts = sorted((live + [d for d in range(rig.tr.ndts) if d not in live])[:31])
        assert len(dts) == 31
        acked = {d: (rig.models[d].s.high_sn - 60 if d in live else 1000) for d in dts}

        def blocks(d, k):
            out = []
            for _ in range(k):
                acked[d] += 1
                out.append(_block(rig, d, acked[d], jitter=acked[d] & 0xFF))
            return out

        for call, n in enumerate((0, 1, 63, 64, 65, 129)):
            entries = []
            for i in range(n):
                d = dts[i // 3] if i < 66 else dts[22 + (i - 66) // 7]
                if i % 3 == 0:
                    data = W.compound(W.pli(9, 0), W.sdes(9))
                elif i % 3 == 1:
                    data = W.compound(W.rr(9, blocks(d, 1)), W.nack(9, 0, [(i, i & 0xFFFF)]))
                else:
                    b3 = blocks(d, 3)
                    data = W.compound(W.rr(9, b3[:2] + [W.report_block(1)]), W.twcc(9, _ssrc(rig, d)), W.rr(9, b3[2:]))
                entries.append((d, data))
            raws, arena, _ = pack(pkg, entries, front=call % 2)
            if n:
                assert int(raws["off"][-1]) + int(raws["len"][-1]) == len(arena)
                assert (int(raws["off"][0]) & 1) == call % 2
            out, res, _ = ingest(rig, entries, EPOCH + (2 + call) * SEC, front=call % 2)
            assert [r["reports"] for r in res] == [(0, 1, 3)[i % 3] for i in range(n)]
            if n > 65:
                assert entries[63][0] == entries[64][0] == entries[65][0]
            rig.check_state(dts)
        assert rig.eng.rtcp_ingested_nacks().size > 0
        ingest(rig, [], EPOCH + 9 * SEC)  # an empty call empties the NACK list
        assert len(rig.eng.rtx_lookup_ingested(EPOCH + 9 * SEC)) == 0
    finally:
        rig.close()


@pytest.mark.parametrize("config", [2, 5])
def test_pli_layer(pkg, workload, config):
    from tests.test_alloc_gpu import allocate, make_alloc_reqs
    import ctypes as C
    rig = _rig(pkg, workload, config, extra_dts=1, nb=2)
    try:
        rig.forward(2)
        abi = pkg.abi
        reqs = make_alloc_reqs(abi, rig.tr.ndts, seed=4)
        reqs["bitrates"][::3] = 0  # a dry feed: no target, so no valid request layer
        reqs["available_layers"][::3] = 0
        al = allocate(rig.eng.api, rig.eng.h, reqs, abi)
        want = {}
        for r in al:
            d = int(r["dt"])
            video = int(rig.tr.tracks[rig.tr.downtracks[d].track].kind) == abi.LKF_KIND_VIDEO
            valid = int(r["target_spatial"]) != -1 and int(r["target_temporal"]) != -1
            if video:
                want[d] = int(r["request_spatial"]) if valid else -1
        assert any(v >= 0 for v in want.values())
        # one more video DownTrack, never allocated: its request layer is invalid
        p = rig.tr.downtracks[next(d for d in sorted(want) if want[d] >= 0)]
        new = rig.eng.api["add_downtrack"](rig.eng.h, C.byref(p))
        assert new == rig.o.api["add_downtrack"](rig.oh, C.byref(p)) == len(rig.models)
        rig.models.append(rtcp_lib.PyRtcp(rtcp_lib.PySender(int(rig.tr.tracks[p.track].clock_rate))))
        want[new] = -1
        dts = [new] + sorted(d for d in want if d != new)  # (its entry is a PLI)
        kinds = (W.pli(9, 0), W.fir(9, 0), W.sdes(9), W.compound(W.fir(9, 0), W.pli(9, 0)))
        entries = [(d, kinds[i % 4]) for i, d in enumerate(dts)]
        out, _, _ = ingest(rig, entries, EPOCH + 2 * SEC)
        assert [int(x) for x in out["pli_layer"]] == [-1 if i % 4 == 2 else want[d] for i, d in enumerate(dts)]
    finally:
        rig.close()


@pytest.mark.parametrize("config", [2, 5])
def test_refs_and_capacities(pkg, workload, config):
    rig = _rig(pkg, workload, config, nb=2)
    try:
        rig.forward(2)
        abi = pkg.abi
        d0, d1 = [d for d, m in enumerate(rig.models) if m.s.init][:2]
        e0 = W.compound(W.remb(9, ssrcs=[5, 6]), W.twcc(9, _ssrc(rig, d0)), W.twcc(9, _ssrc(rig, d1)), W.remb(9))
        e1 = W.compound(W.twcc(9, _ssrc(rig, d0), b"\1" * 12), W.twcc(9, _ssrc(rig, d1), b"\2" * 12),
                        W.rr(9, [_block(rig, d1, rig.models[d1].s.high_sn), _block(rig, d1, rig.models[d1].s.high_sn)]))
        entries = [(d0, e0), (d1, e1)]
        raws, arena, _ = pack(pkg, entries)
        # short capacities first, on the raw call: the needed counts, out[] filled, state applied
        out = np.zeros(2, dtype=abi.RTCP_IN_RESULT_DTYPE)
        fb, fbo = np.zeros(3, dtype=abi.RTCP_FB_DTYPE), np.zeros(3, dtype=abi.RTCP_FB_RESULT_DTYPE)
        refs = np.zeros(4, dtype=abi.RTCP_REF_DTYPE)
        ar = np.frombuffer(arena, dtype=np.uint8)
        import ctypes as C
        nfb, nref, nn = C.c_uint32(), C.c_uint32(), C.c_uint32()

        def call(fb_cap, ref_cap, now):
            return rig.eng.api["rtcp_ingest"](rig.eng.h, raws.ctypes.data, 2, ar.ctypes.data, len(ar), now,
                                              out.ctypes.data, fb.ctypes.data, fbo.ctypes.data, fb_cap, C.byref(nfb),
                                              refs.ctypes.data, ref_cap, C.byref(nref), C.byref(nn))

        assert call(2, 4, EPOCH + 2 * SEC) == -28 and (nfb.value, nref.value) == (3, 4)
        assert call(3, 3, EPOCH + 2 * SEC) == -28 and (nfb.value, nref.value) == (3, 4)
        assert [int(x) for x in out["ref_count"]] == [3, 1] and [int(x) for x in out["fb_count"]] == [1, 2]
        for _ in range(2):  # (the model follows the two calls that were applied)
            m = rig.models[d1]
            for _ in range(2):
                m.receiver_report(EPOCH + 2 * SEC, rr_lsn(m.s.high_sn, m.s.start_sn), 0, 0, 0, 0)
        rig.check_state([d0, d1])
        out2, res, _ = ingest(rig, entries, EPOCH + 3 * SEC)
        kinds = [abi.LKF_RTCP_REF_REMB, abi.LKF_RTCP_REF_TWCC, abi.LKF_RTCP_REF_REMB, abi.LKF_RTCP_REF_TWCC]
        assert call(3, 4, EPOCH + 4 * SEC) == 0
        assert [int(x) for x in refs["kind"]] == kinds and [int(x) for x in refs["entry"]] == [0, 0, 0, 1]
        assert bytes(arena[int(refs[3]["off"]):int(refs[3]["off"]) + int(refs[3]["len"])]) == \
            W.twcc(9, _ssrc(rig, d1), b"\2" * 12)
    finally:
        rig.close()


@pytest.mark.parametrize("config", [2, 5])
def test_behind_queued_batches(pkg, workload, config):
    """lkf_rtcp_ingest with two batches still queued and no lkf_sync in between: the same as after a sync."""
    rig = _rig(pkg, workload, config)
    try:
        rig.forward(2)
        rig.forward(2, sync=False)
        entries = [(d, W.compound(W.rr(9, [_block(rig, d, m.s.high_sn, jitter=d)]), W.pli(9, 0)))
                   for d, m in enumerate(rig.models) if m.s.init]
        ingest(rig, entries, EPOCH + 4 * SEC)
        rig.check_state()
    finally:
        rig.close()


@pytest.mark.parametrize("config", [2, 5])
def test_error_paths(pkg, workload, config):
    import ctypes as C
    rig = _rig(pkg, workload, config, nb=2)
    try:
        rig.forward(2)
        abi = pkg.abi
        d0, d1 = [d for d, m in enumerate(rig.models) if m.s.init][:2]
        entries = [(d0, W.compound(W.rr(9, [_block(rig, d0, rig.models[d0].s.high_sn)]), W.nack(9, 0, [(5, 0)]))),
                   (d1, W.pli(9, 0))]
        ingest(rig, entries, EPOCH + 2 * SEC)
        before = rig.eng.sender_rtcp([d0, d1]).tobytes()
        listed = rig.eng.rtcp_ingested_nacks().tobytes()
        good = W.compound(W.rr(9, [_block(rig, d0, rig.models[d0].s.high_sn)]), W.pli(9, 0))
        ar = np.frombuffer(good, dtype=np.uint8)
        out = np.zeros(3, dtype=abi.RTCP_IN_RESULT_DTYPE)
        fb, fbo = np.zeros(8, dtype=abi.RTCP_FB_DTYPE), np.zeros(8, dtype=abi.RTCP_FB_RESULT_DTYPE)
        refs = np.zeros(8, dtype=abi.RTCP_REF_DTYPE)
        nfb, nref = C.c_uint32(), C.c_uint32()

        def call(rows, ar=ar):
            raws = np.array(rows, dtype=abi.RTCP_RAW_DTYPE)
            return rig.eng.api["rtcp_ingest"](rig.eng.h, raws.ctypes.data, len(raws), ar.ctypes.data, len(ar),
                                              EPOCH + 3 * SEC, out.ctypes.data, fb.ctypes.data, fbo.ctypes.data, 8,
                                              C.byref(nfb), refs.ctypes.data, 8, C.byref(nref), None)

        assert call([(d0, 0, len(good)), (d1, 0, len(good)), (d0, 0, len(good))]) == -34  # LKF_EORDER
        assert call([(d0, 0, len(good)), (d1, 4, len(good))]) == -22                     # beyond the arena
        assert call([(d0, len(good), 1)]) == -22
        assert call([(rig.tr.ndts + 5, 0, len(good))]) == -22
        big = np.zeros(abi.LKF_RTCP_MAX_LEN + 1, dtype=np.uint8)  # inside its arena, longer than a datagram
        assert call([(d0, 0, len(big))], big) == -22
        assert rig.eng.sender_rtcp([d0, d1]).tobytes() == before
        assert rig.eng.rtcp_ingested_nacks().tobytes() == listed  # the last good call's list is still there
        assert call([(d0, len(good), 0)]) == 0 and int(out[0]["status"]) == 1  # an empty entry at the arena's end
    finally:
        rig.close()
