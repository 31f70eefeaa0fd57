"""The dependency-descriptor frame-rate calculator on the GPU
(lkf_stream_fps_enable_dd, lkf_stream_fps_dd_get, lkf_stream_fps_get,
lkf_ingest_fps_changed; ingress_kernels.hip k_ing_fps_dd over fps_dd_device.h)
against tests/fps_dd_lib.PyFpsDD, which restates fps.go the way the Go is
written.  The model is fed from lkf_ingest_flows of the same run, so nothing
here restates ingress; after every ingest the whole calculator state and the
whole lkf_stream_fps are compared, rates as binary32 bits.  Small engines, real
RTP datagrams whose dependency descriptors come from the writer of fps_dd_lib.
"""
import ctypes as C

import numpy as np
import pytest

from tests import fps_dd_lib as D
from tests import fps_lib as F
from tests.fps_dd_lib import PyFpsDD
from tests.fps_lib import PyFps
from tests.test_fps_gpu import EINVAL, KIND_AUDIO, KIND_VIDEO, OPUS, VP8C, VP9C, Rig, ssrc_of, vp8_stream

pytestmark = pytest.mark.gpu
AV1C = 5
DDX = {"dd_ext": 5}
T3 = (0, 2, 1, 2)


class DDRig(Rig):
    """Rig whose step feeds PyFpsDD models (with the parser each needs) and
    compares both state structs of every DD stream after the ingest."""

    def dd_step(self, items, models, parsers, others=None):
        before = {s: m.calculated for s, m in models.items()}
        flows = self.ingest(items)
        for (s, row), fl in zip(items, flows):
            if s in models:
                D.feed(models[s], parsers[s], [row], [fl])
            elif others and s in others:
                F.feed(others[s], [row], [fl])
        for s, m in models.items():
            got = self.eng.stream_fps_dd_get(s).as_dict()
            assert got == m.dd_state(), (s, got, m.dd_state())
            assert self.state(s) == m.state(), (s, self.state(s), m.state())
        changed = sorted(s for s, m in models.items() if m.calculated and not before[s])
        return changed, flows


def l1t3_rows(handle, n, start_fn=100, start_ts=12345678, st=None, vp8=True, first_key=True, step=3000):
    """n single-packet L1T3 frames; the first attaches the structure."""
    st = st or D.l1t3_structure()
    ds = D.DDStream(handle, ssrc_of(handle))
    for i in range(n):
        fn, ts, t = (start_fn + i) & 0xFFFF, (start_ts + i * step) & 0xFFFFFFFF, T3[i % 4]
        key = i == 0 and first_key
        ds.frame(fn, ts, 0 if key else 1 + t if t else 1, structure=st if key else None,
                 payload=F.vp8_payload(fn & 0x7FFF, t, key=key) if vp8 else None)
        if i == 0 and not first_key:
            ds.structure = st
    return ds


def test_l1t3_vp8_batch_sizes(pkg, abi):
    """VP8 with a descriptor, one packet per frame, 100 frames, in ingests of 1, 7, 64 and 65 datagrams: the
    state after every ingest is the model's, and lkf_ingest_fps_changed names the stream in exactly the
    completing ingest."""
    sizes = (1, 7, 64, 65)
    rig = DDRig(pkg, abi, [(KIND_VIDEO, VP8C, 90000)] * 4, [(t, 0, DDX) for t in range(4)])
    try:
        for s in range(4):
            rig.eng.stream_fps_enable_dd(s)
            rig.eng.stream_fps_enable_dd(s)  # idempotent
            assert rig.eng.stream_fps_dd_get(s).as_dict() == PyFpsDD().dd_state()
            assert rig.state(s) == PyFpsDD().state()
        assert rig.eng.ingest_fps_changed() == []
        finals = []
        for s, b in enumerate(sizes):
            rows = l1t3_rows(s, 100).rows
            m, p = {s: PyFpsDD(vp8=True)}, {s: D.Parser()}
            hits = 0
            for lo in range(0, len(rows), b):
                changed, flows = rig.dd_step([(s, r) for r in rows[lo:lo + b]], m, p)
                assert all(int(f["flags"]) & F.FLOW_FORWARD for f in flows)
                assert rig.eng.ingest_fps_changed() == changed, (b, lo)
                hits += len(changed)
            assert hits == 1 and m[s].calculated and (m[s].max_spatial, m[s].max_temporal) == (0, 2)
            finals.append((rig.state(s), rig.eng.stream_fps_dd_get(s).as_dict()))
        assert all(f == finals[0] for f in finals)
        for want, r in zip((7.5, 15, 30), rig.eng.stream_fps_get(0).fps[0]):
            assert want * 0.8 <= r <= want * 1.2  # (8 frames over 7 periods: the reference's own count)
    finally:
        rig.close()


def l3t3_rows(handle, units, mask_at=None, mask=0x3F, drop_s2_after=None, start_fn=40000, start_ts=5000):
    st = D.l3t3_structure()
    ds = D.DDStream(handle, ssrc_of(handle))
    fn = start_fn
    for u in range(units):
        t = T3[u % 4]
        for s in range(3):
            if drop_s2_after is not None and s == 2 and u > drop_s2_after:
                continue
            kw = {}
            if u == 0:  # the key unit: nothing earlier to depend on but the layer below
                kw = dict(structure=st if s == 0 else None, custom_fdiffs=[1] if s else [])
            if u == mask_at and s == 0:
                kw["active_mask"] = mask
            ds.frame(fn, start_ts + u * 3000, 3 * s + t, packets=2, **kw)
            fn = (fn + 1) & 0xFFFF
    return ds


def test_l3t3_mask_change_drops_a_spatial_layer(pkg, abi):
    """L3T3 with inter-layer frame diffs, two packets per frame (the second is a frame already received), the
    structure attached to the key frame in a two-byte extension element; an active mask without the S2
    targets arrives later and the calculator completes on 2 x 3."""
    rig = DDRig(pkg, abi, [(KIND_VIDEO, AV1C, 90000)], [(0, 0, DDX)], max_pkts=1024)
    try:
        rig.eng.stream_fps_enable_dd(0)
        rows = l3t3_rows(0, 56, mask_at=9, drop_s2_after=14).rows
        assert len(rows[0][0]) > 12 + 4 + 2 + 16  # the attach does not fit a one-byte element
        m, p = {0: PyFpsDD()}, {0: D.Parser()}
        hits, cuts = [], (0, 50, 61, 200, len(rows))
        for lo, hi in zip(cuts, cuts[1:]):
            changed, _ = rig.dd_step([(0, r) for r in rows[lo:hi]], m, p)
            assert rig.eng.ingest_fps_changed() == changed
            hits += changed
            if hi == 50:
                assert (m[0].max_spatial, m[0].max_temporal) == (2, 2)
        assert hits == [0] and (m[0].max_spatial, m[0].max_temporal) == (1, 2)
        assert all(r > 0 for row in m[0].rates[:2] for r in row[:3]) and m[0].rates[0][3] == 0
    finally:
        rig.close()


def test_custom_frame_diffs(pkg, abi):
    """Custom lists of every length and nibble count, one longer than the eight a parsed descriptor keeps
    inline, a diff of 4096, custom lists behind an active mask and behind a second attached structure."""
    rig = DDRig(pkg, abi, [(KIND_VIDEO, AV1C, 90000)], [(0, 0, DDX)])
    try:
        rig.eng.stream_fps_enable_dd(0)
        st = D.l1t3_structure(sid=60)  # (template ids wrap past 63)
        ds = D.DDStream(0, ssrc_of(0))
        for i in range(110):
            fn, ts, t = 300 + i, 1000 + i * 3000, T3[i % 4]
            kw, tmpl = {}, 1 + t if t else 1
            own = [(4, 2, 1)[t]]
            if i == 0:
                kw, tmpl = dict(structure=st, custom_fdiffs=[]), 0
            elif i in (1, 2, 3):
                kw = dict(custom_fdiffs=[i])  # all the way back to the key frame
            elif i % 10 == 5:
                kw = dict(custom_fdiffs=own + [1, 2, 3, 5, 7, 9, 11, 13, 200, 4096],
                          fdiff_nibbles=(None, 3)[i % 20 == 5])
            elif i % 10 == 6:
                kw = dict(custom_fdiffs=own * 2, active_mask=0b111)  # (the same mask: no max-layer change)
            elif i == 47:
                kw = dict(structure=st, custom_fdiffs=own + [3, 3, 17, 257, 4, 5, 6, 7, 8])  # attach + 10 diffs
            elif i % 10 == 8:
                kw = dict(custom_fdiffs=[])  # an empty custom list: no dependency at all
            ds.frame(fn, ts, tmpl, **kw)
        assert any(r[7] is not None and len(r[7]) > 8 for r in ds.rows)
        assert any(r[7] is not None and 4096 in r[7] for r in ds.rows)
        m, p = {0: PyFpsDD()}, {0: D.Parser()}
        hits = []
        for lo in range(0, len(ds.rows), 23):
            changed, flows = rig.dd_step([(0, r) for r in ds.rows[lo:lo + 23]], m, p)
            assert all(int(f["flags"]) & F.FLOW_FORWARD for f in flows)
            hits += changed
        assert hits == [0]
    finally:
        rig.close()


def test_stream_faults(pkg, abi):
    """Loss, duplicates, a swap, a frame-number jump of 256 or more, a start at frame number 65516 (the
    16-bit wrap inside the window), a datagram without the extension and a padding-only datagram."""
    rig = DDRig(pkg, abi, [(KIND_VIDEO, VP8C, 90000)] * 2, [(0, 0, dict(DDX, nack=1)), (1, 0, DDX)], max_pkts=2048)
    try:
        for s in (0, 1):
            rig.eng.stream_fps_enable_dd(s)
        a = l1t3_rows(0, 140, start_fn=1000)
        # ... and 140 more frames 300 frame numbers on, their sequence numbers following
        tail2 = D.DDStream(0, ssrc_of(0), sn0=a.sn)
        tail2.structure = a.structure
        for i in range(140):
            fn, t = (1000 + 140 + 300 + i) & 0xFFFF, T3[i % 4]
            tail2.frame(fn, 12345678 + (140 + i) * 3000, 1 + t if t else 1, payload=F.vp8_payload(fn & 0x7FFF, t))
            if i == 20:
                tail2.frame(fn, 12345678 + (140 + i) * 3000, 1, ext=False, payload=F.vp8_payload(fn & 0x7FFF, 0))
            if i == 30:
                tail2.frame(fn, 12345678 + (140 + i) * 3000, 1, payload=b"", padding=8)
        rows = list(a.rows) + tail2.rows
        del rows[8:10]  # loss: the chains through these frames stall until the jump resets the window
        rows[20], rows[21] = rows[21], rows[20]
        rows[33], rows[36] = rows[36], rows[33]
        for i in (5, 40, 150):
            rows.insert(i + 3, rows[i])
        b = l1t3_rows(1, 420, start_fn=65516, start_ts=(1 << 32) - 100 * 3000)
        items, ka, kb = [], 0, 0
        while ka < len(rows) or kb < len(b.rows):
            if ka < len(rows):
                items.append((0, rows[ka]))
                ka += 1
            if kb < len(b.rows):
                items.append((1, b.rows[kb]))
                kb += 1
        m = {0: PyFpsDD(vp8=True), 1: PyFpsDD(vp8=True)}
        p = {0: D.Parser(), 1: D.Parser()}
        seen, hits = 0, []
        for lo in range(0, len(items), 97):
            changed, flows = rig.dd_step(items[lo:lo + 97], m, p)
            assert rig.eng.ingest_fps_changed() == changed
            seen |= int(np.bitwise_or.reduce([int(f["flags"]) for f in flows]))
            hits += changed
        assert seen & F.FLOW_PADDING and seen & 0x02 and seen & 0x04 and seen & 0x08
        assert sorted(hits) == [0, 1]
        assert m[0].resets >= 2  # the jump
        assert m[1].resets >= 2  # nothing completes across the wrap: only after the window ran out
    finally:
        rig.close()


def test_two_keyframes_with_different_structures_in_one_ingest(pkg, abi):
    """Two attached structures with different ids, layers and template diffs inside one ingest, frames of
    each before and after: every datagram is read with the structure that was in force for it."""
    rig = DDRig(pkg, abi, [(KIND_VIDEO, AV1C, 90000)], [(0, 0, DDX)])
    try:
        rig.eng.stream_fps_enable_dd(0)
        sa = D.l1t3_structure(sid=3)
        sw, np_ = D.SWITCH, D.NOT_PRESENT
        sb = D.Structure(20, [(0, 0, [sw, sw], []), (0, 0, [sw, sw], [2]), (0, 1, [np_, sw], [1])], 2)  # L1T2
        ds = D.DDStream(0, ssrc_of(0))
        for i in range(30):
            t = T3[i % 4]
            ds.frame(700 + i, 900 + i * 3000, 0 if i == 0 else 1 + t if t else 1, structure=sa if i == 0 else None)
        for i in range(30, 130):
            t = i % 2
            ds.frame(700 + i, 900 + i * 3000, 0 if i == 30 else 1 + t, structure=sb if i == 30 else None,
                     custom_fdiffs=[] if i == 31 else None)
        m, p = {0: PyFpsDD()}, {0: D.Parser()}
        hits = []
        for lo, hi in ((0, 1), (1, 90), (90, 130)):  # (the second ingest: frames of A, B's key frame, frames of B)
            changed, flows = rig.dd_step([(0, r) for r in ds.rows[lo:hi]], m, p)
            assert all(int(f["flags"]) & F.FLOW_FORWARD for f in flows)
            hits += changed
            if hi == 90:  # A's mask 0b111, then B's 0b11: the max layer went (0, 2) -> (0, 1)
                assert (m[0].max_spatial, m[0].max_temporal) == (0, 1)
        assert hits == [0] and m[0].rates[0][1] > 0 and m[0].rates[0][2] == 0
    finally:
        rig.close()


def test_enable_after_the_structure_has_arrived(pkg, abi):
    """The calculator starts from the parser's structure and active mask (no reference counterpart: the
    model is given both, as the engine documents)."""
    rig = DDRig(pkg, abi, [(KIND_VIDEO, VP8C, 90000)], [(0, 0, DDX)])
    try:
        ds = l1t3_rows(0, 120)
        flows = rig.ingest([(0, r) for r in ds.rows[:15]])
        assert rig.eng.ingest_fps_changed() == []
        rig.eng.stream_fps_enable_dd(0)
        m = {0: PyFpsDD(vp8=True)}
        m[0].set_max_layer(*ds.structure.max_layer(0b111))
        p = {0: D.Parser(ds.structure, 0b111, int(flows[0]["ext_sn"]))}
        assert rig.eng.stream_fps_dd_get(0).as_dict() == m[0].dd_state()
        hits = []
        for lo in range(15, 120, 40):
            hits += rig.dd_step([(0, r) for r in ds.rows[lo:lo + 40]], m, p)[0]
        assert hits == [0] and (m[0].max_spatial, m[0].max_temporal) == (0, 2)
    finally:
        rig.close()


def _mixed(pkg, abi, enable):
    rig = DDRig(pkg, abi, [(KIND_VIDEO, VP8C, 90000), (KIND_VIDEO, AV1C, 90000)], [(0, 0, {}), (1, 0, DDX)],
                max_pkts=1024)
    out = []
    try:
        if enable:
            rig.eng.stream_fps_enable(0)
            rig.eng.stream_fps_enable_dd(1)
        v = vp8_stream(0, n=150)
        d = l1t3_rows(1, 150, vp8=False)
        items = [x for pair in zip(((0, r) for r in v.rows), ((1, r) for r in d.rows)) for x in pair]
        mv, md, pd = {0: PyFps(F.VP8)}, {1: PyFpsDD()}, {1: D.Parser()}
        hits = []
        for lo in range(0, len(items), 60):
            part = items[lo:lo + 60]
            if enable:
                changed, flows = rig.dd_step(part, md, pd, others=mv)
                assert rig.state(0) == mv[0].state()
                got = rig.eng.ingest_fps_changed()
                assert [s for s in got if s == 1] == changed
                hits += got
                flows = rig.eng.flows()
            else:
                rig.ingest(part)
                flows = rig.eng.flows()
            npk = C.c_uint32()
            assert rig.eng.api["ingested"](rig.eng.h, None, 0, C.byref(npk)) in (0, -28)
            pk = (abi.lkf_pkt * max(1, npk.value))()
            assert rig.eng.api["ingested"](rig.eng.h, pk, npk.value, C.byref(npk)) == 0
            out.append((flows.tobytes(), C.string_at(pk, C.sizeof(abi.lkf_pkt) * npk.value)))
        out.append(tuple(rig.eng.stream_stats(s) for s in (0, 1)))
        return out, hits
    finally:
        rig.close()


def test_vp8_and_dd_streams_in_one_engine_and_a_twin_with_nothing_enabled(pkg, abi):
    """Both kernels on the side stream in one ingest: the VP8 stream's state still equals PyFps, the DD
    stream's PyFpsDD, the changed list merges both ascending; flows, ExtPackets and stream statistics equal,
    byte for byte, those of a twin engine with nothing enabled."""
    got, hits = _mixed(pkg, abi, True)
    want, _ = _mixed(pkg, abi, False)
    assert sorted(hits) == [0, 1]
    assert len(got) == len(want)
    for b, (g, w) in enumerate(zip(got, want)):
        assert g == w, b


def test_refusals(pkg, abi):
    tracks = [(KIND_AUDIO, OPUS, 48000), (KIND_VIDEO, VP8C, 90000), (KIND_VIDEO, VP9C, 90000)]
    rig = DDRig(pkg, abi, tracks, [(0, 0, {}), (1, 0, {}), (2, 0, DDX), (0, 0, DDX)])
    try:
        en, old = rig.eng.api["stream_fps_enable_dd"], rig.eng.api["stream_fps_enable"]
        assert en(rig.eng.h, 0) == EINVAL  # an audio stream
        assert en(rig.eng.h, 3) == EINVAL  # ... even with the extension
        assert en(rig.eng.h, 1) == EINVAL  # a video stream without a dependency descriptor
        assert en(rig.eng.h, 4) == EINVAL and en(rig.eng.h, -1) == EINVAL  # no such stream
        assert old(rig.eng.h, 2) == EINVAL  # the PictureID calculators still refuse a DD stream
        st = abi.lkf_fps_dd()
        assert rig.eng.api["stream_fps_dd_get"](rig.eng.h, 2, C.byref(st)) == EINVAL  # never enabled
        assert rig.eng.api["stream_fps_dd_get"](rig.eng.h, 9, C.byref(st)) == EINVAL
        assert rig.state(2) == F.zero_state()
        assert en(rig.eng.h, 2) == 0
        assert rig.state(2) == PyFpsDD().state()
        assert rig.eng.stream_fps_dd_get(2).as_dict() == PyFpsDD().dd_state()
    finally:
        rig.close()


def test_removed_track(pkg, abi):
    """A closed stream's calculator stops where it was and answers its last state."""
    rig = DDRig(pkg, abi, [(KIND_VIDEO, VP8C, 90000)] * 2, [(0, 0, DDX), (1, 0, DDX)])
    try:
        for s in (0, 1):
            rig.eng.stream_fps_enable_dd(s)
        a, b = l1t3_rows(0, 100), l1t3_rows(1, 100, start_fn=9)
        m = {0: PyFpsDD(vp8=True), 1: PyFpsDD(vp8=True)}
        p = {0: D.Parser(), 1: D.Parser()}
        rig.dd_step([(0, r) for r in a.rows[:20]] + [(1, r) for r in b.rows[:20]], m, p)
        assert rig.eng.api["remove_track"](rig.eng.h, 0) == 0
        frozen = rig.eng.stream_fps_dd_get(0).as_dict()
        assert frozen["has_base"] == 1
        changed, flows = rig.dd_step([(0, r) for r in a.rows[20:]] + [(1, r) for r in b.rows[20:]], m, p)
        assert not any(int(f["flags"]) & F.FLOW_FORWARD for f in flows[:80])
        assert changed == [1] and rig.eng.ingest_fps_changed() == [1]
        assert rig.eng.stream_fps_dd_get(0).as_dict() == frozen and not m[0].calculated
    finally:
        rig.close()
