"""The ingress frame-rate calculators on the GPU (lkf_stream_fps_enable,
lkf_stream_fps_get, lkf_ingest_fps_changed; ingress_kernels.hip k_ing_fps over
fps_device.h) against tests/fps_lib.PyFps.  The model is fed from
lkf_ingest_flows of the same run (an ExtPacket with a payload is what reaches
doFpsCalc), so nothing here restates ingress.  The whole lkf_stream_fps is
compared, rates as binary32 bits, state fields included, so a divergence
shows before completion and not only in the final rates.  Small engines, real
VP8 / VP9 RTP datagrams from the trace builder of tests/fps_lib.
"""
import ctypes as C

import numpy as np
import pytest

from tests import fps_lib as F
from tests.fps_lib import PyFps

pytestmark = pytest.mark.gpu
T0 = 1700000000 * 10**9
MS = 10**6
KIND_VIDEO, KIND_AUDIO = 1, 0
OPUS, VP8C, H264C, VP9C = 1, 2, 3, 4
EINVAL, ENOSPC = -22, -28
FULL = (7.5, 15, 30)


class Rig:
    """An engine with `tracks` [(kind, codec, clock)] and `streams` [(track, layer, params)]."""

    def __init__(self, pkg, abi, tracks, streams, max_pkts=4096):
        self.pkg, self.abi = pkg, abi
        self.eng = pkg.Engine(max_tracks=len(tracks) + 4, max_downtracks=16, max_batch_pkts=max_pkts,
                              max_batch_arena=max_pkts * 96, max_out_pkts=4096, max_out_bytes=1 << 22,
                              max_batch_tuples=4096)
        for t, (kind, codec, clock) in enumerate(tracks):
            assert self.eng.api["add_track"](self.eng.h, C.byref(abi.lkf_track_params(
                track_id=500 + t, room=0, publisher=t, kind=kind, codec=codec, clock_rate=clock))) == t
        self.track_of = []
        for s, (track, layer, kw) in enumerate(streams):
            assert self.eng.api["add_stream"](self.eng.h, C.byref(abi.lkf_stream_params(
                track=track, layer=layer, ssrc=ssrc_of(s), **kw))) == s
            self.track_of.append(track)
        self.clock = T0

    def ingest(self, items):
        """items: [(stream handle, Stream row)] in arrival order -> each item's lkf_flow row.  The batch is
        grouped by track as lkf_ingest wants it, arrival order inside (1 ms apart, streams interleaved)."""
        order = sorted(range(len(items)), key=lambda i: (self.track_of[items[i][0]], i))
        rows, buf = [], bytearray()
        for i in order:
            d = items[i][1][0]
            off = (len(buf) + 15) // 16 * 16
            buf += bytes(off - len(buf)) + d
            rows.append((self.clock + i * MS, items[i][0], off, len(d), 0))
        self.clock += (len(items) + 1) * MS
        raws = np.array(rows, dtype=self.abi.RAW_PKT_DTYPE) if rows else np.zeros(0, dtype=self.abi.RAW_PKT_DTYPE)
        arena = np.frombuffer(bytes(buf) + bytes(16), dtype=np.uint8)
        assert self.eng.api["ingest"](self.eng.h, raws.ctypes.data, len(raws), arena.ctypes.data, len(buf)) == 0
        flows = self.eng.flows()
        assert len(flows) == len(items)
        out = [None] * len(items)
        for pos, i in enumerate(order):
            out[i] = flows[pos]
        return out

    def step(self, items, models):
        """Ingests, feeds each stream's model from the flows -> (the streams the model says became
        calculated, the flag bytes)."""
        before = {s: m.calculated for s, m in models.items()}
        flows = self.ingest(items)
        for (s, row), fl in zip(items, flows):
            if s in models:
                F.feed(models[s], [row], [fl])
        return sorted(s for s, m in models.items() if m.calculated and not before[s]), [int(f["flags"]) for f in flows]

    def state(self, s):
        return self.eng.stream_fps_get(s).as_dict()

    def close(self):
        self.eng.close()


def ssrc_of(s):
    return 0x51000000 + s


def interleave(streams):
    """[(handle, row)] of several Streams, one row of each in turn."""
    out, k = [], 0
    while any(k < len(st.rows) for st in streams):
        out += [(st.handle, st.rows[k]) for st in streams if k < len(st.rows)]
        k += 1
    return out


class _Part:
    """Rows lo .. hi - 1 of a Stream, for interleave."""

    def __init__(self, st, lo, hi):
        self.handle, self.rows = st.handle, st.rows[lo:hi]


def vp8_stream(handle, table=FULL, n=200, start_ts=12345678, start_fn=100, packets=lambda i: 1, pid_bits=15):
    st = F.Stream(handle, ssrc_of(handle), F.VP8)
    for i, (fn, ts, t) in enumerate(F.make_frames(table, n, start_ts, start_fn, fn_bits=15)):
        st.frame(fn, ts, t, packets=packets(i), pid_bits=pid_bits)
    return st


def vp9_stream(handle, tables, n, start_ts, start_fn, pid_bits, sids=None):
    st = F.Stream(handle, ssrc_of(handle), F.VP9)
    per = [F.make_frames(tb, n, start_ts, start_fn + 7 * s, fn_bits=pid_bits) for s, tb in enumerate(tables)]
    sids = sids or list(range(len(tables)))
    for i in range(n):
        for s in range(len(per)):
            fn, ts, t = per[s][i]
            st.frame(fn, ts, t, spatial=sids[s], pid_bits=pid_bits)
    return st


def test_vp8_one_ingest(pkg, abi):
    """{7.5, 15, 30}, 200 single-packet frames, one ingest."""
    rig = Rig(pkg, abi, [(KIND_VIDEO, VP8C, 90000)], [(0, 0, {})])
    try:
        rig.eng.stream_fps_enable(0)
        rig.eng.stream_fps_enable(0)  # idempotent
        assert rig.state(0) == PyFps(F.VP8).state()
        assert rig.eng.ingest_fps_changed() == []
        st = vp8_stream(0, n=220)
        m = {0: PyFps(F.VP8)}
        changed, flags = rig.step([(0, r) for r in st.rows[:200]], m)
        assert all(f & F.FLOW_FORWARD for f in flags)
        assert changed == [0] and m[0].calculated
        assert rig.eng.ingest_fps_changed() == [0]
        got = rig.state(0)
        assert got == m[0].state(), (got, m[0].state())
        for want, r in zip(FULL, rig.eng.stream_fps_get(0).fps[0]):  # the reference test's own bound
            assert want * 0.9 <= r <= want * 1.1
        # in no later ingest, and later packets change nothing
        assert rig.step([(0, r) for r in st.rows[200:]], m)[0] == []
        assert rig.eng.ingest_fps_changed() == []
        assert rig.state(0) == got
        rig.ingest([])
        assert rig.eng.ingest_fps_changed() == []
    finally:
        rig.close()


def test_batch_sizes_leave_the_same_state(pkg, abi):
    """The same trace in batches of 1, 7, 64 and 200 datagrams: the state after every prefix is the model's
    (so the same whatever the batching): the state's round trip and the 64-at-a-time walk."""
    sizes = (1, 7, 64, 200)
    rig = Rig(pkg, abi, [(KIND_VIDEO, VP8C, 90000)] * 4, [(t, 0, {}) for t in range(4)])
    try:
        for s in range(4):
            rig.eng.stream_fps_enable(s)
        finals = []
        for s, b in enumerate(sizes):
            rows = vp8_stream(s).rows
            m = {s: PyFps(F.VP8)}
            for lo in range(0, len(rows), b):
                changed, _ = rig.step([(s, r) for r in rows[lo:lo + b]], m)
                assert rig.state(s) == m[s].state(), (b, lo)
                assert rig.eng.ingest_fps_changed() == changed, (b, lo)
            finals.append(rig.state(s))
        assert all(f == finals[0] for f in finals) and finals[0]["calculated"] == 1
    finally:
        rig.close()


def test_vp8_packets_reordering_duplicates_loss(pkg, abi):
    """Frames of 1-5 packets, reordering across frame boundaries, duplicates, a padding-only datagram, a
    descriptor that does not unmarshal, and a 70-frame loss that forces a reset."""
    rig = Rig(pkg, abi, [(KIND_VIDEO, VP8C, 90000)], [(0, 0, {"nack": 1})])
    try:
        rig.eng.stream_fps_enable(0)
        st = F.Stream(0, ssrc_of(0), F.VP8)
        frames = F.make_frames(FULL, 260, 999, 32000, fn_bits=15)
        bounds = []
        for i, (fn, ts, t) in enumerate(frames):
            if 30 <= i < 100:  # the loss
                st.sn = (st.sn + 1 + i % 5) & 0xFFFF
                continue
            bounds.append(len(st.rows))
            st.frame(fn, ts, t, packets=1 + i % 5)
            if i == 10:
                st.padding_only(ts)
            if i == 12:
                st.bad_descriptor(ts)
        for k in (3, 8, 15, 20):  # the last packet of a frame and the first of the next change places
            st.swap(bounds[k] - 1, bounds[k])
        st.swap(bounds[5], bounds[7])  # a whole frame early
        for i in (2, bounds[9], bounds[22] + 1):
            st.duplicate(i)
        st.rows.insert(bounds[25], st.rows[bounds[4]])  # a late duplicate inside the first window
        m = {0: PyFps(F.VP8)}
        seen, cuts = 0, (0, 37, 101, 165, 400, len(st.rows))
        for lo, hi in zip(cuts, cuts[1:]):
            changed, flags = rig.step([(0, r) for r in st.rows[lo:hi]], m)
            seen |= int(np.bitwise_or.reduce(flags))
            assert rig.state(0) == m[0].state(), (lo, hi)
            assert rig.eng.ingest_fps_changed() == changed
        # every kind of datagram was there, the reset happened, and the stream got its rates afterwards
        assert seen & F.FLOW_BAD and seen & F.FLOW_PADDING and seen & 0x02 and seen & 0x04 and seen & 0x08
        c = m[0].calcs[0]
        assert m[0].calculated and c.resets >= 2
        for want, r in zip(FULL, c.rates):
            assert want * 0.9 <= r <= want * 1.1
    finally:
        rig.close()


def test_vp9(pkg, abi):
    """L3T3 with 15-bit and with 7-bit PictureIDs, SID 3 packets mixed in; a one-spatial stream completes
    its one calculator and stays not calculated."""
    t3 = ((5, 10, 15), (5, 10, 15), FULL)
    rig = Rig(pkg, abi, [(KIND_VIDEO, VP9C, 90000)] * 3, [(t, 0, {}) for t in range(3)], max_pkts=2048)
    try:
        for s in range(3):
            rig.eng.stream_fps_enable(s)
        a = vp9_stream(0, t3 + (FULL,), 110, (1 << 32) - 200000, 32700, 15)  # the fourth layer is SID 3
        b = vp9_stream(1, t3, 110, 4242, 1, 7)
        c = vp9_stream(2, (FULL,), 110, 77, 500, 15)
        items = interleave([a, b, c])
        m = {s: PyFps(F.VP9) for s in range(3)}
        got_changed = []
        for lo in range(0, len(items), 470):
            changed, flags = rig.step(items[lo:lo + 470], m)
            assert all(f & F.FLOW_FORWARD for f in flags)
            for s in range(3):
                assert rig.state(s) == m[s].state(), (lo, s)
            assert rig.eng.ingest_fps_changed() == changed
            got_changed += changed
        assert sorted(got_changed) == [0, 1]
        assert m[0].calculated and m[1].calculated
        assert m[2].calcs[0].completed and not m[2].calculated and rig.state(2)["completed"] == (1, 0, 0)
        for s in (0, 1):
            for sp, tb in enumerate(t3):
                for want, r in zip(tb, m[s].rates(sp)):
                    assert want * 0.9 <= r <= want * 1.1, (s, sp, m[s].rates(sp))
    finally:
        rig.close()


def test_many_streams_one_ingest(pkg, abi):
    """130 enabled streams and 20 that are not, three simulcast layers per track, arrival interleaved:
    more waves than one row of CUs takes, every stream with its own table, phase and packet count; some
    complete in the middle of the first ingest (their later packets must change nothing), some in the
    second, some never."""
    ntracks, tables = 50, (FULL, (5, 10, 15), (7.5, 15), (15, 30), (10, 20, 30))
    rig = Rig(pkg, abi, [(KIND_VIDEO, VP8C, 90000)] * ntracks,
              [(s // 3, s % 3, {"nack": s % 2}) for s in range(3 * ntracks)], max_pkts=24576)
    try:
        off = set(range(7, 150, 7)[:20])
        assert len(off) == 20
        enabled = [s for s in range(150) if s not in off]
        for s in reversed(enabled):  # (not in handle order: the changed list is sorted by the engine)
            rig.eng.stream_fps_enable(s)
        streams = []
        for s in range(150):
            # by layer: 150 one-packet frames (complete about two thirds into the first ingest), 35 frames
            # (never enough), 70 frames of 2-4 packets (complete in the second ingest)
            n = (150, 35, 70)[s % 3]
            start_ts = (1000 * s - (3000 * 50 if s % 8 == 5 else 0)) & 0xFFFFFFFF  # (some wrap the timestamp)
            st = vp8_stream(s, tables[s % 5], n, start_ts, (s * 211) % 32768,
                            packets=lambda i, s=s: (1, 1 + (i + s) % 2, 2 + (i + s) % 3)[s % 3])
            if s % 11 == 3:
                st.duplicate(5)
                st.swap(20, 23)
            streams.append(st)
        # the first ingest: every stream's first 100 datagrams
        first = interleave([_Part(st, 0, 100) for st in streams])
        second = interleave([_Part(st, 100, len(st.rows)) for st in streams])
        m = {s: PyFps(F.VP8) for s in enabled}
        total = []
        for part in (first, second):
            changed, _ = rig.step(part, m)
            assert rig.eng.ingest_fps_changed() == changed
            total.append(changed)
            for s in range(150):
                assert rig.state(s) == (m[s].state() if s in m else F.zero_state()), s
        # (the trace reaches all three: completions in the first ingest, in the second, and never)
        assert len(total[0]) >= 30 and len(total[1]) >= 20 and len(enabled) - len(total[0]) - len(total[1]) >= 20
        # cap too small: the count is still answered
        n = C.c_uint32()
        buf = np.zeros(4, dtype=np.int32)
        assert rig.eng.api["ingest_fps_changed"](rig.eng.h, buf.ctypes.data, 4, C.byref(n)) == ENOSPC
        assert n.value == len(total[1])
    finally:
        rig.close()


def _twin_outputs(pkg, workload, abi, tr, nack, enable):
    eng = pkg.Engine.for_trace(tr)
    out = []
    try:
        workload.load_topology(eng.api, eng.h, tr)
        for i in range(tr.nstreams):
            p = abi.lkf_stream_params.from_buffer_copy(tr.streams[i])
            if not nack:
                p.nack = 0
            assert eng.api["add_stream"](eng.h, C.byref(p)) == i
        on = [i for i in range(tr.nstreams) if enable and eng.api["stream_fps_enable"](eng.h, i) == 0]
        for b in range(tr.nbatches):
            workload.queue_events(eng.api, eng.h, tr, b)
            rp, n, ar, alen = tr.batch_raw(b)
            eng.ingest(rp, n, ar, alen)
            recs, pairs = pkg.nacks_arrays(eng.api, eng.h)
            npk = C.c_uint32()
            assert eng.api["ingested"](eng.h, None, 0, C.byref(npk)) in (0, ENOSPC)
            pk = (abi.lkf_pkt * max(1, npk.value))()
            assert eng.api["ingested"](eng.h, pk, npk.value, C.byref(npk)) == 0
            eng.run()
            eng.sync()
            grec, gar = eng.drain()
            out.append((eng.flows().tobytes(), C.string_at(pk, 64 * npk.value), recs.tobytes(), pairs.tobytes(),
                        grec.tobytes(), gar.tobytes()))
        out.append(tuple(eng.stream_stats(i) for i in range(tr.nstreams)))
        fps = [eng.stream_fps_get(i).as_dict() for i in on]
        return out, fps, sum(len(o[4]) for o in out[:-1]), sum(len(o[2]) for o in out[:-1])
    finally:
        eng.close()


@pytest.mark.parametrize("nack", [1, 0])
def test_twin_engine_with_nothing_enabled_is_bit_identical(pkg, workload, abi, nack):
    """Flows, ExtPackets, NACKs, the run's output and the stream statistics of an engine with every video
    stream's calculators enabled equal, byte for byte, those of a twin with none: with NACK-negotiated
    streams (the side stream is forked anyway) and without (only the calculators fork it)."""
    tr = workload.Trace(1, duration_s=2.0, batch_s=0.5, loss=0.02)
    want, _, fwd, nacks = _twin_outputs(pkg, workload, abi, tr, nack, enable=False)
    got, fps, _, _ = _twin_outputs(pkg, workload, abi, tr, nack, enable=True)
    assert fwd > 0 and (nacks > 0) == bool(nack)
    assert len(fps) > 0 and any(f["calc"][0][4] or f["calculated"] for f in fps)  # the calculators did run
    for b, (g, w) in enumerate(zip(got, want)):
        assert g == w, b


def test_refusals(pkg, abi):
    tracks = [(KIND_AUDIO, OPUS, 48000), (KIND_VIDEO, H264C, 90000), (KIND_VIDEO, VP9C, 90000),
              (KIND_VIDEO, VP8C, 90000)]
    rig = Rig(pkg, abi, tracks, [(0, 0, {}), (1, 0, {}), (2, 0, {"dd_ext": 5}), (3, 0, {})])
    try:
        en = rig.eng.api["stream_fps_enable"]
        assert en(rig.eng.h, 0) == EINVAL  # an audio stream
        assert en(rig.eng.h, 1) == EINVAL  # an H.264 track
        assert en(rig.eng.h, 2) == EINVAL  # a stream with a dependency-descriptor extension
        assert en(rig.eng.h, 4) == EINVAL and en(rig.eng.h, -1) == EINVAL  # no such stream
        st = abi.lkf_stream_fps()
        assert rig.eng.api["stream_fps_get"](rig.eng.h, 4, C.byref(st)) == EINVAL
        assert rig.state(0) == F.zero_state() and rig.state(3) == F.zero_state()  # never enabled
        assert en(rig.eng.h, 3) == 0
        assert rig.state(3) == PyFps(F.VP8).state()
        # cap too small
        rows = vp8_stream(3).rows
        m = {3: PyFps(F.VP8)}
        assert rig.step([(3, r) for r in rows], m)[0] == [3]
        n = C.c_uint32()
        assert rig.eng.api["ingest_fps_changed"](rig.eng.h, None, 0, C.byref(n)) == ENOSPC and n.value == 1
        assert rig.eng.ingest_fps_changed() == [3]
    finally:
        rig.close()
