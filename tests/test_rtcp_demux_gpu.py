"""RTCP demultiplexing on the GPU (lkf_set_downtrack_rtcp_transport,
lkf_rtcp_demux, lkf_rtcp_demux_unprotected; rtcp_kernels.hip k_rtcp_dmx_*)
against tests/rtcp_demux_lib.PyRtcpDemux, the restatement written from
include/lkfwd.h: every result field and the entry list, order included.

Bare engines with two tracks and six transports that hold 0, 1, 2, 33, 65 and
70 DownTracks (bitmap rows of 0, 1, 1, 2, 3 and 3 words), and for the
composition the rig of tests/test_srtcp_gpu.py: sealed datagrams through
unprotect -> demux -> ingest on one engine, the restatement's entries through
lkf_rtcp_ingest on its twin, everything equal bit for bit.  With
LKF_LIB=liblkfwd_checked.so the same tests run the bounds-checked kernels.
"""
import ctypes as C
import struct

import numpy as np
import pytest

from tests import rtcp_demux_lib as D
from tests import rtcp_lib, rtx_lib
from tests import rtcp_wire_lib as W
from tests import srtcp_lib as L

pytestmark = pytest.mark.gpu
EPOCH = 1700000000 * 10**9
SEC = 10**9
FIELDS = ("status", "dests", "unrouted", "entries")
OK, EMPTY, BAD = D.DMX_OK, D.DMX_EMPTY, D.DMX_MALFORMED


class Bare:
    """An engine with two tracks, six transports and the tests' topology bound; `rows` follows every
    topology call, so that D.build_table(rows) is the table the engine must route by."""

    def __init__(self, pkg, spare=16):
        abi = pkg.abi
        self.pkg, self.abi = pkg, abi
        self.eng = pkg.Engine(max_tracks=8, max_downtracks=D.NDTS + spare, max_batch_pkts=1024,
                              max_batch_arena=1 << 20, max_out_pkts=4096, max_out_bytes=1 << 22, max_batch_tuples=4096)
        for t, (mk, ms, prof) in enumerate(L.make_keys(len(D.COUNTS))):
            assert self.eng.api["add_transport"](self.eng.h, C.byref(pkg.transport_params(mk, ms, prof))) == t
        tp = abi.lkf_track_params()
        tp.kind, tp.clock_rate = abi.LKF_KIND_VIDEO, 90000
        self.tracks = [self.eng.api["add_track"](self.eng.h, C.byref(tp)) for _ in range(2)]
        assert self.tracks == [0, 1]
        self.rows = []  # [dt, ssrc, transport, active]
        for dt, ssrc, t in D.topology():
            assert self.add(ssrc, t) == dt

    def add(self, ssrc, t, track=None):
        dp = self.abi.lkf_downtrack_params()
        dp.track = self.tracks[len(self.rows) % 2] if track is None else track
        dp.ssrc = ssrc
        dt = self.eng.api["add_downtrack"](self.eng.h, C.byref(dp))
        assert dt == len(self.rows), dt
        self.rows.append([dt, ssrc, -1, True])
        self.bind(dt, t)
        return dt

    def bind(self, dt, t):
        self.eng.set_downtrack_rtcp_transport(dt, t)
        self.rows[dt][2] = t

    def remove(self, dt):
        assert self.eng.api["remove_downtrack"](self.eng.h, dt) == 0
        self.rows[dt][3] = False

    def table(self):
        return D.build_table(self.rows)

    def by_rank(self, t):
        """The transport's routed DownTracks as (ssrc, dt), SSRC ascending: position k is bit k of its rows."""
        return sorted((s, d) for (tt, s), d in self.table().items() if tt == t)

    def close(self):
        self.eng.close()


def _pack(abi, dgrams, front=0):
    arena = bytearray(b"\xee" * front)
    raws = np.zeros(len(dgrams), dtype=abi.SRTCP_RAW_DTYPE)
    for i, (t, data) in enumerate(dgrams):
        raws[i] = (t, len(arena), len(data))
        arena += data
    return raws, bytes(arena)


def _tuples(res):
    return [tuple(int(r[f]) for f in FIELDS) for r in res]


def _pairs(ent):
    return [(int(e["dt"]), int(e["dgram"])) for e in ent]


def _check(b, dgrams, front=0):
    """One lkf_rtcp_demux against the restatement -> (results, entries) as tuples."""
    raws, arena = _pack(b.abi, dgrams, front)
    if len(raws):
        assert int(raws["off"][-1]) + int(raws["len"][-1]) == len(arena)  # the last one ends with the arena
    res, ent = b.eng.rtcp_demux(raws, arena)
    want_res, want_ent = D.PyRtcpDemux.call(b.table(), dgrams)
    got = _tuples(res)
    for i, (g, w) in enumerate(zip(got, want_res)):
        assert g == w, (i, g, w, dgrams[i][0], dgrams[i][1].hex())
    assert len(got) == len(want_res)
    assert _pairs(ent) == want_ent
    return got, want_ent


def _raw_call(b, raws, arena, cap):
    abi = b.abi
    ar = np.frombuffer(arena, dtype=np.uint8)
    res = np.zeros(len(raws), dtype=abi.RTCP_DMX_RESULT_DTYPE)
    ent = np.zeros(max(1, cap), dtype=abi.RTCP_ENTRY_DTYPE)
    k = C.c_uint32(12345)
    rc = b.eng.api["rtcp_demux"](b.eng.h, raws.ctypes.data, len(raws), ar.ctypes.data if len(ar) else None, len(ar),
                                 res.ctypes.data, ent.ctypes.data, cap, C.byref(k))
    return rc, k.value, res, ent


def test_hand_built(pkg, abi):
    b = Bare(pkg)
    try:
        r = {t: b.by_rank(t) for t in range(6)}
        assert [len(r[t]) for t in range(6)] == list(D.COUNTS)
        s3, s4, s5 = ([s for s, _ in r[t]] for t in (3, 4, 5))
        d3, d4, d5 = ([d for _, d in r[t]] for t in (3, 4, 5))
        foreign = 0xDEAD0001
        blocks = lambda *ss: [W.report_block(s) for s in ss]  # noqa: E731
        # before any unprotect: nothing to demultiplex
        res, ent = b.eng.rtcp_demux_unprotected()
        assert len(res) == 0 and len(ent) == 0
        assert _check(b, []) == ([], [])  # n = 0
        assert _check(b, [(3, W.pli(1, s3[0]))]) == ([(OK, 1, 0, 1)], [(d3[0], 0)])  # n = 1
        dgrams = [
            (3, W.rr(9, blocks(s3[4], foreign, s3[20]))),                       # 0: two DownTracks and a stranger
            (2, W.sr(r[2][1][0])),                                             # 1: the sender SSRC is a DownTrack's
            (3, W.compound(W.nack(9, s3[7], [(5, 3)]), W.pli(9, s3[7]))),       # 2: one entry
            (5, W.fir(9, s5[0], [(s5[1], 1), (s5[33], 2), (s5[69], 3)])),       # 3: the media SSRC is no destination
            (4, W.remb(9, ssrcs=[s4[0], foreign, s4[31], s4[64]])),             # 4
            (3, W._hdr(2, 206, struct.pack(">I", s3[0]))),                      # 5: an SLI of 8 bytes
            (1, W.rr(9, blocks(s3[0]))),                                        # 6: that SSRC lives on transport 3
            (4, W.pli(9, 5000)),                                                # 7, 8: one SSRC, two transports
            (5, W.pli(9, 5000)),
            (3, W.sdes(s3[0])),                                                 # 9
            (3, W.rr(9, blocks(s3[1], s3[2])) + b"\x80\xc9"),                   # 10: a malformed tail
            (4, b""),                                                           # 11
            (0, W.rr(9, blocks(s3[0], s4[0]))),                                 # 12: a transport without DownTracks
            (3, W.rr(9, blocks(s3[31], s3[32]))),                               # 13-15: the words' last and first bits
            (4, W.rr(9, blocks(s4[63], s4[64], s4[31], s4[32]))),
            (5, W.rr(9, blocks(s5[69], s5[64], s5[63]))),
            (1, W.sr(9, blocks(r[1][0][0], r[1][0][0]))),                       # 16: twice in one packet
            (3, W._hdr(5, 205, struct.pack(">II", 9, s3[3]))),                  # 17: RRR with a media SSRC
        ]
        first = len(dgrams)
        for k in range(130):  # more than two waves of transport 5's datagrams, interleaved with transport 3's
            dgrams.append((5, W.pli(9, s5[k % 70])))
            if k % 3 == 0:
                dgrams.append((3, W.nack(9, s3[k % 33], [(k, 0)])))
        got, ent = _check(b, dgrams, front=1)
        assert got[:18] == [(OK, 3, 1, 2), (OK, 1, 0, 1), (OK, 2, 0, 1), (OK, 3, 0, 3), (OK, 4, 1, 3), (OK, 0, 0, 0),
                            (OK, 1, 1, 0), (OK, 1, 0, 1), (OK, 1, 0, 1), (OK, 0, 0, 0), (BAD, 0, 0, 0),
                            (EMPTY, 0, 0, 0), (OK, 2, 2, 0), (OK, 2, 0, 2), (OK, 4, 0, 4), (OK, 3, 0, 3),
                            (OK, 3, 1, 1), (OK, 1, 0, 1)]
        where = lambda i: sorted(d for d, g in ent if g == i)  # noqa: E731
        assert where(0) == sorted((d3[4], d3[20])) and where(3) == sorted((d5[1], d5[33], d5[69]))
        assert where(7) == [d4[0]] and where(8) == [d5[0]] and d4[0] != d5[0]
        assert where(10) == where(11) == where(12) == []
        assert where(14) == sorted((d4[63], d4[64], d4[31], d4[32]))
        assert sum(1 for _, g in ent if g >= first) == len(dgrams) - first
        assert sum(g[3] for g in got) == len(ent) > 130
        # cap one short: LKF_ENOSPC with the count and the results; the call repeats to the same answer
        raws, arena = _pack(abi, dgrams)
        rc, k, res, _ = _raw_call(b, raws, arena, len(ent) - 1)
        assert (rc, k) == (-28, len(ent)) and _tuples(res) == got
        rc, k, res, _ = _raw_call(b, raws, arena, 0)
        assert (rc, k) == (-28, len(ent)) and _tuples(res) == got
        for _ in range(2):
            rc, k, res, out = _raw_call(b, raws, arena, len(ent))
            assert (rc, k) == (0, len(ent)) and _tuples(res) == got and _pairs(out) == ent
        # refused before anything runs
        good = W.pli(9, s3[0])
        for row, ar in (((6, 0, len(good)), good), ((-1, 0, len(good)), good), ((3, 4, len(good)), good),
                        ((3, len(good), 1), good), ((3, 0, abi.LKF_RTCP_MAX_LEN + 1), bytes(abi.LKF_RTCP_MAX_LEN + 1))):
            bad = np.array([(3, 0, len(good)), row], dtype=abi.SRTCP_RAW_DTYPE)
            rc, k, _, _ = _raw_call(b, bad, ar, 8)
            assert (rc, k) == (-22, 0), row
        assert b.eng.api["set_downtrack_rtcp_transport"](b.eng.h, len(b.rows), 0) == -22
        assert b.eng.api["set_downtrack_rtcp_transport"](b.eng.h, 0, 6) == -22
        assert b.eng.api["set_downtrack_rtcp_transport"](b.eng.h, 0, -2) == -22
        assert _check(b, dgrams[:20])[0] == got[:20]  # ... and nothing changed
    finally:
        b.close()


def test_random_equals_restatement(pkg, abi):
    b = Bare(pkg)
    try:
        dgrams = D.random_datagrams(D.GPU_SEED, D.GPU_N)
        got, ent = _check(b, dgrams, front=3)
        D.assert_shares(got)  # what tests/test_rtcp_demux_cpu.py vetted the seed for
        assert len(ent) == sum(g[3] for g in got) > D.GPU_N // 2
        assert _check(b, dgrams[100:101] + dgrams[:100]) is not None  # another split of the same bytes
    finally:
        b.close()


def test_topology_changes(pkg, abi):
    b = Bare(pkg, spare=1000)
    try:
        trace = D.random_datagrams(D.GPU_SEED, 120)
        r3, r5 = b.by_rank(3), b.by_rank(5)

        def step(extra):
            got, ent = _check(b, extra + trace)
            return got[:len(extra)], [(d, g) for d, g in ent if g < len(extra)]

        (s_a, d_a), (s_b, d_b), (s_c, d_c) = r3[5], r3[6], r5[10]
        probe = [(3, W.rr(9, [W.report_block(s_a), W.report_block(s_b)])), (5, W.pli(9, s_c)), (4, W.pli(9, s_c)),
                 (2, W.pli(9, s_a))]
        d4_c = dict(b.by_rank(4))[s_c]
        assert step(probe) == ([(OK, 2, 0, 2), (OK, 1, 0, 1), (OK, 1, 0, 1), (OK, 1, 1, 0)],
                               sorted([(d_a, 0), (d_b, 0), (d_c, 1), (d4_c, 2)]))
        b.remove(d_a)  # a removed DownTrack is addressed by nothing
        assert step(probe) == ([(OK, 2, 1, 1), (OK, 1, 0, 1), (OK, 1, 0, 1), (OK, 1, 1, 0)],
                               sorted([(d_b, 0), (d_c, 1), (d4_c, 2)]))
        b.bind(d_b, 2)  # rebound: its SSRC now answers on transport 2 alone
        probe[3] = (2, W.pli(9, s_b))
        assert step(probe) == ([(OK, 2, 2, 0), (OK, 1, 0, 1), (OK, 1, 0, 1), (OK, 1, 0, 1)],
                               sorted([(d_c, 1), (d4_c, 2), (d_b, 3)]))
        b.bind(d_c, -1)  # unbound
        assert step(probe) == ([(OK, 2, 2, 0), (OK, 1, 1, 0), (OK, 1, 0, 1), (OK, 1, 0, 1)],
                               sorted([(d4_c, 2), (d_b, 3)]))
        twin = b.add(s_c, 4)  # the same key as d4_c: the higher handle wins
        assert twin > d4_c
        assert step(probe) == ([(OK, 2, 2, 0), (OK, 1, 1, 0), (OK, 1, 0, 1), (OK, 1, 0, 1)],
                               sorted([(twin, 2), (d_b, 3)]))
        b.remove(twin)  # ... and the lower one again once it is gone
        assert step(probe)[1] == sorted([(d4_c, 2), (d_b, 3)])
        for k in range(900):  # past the table's first allocation; transport 5's rows grow to 31 words
            b.add(200000 + 3 * k, 5)
        assert len(b.table()) > 1024
        probe += [(5, W.rr(9, [W.report_block(200000 + 3 * k) for k in (0, 450, 899)])), (5, W.pli(9, r5[69][0]))]
        got, ent = step(probe)
        assert got[4:] == [(OK, 3, 0, 3), (OK, 1, 0, 1)] and len([1 for _, g in ent if g == 4]) == 3
        assert b.eng.api["remove_track"](b.eng.h, b.tracks[1]) == 0  # every DownTrack of the track
        for row in b.rows:
            if row[0] % 2 == 1 and row[0] != twin:
                row[3] = False
        assert b.rows[twin][3] is False and 400 < len(b.table()) < 600
        got2, ent2 = step(probe)
        assert len(ent2) < len(ent) and all(d % 2 == 0 or d == twin for d, _ in ent2)
    finally:
        b.close()


def _traffic(rig, dts, mate, nacks, lsr, rnd):
    """tests/test_srtcp_gpu._traffic, with the third compound of every DownTrack also carrying a report block
    for its mate, a DownTrack of the same transport: that datagram addresses two DownTracks."""
    from tests.test_rtcp_in_gpu import _block, _compound_like_struct_entry, _nack_compounds
    out = []
    for d in dts:
        m = rig.models[d]
        ssrc = rtcp_lib.ssrc(rig, d)
        lsn = rtcp_lib.rr_lsn(m.s.high_sn if m.s.init else 0, m.s.start_sn)
        out.append(_compound_like_struct_entry(rig, (d, True, lsn, rnd + d % 3, 50 * rnd + d, lsr[d], 0x4000,
                                                     d % 3, rnd, d % 2)))
        mine = nacks[nacks["dt"] == d]
        out.append(_nack_compounds(rig, mine)[0][1] if len(mine) else W.compound(W.nack(1, ssrc, [(9, 1)])))
        mm = rig.models[mate[d]]
        out.append(W.compound(W.rr(1, [_block(rig, d, m.s.high_sn if m.s.init else 0, jitter=7),
                                       _block(rig, mate[d], mm.s.high_sn if mm.s.init else 0, jitter=9)]),
                              W.fir(1, ssrc, [(ssrc, rnd)]), W.remb(1, ssrcs=[ssrc]), W.twcc(1, ssrc), W.pli(1, ssrc)))
    return out


@pytest.mark.parametrize("config", [2])
def test_composes_from_sealed_datagrams(pkg, workload, abi, config):
    """Engine A: lkf_srtcp_unprotect without the plaintext copied back, lkf_rtcp_demux_unprotected, its entries
    unchanged into lkf_rtcp_ingest_unprotected.  Engine B: the entries PyRtcpDemux computes from the plaintext
    the sealer knows, through lkf_rtcp_ingest.  Every output bit for bit."""
    from tests.test_rtcp_in_gpu import _rig
    from tests.test_srtcp_gpu import RES_FIELDS, _add_transports
    a, b = _rig(pkg, workload, config, nb=2), _rig(pkg, workload, config, nb=2)
    try:
        ref = L.PySrtcpRx()
        keys = _add_transports(pkg, a.eng, ref)
        _add_transports(pkg, b.eng)
        for rig in (a, b):
            rig.forward(2)
        live = [d for d, m in enumerate(a.models) if m.s.init]
        dts = sorted((live + [d for d in range(a.tr.ndts) if d not in live])[:12])
        assert len(dts) == 12 and len(live) >= 6
        transport_of = {d: k % L.COMPOSE_TRANSPORTS for k, d in enumerate(dts)}
        mate = {d: dts[(k + L.COMPOSE_TRANSPORTS) % 12] for k, d in enumerate(dts)}
        assert all(transport_of[d] == transport_of[mate[d]] and d != mate[d] for d in dts)
        for d in dts:
            a.eng.set_downtrack_rtcp_transport(d, transport_of[d])
        table = D.build_table([(d, rtcp_lib.ssrc(a, d), transport_of[d], True) for d in dts])
        assert len(table) == 12
        senders = [L.Composer(ref.aes, ref.sess[t], keys[t][2], L.COMPOSE_SEED + t) for t in range(4)]
        nacks = rtx_lib.make_nacks(a.o.api, a.oh, a.tr, seed=5)
        total = rejected = two = 0
        for rnd in range(2):
            now = EPOCH + (2 + rnd) * SEC
            reqs = np.array([(d, 0) for d in range(a.tr.ndts)], dtype=abi.RTCP_SR_REQ_DTYPE)
            rep = [r.eng.rtcp_sender_reports(reqs, now - SEC // 2) for r in (a, b)][0]  # so that the reports carry an RTT
            lsr = [(int(x["ntp"]) >> 16) & 0xFFFFFFFF for x in rep]
            traffic = _traffic(a, dts, mate, nacks, lsr, rnd)
            prot = L.Arena()
            for i, data in enumerate(traffic):
                t = transport_of[dts[i // 3]]
                prot.add(t, senders[t].seal(data))
            want, _ = ref.unprotect(prot.pkts, prot.buf)
            ok = [w[2] == L.OK for w in want]
            total += len(ok)
            rejected += len(ok) - sum(ok)
            # what the sealer knows: the accepted compounds at their datagrams' offsets, nothing of the others
            plain_ar = bytearray(len(prot.buf))
            known = []
            for data, p, w, k in zip(traffic, prot.pkts, want, ok):
                if k:
                    assert w[3] == len(data)
                    plain_ar[p[1]:p[1] + len(data)] = data
                known.append((p[0], data if k else b""))
            res, plain = a.eng.srtcp_unprotect(prot.raws(abi), bytes(prot.buf), want_plain=False)
            assert plain is None and [tuple(int(r[f]) for f in RES_FIELDS) for r in res] == want
            dres, entries = a.eng.rtcp_demux_unprotected()
            want_res, want_ent = D.PyRtcpDemux.call(table, known)
            assert _tuples(dres) == want_res and _pairs(entries) == want_ent
            assert [g[0] == EMPTY for g in want_res] == [not k for k in ok]
            two += sum(1 for g in want_res if g[3] >= 2)
            dres2, entries2 = a.eng.rtcp_demux_unprotected()  # no state: the same again
            assert dres2.tobytes() == dres.tobytes() and entries2.tobytes() == entries.tobytes()
            ga = a.eng.rtcp_ingest_unprotected(entries, now)
            raws = np.array([(d, prot.pkts[i][1], len(traffic[i])) for d, i in want_ent], dtype=abi.RTCP_RAW_DTYPE)
            gb = b.eng.rtcp_ingest(raws, bytes(plain_ar), now)
            for x, y, name in zip(ga, gb, ("out", "fb", "fb_out", "refs", "n_nacks")):
                if name == "n_nacks":
                    assert x == y and x > 0
                else:
                    assert len(x) == len(y) > 0 and x.tobytes() == y.tobytes(), (rnd, name)
            assert len(ga[0]) == len(want_ent) and not ga[0]["status"].any()  # every entry LKF_RTCP_IN_OK
            assert a.eng.rtcp_ingested_nacks().tobytes() == b.eng.rtcp_ingested_nacks().tobytes()
            ra, rb = a.eng.rtx_lookup_ingested(now), b.eng.rtx_lookup_ingested(now)
            assert ra.tobytes() == rb.tobytes() and (rnd or len(ra) > 0)
            every = list(range(a.tr.ndts))
            assert a.eng.sender_rtcp(every).tobytes() == b.eng.sender_rtcp(every).tobytes()
            assert any(int(x) for x in ga[0]["rtt_ms"])  # the reports carried an RTT: otherwise vacuous
        assert rejected >= 1 and 2 * (total - rejected) >= total and two >= 12, (rejected, total, two)
        # an unprotect of nothing: nothing to demultiplex
        a.eng.srtcp_unprotect(np.zeros(0, dtype=abi.SRTCP_RAW_DTYPE), b"", want_plain=False)
        dres, entries = a.eng.rtcp_demux_unprotected()
        assert len(dres) == 0 and len(entries) == 0
    finally:
        a.close()
        b.close()
