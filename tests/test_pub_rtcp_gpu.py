"""The publisher RTCP loop on the GPU (lkf_stream_sender_reports,
lkf_stream_receiver_reports, lkf_stream_rtcp_ingest[_unprotected],
lkf_ingest_nacks_wire, lkf_stream_rtcp_get; rtcp_kernels.hip k_pub_* and
k_nack_wire) against tests/pub_rtcp_lib.PyStreamRtcp fed from
lkf_stream_stats_get.  One small engine: an Opus stream and two VP8 layers of
one track, a few dozen hand-built datagrams per ingest.
"""
import ctypes as C
import struct

import numpy as np
import pytest

from tests import pub_rtcp_lib as P
from tests import rtcp_wire_lib as W
from tests import srtcp_lib as L
from tests.pub_rtcp_lib import PyStreamRtcp
from tests.rtcp_lib import bits, get_rtt_ms, to_ntp
from tests.srtp_rx_lib import rtp_packet

pytestmark = pytest.mark.gpu
T0 = 1700000000 * 10**9
SEC, MS = 10**9, 10**6
SSRCS = (0x0A000001, 0x0B000001, 0x0B000002)
CLOCKS = (48000, 90000, 90000)
TICKS = (960, 900, 900)  # RTP ticks per packet: 20 ms of Opus, 10 ms of video
GAP_NS = (20 * MS, 10 * MS, 10 * MS)
SN0 = (65500, 1000, 30000)  # the Opus stream wraps inside the second ingest
TS0 = (0xFFFF0000, 5000, 123456789)


def _engine(pkg, abi, ssrcs=SSRCS):
    eng = pkg.Engine(max_tracks=16, max_downtracks=16, max_batch_pkts=2048, max_batch_arena=1 << 20,
                     max_out_pkts=4096, max_out_bytes=1 << 22, max_batch_tuples=4096)
    for t, (kind, codec, clock) in enumerate([(0, 1, 48000), (1, 2, 90000)]):
        assert eng.api["add_track"](eng.h, C.byref(abi.lkf_track_params(
            track_id=100 + t, room=0, publisher=t, kind=kind, codec=codec, clock_rate=clock))) == t
    for s, (track, layer) in enumerate([(0, 0), (1, 0), (1, 1)]):
        assert eng.api["add_stream"](eng.h, C.byref(abi.lkf_stream_params(
            track=track, layer=layer, ssrc=ssrcs[s], nack=1 if track else 0))) == s
    return eng


def _datagram(s, k, ssrcs=SSRCS):
    """Stream s's k-th packet: Opus bytes, or a VP8 descriptor (S = 1) and an inter-frame payload."""
    pay = bytes([0x10, 0x01]) + bytes((k + 3 * j) & 255 for j in range(40)) if s else bytes((k + j) & 255 for j in range(60))
    return rtp_packet(ssrcs[s], SN0[s] + k, pay, ts=TS0[s] + k * TICKS[s], pt=111 if s == 0 else 96, marker=k % 3 == 0)


def _ingest(abi, eng, t0, first, count, drop=(), swap=None, ssrcs=SSRCS):
    """Packets first .. first + count - 1 of every stream, arriving from t0 on at the streams' packet
    intervals (+ a per-packet wobble, so the receive jitter is not zero); `drop` ordinals are lost, `swap` =
    (a, b): packets a and b arrive in each other's place.  The batch is grouped by track, as lkf_ingest
    wants it, a track's layers interleaved by arrival.  -> the lkf_raw_pkt rows as ingested."""
    order = list(range(first, first + count))
    if swap:
        a, b = order.index(swap[0]), order.index(swap[1])
        order[a], order[b] = order[b], order[a]
    rows, buf = [], bytearray()
    for i, k in enumerate(order):
        for s in range(3):
            if k in drop:
                continue
            d = _datagram(s, k, ssrcs)
            off = (len(buf) + 15) // 16 * 16
            buf += bytes(off - len(buf)) + d
            rows.append((t0 + i * GAP_NS[s] + ((i * 7 + s) % 5) * 137000, s, off, len(d), 0))
    rows.sort(key=lambda r: (r[1] != 0, r[0]))  # grouped by track (stream 0 is the Opus track's), by arrival inside
    raws = np.array(rows, dtype=abi.RAW_PKT_DTYPE)
    arena = np.frombuffer(bytes(buf), dtype=np.uint8)
    rc = eng.api["ingest"](eng.h, raws.ctypes.data, len(raws), arena.ctypes.data, len(arena))
    assert rc == 0, rc
    return raws


def _stats(abi, eng, s):
    st = abi.lkf_stream_stats()
    assert eng.api["stream_stats_get"](eng.h, s, C.byref(st)) == 0
    return st


def _hot(abi, eng, s):
    return P.hot_of(_stats(abi, eng, s))


def _models():
    return [PyStreamRtcp(CLOCKS[s], SSRCS[s]) for s in range(3)]


def _check_state(abi, eng, models, hots, label):
    rows = eng.stream_rtcp(range(3))
    for s in range(3):
        got, want = P.engine_state(rows[s], _stats(abi, eng, s)), models[s].state(hots[s])
        assert got == want, (label, s, {k: (got.get(k), want.get(k)) for k in want if got.get(k) != want.get(k)})


def _sr_entries(rnd, t, hots):
    """(stream, rtp, ntp) grouped by stream: what each publisher would report at t, with the branches the
    round is meant to reach."""
    out = []
    for s in range(3):
        if not hots[s]["init"]:
            out.append((s, 1, to_ntp(t)))
            continue
        late = (0, 300 * MS, 0)[s]  # stream 1's first packet was 300 ms late: its first time moves earlier
        rtp = (hots[s]["ts_start"] + (t - T0 - 100 * MS + late) * CLOCKS[s] // SEC) & P.M32
        out.append((s, rtp, to_ntp(t - 3 * MS)))
        if s == 1:  # a second report of the same stream in the same call
            out.append((s, (rtp + 90) & P.M32, to_ntp(t - 2 * MS)))
        if s == 2 and rnd == 1:  # twice the nominal rate over the last second
            out[-1] = (s, (rtp + 90000) & P.M32, to_ntp(t - 3 * MS))
        if s == 2 and rnd == 2:  # behind the last one in RTP time
            out[-1] = (s, (rtp - 45000) & P.M32, to_ntp(t - 3 * MS))
        if s == 0 and rnd == 2:  # an anachronous one behind a good one
            out.append((s, rtp, to_ntp(t - 10 * SEC)))
    return out


def _run_round_struct(abi, eng, models, hots, rnd, t):
    ent = _sr_entries(rnd, t, hots)
    got = eng.stream_sender_reports(np.array(ent, dtype=abi.STREAM_SR_DTYPE), t)
    want = [models[s].sender_report(hots[s], rtp, ntp, t) for s, rtp, ntp in ent]
    assert [(int(g["flags"]), int(g["ntp"]), int(g["rtp_ext"])) for g in got] == want, (rnd, want)
    return ent, want


def _run_reports(abi, eng, models, hots, t, proxies):
    reqs = np.array([(s, proxies[s]) for s in (2, 0, 1)], dtype=abi.STREAM_RR_REQ_DTYPE)  # (any order)
    got, wire = eng.stream_receiver_reports(reqs, t, wire=True)
    recs = []
    for i, s in enumerate((2, 0, 1)):
        want = models[s].reception_report(hots[s], proxies[s], t)
        g = {k: int(got[i][k]) for k in P.RR_FIELDS}
        assert int(got[i]["stream"]) == s and g == want, (s, g, want)
        assert bytes(wire[i]) == PyStreamRtcp.wire(want), s
        recs.append(want)
    return recs, wire


def test_struct_reports_three_rounds(pkg, abi):
    eng = _engine(pkg, abi)
    try:
        models = _models()
        hots = [_hot(abi, eng, s) for s in range(3)]
        # before the first packet: sender reports are ignored, reception reports are nil
        _, want = _run_round_struct(abi, eng, models, hots, 0, T0)
        assert all(w[0] == P.SSR_IGNORED_UNINIT for w in want)
        recs, _ = _run_reports(abi, eng, models, hots, T0, (0, 0, 0))
        assert not any(r["flags"] for r in recs)
        _check_state(abi, eng, models, hots, "uninit")
        flags = 0
        valid = 0
        for rnd in range(3):
            # 30 packets per stream; the first round loses two and reorders one
            kw = dict(drop=(7, 8), swap=(15, 17)) if rnd == 0 else {}
            _ingest(abi, eng, T0 + 100 * MS + rnd * SEC, 30 * rnd, 30, **kw)
            hots = [_hot(abi, eng, s) for s in range(3)]
            if rnd == 0:
                assert all(h["init"] and h["packets_lost"] == 2 for h in hots)
            if rnd == 1:  # the Opus stream's sequence numbers and timestamps have wrapped
                assert hots[0]["ext_highest_sn"] == SN0[0] + 59 > 65535
            t = T0 + (rnd + 1) * SEC
            _, want = _run_round_struct(abi, eng, models, hots, rnd, t)
            for w in want:
                flags |= w[0]
            for s in range(3):  # maybeAdjustFirstPacketTime reached StreamHot
                assert _stats(abi, eng, s).first_time_ns == hots[s]["first_time"], (rnd, s)
            recs, _ = _run_reports(abi, eng, models, hots, t + 5 * MS + 1500, (0, 200, 3))
            valid += sum(1 for r in recs if r["flags"])
            if rnd == 0:
                assert recs[1]["fraction_lost"] == int(2 / 30 * 256) and recs[1]["delay"] == 5001 * 65536 // 10**6 \
                    and recs[1]["last_sequence_number"] == SN0[0] + 30 and recs[2]["fraction_lost"] == 200
            _check_state(abi, eng, models, hots, "round %d" % rnd)
        assert valid == 9
        want_flags = P.SSR_FIRST_TIME_ADJUSTED | P.SSR_CLOCK_SKEW | P.SSR_RESET_FIRST | P.SSR_ANACHRONOUS
        assert flags & want_flags == want_flags, flags
        # a second request of one stream in a call, a stream that reappears, an unknown handle
        rq = np.array([(0, 0), (1, 0), (0, 0)], dtype=abi.STREAM_RR_REQ_DTYPE)
        out = np.zeros(3, dtype=abi.STREAM_RR_DTYPE)
        assert eng.api["stream_receiver_reports"](eng.h, rq.ctypes.data, 3, t, out.ctypes.data, None) == -34
        sr = np.array([(0, 1, 2), (1, 1, 2), (0, 1, 3)], dtype=abi.STREAM_SR_DTYPE)
        so = np.zeros(3, dtype=abi.STREAM_SR_RESULT_DTYPE)
        assert eng.api["stream_sender_reports"](eng.h, sr.ctypes.data, 3, t, so.ctypes.data) == -34
        sr["stream"][2] = 3
        assert eng.api["stream_sender_reports"](eng.h, sr.ctypes.data, 3, t, so.ctypes.data) == -22
        _check_state(abi, eng, models, hots, "refused")
        # Buffer.Close: the Opus track is removed
        assert eng.api["remove_track"](eng.h, 0) == 0
        models[0].closed = True
        t += SEC
        _, want = _run_round_struct(abi, eng, models, hots, 0, t)
        assert want[0][0] == P.SSR_CLOSED
        recs, _ = _run_reports(abi, eng, models, hots, t, (9, 9, 9))
        assert recs[1]["flags"] == 0 and recs[0]["flags"] == 0  # (closed; nothing expected since the last report)
        _check_state(abi, eng, models, hots, "closed")
    finally:
        eng.close()


def _pack(abi, entries):
    """entries (stream, bytes) -> (STREAM_RTCP_RAW_DTYPE array, arena bytes), 3 bytes of filler in front."""
    arena = bytearray(b"\xee" * 3)
    raws = np.zeros(len(entries), dtype=abi.STREAM_RTCP_RAW_DTYPE)
    for i, (s, data) in enumerate(entries):
        raws[i] = (s, len(arena), len(data))
        arena += data
    return raws, bytes(arena)


def _compounds(ent):
    """The struct entries of one call as compound packets: one entry per sender report, except stream 1's
    two, which travel in one compound behind an SDES; a malformed entry and a report-less one in between."""
    out = []
    by = {}
    for s, rtp, ntp in ent:
        by.setdefault(s, []).append(W.sr(SSRCS[s] if s != 2 else 0xdeadbeef, ntp=ntp, rtp=rtp, packets=5, octets=500))
    for s in sorted(by):
        if s == 1:
            out.append((s, W.compound(W.sdes(SSRCS[s]), *by[s])))
            bad = bytearray(W.compound(by[s][0], by[s][0]))
            bad[28] |= 1  # the second claims a report block it has no room for
            out.append((s, bytes(bad)))
            out.append((s, W.compound(W.rr(SSRCS[s], [W.report_block(5)]), W.pli(1, 2))))
        else:
            out += [(s, p) for p in by[s]]
    return out


def test_bytes_equal_struct_path(pkg, abi):
    """The same sender reports as compound packets on a twin engine: the state is the struct path's bit for bit."""
    a, b = _engine(pkg, abi), _engine(pkg, abi)
    try:
        models, twin = _models(), _models()
        for rnd in range(3):
            for eng in (a, b):
                _ingest(abi, eng, T0 + 100 * MS + rnd * SEC, 30 * rnd, 30, **(dict(drop=(7, 8), swap=(15, 17)) if rnd == 0 else {}))
            hots = [_hot(abi, a, s) for s in range(3)]
            t = T0 + (rnd + 1) * SEC
            ent, _ = _run_round_struct(abi, a, models, hots, rnd, t)
            entries = _compounds(ent)
            raws, arena = _pack(abi, entries)
            if rnd == 0:  # refused calls leave the state untouched
                before = b.stream_rtcp(range(3)).tobytes()
                first = [_stats(abi, b, s).first_time_ns for s in range(3)]
                out = np.zeros(len(raws) + 1, dtype=abi.STREAM_RTCP_IN_RESULT_DTYPE)
                ar = np.frombuffer(arena, dtype=np.uint8)

                def call(rw):
                    return b.api["stream_rtcp_ingest"](b.h, rw.ctypes.data, len(rw), ar.ctypes.data, len(ar), t,
                                                       out.ctypes.data)

                split = np.concatenate([raws, raws[:1]])  # stream 0 again behind the others
                assert call(split) == -34
                far = raws.copy()
                far["off"][-1] = len(ar) - 4
                assert call(far) == -22
                big = raws.copy()
                big["len"][0] = 65536
                assert call(big) == -22
                assert b.stream_rtcp(range(3)).tobytes() == before
                assert [_stats(abi, b, s).first_time_ns for s in range(3)] == first
            hb = [_hot(abi, b, s) for s in range(3)]
            got = b.stream_rtcp_ingest(raws, arena, t)
            for i, (s, data) in enumerate(entries):
                want = twin[s].ingest(hb[s], data, t)
                g = {k: int(got[i][k]) for k in ("status", "n_sr", "flags", "ntp", "rtp_ext")}
                assert g == want, (rnd, i, g, want)
            assert [int(x) for x in got["status"]].count(P.IN_MALFORMED) == 1
            assert max(int(x) for x in got["n_sr"]) == 2
            assert a.stream_rtcp(range(3)).tobytes() == b.stream_rtcp(range(3)).tobytes(), rnd
            for s in range(3):
                assert _stats(abi, a, s).first_time_ns == _stats(abi, b, s).first_time_ns, (rnd, s)
    finally:
        a.close()
        b.close()


def _jitter_model(st, raws, flows, clock, abi):
    """updateJitter (rtpstats_base.go:775-810) over one ingest's datagrams of one stream, as
    tests/test_ingress_cpu.py's receiver restatement runs it: st = dict(first, lt, ljt, j)."""
    for i in range(len(raws)):
        f = int(flows["flags"][i])
        if f & (abi.LKF_FLOW_NOT_HANDLED | abi.LKF_FLOW_BAD | abi.LKF_FLOW_DUPLICATE):
            continue
        t, ets = int(raws["arrival_ns"][i]), int(flows["ext_ts"][i])
        if st["first"] is None:
            st["first"] = t
        if st["ljt"] == ets:
            continue
        since = (t - st["first"]) & P.M64
        prod = (since * clock) & P.M64
        prod = prod - 2**64 if prod >= 2**63 else prod
        rtp = ((abs(prod) // 10**9) * (1 if prod >= 0 else -1)) & P.M64  # Go's truncating /
        transit = (rtp - ets) & P.M64
        if st["lt"] != 0:
            d = (transit - st["lt"]) & P.M64
            d = d - 2**64 if d >= 2**63 else d
            st["j"] += (float(abs(d)) - st["j"]) / 16
        st["lt"], st["ljt"] = transit, ets


def test_first_time_adjustment_reaches_the_jitter_filter(pkg, abi):
    eng = _engine(pkg, abi)
    try:
        s = 1
        st = dict(first=None, lt=0, ljt=0, j=0.0)
        raws = _ingest(abi, eng, T0 + 100 * MS, 0, 30)
        fl = pkg.flows_array(eng.api, eng.h)
        mine = raws["stream"] == s
        _jitter_model(st, raws[mine], fl[mine], CLOCKS[s], abi)
        g = _stats(abi, eng, s)
        assert g.first_time_ns == st["first"] and bits(g.jitter) == bits(st["j"]) and g.jitter > 0
        # a sender report 1 s later that says 1.3 s of samples have passed: the first packet was 0.3 s late
        m = PyStreamRtcp(CLOCKS[s], SSRCS[s])
        hot = P.hot_of(g)
        t = st["first"] + SEC
        rtp = (TS0[s] + 13 * CLOCKS[s] // 10) & P.M32
        got = eng.stream_sender_reports(np.array([(s, rtp, to_ntp(t))], dtype=abi.STREAM_SR_DTYPE), t)
        want = m.sender_report(hot, rtp, to_ntp(t), t)
        assert (int(got[0]["flags"]), int(got[0]["ntp"]), int(got[0]["rtp_ext"])) == want
        assert want[0] == P.SSR_FIRST_TIME_ADJUSTED and hot["first_time"] == st["first"] - 300 * MS
        assert _stats(abi, eng, s).first_time_ns == hot["first_time"]
        assert int(eng.stream_rtcp([s])[0]["start_time_ns"]) == st["first"]  # startTime keeps the original
        # the next ingest's jitter runs with that first time
        st["first"] = hot["first_time"]
        raws = _ingest(abi, eng, T0 + 100 * MS + 2 * SEC, 30, 30, drop=(40,), swap=(45, 46))
        fl = pkg.flows_array(eng.api, eng.h)
        mine = raws["stream"] == s
        _jitter_model(st, raws[mine], fl[mine], CLOCKS[s], abi)
        g = _stats(abi, eng, s)
        assert g.first_time_ns == st["first"]
        assert g.last_transit == st["lt"] and g.last_jitter_ext_ts == st["ljt"]
        assert bits(g.jitter) == bits(st["j"]), (g.jitter, st["j"])
    finally:
        eng.close()


def test_nacks_wire(pkg, abi):
    eng = _engine(pkg, abi)
    try:
        pk, ar = eng.ingest_nacks_wire()  # before any ingest: no packets
        assert len(pk) == 0 and len(ar) == 0
        # 27 is more than 16 behind 5: when both are due together the record needs two pairs
        _ingest(abi, eng, T0 + 100 * MS, 0, 60, drop=(5, 6, 9, 27))
        recs, pairs = pkg.nacks_arrays(eng.api, eng.h)
        assert len(recs) >= 2 and len(pairs) >= len(recs) and int(recs["n_pairs"].max()) >= 2
        pk, ar = eng.ingest_nacks_wire()
        assert len(pk) == len(recs) and len(ar) == 12 * len(recs) + 4 * len(pairs)
        total = 0
        for i, r in enumerate(recs):
            assert (int(pk[i]["datagram"]), int(pk[i]["stream"])) == (int(r["datagram"]), int(r["stream"]))
            assert int(pk[i]["off"]) == 12 * i + 4 * int(r["pair_off"]) == total
            assert int(pk[i]["len"]) == 12 + 4 * int(r["n_pairs"])
            mine = pairs[int(r["pair_off"]):int(r["pair_off"]) + int(r["n_pairs"])]
            ssrc = int(r["media_ssrc"])
            assert ssrc == SSRCS[int(r["stream"])]
            want = W.nack(ssrc, ssrc, [(int(p["packet_id"]), int(p["lost_packets"])) for p in mine])
            data = bytes(ar[total:total + int(pk[i]["len"])])
            assert data == want, i
            # ... and parsed back by the ingress restatement: framing, then the sequence numbers
            (count, pt, at, body), = W.PyRtcpIn.packets(data)
            assert (count, pt, at) == (1, 205, 0) and struct.unpack(">II", body[4:12]) == (ssrc, ssrc)
            p = W.PyRtcpIn.parse(data, ssrc)
            assert p.status == W.IN_OK and len(p.sns) == int(r["num_nacked"])
            total += len(data)
        assert total == len(ar)
        # short capacities: the counts are set
        n, alen = C.c_uint32(), C.c_uint64()
        pkb = np.zeros(len(pk), dtype=abi.STREAM_RTCP_PKT_DTYPE)
        arb = np.zeros(len(ar), dtype=np.uint8)
        f = eng.api["ingest_nacks_wire"]
        assert f(eng.h, pkb.ctypes.data, len(pk) - 1, arb.ctypes.data, len(ar), C.byref(n), C.byref(alen)) == -28
        assert (n.value, alen.value) == (len(pk), len(ar))
        assert f(eng.h, pkb.ctypes.data, len(pk), arb.ctypes.data, len(ar) - 1, C.byref(n), C.byref(alen)) == -28
        assert (n.value, alen.value) == (len(pk), len(ar))
        assert f(eng.h, pkb.ctypes.data, len(pk), arb.ctypes.data, len(ar), C.byref(n), C.byref(alen)) == 0
        assert pkb.tobytes() == pk.tobytes() and arb.tobytes() == ar.tobytes()
        # the next ingest's list replaces it (the queues may NACK the old losses again)
        _ingest(abi, eng, T0 + 2 * SEC, 60, 10)
        recs, pairs = pkg.nacks_arrays(eng.api, eng.h)
        pk, ar = eng.ingest_nacks_wire()
        assert len(pk) == len(recs) and len(ar) == 12 * len(recs) + 4 * len(pairs)
    finally:
        eng.close()


def test_srtcp_both_ways(pkg, abi):
    """Sealed sender reports -> lkf_srtcp_unprotect(plain = NULL) -> lkf_stream_rtcp_ingest_unprotected equals
    the plaintext path, a tampered datagram arriving as len 0; wire32 -> lkf_srtcp_protect -> the opener."""
    a, b = _engine(pkg, abi), _engine(pkg, abi)
    try:
        ref = L.PySrtcpRx()
        keys = L.make_keys(2)  # AES-CM and GCM
        for eng in (a, b):
            for t, (mk, ms, prof) in enumerate(keys):
                assert eng.api["add_transport"](eng.h, C.byref(pkg.transport_params(mk, ms, prof))) == t
        for mk, ms, prof in keys:
            ref.add_transport(mk, ms, prof)
        for eng in (a, b):
            _ingest(abi, eng, T0 + 100 * MS, 0, 30, drop=(7,))
        hots = [_hot(abi, a, s) for s in range(3)]
        t = T0 + SEC
        ent = _sr_entries(0, t, hots)
        entries = _compounds(ent)
        # engine a: the plaintext path
        raws, arena = _pack(abi, entries)
        plain_res = a.stream_rtcp_ingest(raws, arena, t)
        # engine b: every compound sealed (stream 0 and 1 behind transport 0, stream 2 behind transport 1)
        ar = L.Arena()
        index = {0: 0, 1: 0}
        tampered = None
        for i, (s, data) in enumerate(entries):
            tr = 1 if s == 2 else 0
            index[tr] += 1
            sealed = L.seal(ref.aes, ref.sess[tr], keys[tr][2], data, index[tr])
            if s == 0 and tampered is None:
                tampered = i
                sealed = sealed[:9] + bytes([sealed[9] ^ 4]) + sealed[10:]
            ar.add(tr, sealed)
        src = np.frombuffer(bytes(ar.buf), dtype=np.uint8)
        res = np.zeros(len(entries), dtype=abi.SRTCP_RX_RESULT_DTYPE)
        rw = ar.raws(abi)
        assert b.api["srtcp_unprotect"](b.h, rw.ctypes.data, len(rw), src.ctypes.data, len(src), None,
                                        res.ctypes.data) == 0
        st = [int(x) for x in res["status"]]
        assert st[tampered] == L.AUTH and st.count(L.OK) == len(entries) - 1
        en = np.array([(s, i) for i, (s, _) in enumerate(entries)], dtype=abi.STREAM_RTCP_ENTRY_DTYPE)
        got = b.stream_rtcp_ingest_unprotected(en, t)
        for i in range(len(entries)):
            if i == tampered:
                assert int(got[i]["status"]) == P.IN_MALFORMED and int(got[i]["n_sr"]) == 0
            else:
                assert got[i].tobytes() == plain_res[i].tobytes(), i
        ra, rb = a.stream_rtcp(range(3)), b.stream_rtcp(range(3))
        assert ra[1:].tobytes() == rb[1:].tobytes()
        assert int(ra[0]["sr_newest"]["valid"]) == 1 and int(rb[0]["sr_newest"]["valid"]) == 0  # stream 0's was the tampered one
        bad = np.array([(0, len(entries))], dtype=abi.STREAM_RTCP_ENTRY_DTYPE)
        out = np.zeros(1, dtype=abi.STREAM_RTCP_IN_RESULT_DTYPE)
        assert b.api["stream_rtcp_ingest_unprotected"](b.h, bad.ctypes.data, 1, t, out.ctypes.data) == -22
        # out: the 32 bytes through lkf_srtcp_protect and the Python opener
        reqs = np.array([(s, 0) for s in range(3)], dtype=abi.STREAM_RR_REQ_DTYPE)
        recs, wire = a.stream_receiver_reports(reqs, t + 20 * MS, wire=True)
        assert all(int(r["flags"]) for r in recs)
        praw = np.array([(1 if s == 2 else 0, 32 * s, 32) for s in range(3)], dtype=abi.SRTCP_RAW_DTYPE)
        tx, prot = a.srtcp_protect(praw, wire.tobytes())
        for s in range(3):
            tr = 1 if s == 2 else 0
            pkt = bytes(prot[int(tx[s]["off"]):int(tx[s]["off"]) + int(tx[s]["len"])])
            assert int(tx[s]["ssrc"]) == SSRCS[s]
            assert ref.open(tr, pkt, SSRCS[s], int(tx[s]["index"])) == bytes(wire[s]), s
    finally:
        a.close()
        b.close()


def test_round_trip_between_two_engines(pkg, workload, abi):
    """Engine B (upstream) forwards to a DownTrack and builds its sender report; engine A receives the
    forwarded packets and that report, and answers with a receiver report; B derives the RTT from it."""
    from tests.test_rtcp_in_gpu import _rig
    rig = _rig(pkg, workload, 1, nb=2)
    a = None
    try:
        b = rig.eng
        tr = rig.tr
        rig.forward(1)
        rec, wire = b.drain()
        counts = np.bincount(rec["dt"].astype(np.int64), minlength=tr.ndts)
        d = int(np.argmax(counts))
        assert counts[d] >= 10
        track = tr.tracks[tr.downtracks[d].track]
        ssrc = int(tr.downtracks[d].ssrc)
        t0 = T0 + 3 * SEC
        d1, d2, d3 = 23 * MS + 456789, 410 * MS + 1234, 31 * MS + 987654
        sr, sr_wire = b.rtcp_sender_reports(np.array([(d, 0)], dtype=abi.RTCP_SR_REQ_DTYPE), t0, wire=True)
        assert int(sr[0]["flags"]) & abi.LKF_SR_VALID
        # engine A: one stream with that SSRC
        a = pkg.Engine(max_tracks=16, max_downtracks=16, max_batch_pkts=2048, max_batch_arena=1 << 20,
                       max_out_pkts=4096, max_out_bytes=1 << 22, max_batch_tuples=4096)
        assert a.api["add_track"](a.h, C.byref(abi.lkf_track_params(
            track_id=1, room=0, publisher=0, kind=int(track.kind), codec=int(track.codec),
            clock_rate=int(track.clock_rate)))) == 0
        assert a.api["add_stream"](a.h, C.byref(abi.lkf_stream_params(track=0, layer=0, ssrc=ssrc))) == 0
        mine = rec[rec["dt"] == d]
        rows, buf = [], bytearray()
        for i, r in enumerate(mine):
            p = bytes(wire[int(r["out_off"]):int(r["out_off"]) + int(r["out_len"])])
            off = (len(buf) + 15) // 16 * 16
            buf += bytes(off - len(buf)) + p
            rows.append((t0 - SEC + i * MS, 0, off, len(p), 0))
        raws = np.array(rows, dtype=abi.RAW_PKT_DTYPE)
        arena = np.frombuffer(bytes(buf), dtype=np.uint8)
        assert a.api["ingest"](a.h, raws.ctypes.data, len(raws), arena.ctypes.data, len(arena)) == 0
        hot = _hot(abi, a, 0)
        assert hot["init"]
        m = PyStreamRtcp(int(track.clock_rate), ssrc)
        got = a.stream_rtcp_ingest(np.array([(0, 0, 28)], dtype=abi.STREAM_RTCP_RAW_DTYPE), sr_wire.tobytes(), t0 + d1)
        want = m.ingest(hot, sr_wire.tobytes(), t0 + d1)
        assert {k: int(got[0][k]) for k in want} == want and want["n_sr"] == 1
        assert want["ntp"] == int(sr[0]["ntp"]) and (want["rtp_ext"] & P.M32) == int(sr[0]["rtp"])
        recs, rr_wire = a.stream_receiver_reports(np.array([(0, 0)], dtype=abi.STREAM_RR_REQ_DTYPE), t0 + d1 + d2,
                                                  wire=True)
        rr = m.reception_report(hot, 0, t0 + d1 + d2)
        assert {k: int(recs[0][k]) for k in P.RR_FIELDS} == rr and rr["flags"] == P.SRR_VALID
        assert rr["last_sender_report"] == (int(sr[0]["ntp"]) >> 16) & P.M32
        assert rr["delay"] == (d2 // 1000) * 65536 // 1000000
        # back on B
        now = t0 + d1 + d2 + d3
        out, fb, fbo, _, _ = b.rtcp_ingest(np.array([(d, 0, 32)], dtype=abi.RTCP_RAW_DTYPE), rr_wire.tobytes(), now)
        assert int(out[0]["status"]) == abi.LKF_RTCP_IN_OK and int(out[0]["reports"]) == 1 and len(fb) == 1
        rtt = get_rtt_ms(rr["last_sender_report"], rr["delay"], int(sr[0]["ntp"]), t0, now)
        assert rtt is not None and abs(rtt - (d1 + d3) / MS) <= 1.0  # (1/65536 s units, rounded up to a ms)
        assert int(fbo[0]["flags"]) & abi.LKF_FB_RTT_CHANGED
        assert int(fbo[0]["rtt_ms"]) == rtt == int(out[0]["rtt_ms"])
        for k in ("fraction_lost", "total_lost", "last_sequence_number", "jitter", "last_sender_report", "delay"):
            assert int(fb[0][k]) == rr[k], k
    finally:
        if a is not None:
            a.close()
        rig.close()
