"""SRTCP on the GPU (lkf_srtcp_unprotect, lkf_rtcp_ingest_unprotected,
lkf_srtcp_protect; srtp_kernels.hip k_srtcp_*) against tests/srtcp_lib: the
restatement PySrtcpRx of the receive side (every result field, every plaintext
byte, the slot tables and counters after each call), the Python sealer and index
model for the send side, a twin engine fed the plaintext through lkf_rtcp_ingest
for the composition, and a round trip between two engines with the same keys.

Small engines, four transports (AES-CM, GCM, AES-CM, GCM); everything exact.
"""
import ctypes as C

import numpy as np
import pytest

from tests import rtcp_lib, rtx_lib
from tests import rtcp_wire_lib as W
from tests import srtcp_lib as L
from tests.srtp_lib import GCM

pytestmark = pytest.mark.gpu
EPOCH = 1700000000 * 10**9
SEC = 10**9
RES_FIELDS = ("ssrc", "index", "status", "len")


def _engine(pkg):
    return pkg.Engine(max_tracks=16, max_downtracks=16, max_batch_pkts=2048, max_batch_arena=1 << 20,
                      max_out_pkts=4096, max_out_bytes=1 << 22, max_batch_tuples=4096)


def _add_transports(pkg, eng, ref=None):
    keys = L.make_keys(4)
    for t, (mk, ms, prof) in enumerate(keys):
        assert eng.api["add_transport"](eng.h, C.byref(pkg.transport_params(mk, ms, prof))) == t
        if ref is not None:
            assert ref.add_transport(mk, ms, prof) == t
    return keys


class Sub:
    """One sender SSRC behind transport t."""

    def __init__(self, ref, t, ssrc):
        self.ref, self.t, self.ssrc = ref, t, ssrc

    def seal(self, index, body=20, e_bit=1):
        return L.seal(self.ref.aes, self.ref.sess[self.t], self.ref.keys[self.t][2],
                      L.rtcp_plain(self.ssrc, body, fill=index), index & 0x7FFFFFFF, e_bit)


def _flip(data, byte, bit=0):
    d = bytearray(data)
    d[byte % len(d)] ^= 1 << bit
    return bytes(d)


def _check(abi, eng, ref, ar, label):
    """One lkf_srtcp_unprotect of the arena against the restatement -> the statuses."""
    want, plain = ref.unprotect(ar.pkts, ar.buf)
    raws = ar.raws(abi)
    src = np.frombuffer(bytes(ar.buf), dtype=np.uint8)
    out = np.zeros(len(raws), dtype=abi.SRTCP_RX_RESULT_DTYPE)
    host = np.full(len(src) + 64, 0xEE, dtype=np.uint8)
    rc = eng.api["srtcp_unprotect"](eng.h, raws.ctypes.data, len(raws), src.ctypes.data, len(src), host.ctypes.data,
                                    out.ctypes.data)
    assert rc == 0, (label, rc)
    assert (host[len(src):] == 0xEE).all(), label  # nothing past the arena length
    for i, w in enumerate(want):
        got = tuple(int(out[i][f]) for f in RES_FIELDS)
        assert got == w, (label, i, got, w)
        if w[2] == L.OK:
            off = ar.pkts[i][1]
            assert bytes(host[off:off + w[3]]) == plain[i], (label, i)
    for t, tb in enumerate(ref.tables):
        assert eng.transport_srtcp(t) == tb.as_tuple(), (label, t)
    return [w[2] for w in want]


def _pattern(ar, a, b):
    """One transport's hand-built pattern of the first call: SSRCs a and b (Sub) interleaved."""
    t = a.t
    tag = L.tag_len(a.ref.keys[t][2])
    order = [1, 3, 2, 5, 4, 6, 8, 7, 9, 12, 11, 10]  # reordered inside the window
    for k, n in enumerate(L.BODY_LENS):  # every body length
        ar.add(t, a.seal(order[k], n))
        if k % 4 == 0:
            ar.add(t, b.seal(1 + k // 4, 13))  # the second SSRC interleaved
    ar.add(t, a.seal(100))
    ar.add(t, a.seal(37))  # 63 behind: accepted
    ar.add(t, a.seal(37))  # ... and then a duplicate
    ar.add(t, a.seal(36))  # 64 behind: old
    ar.add(t, a.seal(400))  # a jump of 300
    ar.add(t, a.seal(0xFFFF, 44))
    ar.add(t, a.seal(0x10000, 44))  # carries across the counter's word
    ar.add(t, _flip(a.seal(0x100000), -1))  # forged far ahead ...
    ar.add(t, a.seal(0x10001))  # ... then valid ones
    ar.add(t, a.seal(0x10002))
    good = a.seal(0x10003, 31)
    ar.add(t, _flip(good, 10, 3))  # a forged copy before the valid original
    ar.add(t, good)
    nxt = a.seal(0x10004, 24)
    trailer = len(nxt) - 1 if tag == 16 else len(nxt) - 11
    for byte, bit in ((trailer - 4 if tag == 16 else -1, 7), (9, 0), (1, 2), (trailer, 0), (trailer - 3, 6), (5, 4)):
        ar.add(t, _flip(nxt, byte, bit))  # tag, body, header, index, a high index bit, SSRC
    ar.add(t, nxt)


def _bad_ones(ar, subs):
    """Malformed and unencrypted datagrams under both profiles, an unknown handle, an empty one."""
    for s in subs:
        tag = L.tag_len(s.ref.keys[s.t][2])
        ar.add(s.t, s.seal(5000, e_bit=0))  # E = 0
        ar.add(s.t, s.seal(5001, 0)[:8 + 4 + tag - 1])  # too short by one byte
        ar.add(s.t, s.seal(5002), misalign=8)
        ar.add(s.t, _flip(s.seal(5003), 0, 6))  # version 3
        ar.add(s.t, _flip(_flip(s.seal(5004), 0, 7), 0, 6))  # version 1
        ar.add(s.t, s.seal(5005), length=0)
        ar.add(s.t, s.seal(0x2F000, 0))  # the shortest valid one
    ar.add(7, subs[0].seal(5007))  # unknown handles
    ar.add(-1, subs[0].seal(5008))


def test_hand_built_receive(pkg, abi):
    eng = _engine(pkg)
    try:
        ref = L.PySrtcpRx()
        _add_transports(pkg, eng, ref)
        a = [Sub(ref, t, 0xA0000000 + t) for t in range(2)]
        b = [Sub(ref, t, 0x11112222) for t in range(2)]  # (the same SSRC on both, and on transport 2 below)
        seen = set()
        # call 0: the pattern on transports 0 and 1; the slot tables of 2 and 3 filled
        ar = L.Arena()
        for t in range(2):
            _pattern(ar, a[t], b[t])
        fill = {t: [Sub(ref, t, 0x30000000 + 16 * t + k) for k in range(17)] for t in (2, 3)}
        for t in (2, 3):
            ar.add(t, _flip(Sub(ref, t, 0x66660000 + t).seal(1), 12))  # forged, a fresh SSRC: takes no slot
            for s in fill[t][:16]:
                ar.add(t, s.seal(1))
            ar.add(t, fill[t][16].seal(1))  # the 17th: no slot
            ar.add(t, _flip(fill[t][16].seal(2), 12))  # (no slot comes before authentication)
            ar.add(t, fill[t][3].seal(2))  # an old SSRC is still served
        st = _check(abi, eng, ref, ar, "call 0")
        seen |= set(st)
        for t in (2, 3):
            slots, counters = ref.tables[t].as_tuple()
            assert [s[1] for s in slots] == [x.ssrc for x in fill[t][:16]] and all(s[0] for s in slots)
            assert counters == (17, 1, 0, 0, 0, 2)
        for t in range(2):  # the forged packet far ahead did not move latest; the forged copy did not block
            assert ref.tables[t].slots[0][:3] == [1, a[t].ssrc, 0x10004] and ref.tables[t].auth_failures == 8
        # call 1: more than 64 datagrams per transport, interleaved, with an authentication failure, a
        # duplicate and a forged copy before its original inside (the chunk loop and the commit's second walk)
        ar = L.Arena()
        for k in range(150):
            for t in range(2):
                idx = 0x20000 + k
                d = a[t].seal(idx, (13, 48, 60)[k % 3])
                if k == 70:
                    d = _flip(d, -2)
                if k == 100:
                    d = a[t].seal(idx - 1, (13, 48, 60)[(k - 1) % 3])
                if k == 80:
                    ar.add(t, _flip(d, 11, 5))
                ar.add(t, d)
        _bad_ones(ar, [a[0], a[1]])
        st = _check(abi, eng, ref, ar, "call 1")
        seen |= set(st)
        assert st.count(L.AUTH) == 4 and st.count(L.REPLAY_DUP) == 2 and sum(p[0] == 0 for p in ar.pkts) > 128
        # call 2: the same SSRC on two transports is independent state; the largest index
        ar = L.Arena()
        ar.add(0, Sub(ref, 0, fill[2][0].ssrc).seal(5))
        ar.add(2, fill[2][0].seal(2))
        ar.add(2, b[0].seal(1))  # (transport 2's table is full: 0x11112222 finds no slot there)
        for t in range(2):
            ar.add(t, b[t].seal(4))
            ar.add(t, a[t].seal(0x7FFFFFFF, 56))
            ar.add(t, a[t].seal(0x7FFFFFFF, 56))
        st = _check(abi, eng, ref, ar, "call 2")
        assert st == [L.OK, L.OK, L.NO_SLOT] + [L.OK, L.OK, L.REPLAY_DUP] * 2
        seen |= set(st)
        assert seen == {L.OK, L.MALFORMED, L.REPLAY_OLD, L.REPLAY_DUP, L.AUTH, L.UNENCRYPTED, L.NO_SLOT}
        # a reset clears one table and nothing else
        eng.srtcp_reset(2)
        ref.reset(2)
        assert eng.transport_srtcp(2) == L.Table().as_tuple()
        ar = L.Arena()
        ar.add(2, fill[2][16].seal(1))
        ar.add(3, fill[3][16].seal(3))
        assert _check(abi, eng, ref, ar, "after reset") == [L.OK, L.NO_SLOT]
        # an empty call, and no plaintext wanted
        out, plain = eng.srtcp_unprotect(np.zeros(0, dtype=abi.SRTCP_RAW_DTYPE), b"")
        assert len(out) == 0 and len(plain) == 0
        ar = L.Arena()
        ar.add(0, Sub(ref, 0, 0xC0C0C0C0).seal(1))
        out, plain = eng.srtcp_unprotect(ar.raws(abi), bytes(ar.buf), want_plain=False)
        assert plain is None and int(out[0]["status"]) == L.OK
    finally:
        eng.close()


# ---- composition with RTCP ingress ---------------------------------------------------
def _traffic(rig, dts, nacks, lsr, rnd):
    """Three compounds per DownTrack, built with tests/test_rtcp_in_gpu's builders: a reception report with
    LSR / DLSR and counts; the DownTrack's NACK list and a PLI; FIR, REMB and TWCC."""
    from tests.test_rtcp_in_gpu import _block, _compound_like_struct_entry, _nack_compounds
    out = []
    for d in dts:
        m = rig.models[d]
        ssrc = rtcp_lib.ssrc(rig, d)
        lsn = rtcp_lib.rr_lsn(m.s.high_sn if m.s.init else 0, m.s.start_sn)
        out.append((d, _compound_like_struct_entry(rig, (d, True, lsn, rnd + d % 3, 50 * rnd + d, lsr[d], 0x4000,
                                                         d % 3, rnd, d % 2))))
        mine = nacks[nacks["dt"] == d]
        out.append((d, _nack_compounds(rig, mine)[0][1] if len(mine) else W.compound(W.nack(1, ssrc, [(9, 1)]))))
        out.append((d, W.compound(W.rr(1, [_block(rig, d, m.s.high_sn if m.s.init else 0, jitter=7)]),
                                  W.fir(1, ssrc, [(ssrc, rnd)]), W.remb(1, ssrcs=[ssrc]), W.twcc(1, ssrc),
                                  W.pli(1, ssrc))))
    return out


@pytest.mark.parametrize("config", [2])
def test_composes_with_rtcp_ingest(pkg, workload, abi, config):
    """Engine A: lkf_srtcp_unprotect, then lkf_rtcp_ingest_unprotected.  Engine B: lkf_rtcp_ingest of the
    plaintext, len 0 for exactly the datagrams the restatement rejects.  Every output bit for bit."""
    from tests.test_rtcp_in_gpu import _rig
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
        senders = [L.Composer(ref.aes, ref.sess[t], keys[t][2], L.COMPOSE_SEED + t) for t in range(4)]
        nacks = rtx_lib.make_nacks(a.o.api, a.oh, a.tr, seed=5)
        sent = [0] * 4
        total = rejected = 0
        for rnd in range(2):
            now = EPOCH + (2 + rnd) * SEC
            reqs = np.array([(d, 0) for d in range(a.tr.ndts)], dtype=abi.RTCP_SR_REQ_DTYPE)
            rep = [r.eng.rtcp_sender_reports(reqs, now - SEC // 2) for r in (a, b)][0]  # so that the reports carry an RTT
            lsr = [(int(x["ntp"]) >> 16) & 0xFFFFFFFF for x in rep]
            traffic = _traffic(a, dts, nacks, lsr, rnd)
            prot = L.Arena()
            for d, data in traffic:
                t = transport_of[d]
                prot.add(t, senders[t].seal(data))
                sent[t] += 1
            want, _ = ref.unprotect(prot.pkts, prot.buf)
            plain_ar = bytearray(len(prot.buf))  # engine B's arena: the accepted compounds at their datagrams' offsets
            for (d, data), p, w in zip(traffic, prot.pkts, want):
                if w[2] == L.OK:
                    assert w[3] == len(data)
                    plain_ar[p[1]:p[1] + len(data)] = data
            res, plain = a.eng.srtcp_unprotect(prot.raws(abi), bytes(prot.buf))
            assert [tuple(int(r[f]) for f in RES_FIELDS) for r in res] == want
            ok = [w[2] == L.OK for w in want]
            total += len(ok)
            rejected += len(ok) - sum(ok)
            entries = np.array([(d, i) for i, (d, _) in enumerate(traffic)], dtype=abi.RTCP_ENTRY_DTYPE)
            ga = a.eng.rtcp_ingest_unprotected(entries, now)
            raws = np.array([(d, prot.pkts[i][1] if ok[i] else 0, len(data) if ok[i] else 0)
                             for i, (d, data) in enumerate(traffic)], dtype=abi.RTCP_RAW_DTYPE)
            gb = b.eng.rtcp_ingest(raws, bytes(plain_ar), now)
            for x, y, name in zip(ga, gb, ("out", "fb", "fb_out", "refs", "n_nacks")):
                if name == "n_nacks":
                    assert x == y and x > 0
                else:
                    assert len(x) == len(y) > 0 and x.tobytes() == y.tobytes(), (rnd, name)
            assert [int(s) for s in ga[0]["status"]] == [0 if k else 1 for k in ok]
            for r in ga[3]:  # the pass-through records index the plaintext arena the host got back
                at = int(r["off"])
                assert bytes(plain[at:at + int(r["len"])]) == bytes(plain_ar[at:at + int(r["len"])])
            assert a.eng.rtcp_ingested_nacks().tobytes() == b.eng.rtcp_ingested_nacks().tobytes()
            ra, rb = a.eng.rtx_lookup_ingested(now), b.eng.rtx_lookup_ingested(now)
            assert ra.tobytes() == rb.tobytes() and (rnd or len(ra) > 0)
            every = list(range(a.tr.ndts))
            assert a.eng.sender_rtcp(every).tobytes() == b.eng.sender_rtcp(every).tobytes()
            assert any(int(x) for x in ga[0]["rtt_ms"])  # the reports carried an RTT: otherwise vacuous
        assert sent == [L.COMPOSE_PER_TRANSPORT] * 4  # what tests/test_srtcp_cpu.py checked the seed for
        assert rejected >= 1 and 2 * (total - rejected) >= total, (rejected, total)
        # a datagram index out of range is refused before anything runs
        before = a.eng.sender_rtcp(every).tobytes()
        bad = np.array([(dts[0], total)], dtype=abi.RTCP_ENTRY_DTYPE)
        with pytest.raises(pkg.EngineError, match="rc=-22"):
            a.eng.rtcp_ingest_unprotected(bad, EPOCH + 9 * SEC)
        assert a.eng.sender_rtcp(every).tobytes() == before
    finally:
        a.close()
        b.close()


# ---- send ----------------------------------------------------------------------------
def _protect_call(abi, eng, ref, tx, pkts, label):
    """pkts: (transport, plaintext) -> one lkf_srtcp_protect against the sealer and the index model."""
    plain, raws = bytearray(b"\xee" * 3), np.zeros(len(pkts), dtype=abi.SRTCP_RAW_DTYPE)
    for i, (t, p) in enumerate(pkts):
        raws[i] = (t, len(plain), len(p))  # (the input needs no alignment)
        plain += p + b"\xee" * (i % 5)
    res, out = eng.srtcp_protect(raws, bytes(plain))
    off = 0
    for i, (t, p) in enumerate(pkts):
        ssrc = int.from_bytes(p[4:8], "big")
        idx = tx.next(t, ssrc)
        want = L.seal(ref.aes, ref.sess[t], ref.keys[t][2], p, idx)
        assert tuple(int(res[i][f]) for f in ("ssrc", "index", "off", "len")) == (ssrc, idx, off, len(want)), (label, i)
        slot = (len(p) + 20 + 15) & ~15
        assert bytes(out[off:off + slot]) == want + bytes(slot - len(want)), (label, i)
        off += slot
    assert len(out) == off
    for (t, ssrc), idx in tx.last.items():
        assert eng.srtcp_tx_index(t, ssrc) == idx, (label, t, ssrc)
    return res, out


def test_protect(pkg, abi):
    eng = _engine(pkg)
    try:
        ref, tx = L.PySrtcpRx(), L.TxIndex()
        _add_transports(pkg, eng, ref)
        assert eng.srtcp_tx_index(0, 0xB0000000) == 0
        for call in range(3):
            pkts = [(t, L.rtcp_plain(0xB0000000 + 16 * t + (k + call) % 2, n, fill=k + call))
                    for k, n in enumerate(L.BODY_LENS) for t in range(4)]
            res, _ = _protect_call(abi, eng, ref, tx, pkts, "call %d" % call)
            if call == 0:
                assert int(res[0]["index"]) == 1  # the first index is 1
        assert eng.srtcp_tx_index(0, 0xB0000000) == tx.last[(0, 0xB0000000)] == 18  # consecutive across calls
        # a refused call consumes no index
        good = L.rtcp_plain(0xB0000000, 12)
        plain = np.frombuffer(good + good[:7] + _flip(good, 0, 7), dtype=np.uint8)
        out = np.zeros(4096, dtype=np.uint8)
        res = np.zeros(2, dtype=abi.SRTCP_TX_RESULT_DTYPE)
        n = C.c_uint64()

        def call(rows, cap=4096):
            raws = np.array(rows, dtype=abi.SRTCP_RAW_DTYPE)
            return eng.api["srtcp_protect"](eng.h, raws.ctypes.data, len(raws), plain.ctypes.data, len(plain),
                                            out.ctypes.data, cap, res.ctypes.data, C.byref(n))

        assert call([(0, 0, 20), (0, 20, 7)]) == -22  # shorter than a header
        assert call([(0, 0, 20), (0, 27, 20)]) == -22  # version 0
        assert call([(0, 0, 20), (4, 0, 20)]) == -22  # an unknown transport
        assert call([(0, 0, 20), (0, 40, 20)]) == -22  # beyond the plaintext
        assert call([(0, 0, 20), (1, 0, 20)], cap=95) == -28 and n.value == 96  # a short output
        assert eng.srtcp_tx_index(0, 0xB0000000) == 18 and eng.srtcp_tx_index(1, 0xB0000000) == 0
        assert call([(0, 0, 20), (1, 0, 20)], cap=96) == 0 and n.value == 96
        assert eng.srtcp_tx_index(0, 0xB0000000) == 19 and eng.srtcp_tx_index(1, 0xB0000000) == 1
        eng.srtcp_reset(0)  # a new session: the handle's send indices start again
        assert eng.srtcp_tx_index(0, 0xB0000000) == 0 and eng.srtcp_tx_index(1, 0xB0000000) == 1
    finally:
        eng.close()


# ---- round trip ----------------------------------------------------------------------
@pytest.mark.parametrize("config", [2])
def test_sender_reports_round_trip(pkg, workload, abi, config):
    """lkf_rtcp_sender_reports(wire) -> lkf_srtcp_protect on engine A -> lkf_srtcp_unprotect on engine B, which
    holds the same master keys: the 28 bytes come back, and presented again they are duplicates."""
    from tests.test_rtcp_in_gpu import _rig
    a = _rig(pkg, workload, config, nb=2)
    b = _engine(pkg)
    try:
        _add_transports(pkg, a.eng)
        _add_transports(pkg, b)
        a.forward(2)
        dts = [d for d, m in enumerate(a.models) if m.s.init][:16]  # (four sender SSRCs per transport)
        assert len(dts) >= 8
        for rnd in range(2):
            reqs = np.array([(d, 0) for d in dts], dtype=abi.RTCP_SR_REQ_DTYPE)
            _, wire = a.eng.rtcp_sender_reports(reqs, EPOCH + (2 + rnd) * SEC, wire=True)
            raws = np.array([(i % 4, 28 * i, 28) for i in range(len(dts))], dtype=abi.SRTCP_RAW_DTYPE)
            res, prot = a.eng.srtcp_protect(raws, wire.tobytes())
            assert [int(x) for x in res["len"]] == [28 + (20 if i % 2 else 14) for i in range(len(dts))]
            back = np.array([(i % 4, int(r["off"]), int(r["len"])) for i, r in enumerate(res)],
                            dtype=abi.SRTCP_RAW_DTYPE)
            out, plain = b.srtcp_unprotect(back, prot)
            assert [int(x) for x in out["status"]] == [L.OK] * len(dts)
            assert [int(x) for x in out["len"]] == [28] * len(dts)
            assert [int(x) for x in out["index"]] == [int(x) for x in res["index"]]
            for i, r in enumerate(res):
                assert bytes(plain[int(r["off"]):int(r["off"]) + 28]) == bytes(wire[i]), i
            out, _ = b.srtcp_unprotect(back, prot)
            assert [int(x) for x in out["status"]] == [L.REPLAY_DUP] * len(dts)
    finally:
        a.close()
        b.close()
