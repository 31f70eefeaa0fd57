"""SRTP unprotect on the GPU (lkf_unprotect_device / lkf_ingest_srtp) against
tests/srtp_rx_lib's restatement, and composed with ingest and run.

Hand-built streams: a handful of streams under AES-CM, GCM and no transport;
every status, index and len, every plaintext byte of the accepted datagrams and
lkf_stream_srtp_get must equal the restatement over three calls.  Trace
composition: a protected trace through unprotect -> ingest -> run must equal a
second engine that ingests the plaintext directly (with exactly the
restatement's rejected datagrams at len 0 when the trace is corrupted).
"""
import ctypes as C

import numpy as np
import pytest

from tests import srtp_lib
from tests import srtp_rx_lib as R

pytestmark = pytest.mark.gpu

PAYLOADS = (0, 1, 15, 16, 17, 47, 48, 49, 63, 64, 65, 1200)
KINDS = ("plain", "csrc", "ext1", "ext2")


# ---- device plumbing ---------------------------------------------------------------
class DeviceCall:
    """One unprotect call's device buffers (kept alive until the engine has synchronized)."""

    def __init__(self, raws, srtp):
        import torch

        dev = torch.device("cuda", 0)
        self.n, self.alen = len(raws), len(srtp)
        self.d_pk = torch.from_numpy(np.ascontiguousarray(raws).view(np.uint8).copy()).to(dev)
        self.d_srtp = torch.zeros(self.alen + 64, dtype=torch.uint8, device=dev)
        if self.alen:
            self.d_srtp[:self.alen].copy_(torch.frombuffer(bytearray(srtp), dtype=torch.uint8))
        self.d_out = torch.zeros_like(self.d_pk)
        self.d_plain = torch.full((self.alen + 64,), 0xEE, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)

    def unprotect(self, eng):
        p = lambda t: C.c_void_p(t.data_ptr())
        eng.unprotect_device(p(self.d_pk), self.n, p(self.d_srtp), self.alen, p(self.d_out), p(self.d_plain))

    def ingest(self, eng):
        eng.ingest_device(C.c_void_p(self.d_out.data_ptr()), self.n, C.c_void_p(self.d_plain.data_ptr()), self.alen)

    def outputs(self, abi):
        """(pkts_out, plaintext arena with its 64-byte tail) — after the engine synchronized."""
        return self.d_out.cpu().numpy().view(abi.RAW_PKT_DTYPE), self.d_plain.cpu().numpy()


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _check_call(abi, eng, call, ref, pkts, srtp, label):
    """The last unprotect of `call` on `eng` against the restatement `ref` -> the statuses."""
    want, plain = ref.unprotect(pkts, srtp)
    got = eng.unprotect_results()
    out, arena = call.outputs(abi)
    assert len(got) == len(want) == len(out)
    for i, (v, st, ln) in enumerate(want):
        assert (int(got["index"][i]), int(got["status"][i]), int(got["len"][i])) == (v, st, ln), (label, i, pkts[i])
        assert int(out["len"][i]) == ln and int(out["off"][i]) == pkts[i][1] and int(out["stream"][i]) == pkts[i][0]
        if st == R.OK:
            assert arena[pkts[i][1]:pkts[i][1] + ln].tobytes() == plain[i], (label, i)
    assert np.all(arena[len(srtp):] == 0xEE), "bytes written past the arena"
    for s in range(len(ref.streams)):
        assert eng.stream_srtp(s) == ref.streams[s].as_tuple(), (label, s)
    return [st for _, st, _ in want]


# ---- hand-built streams --------------------------------------------------------------
def _flip(data, byte, bit=0):
    d = bytearray(data)
    d[byte % len(d)] ^= 1 << bit
    return bytes(d)


class Pub:
    """One bound stream's sender: seals packet index idx (ROC = idx >> 16)."""

    def __init__(self, aes, stream, ssrc, key):
        self.aes, self.stream, self.ssrc, self.key = aes, stream, ssrc, key
        self.sess = srtp_lib.session(aes, key[1], key[2], key[3])
        self.tag = 16 if key[3] == srtp_lib.GCM else 10

    def plain(self, idx, plen=20, kind="plain"):
        return R.rtp_packet(self.ssrc, idx, bytes((idx * 31 + j * 7) & 255 for j in range(plen)), kind, ts=idx * 960)

    def seal(self, idx, plen=20, kind="plain"):
        return R.seal(self.aes, self.sess, self.key[3], self.plain(idx, plen, kind), idx >> 16)


def _pattern(pub, ar, call):
    """The sequence patterns of one stream for call 0, 1, 2, appended to arena `ar`."""
    s = pub.stream
    shape = lambda idx: (PAYLOADS[(idx - 65500) % 12], KINDS[((idx - 65500) // 12) % 4])
    if call == 0:
        # every payload length under every header kind, SEQ from 65,500 across the wrap, reordered across it
        order = list(range(65500, 65530)) + [65538, 65535, 65536, 65530, 65537, 65531, 65534, 65539, 65532, 65533] \
            + list(range(65540, 65548))
        for idx in order:
            ar.add(s, pub.seal(idx, *shape(idx)))
        ar.add(s, pub.seal(65536, *shape(65536)))  # exact duplicates
        ar.add(s, pub.seal(65545, *shape(65545)))
        ar.add(s, _flip(pub.seal(65547 + 20000), -1))  # forged far ahead: must not move s_l
        ar.add(s, _flip(pub.seal(65548, 33), 14))  # a forged copy of a valid packet, before it
        ar.add(s, pub.seal(65548, 33))
        ar.add(s, _flip(pub.seal(65549, 40), -1, 3))  # tag bit
        ar.add(s, _flip(pub.seal(65550, 40), 30))  # payload bit
        ar.add(s, _flip(pub.seal(65551, 40), 5))  # header bit (timestamp)
        ar.add(s, pub.plain(65560, 5))  # too short for its tag (17 bytes)
        ar.add(s, pub.seal(65561), misalign=8)  # misaligned off
        v1 = bytearray(pub.seal(65562))
        v1[0] = (v1[0] & 0x3F) | 0x40  # version 1
        ar.add(s, v1)
    elif call == 1:
        for idx in range(65552, 65558):
            ar.add(s, pub.seal(idx))
        x = 65552 + 300
        for idx in (x, x - 64, x - 63, x - 63, x + 1):  # 64 behind: too old; 63 behind: accepted, then a duplicate
            ar.add(s, pub.seal(idx, 25, "ext1"))
    else:
        x = 65552 + 300
        for idx in list(range(x + 2, x + 9)) + [x - 10, x - 10]:
            ar.add(s, pub.seal(idx, 64, "csrc"))
        # two forged jumps of 30,000 each: had they counted, the packets after them would be estimated one
        # rollover ahead; they did not, and those packets authenticate under the unchanged ROC
        ar.add(s, _flip(pub.seal(x + 8 + 30000), -1))
        ar.add(s, _flip(pub.seal(x + 8 + 60000), -1))
        for idx in range(x + 9, x + 14):
            ar.add(s, pub.seal(idx, 49, "ext2"))


def _hand_calls(abi, pubs, long_cm, long_gcm, unbound):
    """Three calls' arenas (grouped by track: the two patterned streams share track 0)."""
    calls = []
    rng = np.random.default_rng(3)
    for call in range(3):
        ar = R.Arena()
        a0, a1 = R.Arena(), R.Arena()
        _pattern(pubs[0], a0, call)
        _pattern(pubs[1], a1, call)
        for (s0, o0, l0), (s1, o1, l1) in zip(a0.pkts, a1.pkts):  # interleaved, misalignment kept
            ar.add(s0, a0.buf[o0:o0 + l0], misalign=o0 % 16)
            ar.add(s1, a1.buf[o1:o1 + l1], misalign=o1 % 16)
        if call == 0:
            ar.add(unbound, rng.integers(0, 256, 30, dtype=np.uint8).tobytes())
            ar.add(unbound, rng.integers(0, 256, 7, dtype=np.uint8).tobytes())
            ar.add(unbound, rng.integers(0, 256, 50, dtype=np.uint8).tobytes(), misalign=4)
            for k in range(150):  # more than 64 datagrams of one stream, a failure and a duplicate inside
                if k == 70:
                    ar.add(long_cm.stream, _flip(long_cm.seal(100 + k), 20))
                if k == 100:
                    ar.add(long_cm.stream, long_cm.seal(100 + 50))
                ar.add(long_cm.stream, long_cm.seal(100 + k))
            for k in range(130):  # more than 64 clean ones under GCM, across the wrap
                ar.add(long_gcm.stream, long_gcm.seal(65480 + k, 31))
        elif call == 1:
            for k in range(150, 160):
                ar.add(long_cm.stream, long_cm.seal(100 + k))
            for k in range(130, 200):
                ar.add(long_gcm.stream, long_gcm.seal(65480 + k, 31))
        else:
            ar.add(long_cm.stream, _flip(long_cm.seal(100 + 160), -1))
            for k in range(200, 205):
                ar.add(long_gcm.stream, long_gcm.seal(65480 + k, 31))
        calls.append(ar)
    return calls


def test_hand_built_streams(pkg, abi):
    aes = R.OpenSSLOpen()
    rng = np.random.default_rng(17)
    eng = pkg.Engine(max_tracks=16, max_downtracks=16, max_batch_pkts=2048, max_batch_arena=1 << 20,
                     max_out_pkts=4096, max_out_bytes=1 << 22, max_batch_tuples=4096)
    try:
        for t, (kind, codec, clock) in enumerate([(1, 2, 90000), (0, 1, 48000), (1, 2, 90000), (1, 2, 90000)]):
            assert eng.api["add_track"](eng.h, C.byref(abi.lkf_track_params(
                track_id=100 + t, room=0, publisher=t, kind=kind, codec=codec, clock_rate=clock))) == t
        ssrcs = (0x1000A001, 0x1000A002, 0x2000B001, 0x3000C001, 0xFFFFFFF0)
        for s, (track, layer) in enumerate([(0, 0), (0, 1), (1, 0), (2, 0), (3, 0)]):
            assert eng.api["add_stream"](eng.h, C.byref(abi.lkf_stream_params(
                track=track, layer=layer, ssrc=ssrcs[s]))) == s
        keys = []
        for prof in (srtp_lib.AES_CM, srtp_lib.GCM, srtp_lib.AES_CM, srtp_lib.GCM):
            mk = rng.integers(0, 256, 16, dtype=np.uint8).tobytes()
            ms = rng.integers(0, 256, 12 if prof == srtp_lib.GCM else 14, dtype=np.uint8).tobytes()
            t = eng.api["add_transport"](eng.h, C.byref(pkg.transport_params(mk, ms, prof)))
            assert t == len(keys)
            keys.append((t, mk, ms, prof))
        ref = R.PyUnprotect(5, aes)
        bound = {0: keys[0], 1: keys[1], 3: keys[2], 4: keys[3]}  # stream 2 stays unbound
        for s, k in bound.items():
            eng.set_stream_transport(s, k[0])
            ref.bind(s, k)
        pubs = {s: Pub(aes, s, ssrcs[s], k) for s, k in bound.items()}
        seen = set()
        for c, ar in enumerate(_hand_calls(abi, pubs, pubs[3], pubs[4], 2)):
            assert max(sum(1 for p in ar.pkts if p[0] == s) for s in range(5)) > 64 or c > 0
            call = DeviceCall(ar.raw_pkts(abi), bytes(ar.buf))
            call.unprotect(eng)
            seen |= set(_check_call(abi, eng, call, ref, ar.pkts, bytes(ar.buf), "call %d" % c))
            if c == 2:
                assert ref.streams[0].s_l == ref.streams[1].s_l == 65552 + 300 + 13
            if c == 0:  # the forged packet far ahead did not move s_l; the forged copy did not block the valid one
                assert ref.streams[0].s_l == ref.streams[1].s_l == 65548
                assert ref.streams[3].accepted == 150 and ref.streams[3].auth_failures == 1
        assert seen == {R.OK, R.MALFORMED, R.REPLAY_OLD, R.REPLAY_DUP, R.AUTH}
        # rebinding resets the receive state; unbinding passes through
        eng.set_stream_transport(0, keys[0][0])
        ref.bind(0, keys[0])
        eng.set_stream_transport(1, -1)
        ref.bind(1, None)
        ar = R.Arena()
        ar.add(0, pubs[0].seal(7))
        ar.add(1, pubs[1].seal(7))
        call = DeviceCall(ar.raw_pkts(abi), bytes(ar.buf))
        call.unprotect(eng)
        assert _check_call(abi, eng, call, ref, ar.pkts, bytes(ar.buf), "rebind") == [R.OK, R.OK]
        assert eng.stream_srtp(0)[:5] == (7, 1, 1, keys[0][0], 1) and eng.stream_srtp(1)[3] == -1
    finally:
        eng.close()


# ---- composition with ingest and run -------------------------------------------------
class Composed:
    """A trace, its keys and its protected batches (clean and corrupted), with
    the restatement's verdict per batch of the corrupted one."""

    def __init__(self, workload, abi, shape):
        cfg, kw = R.CLEAN_SHAPES[shape]
        self.tr = workload.Trace(cfg, **kw)
        self.keys = R.trace_keys(self.tr, R.KEY_SEED)
        self.clean = R.ProtectedTrace(self.tr, abi, self.keys)
        self.dirty = R.ProtectedTrace(self.tr, abi, self.keys, **R.REJECT_MIX)
        ref = self.restatement()
        self.dirty_res = [ref.unprotect(b["pkts"], b["srtp"])[0] for b in self.dirty.batches]

    def restatement(self):
        ref = R.PyUnprotect(self.tr.nstreams, self.clean.aes)
        for s, k in self.keys.items():
            ref.bind(s, k)
        return ref

    def engine(self, pkg, workload, bind):
        eng = pkg.Engine.for_trace(self.tr, headroom=2.0)
        workload.load_topology(eng.api, eng.h, self.tr)
        workload.load_streams(eng.api, eng.h, self.tr)
        if bind:
            for k in R.transports_in_order(self.keys):
                assert eng.api["add_transport"](eng.h, C.byref(pkg.transport_params(k[1], k[2], k[3]))) == k[0]
            for s, k in self.keys.items():
                eng.set_stream_transport(s, k[0])
        return eng


@pytest.fixture(scope="module", params=range(len(R.CLEAN_SHAPES)), ids=["config1", "config2"])
def composed(request, workload, abi):
    c = Composed(workload, abi, request.param)
    yield c
    c.tr.close()


def _ingested(eng, abi):
    n = C.c_uint32()
    assert eng.api["ingested"](eng.h, None, 0, C.byref(n)) in (0, -28)
    buf = (abi.lkf_pkt * max(1, n.value))()
    assert eng.api["ingested"](eng.h, buf, n.value, C.byref(n)) == 0
    return bytes(buf)[:n.value * C.sizeof(abi.lkf_pkt)]


def _after_run(eng, abi):
    eng.run()
    eng.sync()
    rec, arena = eng.drain()
    return eng.flows().tobytes(), _ingested(eng, abi), eng.stats(), rec.tobytes(), arena.tobytes()


def _ingest_plain(eng, b, lens=None):
    praws = b["praws"].copy()
    if lens is not None:
        praws["len"] = lens
    arena = np.frombuffer(b["plain"], dtype=np.uint8)
    eng.ingest(_ptr(praws), len(praws), _ptr(arena), len(arena))


def _compose(pkg, workload, abi, c, pt, expect_res):
    """unprotect -> ingest -> run on one engine against plaintext ingest -> run on another."""
    a, b = c.engine(pkg, workload, True), c.engine(pkg, workload, False)
    try:
        n = rej = fwd = 0
        for i, bt in enumerate(pt.batches):
            call = DeviceCall(bt["raws"], bt["srtp"])
            call.unprotect(a)
            call.ingest(a)
            got = _after_run(a, abi)
            res = a.unprotect_results()
            if expect_res is None:
                assert np.all(res["status"] == R.OK), (i, np.nonzero(res["status"])[0][:5])
                assert np.array_equal(res["len"], bt["praws"]["len"])
                lens = None
            else:
                want = expect_res[i]
                assert [(int(r["index"]), int(r["status"]), int(r["len"])) for r in res] == want, i
                lens = np.array([w[2] for w in want], dtype=np.uint32)
                rej += sum(w[1] != R.OK for w in want)
            _ingest_plain(b, bt, lens)
            want_run = _after_run(b, abi)
            for name, g, w in zip(("flows", "ExtPackets", "stats", "records", "arena"), got, want_run):
                assert g == w, (i, name)
            n += len(res)
            fwd += got[2]["forwarded"]
        assert fwd > 0
        for s in range(c.tr.nstreams):
            assert a.stream_stats(s) == b.stream_stats(s), s
        return n, rej, a
    except BaseException:
        a.close()
        raise
    finally:
        b.close()


def test_clean_trace_composes(pkg, workload, abi, composed):
    n, _, a = _compose(pkg, workload, abi, composed, composed.clean, None)
    try:
        assert n == sum(len(b["pkts"]) for b in composed.clean.batches) > 100
        assert sum(a.stream_srtp(s)[4] for s in range(composed.tr.nstreams)) == n  # every datagram accepted
    finally:
        a.close()


def test_rejects_compose(pkg, workload, abi, composed):
    n, rej, a = _compose(pkg, workload, abi, composed, composed.dirty, composed.dirty_res)
    try:
        assert 0.01 <= rej / n <= 0.05, (rej, n)
        ref = composed.restatement()
        for b in composed.dirty.batches:
            ref.unprotect(b["pkts"], b["srtp"])
        for s in range(composed.tr.nstreams):
            assert a.stream_srtp(s) == ref.streams[s].as_tuple(), s
    finally:
        a.close()


def test_host_form_equals_device_form(pkg, workload, abi, composed):
    a, h = composed.engine(pkg, workload, True), composed.engine(pkg, workload, True)
    try:
        bt = composed.dirty.batches[0]
        call = DeviceCall(bt["raws"], bt["srtp"])
        call.unprotect(a)
        call.ingest(a)
        srtp = np.frombuffer(bt["srtp"], dtype=np.uint8)
        h.ingest_srtp(_ptr(bt["raws"]), len(bt["raws"]), _ptr(srtp), len(srtp))
        assert _after_run(a, abi) == _after_run(h, abi)
        assert np.array_equal(a.unprotect_results(), h.unprotect_results())
        assert len(bt["raws"]) > 0 and a.unprotect_timing_window(1) > 0 and h.unprotect_timing_window(1) > 0
        for s in range(composed.tr.nstreams):
            assert a.stream_srtp(s) == h.stream_srtp(s), s
    finally:
        a.close()
        h.close()
