"""The hand-laid packet shapes of tests/emit_shapes_lib.py through the CPU
oracle alone: every forwarded audio record equals the plain-Python
restatement of the reference's header translation byte for byte, every VP8
record keeps its CSRCs and its bytes after the descriptor, every protected
record equals the OpenSSL composition of tests/srtp_lib.py — and the cases
cover the shapes they were built for, so that the GPU half
(tests/test_emit_shapes_gpu.py), which compares the engine with this oracle
and with the same restatement, cannot pass vacuously.
"""
import pytest

from tests import emit_shapes_lib as sl
from tests import srtp_lib
from tests.hand_lib import Source
from tests.oracle_lib import load as load_oracle


@pytest.fixture(scope="module")
def source(workload, abi):
    return Source(workload, abi)


@pytest.fixture(scope="module")
def oracle_runs(pkg, workload, source):
    """(trace, the oracle's per-batch output, shape classes) per case, computed once."""
    o = load_oracle()
    out = {}
    for name in ("audio", "vp8", "mixed"):
        tr, ops = sl.make_case(source, name)
        run, _, _ = sl.run_oracle(pkg, workload, o, tr, ops)
        tw = sl.Twcc()
        cls = set()
        for b, r in enumerate(run):
            cls |= sl.check_wire(tr, b, r["rec"], r["wire"], tw, "oracle " + name)
        out[name] = (tr, run, cls)
    return out


def _forwarded(tr, run):
    """(records, non-empty packets x DownTracks)"""
    n = sum(len(r["rec"]) for r in run)
    full = sum(1 for b in range(tr.nbatches) for p in tr.pkts(b) if p.payload_len) * tr.ndts
    return n, full


@pytest.mark.parametrize("name", ["audio", "vp8", "mixed"])
def test_oracle_equals_restatement(oracle_runs, name):
    """(check_wire ran in the fixture: a mismatch fails there, naming the byte.)
    No case forwards fewer than 90 % of its non-empty packets, and a
    padding-only packet is never forwarded."""
    tr, run, cls = oracle_runs[name]
    n, full = _forwarded(tr, run)
    print("%s: %d records forwarded of %d, %d shape classes" % (name, n, full, len(cls)))
    assert n >= 0.9 * full, (n, full)
    for b, r in enumerate(run):
        pk = tr.pkts(b)
        assert all(pk[int(i)].payload_len > 0 for i in r["rec"]["pkt"])
        if name != "vp8":  # E0..E3 give extension blocks of 0, 8, 12 and 16 bytes
            for rec in r["rec"]:
                p = pk[int(rec["pkt"])]
                block = sl.EXT_BLOCK[tr.kinds[int(rec["dt"])]]
                assert int(rec["out_len"]) == 12 + 4 * (p.hdr0 & 15) + block + p.payload_len
    if name == "audio":
        assert n == full
        assert sum(1 for b in range(tr.nbatches) for p in tr.pkts(b) if not p.payload_len) >= 4
        for b in range(tr.nbatches):  # the last payload ends the arena (test_device_arena_end relies on it)
            p = tr.pkts(b)[-1]
            assert p.arena_off + p.payload_off + p.payload_len == tr.alens[b]


def test_coverage(oracle_runs):
    """What the cases were built to reach, required of the oracle's output."""
    cls = set().union(*(c for _, _, c in oracle_runs.values()))
    # every source alignment with every clipped-chunk length (and a full chunk, and more)
    missing = [(a, t) for a in range(4) for t in range(1, 18) if not any(c[0] == a and c[4] == t for c in cls)]
    assert not missing, missing
    assert {c[3] for c in cls} == {0, 1}  # the P bit
    # prefix lengths of 12, 16, 20, 24, ... leave 4, 0, 12, 8 payload bytes in the LDS region, a VP8
    # descriptor (the source's are 6 bytes) the numbers between them
    assert {0, 4, 8, 12} <= {c[1] for c in cls} and any(c[1] & 3 for c in cls)
    for name, ccs in (("audio", sl.AUDIO_CCS), ("vp8", sl.VP8_CCS)):
        tr, run, _ = oracle_runs[name]
        seen = set()
        for b, r in enumerate(run):
            pk = tr.pkts(b)
            seen |= {(int(d), pk[int(i)].hdr0 & 15) for d, i in zip(r["rec"]["dt"], r["rec"]["pkt"])}
        assert seen == {(d, cc) for d in range(4) for cc in ccs}, name  # every CC on every one of E0..E3
    # the largest prefix: CC = 15 on E3 with a VP8 descriptor: 12 + 60 + 16 + its length
    tr, run, _ = oracle_runs["vp8"]
    big = 0
    for b, r in enumerate(run):
        pk = tr.pkts(b)
        for rec in r["rec"]:
            p = pk[int(rec["pkt"])]
            if int(rec["dt"]) == 3 and p.hdr0 & 15 == 15:
                pre = int(rec["out_len"]) - sl.tail_len(p)
                assert 12 + 60 + 16 + 1 <= pre <= 12 + 60 + 16 + 6
                big = max(big, pre)
    assert big >= 12 + 60 + 16 + 3, big
    # a wire packet that fits into its 16-byte LDS prefix region, and a VP8 record with no byte after the descriptor
    tr, run, _ = oracle_runs["mixed"]
    assert min(int(x) for r in run for x in r["rec"]["out_len"]) <= 16
    assert any(c[4] == 0 for c in oracle_runs["vp8"][2])


@pytest.mark.parametrize("name", ["audio", "vp8"])
def test_oracle_protect_equals_openssl(pkg, workload, source, name):
    """The same batches protected on the oracle (every second transport
    AEAD_AES_128_GCM, one DownTrack unbound): every record equals the OpenSSL
    composition.  The DownTracks are ordered E1, E0, E2, E3 so that the
    unbound one (the first) is not the one without an extension block."""
    tr, ops = sl.make_case(source, name, kinds=(1, 0, 2, 3))
    bind = lambda api, h: srtp_lib.bind_transports(pkg, api, h, tr, seed=5, gcm_every=2)  # noqa: E731
    run, tmap, _ = sl.run_oracle(pkg, workload, load_oracle(), tr, ops, bind=bind)
    assert sorted(tmap) == [1, 2, 3] and {t[3] for t in tmap.values()} == {srtp_lib.AES_CM, srtp_lib.GCM}
    ck = srtp_lib.Checker(tr, tmap)
    n = 0
    for b, i, r, plain, prot in sl.protected_packets(run, tmap):
        assert prot == ck.expect(r, plain, sl.send_time(b)), (b, i, int(r["dt"]), int(r["ext_sn"]), len(plain))
        n += int(r["dt"]) in tmap
    assert n > 300
