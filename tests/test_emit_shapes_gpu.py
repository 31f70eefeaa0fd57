"""Emit and its siblings (k_emit, k_emit_prelen / k_emit_prefix, k_srtp_protect,
k_rtx) at packet shapes the synthetic generator never makes: CSRCs, the P bit,
payloads of 0 bytes to the MTU at every byte alignment of an arena laid back
to back, one-chunk records beside MTU records, DownTrack boundaries on emit's
64-record groups.  The cases come from tests/emit_shapes_lib.py; each is
compared with the CPU oracle the way run_parity does and, independently of the
oracle, with the plain-Python restatement of the reference's header
translation (tests/test_emit_shapes_cpu.py holds the oracle to the same
restatement and asserts what the cases cover).  A failure names the batch, the
record, its CC and payload length, and the byte.
"""
import numpy as np
import pytest

from tests import emit_shapes_lib as sl
from tests import prefix_lib, srtp_lib
from tests.hand_lib import Source
from tests.oracle_lib import load as load_oracle
from tests.test_parity_gpu import run_parity

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def source(workload, abi):
    return Source(workload, abi)


@pytest.fixture(scope="module")
def oracle_runs(pkg, workload, source):
    """(trace, ops, the oracle's per-batch output) per case, computed once."""
    out = {}
    for name in ("audio", "vp8", "mixed"):
        tr, ops = sl.make_case(source, name)
        out[name] = (tr, ops, sl.run_oracle(pkg, workload, load_oracle(), tr, ops)[0])
    return out


@pytest.mark.parametrize("name", ["audio", "vp8", "mixed"])
def test_wire_shapes(pkg, workload, abi, oracle_runs, name):
    """Records, wire bytes, counters, Forwarder state and sender statistics
    against the oracle; then the engine's drained wire bytes against the
    restatement (audio) / the CSRC and tail check (VP8), with the drain's
    buffers 64 bytes longer than the output and pre-filled: nothing after the
    last wire packet is written."""
    tr, ops, orun = oracle_runs[name]
    t = run_parity(pkg, workload, abi, tr, extra_ops=ops)
    assert t["forwarded"] == sum(len(r["rec"]) for r in orun)
    grun, _, _ = sl.run_engine(pkg, workload, tr, ops)
    tw, cls = sl.Twcc(), set()
    for b, g in enumerate(grun):
        cls |= sl.check_wire(tr, b, g["rec"], g["wire"], tw, "engine " + name)
    print("%s: %d records, %d shape classes compared" % (name, t["forwarded"], len(cls)))
    sl.same_output(abi, grun, orun, name)


def test_device_arena_end(pkg, workload, abi, oracle_runs):
    """The audio batches through lkf_submit_device: the last payload ends at
    arena_len and the device buffer is arena_len + 32 bytes, the documented
    slack; the output equals the host-submit run's (and the oracle's)."""
    tr, ops, orun = oracle_runs["audio"]
    for b in range(tr.nbatches):
        p = tr.pkts(b)[-1]
        assert p.arena_off + p.payload_off + p.payload_len == tr.alens[b]
    host, _, _ = sl.run_engine(pkg, workload, tr, ops)
    dev, _, _ = sl.run_engine(pkg, workload, tr, ops, device=True)
    sl.same_output(abi, dev, host, "device vs host submit")
    sl.same_output(abi, dev, orun, "device submit vs oracle")


@pytest.mark.parametrize("name", ["audio", "vp8", "mixed"])
def test_prefix_egress_shapes(pkg, workload, abi, oracle_runs, name):
    """LKF_EGRESS_PREFIX on the same traces: the lkf_pre records and the
    prefix arena against prefix_lib's derivation from the oracle's wire
    output, and every wire packet rebuilt from prefix ++ input[tail_src :
    tail_src + tail_len] (tail_len 0 included: VP8 records that end with
    their descriptor)."""
    tr, ops, orun = oracle_runs[name]
    grun, _, _ = sl.run_engine(pkg, workload, tr, ops, prefix=True)
    tails = set()
    for b, (g, o) in enumerate(zip(grun, orun)):
        pk, n, ar, alen = tr.batch(b)
        assert g["stats"] == o["stats"], b
        prefix_lib.check_prefix(abi, tr, prefix_lib.pkts_array(pk, n), prefix_lib.arena_array(ar, alen), g["rec"],
                                g["wire"], o["rec"], o["wire"], "%s batch %d" % (name, b))
        tails |= set(int(x) for x in g["rec"]["tail_len"])
    assert name != "vp8" or 0 in tails


def _records_per_dt(rec, ndts):
    return tuple(int((rec["dt"] == d).sum()) for d in range(ndts))


@pytest.mark.parametrize("mode", ["default", "persistent"])
def test_group_boundaries(pkg, workload, abi, source, monkeypatch, mode):
    """DownTrack boundaries against emit's 64-record groups (gFirst, pLo / pHi,
    the short last group): totals of 1, 63, 64, 65, 129 and 8 * 64 + 1 records,
    a DownTrack without records exactly on a group boundary, boundaries at
    record 63 | 64 | 65, one DownTrack over three groups; under the default
    grid and LKF_EMIT_PERSISTENT=1.  The oracle's output must have the shape
    (the mutes cut batch 1 to it), the engine must equal the oracle."""
    if mode == "persistent":
        monkeypatch.setenv("LKF_EMIT_PERSISTENT", "1")
    o = load_oracle()
    for shape in sl.BOUNDARY_SHAPES:
        tr, ops, want = sl.boundary_case(source, shape)
        orun, _, _ = sl.run_oracle(pkg, workload, o, tr, ops)
        assert _records_per_dt(orun[0]["rec"], tr.ndts) == (20,) * tr.ndts, shape
        assert _records_per_dt(orun[1]["rec"], tr.ndts) == want, shape
        t = run_parity(pkg, workload, abi, tr, extra_ops=ops)
        assert t["forwarded"] == 20 * tr.ndts + sum(want), shape


def test_group_boundary_prefix_egress(pkg, workload, abi, source):
    """The 64 | 0 | 64 shape under LKF_EGRESS_PREFIX (k_emit_prelen and
    k_emit_prefix locate their records through the same group index)."""
    tr, ops, want = sl.boundary_case(source, "64_0_64")
    orun, _, _ = sl.run_oracle(pkg, workload, load_oracle(), tr, ops)
    assert _records_per_dt(orun[1]["rec"], tr.ndts) == want
    grun, _, _ = sl.run_engine(pkg, workload, tr, ops, prefix=True)
    for b, (g, o) in enumerate(zip(grun, orun)):
        pk, n, ar, alen = tr.batch(b)
        prefix_lib.check_prefix(abi, tr, prefix_lib.pkts_array(pk, n), prefix_lib.arena_array(ar, alen), g["rec"],
                                g["wire"], o["rec"], o["wire"], "64|0|64 batch %d" % b)


@pytest.mark.parametrize("name", ["audio", "vp8"])
def test_protect_shapes(pkg, workload, abi, source, name):
    """lkf_protect on engine and oracle with transports bound (every second
    one AEAD_AES_128_GCM, the first DownTrack unbound; DownTracks ordered E1,
    E0, E2, E3 so that a header without an extension block is protected):
    every protected record equals the oracle's and the OpenSSL composition.
    k_srtp_protect parses CC and the extension block itself: the protected
    records cover every CC under both profiles and payloads of 1, 15, 16 and
    17 bytes."""
    tr, ops = sl.make_case(source, name, kinds=(1, 0, 2, 3))

    def bind(api, h):
        return srtp_lib.bind_transports(pkg, api, h, tr, seed=5, gcm_every=2)

    orun, tmap, _ = sl.run_oracle(pkg, workload, load_oracle(), tr, ops, bind=bind)
    grun, gmap, _ = sl.run_engine(pkg, workload, tr, ops, bind=bind)
    assert sorted(gmap) == sorted(tmap)
    sl.same_output(abi, grun, orun, name)
    ck = srtp_lib.Checker(tr, tmap)
    seen, n = set(), 0
    for (b, i, r, plain, gp), (_, _, _, _, op) in zip(sl.protected_packets(grun, tmap),
                                                      sl.protected_packets(orun, tmap)):
        d = int(r["dt"])
        p = tr.pkts(b)[int(r["pkt"])]
        what = (b, i, d, p.hdr0 & 15, p.payload_len)
        if gp != op:
            bad = next(k for k in range(len(op)) if gp[k:k + 1] != op[k:k + 1])
            raise AssertionError("protected record differs from the oracle's at byte %d: %s" % (bad, what))
        assert gp == ck.expect(r, plain, sl.send_time(b)), what
        if d in tmap:
            seen.add((tmap[d][3], p.hdr0 & 15, min(sl.tail_len(p), 18)))
            n += 1
    print("%s: %d protected records, %d (profile, CC, payload) classes" % (name, n, len(seen)))
    ccs = sl.AUDIO_CCS if name == "audio" else sl.VP8_CCS
    assert {(prof, cc) for prof, cc, _ in seen} == {(prof, cc) for prof in (srtp_lib.AES_CM, srtp_lib.GCM)
                                                     for cc in ccs}
    assert {t for _, _, t in seen} >= {1, 15, 16, 17}


@pytest.mark.parametrize("name", ["audio", "vp8"])
def test_rtx_shapes(pkg, workload, abi, oracle_runs, name):
    """After the batches, eight forwarded sequence numbers per DownTrack are
    NACKed (every CC of the case) and retransmitted from a source blob laid
    back to back with 1..3 bytes of skew: records and wire bytes equal the
    oracle's; the audio ones equal the restatement with the sequencer's SN /
    TS / marker, where the transport-cc element of E3 carries the number after
    the DownTrack's forwarded packets (k_twcc_stamp steps over the CSRCs)."""
    tr, ops, orun = oracle_runs[name]
    nacks = sl.pick_nacks(abi, tr, orun)
    assert len(nacks) == 8 * tr.ndts
    _, _, (ortx, oout, owire) = sl.run_oracle(pkg, workload, load_oracle(), tr, ops, after=sl.rtx_round(abi, tr, nacks))
    grun, _, (grtx, gout, gwire) = sl.run_engine(pkg, workload, tr, ops, after=sl.rtx_round(abi, tr, nacks))
    assert len(ortx) == len(nacks), (len(ortx), len(nacks))
    for f in ortx.dtype.names:
        assert np.array_equal(grtx[f], ortx[f]), f
    assert len(gout) == len(oout) > 0
    for f in oout.dtype.names:
        assert np.array_equal(gout[f], oout[f]), f
    if not np.array_equal(gwire, owire):
        bad = int(np.nonzero(gwire != owire)[0][0])
        r = int(np.searchsorted(oout["out_off"], bad, side="right") - 1)
        raise AssertionError("rtx wire byte %d differs (record %d, its byte %d)" % (
            bad, r, bad - int(oout["out_off"][r])))
    ccs = {tr.raw[(int(x["layer"]), int(x["source_sn"]))][0] & 15 for x in grtx[gout["pkt"]]}
    assert ccs == set(sl.AUDIO_CCS if name == "audio" else sl.VP8_CCS)
    if name == "audio":
        assert len(gout) == len(nacks)
        assert sl.check_rtx_restated(tr, grun, grtx, gout, gwire) == len(nacks)
    print("%s: %d retransmissions compared" % (name, len(gout)))
