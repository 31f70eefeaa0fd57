"""k_decide_dt's chunk and run structure against the CPU oracle.

The decide wave loads a track's packets 64 at a time (one per lane), decides
the longest covered prefix of lanes together and hands the packet that stops
it to the full per-packet step.  These cases put the events that stop or
reshape a run (a reordered packet, a loss gap, a mute, a layer switch, a 2^32
crossing of the extended SN / TS, a timestamp 2^31 past the batch base) on the
lanes where the indexing changes: lane 0, lane 31, lane 63 and the first
packet of the next chunk.  Batches are hand-built from the packets of a
one-room trace (their VP8 descriptors, payloads and arena stay real); every
case is compared the way tests/test_parity_gpu.py::run_parity does: records,
wire bytes, counters, Forwarder state, RTPStatsSender, sequencer lookups.
"""
import ctypes as C

import numpy as np
import pytest

from tests.hand_lib import AUDIO, VIDEO, Source, start_ops
from tests.oracle_lib import load as load_oracle
from tests.test_parity_gpu import _state_tuple, check_sender_stats, run_parity

pytestmark = pytest.mark.gpu

LANES = [0, 31, 63, 64]      # lane 0, mid-chunk, the chunk's last lane, the next chunk's first


@pytest.fixture(scope="module")
def source(workload, abi):
    return Source(workload, abi)


def one_track(source, kind):
    """(track, its packet stream, the start ops of its two DownTracks)"""
    if kind == "video":  # one simulcast layer's packets: the steady-state chunks (layer lists)
        return VIDEO, source.stream(VIDEO, 2), start_ops(source.abi, (0, 1))
    return AUDIO, source.stream(AUDIO), []


@pytest.mark.parametrize("kind", ["video", "audio"])
def test_chunks_cross_2_32_and_wide(pkg, workload, abi, source, kind):
    """One track, two DownTracks, 130 packets (two full chunks and a partial
    one): the extended SN starts at 2^32 - 40 and crosses inside the first
    chunk, the extended TS crosses 2^32 inside the second, and from packet 100
    on the TS jumps forward by more than 2^31 — those records lie 2^31 or more
    from the batch's base and take the T_WIDE side array.  (The jump is in the
    TS: both sides walk a sequence-number gap slot by slot.)"""
    track, s, ops = one_track(source, kind)
    pk = s[:130]
    ts0 = pk[0].ext_ts
    span70 = pk[70].ext_ts - ts0
    for i, p in enumerate(pk):
        p.ext_sn = (1 << 32) - 40 + i
        p.ext_ts = (1 << 32) - span70 + (p.ext_ts - ts0) + ((1 << 31) + 4321 if i >= 100 else 0)
    assert pk[69].ext_ts < (1 << 32) <= pk[70].ext_ts
    tr = source.trace([track], 2, [pk])
    t = run_parity(pkg, workload, abi, tr, extra_ops={0: ops})
    assert t["forwarded"] >= 2 * 100  # (video: the temporal filter may drop a few)


def reorder_batches(s):
    """Batch 0: 20 packets without three of them; batch 1: 130 packets with
    those three arriving late at lane 0, lane 63 and as the second chunk's
    first packet."""
    late = (5, 9, 13)
    b0 = [p for i, p in enumerate(s[:20]) if i not in late]
    rest = s[20:20 + 127]
    b1 = rest[:]
    for pos, i in zip((0, 63, 64), late):
        b1.insert(pos, s[i])
    assert len(b1) == 130 and [b1[k].ext_sn for k in (0, 63, 64)] == [s[i].ext_sn for i in late]
    return [b0, b1]


def gap_batches(s):
    """Batch 0: 20 packets; batch 1: 130 packets, two lost in front of the
    packets at lane 0, lane 63 and the second chunk's first lane."""
    b1, idx = [], 20
    for pos in range(130):
        if pos in (0, 63, 64):
            idx += 2
        b1.append(s[idx])
        idx += 1
    for k in (0, 63, 64):
        assert b1[k].ext_sn - (b1[k - 1].ext_sn if k else s[19].ext_sn) == 3
    return [s[:20], b1]


@pytest.mark.parametrize("kind", ["video", "audio"])
@pytest.mark.parametrize("shape", [reorder_batches, gap_batches], ids=["reorder", "gap"])
def test_reorder_and_gap_at_chunk_lanes(pkg, workload, abi, source, kind, shape):
    track, s, ops = one_track(source, kind)
    tr = source.trace([track], 2, shape(s))
    t = run_parity(pkg, workload, abi, tr, extra_ops={0: ops})
    assert t["forwarded"] >= 2 * 100


@pytest.mark.parametrize("kind", ["video", "audio"])
@pytest.mark.parametrize("at", LANES)
def test_mute_at_chunk_lanes(pkg, workload, abi, source, kind, at):
    """A mute landing on packet `at` of a 130-packet batch (DownTrack 0; lifted
    64 packets later, so that op lands on the other lanes) while DownTrack 1
    keeps forwarding."""
    track, s, ops = one_track(source, kind)
    tr = source.trace([track], 2, [s[:20], s[20:150]])
    mute = [(0, abi.LKF_CTL_MUTE, 1, 1, 0, 0, at), (0, abi.LKF_CTL_MUTE, 0, 1, 0, 0, at + 64)]
    t = run_parity(pkg, workload, abi, tr, extra_ops={0: ops, 1: mute})
    assert 150 < t["forwarded"] < 2 * 150 - 40


@pytest.mark.parametrize("at", LANES)
def test_layer_switch_at_chunk_lanes(pkg, workload, abi, source, at):
    """Three simulcast layers interleaved, both DownTracks on layer 2; DownTrack
    0 is re-allocated to layer 0 at the head of the batch and the layer-0 key
    frame that lets it switch arrives as packet `at` (while the switch is
    pending the chunks are the track's packets, 64 at a time, so `at` is the
    lane).  DownTrack 1 stays in the steady state and is muted at `at`."""
    s = source.stream(VIDEO)
    # a layer-0 packet that starts a picture, far enough in for `at` packets in front of it
    starts = [i for i in range(200, len(s) - 200)
              if s[i].layer == 0 and s[i].vp8_picture_id != next(p.vp8_picture_id for p in reversed(s[:i]) if p.layer == 0)]
    j = starts[0]
    b0, b1 = s[:j - at], s[j - at:j - at + 200]
    assert b1[at].layer == 0 and b1[at].ext_sn == s[j].ext_sn
    b1[at].flags |= 1  # LKF_PKT_KEYFRAME
    tr = source.trace([VIDEO], 2, [b0, b1])
    ops1 = [(0, abi.LKF_CTL_SET_ALLOCATION, 0, 2, 0, 0, 0), (1, abi.LKF_CTL_MUTE, 1, 1, 0, 0, at)]
    t = run_parity(pkg, workload, abi, tr, extra_ops={0: start_ops(abi, (0, 1)), 1: ops1})
    assert t["forwarded"] > 100


def test_downtrack_with_op_but_no_packet(pkg, workload, abi, source):
    """Batch 1 holds only the audio track's packets while the video DownTracks
    get ops (a mute, a new allocation): their waves run for the ops alone.
    Batch 2 brings the video packets back."""
    v, a = source.stream(VIDEO, 2), source.stream(AUDIO)
    tr = source.trace([VIDEO, AUDIO], 2, [v[:70] + a[:20], a[20:90], v[70:200] + a[90:110]])
    ops1 = [(0, abi.LKF_CTL_MUTE, 1, 1, 0, 0, 0), (1, abi.LKF_CTL_SET_MAX_TEMPORAL, 1, 0, 0, 0, 5)]
    t = run_parity(pkg, workload, abi, tr, extra_ops={0: start_ops(abi, (0, 1)), 1: ops1})
    assert t["forwarded"] > 2 * 110


def test_config2_ingest_four_steps_no_sync(pkg, workload, abi):
    """The configs[1] shape on 2 rooms at loss 0.3 / reorder 0.1 (the generator
    parameters of test_ingress_nack_lane_parallel's heavy case), raw datagrams
    through lkf_ingest and lkf_run for four consecutive steps with no sync
    between them (the three batch contexts reused): cumulative counters, the
    last step's records and wire bytes, every Forwarder's state, every
    RTPStatsSender and every stream's receiver statistics equal the oracle's."""
    tr = workload.Trace(2, duration_s=4.0, batch_s=1.0, rooms=2, loss=0.3, reorder=0.1, seed=7)
    assert tr.nbatches >= 4
    o = load_oracle()
    eng = pkg.Engine.for_trace(tr)
    oh = o.create(500)
    try:
        for api, h in ((eng.api, eng.h), (o.api, oh)):
            workload.load_topology(api, h, tr)
            workload.load_streams(api, h, tr)
        tot = None
        for b in range(4):
            workload.queue_events(eng.api, eng.h, tr, b)
            workload.queue_events(o.api, oh, tr, b)
            rp, n, ar, alen = tr.batch_raw(b)
            eng.ingest(rp, n, ar, alen)
            eng.run()
            assert o.api["ingest"](oh, rp, n, ar, alen) == 0
            m = C.c_uint32()
            assert o.api["ingested"](oh, None, 0, C.byref(m)) in (0, -28)
            ext = (abi.lkf_pkt * max(1, m.value))()
            assert o.api["ingested"](oh, ext, m.value, C.byref(m)) == 0
            o.run(oh, ext if m.value else None, m.value, ar, alen)
            ost = abi.lkf_stats()
            o.api["get_stats"](oh, C.byref(ost))
            d = ost.as_dict()
            if tot is None:
                tot = d
            else:
                for k in ("tuples", "forwarded", "out_bytes", "arena_bytes"):
                    tot[k] += d[k]
                tot["drops"] = [x + y for x, y in zip(tot["drops"], d["drops"])]
        eng.sync()
        assert eng.cumulative() == tot
        assert tot["forwarded"] > 1000
        grec, gar = eng.drain()
        orec, oar = pkg.drain_arrays(o.api, oh)
        assert len(grec) == len(orec)
        for f in abi.OUT_DTYPE.names:
            assert np.array_equal(grec[f], orec[f]), f
        assert np.array_equal(gar, oar)
        for dt in range(tr.ndts):
            assert _state_tuple(eng.api, eng.h, dt, abi) == _state_tuple(o.api, oh, dt, abi), dt
        check_sender_stats(pkg, eng.api, eng.h, o.api, oh, range(tr.ndts))
        for s in range(tr.nstreams):
            assert eng.stream_stats(s) == pkg.stream_stats(o.api, oh, s), s
    finally:
        eng.close()
        o.destroy(oh)
