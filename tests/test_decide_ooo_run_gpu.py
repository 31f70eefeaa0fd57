"""Late (reordered) packets settled inside k_decide_dt's runs, against the CPU oracle.

A packet behind the highest SN its stream has reached no longer ends the run
it falls in: the run leaves it out of the in-order chain and settles it as the
per-packet step would at that position (RTPMunger's out-of-order branch, the
VP8 munger's missing-picture lookup, a push into a past sequencer slot), and
hands it back to that step when it cannot (a copy of a forwarded packet, a key
below the RangeMap's open range, a slot a ring away, a switch point).  Either
way the outcome is the oracle's.  These cases put late packets on the lanes
where the indexing changes and next to everything a run decides: gaps, temporal
drops, missing pictures, duplicates, control ops, SN wraps.

Batches are hand-built (tests/hand_lib.Source): one track, two DownTracks, a
20-packet warm-up batch and then at most 200 packets; every case is compared
the way tests/test_parity_gpu.py::run_parity does: records, wire bytes,
counters, Forwarder state, RTPStatsSender, sequencer lookups.  DownTrack 0 of
a video case may sit on temporal layer 0 (the filter then drops the upper
layers' packets in the runs), DownTrack 1 always takes every layer.
"""
import ctypes as C

import pytest

from tests.hand_lib import AUDIO, VIDEO, Source, start_ops
from tests.oracle_lib import load as load_oracle
from tests.test_parity_gpu import run_parity

pytestmark = pytest.mark.gpu

WARM = 20                    # packets of batch 0
KINDS = ["video", "audio"]
# (kind, DownTrack 0 on temporal layer 0)
FILTERS = [pytest.param("video", False, id="video"), pytest.param("video", True, id="video-temporal0"),
           pytest.param("audio", False, id="audio")]


@pytest.fixture(scope="module")
def source(workload, abi):
    return Source(workload, abi)


def one_track(source, kind, low_temporal=False):
    """(track, its packet stream, batch 0's ops).  Video: one simulcast layer's
    packets (the steady-state chunks go through the layer lists)."""
    if kind == "audio":
        return AUDIO, source.stream(AUDIO), []
    abi = source.abi
    ops = start_ops(abi, (0, 1))
    if low_temporal:  # DownTrack 0 down to temporal layer 0: it switches at the first marker
        ops.append((0, abi.LKF_CTL_SET_ALLOCATION, 2, 0, 2, 0, 0))
    return VIDEO, source.stream(VIDEO, 2), ops


def arrange(s, n, moves, lost=(), warm_lost=()):
    """[batch 0, batch 1]: batch 0 is s[:WARM] without `warm_lost`; batch 1 is
    s[WARM:WARM + n] without `lost`, then each (i, pos) of `moves` (ascending
    pos) takes packet s[i] out of its place (or from before the batch) and
    puts it at position pos of batch 1."""
    moved = {i for i, _ in moves}
    b0 = [p for i, p in enumerate(s[:WARM]) if i not in warm_lost and i not in moved]
    b1 = [s[i] for i in range(WARM, WARM + n) if i not in moved and i not in lost]
    for i, pos in sorted(moves, key=lambda m: m[1]):
        assert pos <= len(b1)
        b1.insert(pos, s[i])
    assert len(b1) <= 200
    return [b0, b1]


def check(pkg, workload, abi, source, track, batches, ops0, ops1=(), least=100):
    tr = source.trace([track], 2, batches)
    t = run_parity(pkg, workload, abi, tr, extra_ops={0: list(ops0), 1: list(ops1)})
    assert t["forwarded"] >= least
    return t


def pictures(s, lo, hi):
    """[(first index, count)] of the pictures that lie whole inside s[lo:hi]"""
    out, i = [], lo
    while i < hi and s[i].vp8_picture_id == s[i - 1].vp8_picture_id:
        i += 1
    while i < hi:
        j = i
        while j < hi and s[j].vp8_picture_id == s[i].vp8_picture_id:
            j += 1
        if j < hi:
            out.append((i, j - i))
        i = j
    return out


@pytest.mark.parametrize("kind,low", FILTERS)
@pytest.mark.parametrize("at", [0, 31, 63, 64])
def test_late_packet_at_lane(pkg, workload, abi, source, kind, low, at):
    """A packet lost from batch 0 (video: the gap there recorded its picture as
    missing) arrives in batch 1 at lane 0, 31, 63, or as the next chunk's first."""
    track, s, ops = one_track(source, kind, low)
    check(pkg, workload, abi, source, track, arrange(s, 129, [(9, at)]), ops)


@pytest.mark.parametrize("kind,low", FILTERS)
def test_swaps_inside_runs(pkg, workload, abi, source, kind, low):
    """The generator's own pattern, a packet delayed by 1-3 places (a gap lane,
    then the late packet), several times in one chunk: two swaps back to back,
    one apart, two packets late behind one gap, three late behind one gap, and
    a late packet right at the head of the second chunk."""
    track, s, ops = one_track(source, kind, low)
    w = WARM
    moves = [(w + 10, 11), (w + 12, 14),               # depth 1, then depth 2 right behind it
             (w + 30, 33),                             # depth 3
             (w + 40, 43), (w + 41, 44),               # two late packets behind one gap, adjacent
             (w + 50, 54), (w + 51, 56), (w + 52, 58),  # three, apart
             (w + 62, 64)]                             # across the chunk boundary
    check(pkg, workload, abi, source, track, arrange(s, 150, moves), ops)


@pytest.mark.parametrize("low", [False, True], ids=["all-layers", "temporal0"])
def test_late_pictures_behind_their_gap(pkg, workload, abi, source, low):
    """Whole pictures arrive late, directly behind the gap lane that recorded
    them as missing in the same run: their packets forward with the recorded
    picture-id offset.  A third picture was lost from batch 0 and recorded
    there; a packet out of the middle of a picture misses the map and drops."""
    track, s, ops = one_track(source, "video", low)
    pics = [p for p in pictures(s, WARM + 5, WARM + 120) if p[1] <= 8]
    assert len(pics) >= 2
    (a, na), (b, nb) = pics[0], pics[-1]
    assert b > a + na + 4
    moves = [(a + k, a - WARM + 1 + k) for k in range(na)]    # behind the next picture's first packet
    moves += [(b + k, b - WARM + 2 + k) for k in range(nb)]   # behind its first two
    mid = next(i for i in range(a + na + 6, b - 2)
               if s[i - 1].vp8_picture_id == s[i].vp8_picture_id == s[i + 1].vp8_picture_id)
    moves.append((mid, mid - WARM + 2))
    early = [p for p in pictures(s, 3, WARM - 3) if p[1] <= 8][0]
    moves += [(early[0] + k, 150 + k) for k in range(early[1])]
    check(pkg, workload, abi, source, track, arrange(s, 160, moves), ops)


def test_late_copy_of_a_temporal_drop(pkg, workload, abi, source):
    """DownTrack 0 filters the upper temporal layers: a second copy of a packet
    the filter dropped earlier in the same run lies inside that drop's
    exclusion (a cache miss), for DownTrack 1 it is a copy of a forwarded
    packet.  Also a late packet whose own layer the filter would drop."""
    track, s, ops = one_track(source, "video", True)
    up = [i for i in range(WARM + 10, WARM + 120) if s[i].vp8_tid > 0]
    assert len(up) >= 4
    b0, b1 = arrange(s, 150, [(up[-1], up[-1] - WARM + 3)])   # an upper-layer packet, late
    for i in (up[0], up[len(up) // 2]):                       # copies, four places behind the original
        j = next(k for k, p in enumerate(b1) if p.ext_sn == s[i].ext_sn)
        b1.insert(j + 4, abi.lkf_pkt.from_buffer_copy(s[i]))
    check(pkg, workload, abi, source, track, [b0, b1], ops)


@pytest.mark.parametrize("kind", KINDS)
def test_duplicates(pkg, workload, abi, source, kind):
    """Copies of forwarded packets: right behind the original (a copy of the
    highest SN), a few places behind it in the same run, in the next chunk, and
    of a packet of the batch before."""
    track, s, ops = one_track(source, kind)
    b0, b1 = arrange(s, 150, [])
    for src, pos in ((WARM + 100, 140), (WARM - 3, 90), (WARM + 20, 70), (WARM + 40, 45), (WARM + 10, 11)):
        b1.insert(pos, abi.lkf_pkt.from_buffer_copy(s[src]))
    check(pkg, workload, abi, source, track, [b0, b1], ops)


@pytest.mark.parametrize("kind", KINDS)
def test_older_than_the_open_range_and_the_ring(pkg, workload, abi, source, kind):
    """Packets lost from batch 0 arrive late in batch 1: one after the temporal
    filter's exclusions have closed RangeMap ranges above it (video DownTrack
    0), one after a 2,000-SN jump has put it more than a sequencer ring back."""
    track, s, ops = one_track(source, kind, kind == "video")
    b0, b1 = arrange(s, 150, [(5, 60), (9, 130)])
    for p in b1[100:]:
        if p.ext_sn > s[WARM].ext_sn:
            p.ext_sn += 2000
    check(pkg, workload, abi, source, track, [b0, b1], ops)


@pytest.mark.parametrize("kind,op", [("video", "mute"), ("video", "switch"), ("audio", "mute")])
@pytest.mark.parametrize("where", ["on", "before", "between"])
def test_op_next_to_a_late_packet(pkg, workload, abi, source, kind, op, where):
    """A packet three places late (gap lane at 40, late packet at 43) with a
    mute or a re-allocation to layer 0 of DownTrack 0 landing on it, on the
    packet before it, or between it and the gap it fills; the mute is lifted
    ten packets on.  DownTrack 1 decides the same packets undisturbed."""
    track, s, ops = one_track(source, kind)
    at = {"on": 43, "before": 42, "between": 41}[where]
    if op == "mute":
        ops1 = [(0, abi.LKF_CTL_MUTE, 1, 1, 0, 0, at), (0, abi.LKF_CTL_MUTE, 0, 1, 0, 0, at + 10)]
    else:
        ops1 = [(0, abi.LKF_CTL_SET_ALLOCATION, 0, 2, 0, 0, at)]
    check(pkg, workload, abi, source, track, arrange(s, 150, [(WARM + 40, 43), (WARM + 80, 82)]), ops, ops1)


def test_late_packet_of_another_layer(pkg, workload, abi, source):
    """Three simulcast layers interleaved, both DownTracks on layer 2: late
    packets of layers 0 and 1 are dropped as not selected and change nothing;
    a late layer-2 packet among them is settled as usual."""
    s = source.stream(VIDEO)
    n = 200
    moves = []
    for layer, gap in ((0, 5), (1, 9), (2, 6), (0, 2)):
        i = next(k for k in range(WARM + 20 + 40 * len(moves), WARM + n - 20) if s[k].layer == layer)
        moves.append((i, i - WARM + gap))
    check(pkg, workload, abi, source, VIDEO, arrange(s, n, moves), start_ops(abi, (0, 1)), least=60)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("bits", [16, 32])
def test_late_across_a_wrap(pkg, workload, abi, source, kind, bits):
    """The extended SN crosses 2^16 (the wire SN wraps) or 2^32 inside batch
    1; the packets just below the crossing arrive behind packets above it."""
    track, s, ops = one_track(source, kind)
    for i, p in enumerate(s[:WARM + 150]):
        p.ext_sn = (1 << bits) - WARM - 50 + i
    w = WARM
    assert s[w + 49].ext_sn == (1 << bits) - 1
    moves = [(w + 49, 51), (w + 48, 53), (w + 45, 46), (w + 52, 55)]
    check(pkg, workload, abi, source, track, arrange(s, 150, moves), ops)


def probe_whole_ring(pkg, workload, abi, trace, ops0, back=520):
    """The batches again on a fresh engine and oracle, then the sequencer
    looked up at every SN of the last `back` (more than the 500-slot ring):
    the same slots filled, with the same records."""
    o = load_oracle()
    eng = pkg.Engine.for_trace(trace)
    oh = o.create(500)
    try:
        for api, h in ((eng.api, eng.h), (o.api, oh)):
            workload.load_topology(api, h, trace)
            for (dt, op, a0, a1, a2, a3, at) in ops0:
                assert api["ctl"](h, dt, op, a0, a1, a2, a3, at) == 0
        for b in range(trace.nbatches):
            pk, n, ar, alen = trace.batch(b)
            eng.submit(pk, n, ar, alen, None)
            eng.run()
            eng.sync()
            o.run(oh, pk, n, ar, alen, None)
        now = 1700000000 * 10**9 + int(trace.nbatches * 1.5e9)
        found = 0
        for dt in range(trace.ndts):
            st = abi.lkf_fwd_state()
            eng.api["get_state"](eng.h, dt, C.byref(st))
            for base in range(0, back, 40):
                sns = (C.c_uint16 * 40)(*[(st.ext_last_sn - base - i) & 0xFFFF for i in range(40)])
                gm, om = (abi.lkf_seq_meta * 64)(), (abi.lkf_seq_meta * 64)()
                gn, on = C.c_uint32(), C.c_uint32()
                assert eng.api["seq_lookup"](eng.h, dt, sns, 40, now, gm, C.byref(gn)) == 0
                assert o.api["seq_lookup"](oh, dt, sns, 40, now, om, C.byref(on)) == 0
                assert gn.value == on.value, (dt, base, gn.value, on.value)
                for i in range(gn.value):
                    assert bytes(gm[i]) == bytes(om[i]), (dt, base, i)
                found += gn.value
        return found
    finally:
        eng.close()
        o.destroy(oh)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("jump", [350, 380, 420])
def test_late_a_ring_behind_a_run_with_gaps(pkg, workload, abi, source, kind, jump):
    """Late packets about one sequencer ring (500 slots) behind a run that
    holds gap lanes.  Batch 1 jumps `jump` SNs ahead; batch 2's first chunk
    loses two packets in front of lanes 10 and 32 (gap lanes) and takes four
    packets lost from batch 0 at lanes 20, 25, 40 and 45.  Their slots lie
    i + 411 - jump past the run-start highest slot (i = 3, 5, 7, 9), modulo the
    ring: with 380 inside the run's reach, where they meet a push or an
    invalidated slot of this run that comes after them (lanes 20, 25) or came
    before them (40, 45); with 350 on either side of the run's furthest push
    (66 past the start); with 420 a ring or more behind the start.  Besides
    run_parity's checks the whole ring is looked up on both sides."""
    track, s, ops = one_track(source, kind)
    late = (3, 5, 7, 9)
    b0 = [p for i, p in enumerate(s[:WARM]) if i not in late]
    for p in s[WARM:190]:
        p.ext_sn += jump
    b1 = s[WARM:90]
    b2 = [p for i, p in enumerate(s[90:186]) if i not in (10, 11, 33, 34)]
    for i, pos in zip(late, (20, 25, 40, 45)):
        b2.insert(pos, s[i])
    assert b2[20].ext_sn - b1[-1].ext_sn + 500 == 3 + 411 - jump
    tr = source.trace([track], 2, [b0, b1, b2])
    t = run_parity(pkg, workload, abi, tr, extra_ops={0: list(ops)})
    assert t["forwarded"] >= 2 * 150
    assert probe_whole_ring(pkg, workload, abi, source.trace([track], 2, [b0, b1, b2]), ops) > 2 * 150
