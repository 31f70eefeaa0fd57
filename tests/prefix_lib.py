"""Test-side model of the prefix egress (lkf_set_egress(LKF_EGRESS_PREFIX)).

From the wire output of a run (the oracle's records and wire arena) it derives
what the prefix mode must produce for the same run: the lkf_pre records and
the prefix arena.  The split point of a wire packet is found by parsing its
bytes, not from the engine: 12 + 4 * CC, the RFC 8285 extension block in
either profile, and — on the DownTracks of a VP8 track, for packets carrying
LKF_PKT_VP8 — the VP8 payload descriptor (RFC 7741 X / I / M / L / T / K
bits), which is the part of the payload the VP8 munger rewrites.  No GPU.
"""
import ctypes as C

import numpy as np

LKF_CODEC_VP8 = 2
LKF_PKT_VP8 = 0x02

# the lkf_pkt fields the model reads (64-B records)
_PKT_VIEW = np.dtype({"names": ["arena_off", "payload_off", "payload_len", "hdr0", "flags", "vp8_hdr_size"],
                      "formats": ["<u4", "<u2", "<u2", "u1", "u1", "u1"],
                      "offsets": [24, 36, 38, 40, 44, 47], "itemsize": 64})


def pkts_array(pk, n):
    """A ctypes lkf_pkt pointer / array of n packets as a numpy view."""
    if n == 0:
        return np.zeros(0, dtype=_PKT_VIEW)
    addr = C.cast(pk, C.c_void_p).value
    return np.frombuffer((C.c_uint8 * (64 * n)).from_address(addr), dtype=_PKT_VIEW)


def arena_array(ar, alen):
    if alen == 0:
        return np.zeros(0, dtype=np.uint8)
    return np.frombuffer((C.c_uint8 * alen).from_address(C.cast(ar, C.c_void_p).value), dtype=np.uint8)


def round16(x):
    return (x + 15) & ~np.int64(15)


def _ranges(starts, lens):
    """Concatenation of arange(starts[i], starts[i] + lens[i])."""
    lens = lens.astype(np.int64)
    tot = int(lens.sum())
    first = np.cumsum(lens) - lens
    return np.repeat(starts.astype(np.int64) - first, lens) + np.arange(tot, dtype=np.int64)


def vp8_downtracks(trace):
    """Per DownTrack handle: its track's codec is VP8 (the munged descriptor is engine-made)."""
    return np.array([trace.tracks[trace.downtracks[d].track].codec == LKF_CODEC_VP8 for d in range(trace.ndts)],
                    dtype=bool)


def split_points(trace, pkts, orec, owire):
    """pre_len per wire record, parsed from the wire bytes."""
    n = len(orec)
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    off = orec["out_off"].astype(np.int64)
    olen = orec["out_len"].astype(np.int64)
    last = len(owire) - 1

    def at(i):  # wire byte at record offset i (clipped: masked out where it does not apply)
        return owire[np.minimum(off + i, last)].astype(np.int64)

    b0 = at(0)
    pre = 12 + 4 * (b0 & 15)
    has_ext = (b0 & 0x10) != 0
    words = (at(pre + 2) << 8) | at(pre + 3)
    pre = pre + np.where(has_ext, 4 + 4 * words, 0)
    is_vp8 = vp8_downtracks(trace)[orec["dt"]] & ((pkts["flags"][orec["pkt"]] & LKF_PKT_VP8) != 0)
    d0, d1, d2 = at(pre), at(pre + 1), at(pre + 2)
    x = (d0 & 0x80) != 0
    i_, l_, tk = (d1 & 0x80) != 0, (d1 & 0x40) != 0, (d1 & 0x30) != 0
    m = (d2 & 0x80) != 0
    vlen = 1 + np.where(x, 1 + np.where(i_, 1 + m.astype(np.int64), 0) + l_ + tk, 0)
    pre = pre + np.where(is_vp8, vlen, 0)
    assert (pre <= olen).all()
    return pre


def expected_prefix(trace, pkts, orec, owire):
    """(records PRE_DTYPE, prefix arena) the prefix mode must produce for the run
    whose wire output is (orec, owire)."""
    from importlib import import_module
    abi = import_module("livekit-server_amd.abi")
    n = len(orec)
    pre = np.zeros(n, dtype=abi.PRE_DTYPE)
    if n == 0:
        return pre, np.zeros(0, dtype=np.uint8)
    plen = split_points(trace, pkts, orec, owire)
    rlen = round16(plen)
    poff = np.cumsum(rlen) - rlen
    for f in ("ext_sn", "ext_ts", "dt", "pkt", "out_len", "flags", "layer"):
        pre[f] = orec[f]
    pre["pre_off"] = poff
    pre["pre_len"] = plen
    tail = orec["out_len"].astype(np.int64) - plen
    pre["tail_len"] = tail
    p = pkts[orec["pkt"]]
    # the tail ends where the input packet's payload ends
    pre["tail_src"] = p["arena_off"].astype(np.int64) + p["payload_off"] + p["payload_len"] - tail
    arena = np.zeros(int(rlen.sum()), dtype=np.uint8)
    arena[_ranges(poff, plen)] = owire[_ranges(orec["out_off"], plen)]
    return pre, arena


def wire_layout(out_len):
    """Wire-mode layout: 16-B aligned packets in record order -> (out_off, arena bytes)."""
    r = round16(out_len.astype(np.int64))
    return np.cumsum(r) - r, int(r.sum())


def reassemble(pre, prefix_arena, input_arena):
    """The wire arena (wire-mode layout, zero padding) from prefix records, the
    prefix arena and the batch's input arena."""
    if len(pre) == 0:
        return np.zeros(0, dtype=np.uint8)
    off, total = wire_layout(pre["out_len"])
    wire = np.zeros(total, dtype=np.uint8)
    plen, tlen = pre["pre_len"].astype(np.int64), pre["tail_len"].astype(np.int64)
    wire[_ranges(off, plen)] = prefix_arena[_ranges(pre["pre_off"], plen)]
    wire[_ranges(off + plen, tlen)] = input_arena[_ranges(pre["tail_src"], tlen)]
    return wire


def check_prefix(abi, trace, pkts, inp, grec, garena, orec, owire, what=""):
    """The per-batch checks on a prefix-mode drain (grec, garena) against the
    oracle's wire output (orec, owire) of the same batch: records, prefix arena
    and the reassembled wire.  pkts / inp: the batch's ExtPackets (pkts_array)
    and input arena (arena_array)."""
    erec, earena = expected_prefix(trace, pkts, orec, owire)
    assert len(grec) == len(erec), (what, len(grec), len(erec))
    for f in abi.PRE_DTYPE.names:
        if not np.array_equal(grec[f], erec[f]):
            bad = np.nonzero(grec[f] != erec[f])[0][:5]
            raise AssertionError("%s: lkf_pre field %s differs at %s: engine %s expected %s" % (
                what, f, bad, grec[bad], erec[bad]))
    assert garena.shape == earena.shape, (what, garena.shape, earena.shape)
    if not np.array_equal(garena, earena):
        bad = int(np.nonzero(garena != earena)[0][0])
        r = int(np.searchsorted(erec["pre_off"], bad, side="right") - 1)
        raise AssertionError("%s: prefix arena differs at byte %d (record %d: %s)" % (what, bad, r, erec[r]))
    wire = reassemble(grec, garena, inp)
    assert wire.shape == owire.shape and np.array_equal(wire, owire), "%s: reassembled wire differs" % what
    if len(orec):
        assert np.array_equal(wire_layout(grec["out_len"])[0], orec["out_off"].astype(np.int64)), what
