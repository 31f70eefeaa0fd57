"""Packet shapes the synthetic generator never makes, for the code that builds
what a subscriber receives (test infrastructure; no GPU needed to import).

The generator's packets all start with byte 0x90 (CC = 0, P = 0), lie on
16-byte boundaries of the arena and carry 40 payload bytes or more.  Here the
raw packets are laid down by the test, back to back in an arena of its own:
CSRCs, the P bit (with real padding bytes behind the payload), with or without
an input extension block, payloads from 0 bytes to the MTU, at every byte
alignment.  Three things are built on that:

- the cases (`audio_case`, `vp8_case`, `mixed_case`, `boundary_case`): a
  ShapeTrace (what run_parity reads of a trace) plus the ops that start it;
- `restate`: the wire bytes of one forwarded audio record in plain Python, from
  DownTrack.getTranslatedRTPHeader (downtrack.go:1714-1726), pion's
  Header.MarshalTo (one-byte profile) and the pacer's extension order
  (pacer/base.go:71-100: playout delay, abs-send-time placeholder; then the
  TWCC interceptor's transport-cc element).  `check_vp8` checks of a VP8
  record what needs no descriptor model.  Neither shares code with the oracle;
- `classes`: which shape classes a list of forwarded records covers, so that
  a test can require its coverage instead of assuming it.
"""
import ctypes as C
import importlib

import numpy as np

from tests.hand_lib import AUDIO, T0, VIDEO, HandTrace, start_ops

LKF_PKT_VP8 = 0x02
LKF_OUT_MARKER = 0x08
EPOCH = 1700000000 * 10**9

# payload lengths of the audio case: around every multiple of 16 up to 64 (the
# copy loop's chunk), 1..17 complete (keep_bytes clips a last chunk of 1..15
# bytes; every tail length must meet every source alignment), 255..257, and
# around the MTU
AUDIO_LENS = tuple(range(1, 18)) + (19, 20, 21, 31, 32, 33, 47, 48, 49, 63, 64, 65, 255, 256, 257, 1199, 1200,
                                    1201, 1400)
AUDIO_CCS = (0, 1, 2, 15)
VP8_CCS = (0, 3, 15)
VP8_TAILS = (0, 1, 2, 3, 4, 15, 16, 17, None)  # payload bytes kept after the descriptor (None: all of them)
E_KINDS = (0, 1, 2, 3)  # E0: no extension, E1: abs-send-time, E2: + playout delay, E3: + transport-cc
EXT_BLOCK = {0: 0, 1: 8, 2: 12, 3: 16}  # bytes of the one-byte-profile block
PLAYOUT = (0x01, 0x40, 0x64)
IN_EXT = bytes([0xBE, 0xDE, 0x00, 0x01, 0x10, 0x55, 0x00, 0x00])  # an input block: audio level (id 1), 2 pad bytes


class Arena:
    """One batch's raw packets, back to back."""

    def __init__(self):
        self.buf = bytearray()
        self.raw = []  # (start, end) of every packet laid, padding included

    def __len__(self):
        return len(self.buf)


def lay(arena, tmpl, raw_bytes, cc, pbit, xbit, payload, skew):
    """Appends one raw RTP packet to `arena` and returns its lkf_pkt.

    `tmpl` gives every field the shape does not set (ext_sn / ext_ts / flags /
    layer / descriptor fields / PT / SSRC) and `raw_bytes` is the arena its
    arena_off points into (the fixed header's bytes 1 and 8..11 come from
    there).  `skew` (0..3) filler bytes go in front; nothing is rounded to 16.
    cc CSRCs of recognisable bytes (every byte of a CSRC differs from its
    neighbours'), the P bit with real padding behind the payload (1..4 bytes,
    the last one their count, as pion's Unmarshal expects), an 8-byte input
    extension block under the X bit (it only moves payload_off)."""
    assert 0 <= skew <= 3 and 0 <= cc <= 15
    n = len(arena.raw)
    arena.buf += bytes([0xF0 | skew] * skew)
    start = len(arena.buf)
    b0 = 0x80 | (0x20 if pbit else 0) | (0x10 if xbit else 0) | cc
    hdr = bytearray(raw_bytes[tmpl.arena_off:tmpl.arena_off + 12])
    hdr[0] = b0
    hdr[2:4] = (tmpl.ext_sn & 0xFFFF).to_bytes(2, "big")
    hdr[4:8] = (tmpl.ext_ts & 0xFFFFFFFF).to_bytes(4, "big")
    arena.buf += hdr
    for i in range(cc):
        arena.buf += bytes([0xC0 | i, n & 0xFF, 0x80 | ((n >> 8) & 0x7F), 0x5A ^ (3 * i)])
    if xbit:
        arena.buf += IN_EXT
    arena.buf += payload
    if pbit:
        k = 1 + n % 4
        arena.buf += bytes(k - 1) + bytes([k])
    arena.raw.append((start, len(arena.buf)))
    p = type(tmpl).from_buffer_copy(tmpl)
    p.arena_off = start
    p.hdr0 = b0
    p.payload_off = 12 + 4 * cc + (len(IN_EXT) if xbit else 0)
    p.payload_len = len(payload)
    return p


def lay_at(arena, align, *a, **kw):
    """lay() with the filler chosen so that the packet starts at `align` modulo
    4 (the header, the CSRCs and the input block are multiples of 4, so that
    is the payload's alignment as well)."""
    kw["skew"] = (align - len(arena.buf)) & 3
    return lay(arena, *a, **kw)


class ShapeTrace(HandTrace):
    """A HandTrace whose batches each have an arena of their own, exactly as
    long as their packets (the last packet ends at arena_len)."""

    def __init__(self, abi, src, track, kinds, batches, arenas):
        self.arenas = [C.create_string_buffer(bytes(a.buf), max(1, len(a.buf))) for a in arenas]
        self.alens = [len(a.buf) for a in arenas]
        big = max(self.arenas, key=len)
        super().__init__(abi, src, [track], len(kinds), batches, big)
        self.kinds = tuple(kinds)
        for d, k in enumerate(kinds):
            set_extensions(self.downtracks[d], k)
        self.raw = {}  # (layer, sn16) -> the raw packet (what Receiver.ReadRTP returns for an RTX)
        for b, (pk, a) in enumerate(zip(batches, arenas)):
            for p, (s, e) in zip(pk, a.raw):
                assert p.arena_off == s
                self.raw[(int(p.layer), int(p.ext_sn) & 0xFFFF)] = bytes(a.buf[s:e])

    def batch(self, b):
        arr, n = self.batches[b]
        return arr, n, C.cast(self.arenas[b], C.POINTER(C.c_uint8)), self.alens[b]

    def arena_bytes(self, b):
        return self.arenas[b].raw[:self.alens[b]]

    def pkts(self, b):
        arr, n = self.batches[b]
        return [arr[i] for i in range(n)]


def set_extensions(dtp, kind):
    """The DownTrack's extension ids for E0..E3: an id the source trace set is
    kept where the kind has that extension, the others take the lowest free
    ids; an extension the kind lacks is cleared."""
    want = {"ext_abs_send_time": kind >= 1, "ext_playout": kind >= 2, "ext_transport_cc": kind >= 3}
    used = {int(dtp.ext_dd)} | {int(getattr(dtp, f)) for f, w in want.items() if w}
    for f, w in want.items():
        if not w:
            setattr(dtp, f, 0)
        elif not getattr(dtp, f):
            setattr(dtp, f, next(i for i in range(1, 15) if i not in used))
            used.add(int(getattr(dtp, f)))
    for i in range(3):
        dtp.playout_delay[i] = PLAYOUT[i] if kind >= 2 else 0
    assert len({i for i in (dtp.ext_abs_send_time, dtp.ext_playout, dtp.ext_transport_cc) if i}) == max(0, kind)


def _stamp(batches):
    for b, pk in enumerate(batches):  # arrival: the batch's order, 100 us apart (as Source.trace)
        for i, p in enumerate(pk):
            p.arrival_ns = T0 + b * 10**9 + i * 100000


def _audio_tmpl(source, i):
    """Template i of a loss-free, in-order audio stream of any length: the
    source stream's first SN / TS continued in 20 ms steps."""
    if not hasattr(source, "_audio"):
        source._audio = source.stream(AUDIO)
    s = source._audio
    t = type(s[0]).from_buffer_copy(s[i % len(s)])
    t.ext_sn = s[0].ext_sn + i
    t.ext_ts = s[0].ext_ts + 960 * i
    return t


def _payload(rng, n):
    return rng.integers(1, 256, n, dtype=np.uint8).tobytes()


def audio_case(source, kinds=E_KINDS):
    """Every length of AUDIO_LENS at every alignment with every CC of
    AUDIO_CCS (P = 1 on every fifth packet, X = 0 on every third), over two
    batches, with padding-only packets (payload_len 0) between them; each
    batch's last packet has no padding, so its payload ends the arena."""
    raw = source.arena.raw
    rng = np.random.default_rng(11)
    shapes = [(ln, al, cc) for ln in AUDIO_LENS for al in range(4) for cc in AUDIO_CCS]
    half = len(shapes) // 2
    batches, arenas, i = [], [], 0
    for part in (shapes[:half], shapes[half:]):
        a, pk = Arena(), []
        for k, (ln, al, cc) in enumerate(part):
            last = k == len(part) - 1
            if k % 97 == 50:  # padding only: dropped, and the neighbours' offsets stay right
                pk.append(lay_at(a, (al + 1) & 3, _audio_tmpl(source, i), raw, cc, True, True, b""))
                i += 1
            pk.append(lay_at(a, al, _audio_tmpl(source, i), raw, cc, i % 5 == 4 and not last, i % 3 != 2,
                             _payload(rng, ln)))
            i += 1
        batches.append(pk)
        arenas.append(a)
    _stamp(batches)
    return ShapeTrace(source.abi, source.tr, AUDIO, kinds, batches, arenas), {}


def mixed_case(source):
    """Forty 1..4-byte payloads, five of 1400 bytes, nineteen of 1..4 bytes,
    twice, on one E0 DownTrack: 128 records in two groups, one-chunk records
    (the whole wire packet inside its LDS prefix region) beside MTU records
    in the same copy windows, and records across the window edges."""
    raw = source.arena.raw
    rng = np.random.default_rng(12)
    a, pk = Arena(), []
    lens = ([1 + k % 4 for k in range(40)] + [1400] * 5 + [1 + k % 4 for k in range(19)]) * 2
    for i, ln in enumerate(lens):
        pk.append(lay_at(a, (i // 4) & 3, _audio_tmpl(source, i), raw, 0, False, False, _payload(rng, ln)))
    _stamp([pk])
    return ShapeTrace(source.abi, source.tr, AUDIO, (0,), [pk], [a]), {}


def vp8_case(source, kinds=E_KINDS, npkts=216):
    """The source trace's layer-2 packets (real descriptors, flags and
    descriptor fields kept) re-laid with the CCs of VP8_CCS, the payload cut
    to the descriptor plus VP8_TAILS bytes, at every alignment of the first
    byte after the descriptor."""
    raw = source.arena.raw
    s = source.stream(VIDEO, 2)[:npkts]
    assert len(s) == npkts and all(p.flags & LKF_PKT_VP8 for p in s)
    half = npkts // 2
    batches, arenas = [], []
    for lo, hi in ((0, half), (half, npkts)):
        a, pk = Arena(), []
        for i in range(lo, hi):
            t = s[i]
            cc, keep, al = VP8_CCS[i % 3], VP8_TAILS[(i // 3) % 9], (i // 27) & 3
            pay = raw[t.arena_off + t.payload_off:t.arena_off + t.payload_off + t.payload_len]
            if keep is not None and t.vp8_hdr_size + keep < len(pay):
                pay = pay[:t.vp8_hdr_size + keep]
            # `al` is the alignment of the byte after the descriptor, the copy's source
            pk.append(lay_at(a, (al - t.vp8_hdr_size) & 3, t, raw, cc, i % 5 == 4 and i != hi - 1, i % 4 != 3, pay))
        batches.append(pk)
        arenas.append(a)
    _stamp(batches)
    tr = ShapeTrace(source.abi, source.tr, VIDEO, kinds, batches, arenas)
    return tr, {0: start_ops(source.abi, range(len(kinds)))}


def make_case(source, name, kinds=E_KINDS):
    """(trace, ops) of the case `name`: audio, vp8 or mixed."""
    if name == "audio":
        return audio_case(source, kinds)
    if name == "vp8":
        return vp8_case(source, kinds)
    return mixed_case(source)


# ---- emit's group bookkeeping: 64 records per group, DownTrack-major -----------------------------------------------
# (DownTracks, packets of the batch, {DownTrack: muted from this packet on}) -> records per DownTrack
BOUNDARY_SHAPES = {
    "total1": (2, 1, {1: 0}, (1, 0)),
    "total63": (2, 40, {1: 23}, (40, 23)),
    "total64": (2, 40, {1: 24}, (40, 24)),
    "total65": (2, 40, {1: 25}, (40, 25)),
    "total129": (2, 100, {1: 29}, (100, 29)),
    "total513": (2, 300, {1: 213}, (300, 213)),   # 8 * 64 + 1
    "64_0_64": (3, 64, {1: 0}, (64, 0, 64)),      # a DownTrack without records exactly on the group boundary
    "63_0_66": (3, 66, {0: 63, 1: 0}, (63, 0, 66)),  # DownTrack boundaries at records 63 | 63 | 129
    "130_0": (2, 130, {1: 0}, (130, 0)),          # one DownTrack over three groups
    "0_130": (2, 130, {0: 0}, (0, 130)),
}


def boundary_case(source, shape):
    """One audio track, 20-byte payloads: batch 0 (20 packets) starts the
    DownTracks (E0, E1, E3), batch 1 is cut by mute ops to `shape`'s records
    per DownTrack.  Returns (trace, ops, records per DownTrack in batch 1)."""
    ndts, n, mutes, want = BOUNDARY_SHAPES[shape]
    raw = source.arena.raw
    abi = source.abi
    rng = np.random.default_rng(13)
    batches, arenas, i = [], [], 0
    for cnt in (20, n):
        a, pk = Arena(), []
        for _ in range(cnt):
            pk.append(lay_at(a, i & 3, _audio_tmpl(source, i), raw, 0, False, True, _payload(rng, 20)))
            i += 1
        batches.append(pk)
        arenas.append(a)
    _stamp(batches)
    ops = {1: [(d, abi.LKF_CTL_MUTE, 1, 1, 0, 0, at) for d, at in sorted(mutes.items())]}
    return ShapeTrace(abi, source.tr, AUDIO, (0, 1, 3)[:ndts], batches, arenas), ops, want


# ---- the restatement -----------------------------------------------------------------------------------------------
def restate(dtp, pkt, rec, raw, twcc_seq, playout=True):
    """The wire bytes of one forwarded audio record: `dtp` the DownTrack's
    lkf_downtrack_params, `pkt` the input lkf_pkt, `rec` the output record
    (ext_sn, ext_ts, flags), `raw` the batch's input arena, `twcc_seq` the
    transport-wide sequence number of this packet.  playout=False: a
    retransmission (downtrack.go:1640-1698 hands the pacer no playout delay)."""
    cc = pkt.hdr0 & 0x0F
    elems = []
    if playout and dtp.ext_playout:
        elems.append((dtp.ext_playout, bytes(dtp.playout_delay)))
    if dtp.ext_abs_send_time:
        elems.append((dtp.ext_abs_send_time, bytes(3)))
    if dtp.ext_transport_cc:
        elems.append((dtp.ext_transport_cc, (twcc_seq & 0xFFFF).to_bytes(2, "big")))
    out = bytearray()
    out.append((pkt.hdr0 & 0xE0) | (0x10 if elems else 0) | cc)  # V and P of the input, X by the new block
    out.append((0x80 if int(rec["flags"]) & LKF_OUT_MARKER else 0) | (dtp.payload_type & 0x7F))
    out += (int(rec["ext_sn"]) & 0xFFFF).to_bytes(2, "big")
    out += (int(rec["ext_ts"]) & 0xFFFFFFFF).to_bytes(4, "big")
    out += int(dtp.ssrc).to_bytes(4, "big")
    out += raw[pkt.arena_off + 12:pkt.arena_off + 12 + 4 * cc]
    if elems:
        body = b"".join(bytes([(i << 4) | (len(v) - 1)]) + v for i, v in elems)
        body += bytes(-len(body) % 4)
        out += b"\xBE\xDE" + (len(body) // 4).to_bytes(2, "big") + body
    out += raw[pkt.arena_off + pkt.payload_off:pkt.arena_off + pkt.payload_off + pkt.payload_len]
    return bytes(out)


def check_vp8(dtp, pkt, rec, raw, wire, what=""):
    """What a VP8 record must satisfy whatever its munged descriptor is: byte
    0, the SSRC, the CSRCs, and the input's bytes after the descriptor at the
    end of the wire packet."""
    cc = pkt.hdr0 & 0x0F
    has_ext = bool(dtp.ext_playout or dtp.ext_abs_send_time or dtp.ext_transport_cc)
    assert wire[0] == (pkt.hdr0 & 0xE0) | (0x10 if has_ext else 0) | cc, (what, "byte 0")
    assert wire[8:12] == int(dtp.ssrc).to_bytes(4, "big"), (what, "ssrc")
    assert wire[12:12 + 4 * cc] == raw[pkt.arena_off + 12:pkt.arena_off + 12 + 4 * cc], (what, "csrc")
    k = pkt.payload_len - pkt.vp8_hdr_size
    end = pkt.arena_off + pkt.payload_off + pkt.payload_len
    assert k >= 0 and wire[len(wire) - k:] == raw[end - k:end], (what, "tail")


def tail_len(pkt):
    return pkt.payload_len - (pkt.vp8_hdr_size if pkt.flags & LKF_PKT_VP8 else 0)


def shape_class(rec, pkt):
    t = tail_len(pkt)
    src = pkt.arena_off + pkt.payload_off + pkt.payload_len - t
    return (src & 3, (int(rec["out_len"]) - t) & 15, pkt.hdr0 & 0x0F, (pkt.hdr0 >> 5) & 1, min(t, 17))


def classes(records, pkts):
    """The shape classes a list of forwarded records covers: (source
    alignment, prefix length mod 16, CC, P, min(tail length, 17))."""
    return {shape_class(r, pkts[int(r["pkt"])]) for r in records}


class Twcc:
    """The transport-wide sequence numbers in send (record) order: one counter
    per transport, or per DownTrack where none is bound."""

    def __init__(self, tmap=None):
        self.tmap, self.next = tmap or {}, {}

    def take(self, dt):
        k = ("t", self.tmap[dt][0]) if dt in self.tmap else ("d", dt)
        v = self.next.get(k, 0)
        self.next[k] = v + 1
        return v


def check_wire(trace, b, rec, wire, twcc, what=""):
    """Every record of batch b's drain (rec, wire) against restate / check_vp8.
    Returns the shape classes covered."""
    raw = trace.arena_bytes(b)
    pkts = trace.pkts(b)
    for i, r in enumerate(rec):
        d = int(r["dt"])
        dtp, p = trace.downtracks[d], pkts[int(r["pkt"])]
        w = bytes(wire[int(r["out_off"]):int(r["out_off"]) + int(r["out_len"])])
        seq = twcc.take(d) if dtp.ext_transport_cc else 0
        if p.flags & LKF_PKT_VP8:
            check_vp8(dtp, p, r, raw, w, (what, b, i))
        else:
            exp = restate(dtp, p, r, raw, seq)
            if w != exp:
                bad = next((k for k in range(min(len(w), len(exp))) if w[k] != exp[k]), min(len(w), len(exp)))
                raise AssertionError("%s batch %d record %d (dt %d pkt %d cc %d len %d): byte %d of %d/%d is %s, "
                                     "restated %s" % (what, b, i, d, int(r["pkt"]), p.hdr0 & 15, p.payload_len, bad,
                                                      len(w), len(exp), w[bad:bad + 1].hex(), exp[bad:bad + 1].hex()))
    return classes(rec, pkts)


# ---- runners -------------------------------------------------------------------------------------------------------
def _queue(api, h, ops, b):
    for (dt, op, a0, a1, a2, a3, at) in (ops or {}).get(b, ()):
        assert api["ctl"](h, dt, op, a0, a1, a2, a3, at) == 0


def send_time(b):
    return EPOCH + b * 10**9 + 987654321


def run_oracle(pkg, workload, o, trace, ops=None, bind=None, after=None):
    """The trace through the oracle alone -> per batch dict(rec, wire, stats,
    prot).  `bind(api, h)` binds transports (the batches are then protected at
    send_time(b)) and returns their map; `after(api, h)` runs before the
    engine is destroyed and its result is returned as well."""
    h = o.create(500)
    try:
        workload.load_topology(o.api, h, trace)
        tmap = bind(o.api, h) if bind else None
        out = []
        for b in range(trace.nbatches):
            _queue(o.api, h, ops, b)
            pk, n, ar, alen = trace.batch(b)
            o.run(h, pk, n, ar, alen)
            st = pkg.abi.lkf_stats()
            o.api["get_stats"](h, C.byref(st))
            if bind:
                assert o.api["protect"](h, send_time(b)) == 0
            rec, wire = pkg.drain_arrays(o.api, h)
            out.append(dict(rec=rec, wire=wire, stats=st.as_dict(),
                            prot=pkg.drain_protected(o.api, h) if bind else None))
        return out, tmap, (after(o.api, h) if after else None)
    finally:
        o.destroy(h)


def drain_filled(eng, fill=0xEE, slack=64):
    """lkf_drain into buffers `slack` bytes (and one record) larger than the
    run's output, pre-filled: the drain must leave the slack untouched."""
    abi = importlib.import_module("livekit-server_amd.abi")
    n, alen = C.c_uint64(), C.c_uint64()
    rc = eng.api["drain"](eng.h, None, 0, None, 0, C.byref(n), C.byref(alen))
    assert rc in (0, -28), rc
    recs = np.zeros(n.value + 1, dtype=abi.OUT_DTYPE)
    recs.view(np.uint8)[:] = fill
    arena = np.full(alen.value + slack, fill, dtype=np.uint8)
    rc = eng.api["drain"](eng.h, recs.ctypes.data, len(recs), arena.ctypes.data, len(arena), C.byref(n), C.byref(alen))
    assert rc == 0, rc
    assert (arena[alen.value:] == fill).all(), "drain wrote past the run's wire bytes"
    assert (recs[n.value:].view(np.uint8) == fill).all(), "drain wrote past the run's records"
    return recs[:n.value], arena[:alen.value]


def run_engine(pkg, workload, trace, ops=None, bind=None, prefix=False, device=False, after=None):
    """The trace through the engine alone -> per batch dict(rec, wire, stats,
    prot) (prefix=True: the lkf_pre records and the prefix arena of
    LKF_EGRESS_PREFIX).  device=True: lkf_submit_device from device buffers
    of exactly arena_len + 32 bytes (the documented slack)."""
    eng = pkg.Engine.for_trace(trace)
    try:
        workload.load_topology(eng.api, eng.h, trace)
        tmap = bind(eng.api, eng.h) if bind else None
        if prefix:
            eng.set_egress(pkg.abi.LKF_EGRESS_PREFIX)
        out = []
        for b in range(trace.nbatches):
            _queue(eng.api, eng.h, ops, b)
            pk, n, ar, alen = trace.batch(b)
            if device:
                import torch
                dpk = torch.frombuffer(bytearray(C.string_at(pk, max(1, n) * 64)), dtype=torch.uint8).to("cuda")
                dar = torch.empty(alen + 32, dtype=torch.uint8, device="cuda")
                dar[:alen] = torch.frombuffer(bytearray(trace.arena_bytes(b)), dtype=torch.uint8).to("cuda")
                dar[alen:] = 0xA5
                torch.cuda.synchronize()
                eng.submit_device(C.c_void_p(dpk.data_ptr()), n, C.c_void_p(dar.data_ptr()), alen)
            else:
                eng.submit(pk, n, ar, alen)
            eng.run()
            if bind:
                assert eng.api["protect"](eng.h, send_time(b)) == 0
            eng.sync()
            st = eng.stats()
            rec, wire = eng.drain_prefix() if prefix else drain_filled(eng)
            out.append(dict(rec=rec, wire=wire, stats=st,
                            prot=pkg.drain_protected(eng.api, eng.h) if bind else None))
        return out, tmap, (after(eng.api, eng.h) if after else None)
    finally:
        eng.close()


def same_output(abi, got, exp, what=""):
    """Two runs' per-batch records, wire bytes and counters are identical."""
    assert len(got) == len(exp)
    for b, (g, e) in enumerate(zip(got, exp)):
        assert g["stats"] == e["stats"], (what, b, g["stats"], e["stats"])
        assert len(g["rec"]) == len(e["rec"]), (what, b)
        for f in abi.OUT_DTYPE.names:
            assert np.array_equal(g["rec"][f], e["rec"][f]), (what, b, f)
        if not np.array_equal(g["wire"], e["wire"]):
            bad = int(np.nonzero(g["wire"][:len(e["wire"])] != e["wire"][:len(g["wire"])])[0][0])
            r = int(np.searchsorted(e["rec"]["out_off"], bad, side="right") - 1)
            raise AssertionError("%s batch %d: wire byte %d differs (record %d, its byte %d: %s)" % (
                what, b, bad, r, bad - int(e["rec"]["out_off"][r]), e["rec"][r]))


def protected_packets(run, tmap):
    """Per batch, per record: (record, plain wire packet, protected packet)."""
    for b, o in enumerate(run):
        for i, r in enumerate(o["rec"]):
            off, ln = int(r["out_off"]), int(r["out_len"])
            d = int(r["dt"])
            grow = (16 if tmap[d][3] == 2 else 10) if d in tmap else 0
            yield b, i, r, bytes(o["wire"][off:off + ln]), bytes(o["prot"][off + 16 * i:off + 16 * i + ln + grow])


# ---- retransmissions -----------------------------------------------------------------------------------------------
def pick_nacks(abi, trace, run, per_dt=8):
    """Per DownTrack, `per_dt` forwarded sequence numbers of the last batch,
    cycling through the CCs its packets carry (grouped by DownTrack)."""
    b = trace.nbatches - 1
    pkts, rec = trace.pkts(b), run[b]["rec"]
    rows = []
    for d in range(trace.ndts):
        by_cc = {}
        for r in rec[rec["dt"] == d]:
            by_cc.setdefault(pkts[int(r["pkt"])].hdr0 & 15, []).append(int(r["ext_sn"]) & 0xFFFF)
        ccs = sorted(by_cc)
        take = [by_cc[ccs[k % len(ccs)]][-1 - 5 * (k // len(ccs))] for k in range(per_dt)]
        rows += [(d, sn, 0) for sn in take]
    return np.array(rows, dtype=abi.NACK_DTYPE)


def rtx_emit_packed(abi, api, h, trace, rtx):
    """lkf_rtx_emit with the source packets laid back to back, 1..3 filler
    bytes in front of each (tests/rtx_lib.py rounds every source to 16)."""
    n = len(rtx)
    src = (abi.lkf_raw_pkt * max(1, n))()
    blob = bytearray()
    for i in range(n):
        raw = trace.raw.get((int(rtx["layer"][i]), int(rtx["source_sn"][i])), b"")
        blob += bytes([0xF7] * (1 + i % 3))
        src[i].off, src[i].len = len(blob), len(raw)
        blob += raw
    blob += bytes(64)  # (the kernels may read whole words past the last source)
    arena = (C.c_uint8 * len(blob)).from_buffer_copy(bytes(blob))
    out = np.zeros(max(1, n), dtype=abi.OUT_DTYPE)
    cap = len(blob) + 320 * n + 64
    wire = np.zeros(cap, dtype=np.uint8)
    k, ol = C.c_uint32(), C.c_uint64()
    rc = api["rtx_emit"](h, rtx.ctypes.data, n, src, arena, len(blob), out.ctypes.data, wire.ctypes.data, cap,
                         C.byref(k), C.byref(ol))
    assert rc == 0, rc
    return out[:k.value], wire[:ol.value]


def rtx_round(abi, trace, nacks):
    """An `after` for run_oracle / run_engine: lkf_rtx_lookup of `nacks` half
    a second after the last batch, then rtx_emit_packed -> (rtx records, out
    records, wire bytes)."""
    from tests import rtx_lib

    def after(api, h):
        rtx = rtx_lib.rtx_lookup(api, h, nacks, EPOCH + trace.nbatches * 10**9 + 500 * 10**6)
        out, wire = rtx_emit_packed(abi, api, h, trace, rtx)
        return rtx, out, wire
    return after


def check_rtx_restated(trace, run, rtx, out, wire):
    """The audio retransmissions against restate with the sequencer's SN / TS
    / marker (no playout delay); on a transport-cc DownTrack the element
    carries the number after the DownTrack's forwarded packets."""
    sent = {d: sum(int((o["rec"]["dt"] == d).sum()) for o in run) for d in range(trace.ndts)}
    src = {}  # (layer, sn16) -> the input lkf_pkt and its batch
    for b in range(trace.nbatches):
        for p in trace.pkts(b):
            src[(int(p.layer), int(p.ext_sn) & 0xFFFF)] = (b, p)
    n = 0
    for r in out:
        x = rtx[int(r["pkt"])]
        d = int(r["dt"])
        b, p = src[(int(x["layer"]), int(x["source_sn"]))]
        fake = dict(flags=LKF_OUT_MARKER if x["marker"] else 0, ext_sn=int(x["target_sn"]), ext_ts=int(x["timestamp"]))
        exp = restate(trace.downtracks[d], p, fake, trace.arena_bytes(b), sent[d], playout=False)
        sent[d] += 1
        w = bytes(wire[int(r["out_off"]):int(r["out_off"]) + int(r["out_len"])])
        assert w == exp, ("rtx", int(r["pkt"]), d, p.hdr0 & 15, p.payload_len, w.hex(), exp.hex())
        n += 1
    return n
