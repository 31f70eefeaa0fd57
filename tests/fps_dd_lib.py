"""The dependency-descriptor frame-rate calculator restated on plain Python
objects, a small dependency-descriptor writer, and the trace builder of their
tests.

PyFpsDD is written as buffer/fps.go:319-570 is (FrameRateCalculatorDD under
buffer.go:518-543 doFpsCalc): a real sorted list per (spatial, temporal) with
the reference's own insertion loop, frame records with their frame numbers,
and calc() walking list and records.  It knows nothing of the masks, slots and
walk-order rotation of livekit-server_amd/csrc/fps_dd_device.h, so the two
restatements can disagree; state() translates its records into the shape the
engine and the unit program show.  Every frame-number operation is `& 0xffff`,
every timestamp one `& 0xffffffff`, the rate is fps_lib.rate_of.

Two places where the reference panics are restated as the engine has them:
no rate for temporal layer 3 (minFramesForCalculation[3]), and a max layer
beyond (2, 3) never completes (frameRates[3] / [..][4]).

The writer makes the AV1 dependency descriptor (structure with templates,
decode targets and chains; descriptor with a template id, an optional attached
structure, active mask and custom frame diffs) and RTP datagrams that carry it
in a header extension: the one-byte form up to 16 bytes, the two-byte form
beyond.  tests/test_fps_dd_cpu.py reads its output back with the reader of
tests/test_dd_wide_cpu.py.
"""
import struct

from tests.fps_lib import M16, M32, MIN_FRAMES, f32, f32_bits, rate_of

WINDOW = 256  # len(fnReceived)
DD = 3        # LKF_FPS_DD
FLOW_FORWARD = 0x20
FLOW_BUCKET = 0x80


# ---- the calculator, as the Go is --------------------------------------------
class _Frame:
    __slots__ = ("ts", "fn", "spatial", "temporal")

    def __init__(self, ts, fn, spatial=0, temporal=0):
        self.ts, self.fn, self.spatial, self.temporal = ts, fn, spatial, temporal


class PyFpsDD:
    """One Buffer's doFpsCalc over its FrameRateCalculatorDD.  packet() takes
    what reaches RecvPacket with a descriptor: an ExtPacket with a payload."""

    def __init__(self, clock=90000, vp8=False):
        self.clock, self.vp8 = clock, vp8
        self.rates = [[0.0] * 4 for _ in range(3)]
        self.completed = False
        self.calculated = False  # Buffer.frameRateCalculated
        self.max_spatial, self.max_temporal = 2, 3
        self.resets = 0
        self._clear()

    def _clear(self):
        self.first = [[None] * 4 for _ in range(3)]
        self.second = [[None] * 4 for _ in range(3)]
        self.received = [None] * WINDOW
        self.base = None
        self.chains = [[[] for _ in range(4)] for _ in range(3)]  # container/list of uint16

    def set_max_layer(self, spatial, temporal):
        self.max_spatial, self.max_temporal = spatial, temporal

    def packet(self, fn, ts, spatial, temporal, diffs):
        """doFpsCalc -> RecvPacket's result (False once the stream is calculated)."""
        if self.calculated:
            return False
        if self.vp8:
            spatial = -1  # buffer.go:640
        ret = self.recv(fn & M16, ts & M32, spatial, temporal, diffs)
        if ret and self.completed:
            self.calculated = True
        return ret

    def recv(self, fn, ts, spatial, temporal, diffs):
        if self.completed:
            return True
        if spatial < 0:
            spatial = 0
        if temporal < 0 or temporal > 3 or spatial > 2:
            return False
        if self.base is None:
            self.base = _Frame(ts, fn)
            self.received[0] = self.base
            self.first[spatial][temporal] = self.base
            self.second[spatial][temporal] = self.base
            return False
        base_diff = (fn - self.base.fn) & M16
        if base_diff == 0 or base_diff > 0x8000:
            return False
        if base_diff >= WINDOW:
            self._clear()
            self.resets += 1
            return False
        if self.received[base_diff] is not None:
            return False
        fi = _Frame(ts, fn, spatial, temporal)
        self.received[base_diff] = fi
        if self.first[spatial][temporal] is None:
            self.first[spatial][temporal] = fi
            self.second[spatial][temporal] = fi
            return False
        chain = self.chains[spatial][temporal]
        if not chain:
            chain.append(fn)
        for fdiff in diffs:
            depend = (fn - (fdiff & M16)) & M16
            if ((depend - self.second[spatial][temporal].fn) & M16) > 0x8000:
                continue
            e = len(chain) - 1  # chain.Back()
            while e >= 0:
                val = chain[e]
                if val == depend:
                    break
                if val < depend:
                    chain.insert(e + 1, depend)  # InsertAfter
                    break
                if e == 0:
                    chain.insert(0, depend)  # PushFront; e.Prev() is then the new element
                    break
                e -= 1
        return self.calc()

    def calc(self):
        counter = 0
        for s in range(min(self.max_spatial, 2) + 1):
            spatial_counter = 0
            for t in range(min(self.max_temporal, 3) + 1):
                if self.rates[s][t] > 0:
                    counter += 1
                    spatial_counter += 1
                    continue
                first = self.first[s][t]
                if spatial_counter > 0 and first is None:
                    spatial_counter += 1
                    counter += 1
                    continue
                last = None
                for val in self.chains[s][t]:
                    diff = (val - self.base.fn) & M16
                    if diff >= WINDOW:
                        continue
                    fi = self.received[diff]
                    if fi is None:
                        break
                    last = fi
                    if first is None and fi.spatial == s and fi.temporal == t:
                        first = fi
                if last is not None and last.fn > self.second[s][t].fn:
                    self.second[s][t] = last
                else:
                    continue
                if t == 3:  # the reference indexes minFramesForCalculation[3] and panics
                    continue
                count = 0
                i, end = (first.fn - self.base.fn) & M16, (last.fn - self.base.fn) & M16
                while i <= end:
                    fi = self.received[i]
                    if fi is not None and fi.spatial == s and fi.temporal <= t:
                        count += 1
                    i += 1
                if count >= MIN_FRAMES[t] and last.ts > first.ts:
                    self.rates[s][t] = rate_of(self.clock, last.ts, first.ts, count)
                    counter += 1
        if counter == (self.max_spatial + 1) * (self.max_temporal + 1):
            self.completed = True
            self._clear()  # close()
            self.resets += 1
            return True
        return False

    # ---- the state as the engine and the unit program show it
    def _slot(self, f):
        return -1 if f is None else (f.fn - self.base.fn) & M16

    def _words(self, slots):
        m = sum(1 << k for k in slots)
        return tuple((m >> (64 * j)) & ((1 << 64) - 1) for j in range(4))

    def chain_words(self, s, t):
        slots = [(v - self.base.fn) & M16 for v in self.chains[s][t]]
        assert all(k < WINDOW for k in slots), "a chain member outside the window"
        return self._words(slots)

    def dd_state(self):
        """lkf_fps_dd.as_dict()."""
        return {
            "base_fn": self.base.fn if self.base else 0, "has_base": 1 if self.base else 0,
            "completed": 1 if self.completed else 0, "max_spatial": self.max_spatial,
            "max_temporal": self.max_temporal, "resets": self.resets,
            "present": self._words(k for k, f in enumerate(self.received) if f is not None),
            "first": tuple(tuple(self._slot(f) for f in row) for row in self.first),
            "second": tuple(tuple(self._slot(f) for f in row) for row in self.second),
            "chain": tuple(tuple(self.chain_words(s, t) for t in range(4)) for s in range(3))}

    def state(self):
        """lkf_stream_fps.as_dict() of a DD stream."""
        c = 1 if self.completed else 0
        z = (0, (0,) * 4, (0,) * 4, 0, 0, 0)
        return {"kind": DD, "calculated": 1 if self.calculated else 0, "completed": (c, c, c),
                "fps_bits": tuple(tuple(f32_bits(r) for r in row) for row in self.rates), "calc": (z,) * 3}

    def unit_line(self, ret):
        d = self.dd_state()
        flat = lambda rows: " ".join("%d" % v for row in rows for v in row)
        return "%d %d | %d %d %d %d %d %d | %s | %s | %s | %s | %s" % (
            1 if ret else 0, 1 if self.calculated else 0, d["base_fn"], d["has_base"], d["completed"],
            d["max_spatial"], d["max_temporal"], d["resets"], " ".join("%016x" % w for w in d["present"]),
            flat(d["first"]), flat(d["second"]),
            " ".join("%016x" % w for row in d["chain"] for ws in row for w in ws),
            " ".join("%08x" % f32_bits(r) for row in self.rates for r in row))


# ---- the reference test's frame generator (fps_test.go:61-126) ----------------
def create_frames(start_fn, start_ts, total, fps, spatial_dependency):
    """-> per spatial layer a list of [fn, ts, spatial, temporal, diffs]."""
    ns, nt = len(fps), len(fps[0])
    frames = [[] for _ in range(ns)]
    fn = start_fn & M16
    step = [[int(f32(f32(90000.0) / f32(fps[i][j]))) & M32 for j in range(nt)] for i in range(ns)]
    nxt = [[start_ts & M32] * nt for _ in range(ns)]
    cur = [start_ts & M32] * ns
    for _ in range(total):
        for s in range(ns):
            fr = [fn, cur[s], s, 0, []]
            for t in range(nt):
                if cur[s] >= nxt[s][t]:
                    fr[3] = t
                    for u in range(t, nt):
                        nxt[s][u] = (nxt[s][u] + step[s][u]) & M32
                    break
            cur[s] = (cur[s] + step[s][nt - 1]) & M32
            frames[s].append(fr)
            fn = (fn + 1) & M16
            for cf in reversed(frames[s]):
                if ((cf[1] - fr[1]) & M32) > 0x80000000:
                    fr[4].append((fr[0] - cf[0]) & M16)
                    break
            if spatial_dependency and s > 0:
                for cf in reversed(frames[s - 1]):
                    if cf[1] == fr[1]:
                        fr[4].append((fr[0] - cf[0]) & M16)
                        break
    return frames


# ---- the dependency-descriptor writer -----------------------------------------
class BitW:
    def __init__(self):
        self.bits = []

    def put(self, v, n):
        assert 0 <= v < (1 << n) or n == 0
        self.bits += [(v >> (n - 1 - k)) & 1 for k in range(n)]

    def ns(self, v, n):
        if n <= 1:
            return
        w = n.bit_length()
        m = (1 << w) - n
        if v < m:
            self.put(v, w - 1)
        else:
            self.put(v + m, w)

    def bytes(self):
        b = self.bits + [0] * (-len(self.bits) % 8)
        return bytes(sum(b[i + k] << (7 - k) for k in range(8)) for i in range(0, len(b), 8))


NOT_PRESENT, DISCARDABLE, SWITCH, REQUIRED = 0, 1, 2, 3


class Structure:
    """A FrameDependencyStructure: templates [(sid, tid, dtis, fdiffs)] in layer
    order (each dtis one DTI per decode target, fdiffs 1..16 each), optionally
    chains: protected_by per decode target and chain diffs per template."""

    def __init__(self, sid, templates, ndt, protected_by=(), chain_diffs=(), resolutions=()):
        self.id, self.templates, self.ndt = sid, list(templates), ndt
        self.protected_by, self.chain_diffs, self.resolutions = list(protected_by), list(chain_diffs), list(resolutions)
        self.nchains = (max(self.protected_by) + 1) if self.protected_by else 0

    def write(self, w):
        w.put(self.id, 6)
        w.put(self.ndt - 1, 5)
        for k, (sid, tid, _, _) in enumerate(self.templates):
            if k + 1 == len(self.templates):
                idc = 3
            else:
                nsid, ntid = self.templates[k + 1][:2]
                idc = 0 if (nsid, ntid) == (sid, tid) else 1 if (nsid, ntid) == (sid, tid + 1) else 2
                assert idc != 2 or (nsid, ntid) == (sid + 1, 0)
            w.put(idc, 2)
        for _, _, dtis, _ in self.templates:
            assert len(dtis) == self.ndt
            for d in dtis:
                w.put(d, 2)
        for _, _, _, fdiffs in self.templates:
            for f in fdiffs:
                w.put(1, 1)
                w.put(f - 1, 4)
            w.put(0, 1)
        w.ns(self.nchains, self.ndt + 1)
        if self.nchains:
            for p in self.protected_by:
                w.ns(p, self.nchains)
            for row in self.chain_diffs:
                assert len(row) == self.nchains
                for c in row:
                    w.put(c, 4)
        w.put(1 if self.resolutions else 0, 1)
        for wd, ht in self.resolutions:
            w.put(wd - 1, 16)
            w.put(ht - 1, 16)

    def template_id(self, idx):
        return (self.id + idx) % 64

    def layer_of_target(self, target):
        """ProcessFrameDependencyStructure: the maximum sid / tid over the templates that have the target."""
        ls = lt = 0
        for sid, tid, dtis, _ in self.templates:
            if dtis[target] != NOT_PRESENT:
                ls, lt = max(ls, sid), max(lt, tid)
        return ls, lt

    def max_layer(self, mask):
        """What Parse hands onMaxLayerChanged for an active mask."""
        ms = mt = 0
        for target in range(self.ndt):
            if (mask >> target) & 1:
                ls, lt = self.layer_of_target(target)
                ms, mt = max(ms, ls), max(mt, lt)
        return ms, mt


def l1t3_structure(sid=3, diffs=(4, 2, 1)):
    """One spatial, three temporal layers, a decode target per temporal layer;
    templates: key, T0, T1, T2 with one frame diff each (the key frame none)."""
    sw, np_, dc = SWITCH, NOT_PRESENT, DISCARDABLE
    return Structure(sid, [(0, 0, [sw, sw, sw], []), (0, 0, [sw, sw, sw], [diffs[0]]),
                           (0, 1, [np_, dc, sw], [diffs[1]]),
                           (0, 2, [np_, np_, dc], [diffs[2]])], 3)


def l3t3_structure(sid=7):
    """Three spatial by three temporal layers, one decode target per layer
    (target 3 s + t), no chains; template 3 s + t: the frame of the same
    spatial layer one period of its temporal layer back (12, 6 or 3 frames),
    and for s > 0 the frame below it."""
    tm = []
    for s in range(3):
        for t in range(3):
            dtis = [NOT_PRESENT] * 9
            for s2 in range(s, 3):
                for t2 in range(t, 3):
                    dtis[3 * s2 + t2] = REQUIRED if (s2, t2) == (s, t) else SWITCH
            tm.append((s, t, dtis, [(12, 6, 3)[t]] + ([1] if s else [])))
    return Structure(sid, tm, 9)


def descriptor(template_id, fn, first=True, last=True, structure=None, active_mask=None, ndt=None, custom_dtis=None,
               custom_fdiffs=None, fdiff_nibbles=None):
    """One descriptor's bytes.  active_mask needs ndt (the decode targets of the
    structure in force) unless a structure is attached; custom_fdiffs is the
    whole list (1..4096 each), each written in the fewest nibbles or in
    fdiff_nibbles (1..3)."""
    w = BitW()
    w.put(1 if first else 0, 1)
    w.put(1 if last else 0, 1)
    w.put(template_id, 6)
    w.put(fn & M16, 16)
    if structure is None and active_mask is None and custom_dtis is None and custom_fdiffs is None:
        return w.bytes()
    w.put(1 if structure else 0, 1)
    w.put(1 if active_mask is not None else 0, 1)
    w.put(1 if custom_dtis is not None else 0, 1)
    w.put(1 if custom_fdiffs is not None else 0, 1)
    w.put(0, 1)  # no custom chain diffs
    if structure:
        structure.write(w)
        ndt = structure.ndt
    if active_mask is not None:
        w.put(active_mask, ndt)
    if custom_dtis is not None:
        for d in custom_dtis:
            w.put(d, 2)
    if custom_fdiffs is not None:
        for f in custom_fdiffs:
            assert 1 <= f <= 4096
            size = fdiff_nibbles or (1 if f <= 16 else 2 if f <= 256 else 3)
            w.put(size, 2)
            w.put(f - 1, 4 * size)
        w.put(0, 2)
    return w.bytes()


def rtp_ext(ssrc, sn, ts, ext_id, ext, payload, pt=96, marker=0, padding=0):
    """An RTP datagram with one header-extension element (ext None: no
    extension at all): RFC 8285 one-byte form up to 16 bytes, two-byte beyond."""
    h = bytes([0x80 | (0x20 if padding else 0) | (0x10 if ext is not None else 0), (marker << 7) | pt])
    h += struct.pack(">HII", sn & M16, ts & M32, ssrc)
    if ext is not None:
        if len(ext) <= 16:
            profile, el = 0xBEDE, bytes([(ext_id << 4) | (len(ext) - 1)]) + ext
        else:
            profile, el = 0x1000, bytes([ext_id, len(ext)]) + ext
        el += bytes(-len(el) % 4)
        h += struct.pack(">HH", profile, len(el) // 4) + el
    pad = bytes(padding - 1) + bytes([padding]) if padding else b""
    return h + bytes(payload) + pad


class DDStream:
    """One received DD stream's datagrams in arrival order with what each one
    carries: rows of (datagram, payload_len, fn, ts, template index, attached
    Structure or None, active mask or None, custom frame diffs or None, has the
    extension).  The sender keeps the structure it last attached, so a frame is
    named by its template index."""

    def __init__(self, handle, ssrc, ext_id=5, sn0=1000, payload=b"\x01" + b"\x42" * 20):
        self.handle, self.ssrc, self.ext_id, self.sn = handle, ssrc, ext_id, sn0
        self.payload = payload
        self.structure = None
        self.rows = []

    def frame(self, fn, ts, tmpl, structure=None, active_mask=None, custom_fdiffs=None, fdiff_nibbles=None,
              packets=1, ext=True, payload=None, padding=0):
        """One frame as `packets` datagrams; a structure or mask rides on the first."""
        for k in range(packets):
            st = structure if k == 0 else None
            am = active_mask if k == 0 else None
            if st is not None:
                self.structure = st
            cur = self.structure
            d = descriptor(cur.template_id(tmpl), fn, first=k == 0, last=k == packets - 1, structure=st,
                           active_mask=am, ndt=cur.ndt, custom_fdiffs=custom_fdiffs, fdiff_nibbles=fdiff_nibbles)
            body = self.payload if payload is None else payload
            dg = rtp_ext(self.ssrc, self.sn, ts, self.ext_id, d if ext else None, body,
                         marker=1 if k == packets - 1 else 0, padding=padding)
            self.sn = (self.sn + 1) & M16
            self.rows.append((dg, len(body), fn & M16, ts & M32, tmpl, st, am, custom_fdiffs, ext))

    def duplicate(self, i):
        self.rows.append(self.rows[i])

    def swap(self, i, j):
        self.rows[i], self.rows[j] = self.rows[j], self.rows[i]


class Parser:
    """What the calculator needs of the stream's DependencyDescriptorParser
    (dependencydescriptorparser.go:75-163): the structure in force, the active
    mask and the sequence number it was taken at."""

    def __init__(self, structure=None, mask=0, active_ext_seq=0):
        self.structure, self.mask, self.active_ext_seq = structure, mask, active_ext_seq


def feed(model, parser, rows, flows):
    """What the calculator sees of `rows` given their lkf_flow rows of the same
    ingest.  A datagram with a payload that reached the RTX bucket is parsed
    (buffer.go:471-481, :617): an attached structure comes into force, and a
    mask newer than the parser's and different from it is SetMaxLayer; then
    RecvPacket for an ExtPacket (LKF_FLOW_FORWARD) with a descriptor."""
    for (dg, plen, fn, ts, tmpl, st, am, custom, ext), fl in zip(rows, flows):
        flags = int(fl["flags"])
        if not (flags & FLOW_BUCKET) or plen == 0 or not ext:
            continue
        if st is not None:
            parser.structure = st
            if am is None:
                am = (1 << st.ndt) - 1
        cur = parser.structure
        if cur is None:
            continue  # (ErrDDReaderNoStructure: no ExtPacket)
        ext_seq = int(fl["ext_sn"])
        if am is not None and ext_seq > parser.active_ext_seq:
            parser.active_ext_seq = ext_seq
            if am != parser.mask:
                parser.mask = am
                model.set_max_layer(*cur.max_layer(am))
        if flags & FLOW_FORWARD:
            sid, tid, _, tdiffs = cur.templates[tmpl]
            model.packet(fn, ts, sid, tid, list(custom) if custom is not None else list(tdiffs))
