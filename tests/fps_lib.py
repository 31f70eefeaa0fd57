"""The ingress frame-rate calculators restated on plain Python ints, and the
trace builder of their tests.

PyFps is written from buffer/fps.go:24-315 (frameRateCalculatorVPx,
FrameRateCalculatorVP8, FrameRateCalculatorVP9), buffer.go:518-543 (doFpsCalc)
and the text of livekit-server_amd/csrc/fps_device.h, not from its code: the
window is a list of frame records as in the reference, not a lane mask; every
frame-number operation is `& 0xffff`, every timestamp one `& 0xffffffff`, and
the rate is rounded to binary32 through struct after each of its two
operations (a binary64 quotient or product of two binary32 values rounds to
the same binary32 as the exact one: 53 >= 2 * 24 + 2).

The one divergence of the engine is restated too: no rate is computed for
temporal layer 3 (the reference panics there, fps.go:155).

The trace builder makes frames at a per-temporal-layer fps table (the layout
the reference's own test uses: a frame belongs to the lowest layer that is due)
and real VP8 / VP9 RTP datagrams of them for lkf_ingest.
"""
import struct

M16, M32 = 0xFFFF, 0xFFFFFFFF
MIN_FRAMES = (8, 15, 40)  # minFramesForCalculation fps.go:24
WINDOW = 64               # len(fnReceived)
NONE, VP8, VP9 = 0, 1, 2  # LKF_FPS_*

FLOW_FORWARD = 0x20
FLOW_BAD = 0x40
FLOW_PADDING = 0x10


def f32(x):
    """The binary32 nearest to x, as a Python float."""
    return struct.unpack("<f", struct.pack("<f", x))[0]


def f32_bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def rate_of(clock, last_ts, first_ts, frames):
    """fps.go:156: float32(clock) / float32(lastTs - ff.ts) * float32(frames)."""
    a, b = f32(float(clock)), f32(float((last_ts - first_ts) & M32))
    if b == 0.0:
        q = float("inf") if a > 0 else float("nan")
    else:
        q = f32(a / b)
    return f32(q * f32(float(frames)))


class _Frame:
    __slots__ = ("ts", "fn", "temporal")

    def __init__(self, ts, fn, temporal=0):
        self.ts, self.fn, self.temporal = ts, fn, temporal


class PyCalc:
    """frameRateCalculatorVPx."""

    def __init__(self, clock):
        self.clock = clock
        self.rates = [0.0] * 4
        self.completed = False
        self.resets = 0
        self._clear()

    def _clear(self):
        self.first = [None] * 4
        self.second = [None] * 4
        self.received = [None] * WINDOW
        self.base = None

    def reset(self):
        self._clear()
        self.resets += 1

    def recv(self, fn, ts, temporal):
        if self.completed:
            return True
        if temporal >= 4:
            return False
        if temporal < 0:
            temporal = 0
        if self.base is None:
            self.base = _Frame(ts, fn)  # (temporal stays 0)
            self.received[0] = self.base
            self.first[temporal] = self.base
            return False
        base_diff = (fn - self.base.fn) & M16
        if base_diff == 0 or base_diff > 0x4000:
            return False
        if base_diff >= WINDOW:
            self.reset()
            return False
        if self.received[base_diff] is not None:
            return False
        fi = _Frame(ts, fn, temporal)
        self.received[base_diff] = fi
        ff, sf = self.first[temporal], self.second[temporal]
        if ff is None:
            self.first[temporal] = fi
        elif (sf is None or sf.fn < fn) and fn != ff.fn and ((fn - ff.fn) & M16) < 0x4000:
            self.second[temporal] = fi
        return self.calc()

    def calc(self):
        counter = 0
        for t in range(4):
            if self.rates[t] > 0:
                counter += 1
                continue
            ff, sf = self.first[t], self.second[t]
            if counter > 0 and ff is None:
                counter += 1
                continue
            if ff is None or sf is None:
                continue
            if t == 3:  # the engine's divergence: the reference indexes minFramesForCalculation[3] and panics
                continue
            count, last_ts = 0, ff.ts
            j = ((ff.fn - self.base.fn) & M16) + 1
            end = ((sf.fn - self.base.fn) & M16) + 1
            while j < end:
                f = self.received[j]
                if f is None:
                    break
                if f.temporal <= t:
                    count += 1
                    last_ts = f.ts
                j += 1
            if count >= MIN_FRAMES[t]:
                self.rates[t] = rate_of(self.clock, last_ts, ff.ts, count)
                counter += 1
        if counter == 4:
            self.completed = True
            if self.rates[2] > 0 and self.rates[2] > f32(self.rates[1] * 3):
                self.rates[1] = f32(self.rates[2] / 2)
            self.reset()
            return True
        return False

    # ---- the state as the engine and the unit program show it
    def _slot(self, f):
        return -1 if f is None else (f.fn - self.base.fn) & M16

    def present(self):
        return sum(1 << j for j, f in enumerate(self.received) if f is not None)

    def state(self):
        """(present, first, second, base_fn, has_base, resets): lkf_fps_calc."""
        return (self.present(), tuple(self._slot(f) for f in self.first), tuple(self._slot(f) for f in self.second),
                self.base.fn if self.base else 0, 1 if self.base else 0, self.resets)

    def unit_words(self):
        pack = lambda fr: sum(((self._slot(f) + 1) & 0xFF) << (8 * t) for t, f in enumerate(fr))
        return "%016x %08x %08x %d %d %d %d %s" % (
            self.present(), pack(self.first), pack(self.second), self.base.fn if self.base else 0,
            1 if self.base else 0, 1 if self.completed else 0, self.resets,
            " ".join("%08x" % f32_bits(r) for r in self.rates))


class PyFps:
    """One Buffer's doFpsCalc over FrameRateCalculatorVP8 (kind VP8) or
    FrameRateCalculatorVP9 (kind VP9).  packet() takes what reaches doFpsCalc:
    an ExtPacket with a non-empty payload."""

    def __init__(self, kind, clock=90000):
        self.kind, self.clock = kind, clock
        self.calcs = [PyCalc(clock) for _ in range(1 if kind == VP8 else 3)]
        self.calculated = False

    def packet(self, fn, ts, temporal, spatial=-1):
        """-> RecvPacket's result (False when the stream is already calculated)."""
        if self.calculated:
            return False
        if self.kind == VP8:
            ret = self.calcs[0].recv(fn & M16, ts & M32, temporal)
            done = self.calcs[0].completed
        else:
            if spatial < 0 or spatial >= 3:
                return False
            ret = self.calcs[spatial].recv(fn & M16, ts & M32, temporal)
            done = all(c.completed for c in self.calcs)
        if ret and done:
            self.calculated = True
        return ret

    def rates(self, spatial=0):
        return list(self.calcs[spatial].rates)

    def state(self):
        """lkf_stream_fps.as_dict()."""
        z = (0, (-1,) * 4, (-1,) * 4, 0, 0, 0)
        cs = [c.state() for c in self.calcs] + [z] * (3 - len(self.calcs))
        fps = [tuple(f32_bits(r) for r in c.rates) for c in self.calcs] + [(0,) * 4] * (3 - len(self.calcs))
        comp = [1 if c.completed else 0 for c in self.calcs] + [0] * (3 - len(self.calcs))
        return {"kind": self.kind, "calculated": 1 if self.calculated else 0, "completed": tuple(comp),
                "fps_bits": tuple(fps), "calc": tuple(cs)}

    def unit_line(self, ret):
        return "%d %d | %s" % (1 if ret else 0, 1 if self.calculated else 0,
                               " | ".join(c.unit_words() for c in self.calcs))


def zero_state():
    """lkf_stream_fps.as_dict() of a stream that was never enabled (the engine
    answers first / second 0 there: the struct is all zero)."""
    z = (0, (0,) * 4, (0,) * 4, 0, 0, 0)
    return {"kind": NONE, "calculated": 0, "completed": (0, 0, 0), "fps_bits": ((0,) * 4,) * 3, "calc": (z,) * 3}


# ---- the trace builder -------------------------------------------------------
def make_frames(table, n, start_ts, start_fn, clock=90000, fn_bits=16):
    """n frames of one spatial layer at the cumulative per-temporal-layer rates
    `table` (table[t] = fps of layers 0..t together): -> [(fn, ts, temporal)].
    A frame comes every clock / table[-1] ticks and belongs to the lowest layer
    that is due, which then pushes that layer's and every higher layer's next
    due time on by its own period.  fn counts on in fn_bits bits."""
    step = [int(f32(f32(float(clock)) / f32(float(r)))) & M32 for r in table]
    due = [start_ts] * len(table)
    ts, fn, out = start_ts, start_fn, []
    for _ in range(n):
        temporal = 0
        for t in range(len(table)):
            if ts >= due[t]:
                temporal = t
                for u in range(t, len(table)):
                    due[u] = (due[u] + step[u]) & M32
                break
        out.append((fn, ts, temporal))
        ts = (ts + step[-1]) & M32
        fn = (fn + 1) & ((1 << fn_bits) - 1)
    return out


def rtp(ssrc, sn, ts, payload, pt=96, marker=0, padding=0):
    """An RTP datagram; padding > 0 appends that many padding bytes (P bit)."""
    h = bytes([0x80 | (0x20 if padding else 0), (marker << 7) | pt]) + struct.pack(">HII", sn & M16, ts & M32, ssrc)
    pad = bytes(padding - 1) + bytes([padding]) if padding else b""
    return h + bytes(payload) + pad


def vp8_payload(pid, tid, pid_bits=15, start=True, body=b"\x55" * 20, key=False):
    """VP8 payload descriptor (RFC 7741) with X, the PictureID in pid_bits (15,
    7, or 0: no I bit) and the TID, then the payload header's first byte."""
    x = (0x80 if pid_bits else 0) | 0x20
    d = bytes([0x80 | (0x10 if start else 0), x])
    if pid_bits == 15:
        d += bytes([0x80 | ((pid >> 8) & 0x7F), pid & 0xFF])
    elif pid_bits == 7:
        d += bytes([pid & 0x7F])
    d += bytes([(tid & 3) << 6])
    return d + bytes([0 if key else 1]) + body


def vp8_bad_payload():
    """L without T: the descriptor does not unmarshal (helpers.go:102-104)."""
    return bytes([0x90, 0x40, 0x11, 0x01, 0x02])


def vp9_payload(pid, sid, tid, pid_bits=15, start=True, body=b"\x66" * 20):
    """VP9 payload descriptor, non-flexible mode: I (unless pid_bits 0), P, L,
    B when `start`; the PictureID in 7 or 15 bits, the layer byte, TL0PICIDX."""
    b0 = (0x80 if pid_bits else 0) | 0x40 | 0x20 | (0x08 if start else 0)
    d = bytes([b0])
    if pid_bits == 15:
        d += bytes([0x80 | ((pid >> 8) & 0x7F), pid & 0xFF])
    elif pid_bits == 7:
        d += bytes([pid & 0x7F])
    d += bytes([((tid & 7) << 5) | ((sid & 7) << 1), 0x11])
    return d + body


def wire_fn(pid, pid_bits):
    """The PictureID a parser reads back from a descriptor written with pid_bits."""
    return pid & 0x7FFF if pid_bits == 15 else pid & 0x7F if pid_bits == 7 else 0


class Stream:
    """One received stream's datagrams in arrival order, with what each tells
    the calculator: rows of (datagram bytes, payload_len, fn, ts, temporal, spatial)."""

    def __init__(self, handle, ssrc, kind, sn0=1000):
        self.handle, self.ssrc, self.kind, self.sn = handle, ssrc, kind, sn0
        self.rows = []

    def _push(self, payload, ts, fn, temporal, spatial, padding=0, marker=0):
        d = rtp(self.ssrc, self.sn, ts, payload, marker=marker, padding=padding)
        self.sn = (self.sn + 1) & M16
        self.rows.append((d, len(payload), fn, ts, temporal, spatial))

    def frame(self, fn, ts, temporal, spatial=0, packets=1, pid_bits=15):
        """One frame as `packets` datagrams (the first carries S / B)."""
        for k in range(packets):
            if self.kind == VP8:
                p = vp8_payload(fn, temporal, pid_bits, start=k == 0, body=bytes([k]) * (12 + 3 * k))
            else:
                p = vp9_payload(fn, spatial, temporal, pid_bits, start=k == 0, body=bytes([k]) * (12 + 3 * k))
            self._push(p, ts, wire_fn(fn, pid_bits), temporal, spatial if self.kind == VP9 else -1,
                       marker=1 if k == packets - 1 else 0)

    def padding_only(self, ts):
        self._push(b"", ts, 0, 0, -1, padding=8)

    def bad_descriptor(self, ts):
        self._push(vp8_bad_payload(), ts, 0, 0, -1)

    def duplicate(self, i):
        """Row i once more, as it was sent (same sequence number)."""
        self.rows.append(self.rows[i])

    def swap(self, i, j):
        self.rows[i], self.rows[j] = self.rows[j], self.rows[i]

    def drop(self, lo, hi):
        del self.rows[lo:hi]


def feed(model, rows, flows, first=0):
    """What doFpsCalc sees of `rows` (Stream rows) given their lkf_flow rows of
    the same ingest: an ExtPacket (LKF_FLOW_FORWARD) with a payload."""
    for (d, plen, fn, ts, temporal, spatial), fl in zip(rows, flows):
        if (int(fl["flags"]) & FLOW_FORWARD) and plen != 0:
            model.packet(fn, ts, temporal, spatial)
