"""RTCP demultiplexing helpers: PyRtcpDemux, a plain-Python restatement of
what include/lkfwd.h defines for lkf_rtcp_demux ("RTCP demultiplexing: which
DownTracks a compound addresses"): the routing table's rule, the table of
destination SSRCs, the size checks of the RTCP ingress table, the result
fields and the order of the entries.  Written from the header's text on Python
bytes with struct; it shares no code with rtcp_dmx_device.h.

Also the topology and the seeded datagrams the CPU and GPU tests share: the CPU
test vets the seeds with the restatement alone, the GPU tests assert the same
shares, so a trace that exercises nothing fails in both.
"""
import random
import struct

from tests import rtcp_wire_lib as W

DMX_OK, DMX_EMPTY, DMX_MALFORMED = 0, 1, 2


def build_table(downtracks):
    """downtracks: (dt, ssrc, transport, active) -> {(transport, ssrc): dt}: the active DownTracks with a
    binding; of two with one key the higher handle."""
    table = {}
    for dt, ssrc, transport, active in downtracks:
        if active and transport >= 0 and table.get((transport, ssrc), -1) < dt:
            table[(transport, ssrc)] = dt
    return table


class PyRtcpDemux:
    @staticmethod
    def destinations(data):
        """The destination SSRCs of one datagram in packet order, repeats included; None when malformed."""
        data = bytes(data)
        if not data:
            return None
        out, at = [], 0
        while at < len(data):
            if len(data) - at < 4:
                return None
            b0, pt, length = struct.unpack_from(">BBH", data, at)
            size = 4 * (length + 1)
            if b0 >> 6 != 2 or size > len(data) - at:
                return None
            p, fmt = data[at:at + size], b0 & 0x1F
            word = lambda o: struct.unpack_from(">I", p, o)[0]  # noqa: E731
            if pt == 201:
                if size < 8 + 24 * fmt:
                    return None
                out += [word(8 + 24 * k) for k in range(fmt)]
            elif pt == 200:
                if size < 28 + 24 * fmt:
                    return None
                out += [word(28 + 24 * k) for k in range(fmt)] + [word(4)]
            elif (pt, fmt) in ((205, 1), (206, 1)):
                if size < 12:
                    return None
                out.append(word(8))
            elif (pt, fmt) == (205, 15):
                if size < 20:
                    return None
                out.append(word(8))
            elif (pt, fmt) in ((205, 5), (206, 2)):
                if size >= 12:
                    out.append(word(8))
            elif (pt, fmt) == (206, 4):
                if size < 12 or (size - 12) % 8:
                    return None
                out += [word(12 + 8 * k) for k in range((size - 12) // 8)]
            elif (pt, fmt) == (206, 15):
                if size < 20 or p[12:16] != b"REMB" or size < 20 + 4 * p[16]:
                    return None
                out += [word(20 + 4 * k) for k in range(p[16])]
            at += size
        return out

    @classmethod
    def call(cls, table, dgrams):
        """One demux call: dgrams (transport, bytes) -> ([(status, dests, unrouted, entries)] per datagram,
        [(dt, dgram)] sorted by DownTrack, then datagram)."""
        res, entries = [], []
        for i, (t, data) in enumerate(dgrams):
            if len(data) == 0:
                res.append((DMX_EMPTY, 0, 0, 0))
                continue
            dests = cls.destinations(data)
            if dests is None:
                res.append((DMX_MALFORMED, 0, 0, 0))
                continue
            hit = [table[(t, s)] for s in dests if (t, s) in table]
            res.append((DMX_OK, len(dests), len(dests) - len(hit), len(set(hit))))
            entries += [(d, i) for d in set(hit)]
        return res, sorted(entries)


# ---- the tests' topology: six transports that hold 0, 1, 2, 33, 65 and 70 DownTracks ------------
COUNTS = (0, 1, 2, 33, 65, 70)
NDTS = sum(COUNTS)


def topology():
    """[(dt, ssrc, transport)] for dt = 0 .. NDTS - 1.  The handles are dealt over the transports in a seeded
    shuffle, so neither the SSRC order nor the transport order is the handle order; transports 4 and 5 use the
    same SSRCs (5000 + 13k), the others their own."""
    slots = [(t, k) for t, n in enumerate(COUNTS) for k in range(n)]
    random.Random(4).shuffle(slots)
    return [(dt, 5000 + 13 * k if t >= 4 else 0x10000 * t + 7 * (COUNTS[t] - k), t) for dt, (t, k) in enumerate(slots)]


def ssrcs_by_transport(topo):
    by = {t: [] for t in range(len(COUNTS))}
    for _, ssrc, t in topo:
        by[t].append(ssrc)
    return by


def _packet(rnd, who):
    k = rnd.randrange(15)
    if k == 0:
        return W.rr(who(), [W.report_block(who()) for _ in range(rnd.choice((0, 1, 1, 2, 3, 31)))],
                    extension=b"\xca\xfe\xf0\x0d" if rnd.random() < 0.2 else b"")
    if k == 1:
        return W.sr(who(), [W.report_block(who()) for _ in range(rnd.randrange(3))])
    if k == 2:
        return W.sdes(who())
    if k == 3:
        return W.bye(*[who() for _ in range(rnd.randrange(3))])
    if k in (4, 5):
        return W.nack(1, who(), [(rnd.randrange(65536), rnd.randrange(65536)) for _ in range(rnd.randrange(4))])
    if k == 6:
        return W.twcc(1, who(), bytes(rnd.randrange(256) for _ in range(4 * rnd.choice((1, 2, 2, 3, 3, 4)))))
    if k == 7:
        return W.pli(1, who())
    if k == 8:
        return W.fir(1, who(), [(who(), rnd.randrange(256)) for _ in range(rnd.randrange(4))])
    if k == 9:
        n = rnd.randrange(5)
        return W.remb(1, ssrcs=[who() for _ in range(n)], ident=b"REMB" if rnd.random() < 0.93 else b"RAMB",
                      num=n if rnd.random() < 0.93 else n + 1)
    if k == 10:
        return W.xr(who())
    if k == 11:  # RRR and SLI: 8, 12 or 16 bytes
        return W._hdr(rnd.choice((2, 5)), rnd.choice((205, 206)),
                      struct.pack(">III", 1, who(), who())[:4 * rnd.randrange(1, 4)])
    if k == 12:  # feedback formats without destinations
        return W._hdr(rnd.choice((3, 8, 11)), rnd.choice((205, 206)), struct.pack(">II", 1, who()))
    if k == 13:  # the same SSRC twice in one packet
        s = who()
        return W.rr(1, [W.report_block(s), W.report_block(s)])
    return W.unknown(rnd.choice((192, 199, 204, 208, 255)), rnd.randrange(32), struct.pack(">II", who(), who()))


def _mutate(rnd, data, starts):
    """Truncation, a version flip, a length edit, an inflated REMB numSSRC, or stray bytes behind."""
    b = bytearray(data)
    m = rnd.randrange(5)
    if m == 0 and b:
        del b[rnd.randrange(len(b)):]
    elif m == 1 and starts:
        b[rnd.choice(starts)] ^= rnd.choice((0x40, 0x80, 0xC0))
    elif m == 2 and starts:
        at = rnd.choice(starts) + 3
        b[at] = (b[at] + rnd.choice((-2, -1, 1, 2, 7))) & 0xFF
    elif m == 3:
        at = bytes(b).find(b"REMB")
        if at >= 0 and at + 4 < len(b):
            b[at + 4] = min(255, b[at + 4] + rnd.choice((1, 2, 200)))
        else:
            b += bytes(rnd.randrange(256) for _ in range(rnd.randrange(1, 4)))
    else:
        b += bytes(rnd.randrange(256) for _ in range(rnd.randrange(1, 4)))
    return bytes(b)


def random_datagrams(seed, n, topo=None):
    """n datagrams (transport, bytes) over the six transports: one to five packets whose SSRCs are mostly
    DownTracks of the datagram's transport, sometimes another transport's or nobody's; about a fifth mutated,
    a few empty (what lkf_srtcp_unprotect leaves of a rejected datagram)."""
    rnd = random.Random(seed)
    by = ssrcs_by_transport(topo or topology())
    every = [s for v in by.values() for s in v]
    out = []
    for _ in range(n):
        t = rnd.choice((0, 1, 2, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5))

        def who():
            r = rnd.random()
            if r < 0.75 and by[t]:
                return rnd.choice(by[t])
            return rnd.choice(every) if r < 0.88 else rnd.randrange(1 << 32)

        if rnd.random() < 0.04:
            out.append((t, b""))
            continue
        pk = [_packet(rnd, who) for _ in range(rnd.randrange(1, 6))]
        data = W.compound(*pk)
        if rnd.random() < 0.2:
            starts, at = [], 0
            for p in pk:
                starts.append(at)
                at += len(p)
            data = _mutate(rnd, data, starts)
        out.append((t, data))
    return out


def shares(res):
    """What a trace must exercise, from the results alone -> dict of counts."""
    return dict(
        n=len(res),
        routed=sum(1 for r in res if r[3] >= 1),
        empty=sum(1 for r in res if r[0] == DMX_EMPTY),
        malformed=sum(1 for r in res if r[0] == DMX_MALFORMED),
        all_unrouted=sum(1 for r in res if r[0] == DMX_OK and r[1] > 0 and r[2] == r[1]),
        multi=sum(1 for r in res if r[3] >= 2),
        duplicate=sum(1 for r in res if r[0] == DMX_OK and r[1] - r[2] > r[3]))


def assert_shares(res):
    s = shares(res)
    assert 2 * s["routed"] >= s["n"], s
    for k in ("empty", "malformed", "all_unrouted", "multi", "duplicate"):
        assert s[k] >= 1, (k, s)


# the GPU tests' random trace (tests/test_rtcp_demux_cpu.py vets it)
GPU_SEED, GPU_N = 11, 300
