"""RTCP ingress helpers: an independent marshaller of RTCP packets and
PyRtcpIn, a plain-Python restatement of the parse that include/lkfwd.h
defines for lkf_rtcp_ingest ("RTCP ingress: DownTrack.handleRTCP from the
bytes").  Written from the header's text (framing, the table of size checks,
the entry rules), not from rtcp_in_device.h; it works on Python bytes with
struct.unpack and slices, so it shares no code and no idiom with the C++.

Marshallers return bytes; compound(*packets) joins them.
"""
import struct

IN_OK, IN_MALFORMED = 0, 1
REF_REMB, REF_TWCC = 1, 2
FB_HAS_RR = 1


# ---- marshaller ---------------------------------------------------------------------------
def _hdr(count, pt, body, padding=False):
    assert len(body) % 4 == 0 and 0 <= count < 32
    return struct.pack(">BBH", 0x80 | (0x20 if padding else 0) | count, pt, len(body) // 4) + body


def report_block(ssrc, fraction_lost=0, total_lost=0, lsn=0, jitter=0, lsr=0, dlsr=0):
    return struct.pack(">IIIIII", ssrc, ((fraction_lost & 0xFF) << 24) | (total_lost & 0xFFFFFF), lsn, jitter, lsr, dlsr)


def rr(sender_ssrc, blocks=(), extension=b""):
    return _hdr(len(blocks), 201, struct.pack(">I", sender_ssrc) + b"".join(blocks) + extension)


def sr(sender_ssrc, blocks=(), ntp=0, rtp=0, packets=0, octets=0):
    return _hdr(len(blocks), 200, struct.pack(">IQIII", sender_ssrc, ntp, rtp, packets, octets) + b"".join(blocks))


def sdes(ssrc, cname=b"cname"):
    item = struct.pack(">IBB", ssrc, 1, len(cname)) + cname + b"\0"
    item += b"\0" * (-len(item) % 4)
    return _hdr(1, 202, item)


def bye(*ssrcs):
    return _hdr(len(ssrcs), 203, b"".join(struct.pack(">I", s) for s in ssrcs))


def nack(sender_ssrc, media_ssrc, pairs):
    """pairs: (pid, blp)"""
    return _hdr(1, 205, struct.pack(">II", sender_ssrc, media_ssrc) +
                b"".join(struct.pack(">HH", p & 0xFFFF, b & 0xFFFF) for p, b in pairs))


def nack_pairs(sns):
    """The (pid, blp) pairs that carry the sequence numbers `sns` in this order, one pair per run a BLP can
    hold: a following SN joins the pair when it lies 1..16 ahead of the PID and above every SN in it."""
    pairs = []
    for sn in sns:
        if pairs:
            pid, blp, top = pairs[-1]
            d = (sn - pid) & 0xFFFF
            if 1 <= d <= 16 and d > top:
                pairs[-1] = (pid, blp | (1 << (d - 1)), d)
                continue
        pairs.append((sn, 0, 0))
    return [(p, b) for p, b, _ in pairs]


def twcc(sender_ssrc, media_ssrc, body=b"\0" * 8):
    return _hdr(15, 205, struct.pack(">II", sender_ssrc, media_ssrc) + body)


def pli(sender_ssrc, media_ssrc):
    return _hdr(1, 206, struct.pack(">II", sender_ssrc, media_ssrc))


def fir(sender_ssrc, media_ssrc, entries=((0, 0),)):
    return _hdr(4, 206, struct.pack(">II", sender_ssrc, media_ssrc) +
                b"".join(struct.pack(">IBBH", s, seq & 0xFF, 0, 0) for s, seq in entries))


def remb(sender_ssrc, bitrate_exp=3, mantissa=0x12345, ssrcs=(), ident=b"REMB", num=None):
    n = len(ssrcs) if num is None else num
    return _hdr(15, 206, struct.pack(">II", sender_ssrc, 0) + ident +
                struct.pack(">I", (n << 24) | ((bitrate_exp & 0x3F) << 18) | (mantissa & 0x3FFFF)) +
                b"".join(struct.pack(">I", s) for s in ssrcs))


def xr(ssrc, block=b"\x04\x00\x00\x02" + b"\0" * 8):
    return _hdr(0, 207, struct.pack(">I", ssrc) + block)


def unknown(pt, count=0, body=b"\xff" * 8):
    return _hdr(count, pt, body)


def compound(*packets):
    return b"".join(packets)


# ---- the restatement ----------------------------------------------------------------------
class Parsed:
    """One entry's outcome.  fb: dicts of the lkf_rtcp_fb fields (without dt); sns: the NACKed sequence
    numbers; refs: (kind, offset inside the entry, length)."""

    def __init__(self):
        self.status = IN_MALFORMED
        self.reports = self.nacks = self.plis = self.firs = 0
        self.fb, self.sns, self.refs = [], [], []


def _blank_fb():
    return dict(flags=0, last_sequence_number=0, total_lost=0, jitter=0, last_sender_report=0, delay=0, nacks=0,
                plis=0, firs=0, fraction_lost=0)


class PyRtcpIn:
    @staticmethod
    def packets(data):
        """Framing -> [(count, pt, offset, packet bytes)] or None when malformed."""
        if len(data) == 0:
            return None
        out, at = [], 0
        while at < len(data):
            left = data[at:]
            if len(left) < 4:
                return None
            b0, pt, length = struct.unpack(">BBH", left[:4])
            if b0 >> 6 != 2:
                return None
            size = 4 * (length + 1)
            if size > len(left):
                return None
            out.append((b0 & 0x1F, pt, at, left[:size]))  # (the P bit, b0 & 0x20, is ignored)
            at += size
        return out

    @classmethod
    def parse(cls, data, ssrc):
        """One handleRTCP(data) call on a DownTrack whose SSRC is `ssrc` -> Parsed."""
        bad = Parsed()
        pkts = cls.packets(bytes(data))
        if pkts is None:
            return bad
        r = Parsed()
        for count, pt, at, p in pkts:
            size = len(p)
            if pt == 201:
                if size < 8 + 24 * count:
                    return bad
                for k in range(count):
                    blk = p[8 + 24 * k:32 + 24 * k]
                    who, fl_lost, lsn, jitter, lsr, dlsr = struct.unpack(">IIIIII", blk)
                    if who != ssrc:
                        continue
                    f = _blank_fb()
                    f.update(flags=FB_HAS_RR, fraction_lost=fl_lost >> 24, total_lost=fl_lost & 0xFFFFFF,
                             last_sequence_number=lsn, jitter=jitter, last_sender_report=lsr, delay=dlsr)
                    r.fb.append(f)
            elif pt == 200:
                if size < 28 + 24 * count:
                    return bad
            elif pt == 205 and count == 1:
                if size < 12:
                    return bad
                for k in range((size - 12) // 4):
                    pid, blp = struct.unpack(">HH", p[12 + 4 * k:16 + 4 * k])
                    r.sns.append(pid)
                    r.sns += [(pid + i + 1) & 0xFFFF for i in range(16) if blp >> i & 1]
            elif pt == 205 and count == 15:
                if size < 20:
                    return bad
                if struct.unpack(">I", p[8:12])[0] == ssrc:
                    r.refs.append((REF_TWCC, at, size))
            elif pt == 206 and count == 1:
                if size < 12:
                    return bad
                r.plis += 1
            elif pt == 206 and count == 4:
                if size < 12 or (size - 12) % 8 != 0:
                    return bad
                r.firs += 1
            elif pt == 206 and count == 15:
                if size < 20 or p[12:16] != b"REMB" or size < 20 + 4 * p[16]:
                    return bad
                r.refs.append((REF_REMB, at, size))
            # anything else: skipped by size
        r.status = IN_OK
        r.reports = len(r.fb)
        r.nacks = len(r.sns)
        if not r.fb:
            r.fb.append(_blank_fb())
        r.fb[-1].update(nacks=r.nacks, plis=r.plis, firs=r.firs)
        return r

    @classmethod
    def call(cls, entries, ssrc_of):
        """One lkf_rtcp_ingest: entries (dt, bytes) grouped by DownTrack -> (per entry dict of the
        lkf_rtcp_in_result fields but rtt_ms and pli_layer, fb list [(dt, fields)], NACK list [(dt, sn)],
        refs [(entry, kind, offset inside the entry, len)], [Parsed])."""
        res, fbs, nacks, refs, parsed = [], [], [], [], []
        for i, (dt, data) in enumerate(entries):
            p = cls.parse(data, ssrc_of(dt))
            parsed.append(p)
            res.append(dict(status=p.status, fb_first=len(fbs), fb_count=len(p.fb), reports=p.reports, nacks=p.nacks,
                            plis=p.plis, firs=p.firs, nack_first=len(nacks), ref_first=len(refs),
                            ref_count=len(p.refs)))
            fbs += [(dt, f) for f in p.fb]
            nacks += [(dt, sn) for sn in p.sns]
            refs += [(i, k, o, n) for k, o, n in p.refs]
        return res, fbs, nacks, refs, parsed
