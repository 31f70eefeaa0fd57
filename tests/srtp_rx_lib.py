"""SRTP unprotect test helpers (test infrastructure).

PyUnprotect restates include/lkfwd.h "SRTP unprotect" from its text and RFC
3711 §3.3 / RFC 7714: per stream the state (started, s_l, mask) and, for every
datagram in list order, parse -> index -> replay -> authenticate -> accept.
The verification is real: HMAC-SHA1 through hmac/hashlib, the AES-CM keystream
from OpenSSL AES-128 single blocks, GCM open through libcrypto's EVP.  It keeps
no record of which packets a test tampered with.  Test traffic is protected
with the independent tests/srtp_lib.protect / protect_gcm.
"""
import ctypes as C
import hashlib
import hmac

import numpy as np

from tests import srtp_lib
from tests.srtp_lib import AES_CM, GCM

OK, MALFORMED, REPLAY_OLD, REPLAY_DUP, AUTH = 0, 1, 2, 3, 4
WINDOW = 64
# the traces the composition tests run: (config, Trace arguments)
CLEAN_SHAPES = ((1, dict(rooms=1, seed=4, batch_s=0.05, duration_s=1.0)),
                (2, dict(rooms=2, seed=5, batch_s=0.25, duration_s=1.0)))
KEY_SEED = 99
REJECT_MIX = dict(seed=31, corrupt=0.02, duplicate=0.01)  # ProtectedTrace arguments of the rejects test
M64 = (1 << 64) - 1


class OpenSSLOpen(srtp_lib.OpenSSLAes):
    """+ AES-128-GCM open (EVP decrypt with the expected tag)."""

    def gcm_open(self, key, iv, aad, ct, tag):
        """The plaintext, or None when the tag does not verify."""
        c = self.c
        if not hasattr(self, "_open"):
            c.EVP_aes_128_gcm.restype = C.c_void_p
            c.EVP_CIPHER_CTX_ctrl.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
            c.EVP_DecryptInit_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_char_p]
            c.EVP_DecryptUpdate.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int), C.c_char_p, C.c_int]
            c.EVP_DecryptFinal_ex.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int)]
            self._open = True
        ctx = c.EVP_CIPHER_CTX_new()
        try:
            assert c.EVP_DecryptInit_ex(ctx, c.EVP_aes_128_gcm(), None, None, None) == 1
            assert c.EVP_CIPHER_CTX_ctrl(ctx, 0x9, 12, None) == 1  # EVP_CTRL_GCM_SET_IVLEN
            assert c.EVP_DecryptInit_ex(ctx, None, None, bytes(key), bytes(iv)) == 1
            n = C.c_int(0)
            if aad:
                assert c.EVP_DecryptUpdate(ctx, None, C.byref(n), bytes(aad), len(aad)) == 1
            out = C.create_string_buffer(len(ct) + 32)
            got = 0
            if ct:
                assert c.EVP_DecryptUpdate(ctx, out, C.byref(n), bytes(ct), len(ct)) == 1
                got = n.value
            tbuf = C.create_string_buffer(bytes(tag), 16)
            assert c.EVP_CIPHER_CTX_ctrl(ctx, 0x11, 16, tbuf) == 1  # EVP_CTRL_GCM_SET_TAG
            tail = C.create_string_buffer(32)
            if c.EVP_DecryptFinal_ex(ctx, tail, C.byref(n)) <= 0:
                return None
            return out.raw[:got] + tail.raw[:n.value]
        finally:
            c.EVP_CIPHER_CTX_free(ctx)


def parse(arena, arena_len, off, ln, tag):
    """Step 1: (SEQ, h), or None for a malformed datagram."""
    if off % 16 or off + ln > arena_len or ln < 12:
        return None
    d = arena[off:off + ln]
    if d[0] >> 6 != 2:
        return None
    h = 12 + 4 * (d[0] & 15)
    if d[0] & 0x10:
        if h + 4 > ln:
            return None
        h += 4 + 4 * ((d[h + 2] << 8) | d[h + 3])
    if h + tag > ln:
        return None
    return (d[2] << 8) | d[3], h


class RxState:
    def __init__(self, transport=-1):
        self.started, self.s_l, self.mask, self.transport = 0, 0, 0, transport
        self.accepted = self.auth_failures = self.replays = self.malformed = 0

    def check(self, seq):
        """Steps 2 and 3 -> (v, verdict before authentication)."""
        if not self.started:
            return seq, OK
        d = (seq - (self.s_l & 0xFFFF)) & 0xFFFF
        v = self.s_l + (d - 0x10000 if d & 0x8000 else d)
        if v < 0:
            v = seq
        if v <= self.s_l:
            if self.s_l - v >= WINDOW:
                return v, REPLAY_OLD
            if (self.mask >> (self.s_l - v)) & 1:
                return v, REPLAY_DUP
        return v, OK

    def accept(self, v):
        if not self.started:
            self.started, self.s_l, self.mask = 1, v, 1
        elif v > self.s_l:
            sh = v - self.s_l
            self.mask = ((self.mask << sh) & M64 if sh < 64 else 0) | 1
            self.s_l = v
        else:
            self.mask |= 1 << (self.s_l - v)
        self.accepted += 1

    def step(self, malformed, seq, auth):
        """One datagram with its authentication outcome given (auth: a callable of v) -> (status, v)."""
        if malformed:
            self.malformed += 1
            return MALFORMED, 0
        v, st = self.check(seq)
        if st != OK:
            self.replays += 1
            return st, v
        if not auth(v):
            self.auth_failures += 1
            return AUTH, v
        self.accept(v)
        return OK, v

    def as_tuple(self):
        return (self.s_l, self.mask, self.started, self.transport, self.accepted, self.auth_failures, self.replays,
                self.malformed)


class PyUnprotect:
    """The engine's receive side restated: bind(), then unprotect() per call."""

    def __init__(self, nstreams, aes=None):
        self.aes = aes or OpenSSLOpen()
        self.streams = [RxState() for _ in range(nstreams)]
        self.keys = {}   # stream -> (transport, master key, master salt, profile)
        self.sess = {}   # transport -> session keys

    def bind(self, stream, key):
        """key: (transport handle, master key, master salt, profile), or None to unbind."""
        self.streams[stream] = RxState(key[0] if key else -1)
        if key:
            self.keys[stream] = key
            if key[0] not in self.sess:
                self.sess[key[0]] = srtp_lib.session(self.aes, key[1], key[2], key[3])
        else:
            self.keys.pop(stream, None)

    def _open(self, key, pkt, h, roc):
        """Step 4 -> the plaintext packet, or None."""
        t, _, _, prof = key
        sk, salt, auth = self.sess[t]
        seq = (pkt[2] << 8) | pkt[3]
        roc &= 0xFFFFFFFF
        if prof == GCM:
            iv = bytes(2) + bytes(pkt[8:12]) + roc.to_bytes(4, "big") + seq.to_bytes(2, "big")
            iv = bytes(a ^ b for a, b in zip(iv, salt))
            pt = self.aes.gcm_open(sk, iv, pkt[:h], pkt[h:-16], pkt[-16:])
            return None if pt is None else bytes(pkt[:h]) + pt
        m = bytes(pkt[:-10])
        want = hmac.new(auth, m + roc.to_bytes(4, "big"), hashlib.sha1).digest()[:10]
        if not hmac.compare_digest(want, bytes(pkt[-10:])):
            return None
        iv = int.from_bytes(salt + b"\0\0", "big") ^ (int.from_bytes(pkt[8:12], "big") << 64) \
            ^ (((roc << 16) | seq) << 16)
        nblk = (len(m) - h + 15) // 16
        ks = self.aes.ecb(sk, b"".join(((iv + j) % (1 << 128)).to_bytes(16, "big") for j in range(nblk)))
        return m[:h] + bytes(a ^ b for a, b in zip(m[h:], ks))

    def unprotect(self, pkts, arena):
        """pkts: (stream, off, len) per datagram; arena: the protected bytes.
        -> (results [(index, status, len)], {datagram: plaintext} of the accepted ones)."""
        arena = bytes(arena)
        res, plain = [], {}
        for i, (s, off, ln) in enumerate(pkts):
            if s >= len(self.streams):
                res.append((0, MALFORMED, 0))
                continue
            st = self.streams[s]
            if s not in self.keys:  # unbound: passes through
                if off + ln > len(arena):
                    res.append((0, MALFORMED, 0))
                else:
                    res.append((0, OK, ln))
                    plain[i] = arena[off:off + ln]
                continue
            key = self.keys[s]
            tag = 16 if key[3] == GCM else 10
            p = parse(arena, len(arena), off, ln, tag)
            got = []

            def auth(v, p=p, off=off, ln=ln, key=key, got=got):
                got.append(self._open(key, arena[off:off + ln], p[1], v >> 16))
                return got[0] is not None

            status, v = st.step(p is None, p[0] if p else 0, auth)
            if status == OK:
                plain[i] = got[0]
            res.append((v, status, ln - tag if status == OK else 0))
        return res, plain

    def results_array(self, res):
        out = np.zeros(len(res), dtype=[("index", "<u8"), ("status", "<u4"), ("len", "<u4")])
        for i, (v, st, ln) in enumerate(res):
            out[i] = (v, st, ln)
        return out


# ---- traffic ---------------------------------------------------------------------
class Sender:
    """The publisher's side of one SSRC: the rollover counter of each packet it
    sends (first packet: ROC 0; the sequence moves by less than 2^15 between
    packets)."""

    def __init__(self):
        self.ext = None

    def roc(self, seq):
        if self.ext is None:
            self.ext = seq
            return 0
        d = (seq - (self.ext & 0xFFFF)) & 0xFFFF
        e = self.ext + (d - 0x10000 if d & 0x8000 else d)
        self.ext = max(self.ext, e)
        return max(e, 0) >> 16


def rtp_packet(ssrc, seq, payload, kind="plain", ts=0, pt=96, marker=0):
    """A plain RTP packet: kind in plain / csrc (2 CSRCs) / ext1 (one-byte
    extension block) / ext2 (two-byte block)."""
    cc = 2 if kind == "csrc" else 0
    x = 0x10 if kind in ("ext1", "ext2") else 0
    h = bytes([0x80 | x | cc, (marker << 7) | pt]) + (seq & 0xFFFF).to_bytes(2, "big") + (ts & 0xFFFFFFFF).to_bytes(
        4, "big") + ssrc.to_bytes(4, "big")
    if cc:
        h += (0x11111111).to_bytes(4, "big") + (0x22222222).to_bytes(4, "big")
    if kind == "ext1":
        h += bytes([0xBE, 0xDE, 0, 2]) + bytes([0x32, 1, 2, 3, 0x51, 9, 8, 0])
    if kind == "ext2":
        h += bytes([0x10, 0x00, 0, 1]) + bytes([7, 2, 0xAA, 0xBB])
    return h + bytes(payload)


def seal(aes, sess, prof, pkt, roc):
    return (srtp_lib.protect_gcm if prof == GCM else srtp_lib.protect)(aes, sess, pkt, roc)


class Arena:
    """Datagrams laid out at 16-aligned offsets (or a forced one)."""

    def __init__(self):
        self.buf = bytearray()
        self.pkts = []  # (stream, off, len)

    def add(self, stream, data, misalign=0, length=None):
        off = (len(self.buf) + 15) // 16 * 16 + misalign
        self.buf += bytes(off - len(self.buf)) + bytes(data)
        self.pkts.append((stream, off, len(data) if length is None else length))
        return len(self.pkts) - 1

    def raw_pkts(self, abi, arrival0=10**9):
        out = np.zeros(len(self.pkts), dtype=abi.RAW_PKT_DTYPE)
        for i, (s, off, ln) in enumerate(self.pkts):
            out[i] = (arrival0 + 1000 * i, s, off, ln, 0)
        return out


def trace_keys(trace, seed, gcm_every=2):
    """One receive transport per (room, participant) that publishes: every
    gcm_every-th one AEAD_AES_128_GCM -> {stream: (index, master key, master salt, profile)};
    the index is the transport handle when they are added in this order."""
    rng = np.random.default_rng(seed)
    per_pub, out = {}, {}
    for s in range(trace.nstreams):
        t = trace.tracks[trace.streams[s].track]
        k = (int(t.room), int(t.publisher))
        if k not in per_pub:
            mk = rng.integers(0, 256, 16, dtype=np.uint8).tobytes()
            ms = rng.integers(0, 256, 14, dtype=np.uint8).tobytes()
            prof = GCM if len(per_pub) % gcm_every == gcm_every - 1 else AES_CM
            per_pub[k] = (len(per_pub), mk, ms[:12] if prof == GCM else ms, prof)
        out[s] = per_pub[k]
    return out


def transports_in_order(keys):
    """The distinct transports of trace_keys in handle order."""
    seen = {}
    for k in keys.values():
        seen[k[0]] = k
    return [seen[i] for i in range(len(seen))]


class ProtectedTrace:
    """Every raw batch of a trace protected in Python into a fresh 16-aligned
    arena, next to the plaintext batch laid out at the same offsets.
    corrupt / duplicate: seeded shares of datagrams with one bit flipped
    (anywhere in the protected datagram) / sent twice in a row."""

    def __init__(self, trace, abi, keys, seed=0, corrupt=0.0, duplicate=0.0, aes=None):
        self.aes = aes or OpenSSLOpen()
        rng = np.random.default_rng(seed)
        sess = {k[0]: srtp_lib.session(self.aes, k[1], k[2], k[3]) for k in keys.values()}
        senders = {}
        self.batches = []
        for b in range(trace.nbatches):
            rp, n, ar, alen = trace.batch_raw(b)
            src = C.string_at(ar, alen) if alen else b""
            prot, plain = Arena(), Arena()
            arrival = []
            for i in range(n):
                s, off, ln = int(rp[i].stream), int(rp[i].off), int(rp[i].len)
                pkt = src[off:off + ln]
                t, _, _, prof = keys[s]
                seq = (pkt[2] << 8) | pkt[3]
                sealed = seal(self.aes, sess[t], prof, pkt, senders.setdefault(s, Sender()).roc(seq))
                copies = 2 if rng.random() < duplicate else 1
                for _ in range(copies):
                    data = bytearray(sealed)
                    if rng.random() < corrupt:
                        bit = int(rng.integers(0, 8 * len(data)))
                        data[bit // 8] ^= 1 << (bit % 8)
                    prot.add(s, data)
                    plain.buf += bytes(prot.pkts[-1][1] - len(plain.buf)) + pkt + bytes(len(data) - ln)
                    plain.pkts.append((s, prot.pkts[-1][1], ln))
                    arrival.append(int(rp[i].arrival_ns))
            raws = np.zeros(len(prot.pkts), dtype=abi.RAW_PKT_DTYPE)
            praws = np.zeros(len(prot.pkts), dtype=abi.RAW_PKT_DTYPE)
            for j, ((s, off, ln), (_, _, pln)) in enumerate(zip(prot.pkts, plain.pkts)):
                raws[j] = (arrival[j], s, off, ln, 0)
                praws[j] = (arrival[j], s, off, pln, 0)
            self.batches.append(dict(raws=raws, srtp=bytes(prot.buf), praws=praws, plain=bytes(plain.buf),
                                     pkts=prot.pkts))
