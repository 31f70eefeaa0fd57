"""SRTCP test helpers (test infrastructure).

Written from include/lkfwd.h "SRTCP" and RFC 3711 §3.4 / RFC 7714 §9, not from
srtcp_device.h or the kernels:

- session_rtcp: the second session key set (labels 3, 4, 5) through
  tests/srtp_lib.kdf.
- seal_cm / seal_gcm: the sender's side on hmac/hashlib, OpenSSL AES-128
  single blocks and libcrypto's EVP AES-128-GCM.
- PySrtcpRx: the receive side restated, per transport the 16 slots and the six
  counters.  The verification is real (hmac.compare_digest, EVP GCM open); it
  keeps no record of what a test tampered with.
- TxIndex: the send side's per (transport, SSRC) index model.
- Arena: datagrams laid out at 16-aligned offsets, as tests/srtp_rx_lib.Arena.
"""
import hashlib
import hmac

import numpy as np

from tests import srtp_lib
from tests.srtp_lib import AES_CM, GCM
from tests.srtp_rx_lib import OpenSSLOpen

OK, MALFORMED, REPLAY_OLD, REPLAY_DUP, AUTH, UNENCRYPTED, NO_SLOT = range(7)
SSRCS = 16
WINDOW = 64
M64 = (1 << 64) - 1
BODY_LENS = (0, 4, 13, 31, 44, 48, 52, 56, 60, 64, 68, 1200)


def tag_len(prof):
    return 16 if prof == GCM else 10


def session_rtcp(aes, mk, ms, prof=AES_CM):
    """(encryption key, salt, authentication key or None) of RFC 3711 §4.3.2's labels 3, 5, 4."""
    if prof == GCM:
        return srtp_lib.kdf(aes, 3, mk, ms, 16), srtp_lib.kdf(aes, 5, mk, ms, 12), None
    return srtp_lib.kdf(aes, 3, mk, ms, 16), srtp_lib.kdf(aes, 5, mk, ms, 14), srtp_lib.kdf(aes, 4, mk, ms, 20)


def cm_iv(salt, ssrc, index):
    """The AES-CM counter block 0 as an integer: (salt << 16) ^ (SSRC << 64) ^ (index << 16)."""
    return (int.from_bytes(salt, "big") << 16) ^ (ssrc << 64) ^ (index << 16)


def cm_keystream(aes, key, salt, ssrc, index, n):
    iv = cm_iv(salt, ssrc, index)
    nblk = (n + 15) // 16
    return aes.ecb(key, b"".join(((iv + j) % (1 << 128)).to_bytes(16, "big") for j in range(nblk)))[:n] if n else b""


def gcm_iv(salt, ssrc, index):
    iv = bytes(2) + ssrc.to_bytes(4, "big") + bytes(2) + index.to_bytes(4, "big")
    return bytes(a ^ b for a, b in zip(iv, salt))


def seal_cm(aes, sess, pkt, index, e_bit=1):
    """hdr[0:8] || enc(body) || E|index || tag[10]"""
    key, salt, auth = sess
    ssrc = int.from_bytes(pkt[4:8], "big")
    ks = cm_keystream(aes, key, salt, ssrc, index, len(pkt) - 8)
    m = bytes(pkt[:8]) + bytes(a ^ b for a, b in zip(pkt[8:], ks)) + ((e_bit << 31) | index).to_bytes(4, "big")
    return m + hmac.new(auth, m, hashlib.sha1).digest()[:10]


def seal_gcm(aes, sess, pkt, index, e_bit=1):
    """hdr[0:8] || ciphertext || tag[16] || E|index"""
    key, salt, _ = sess
    ssrc = int.from_bytes(pkt[4:8], "big")
    trailer = ((e_bit << 31) | index).to_bytes(4, "big")
    aad = bytes(pkt[:8]) + ((1 << 31) | index).to_bytes(4, "big")
    return bytes(pkt[:8]) + aes.gcm_seal(key, gcm_iv(salt, ssrc, index), aad, pkt[8:]) + trailer


def seal(aes, sess, prof, pkt, index, e_bit=1):
    return (seal_gcm if prof == GCM else seal_cm)(aes, sess, pkt, index, e_bit)


def rtcp_plain(ssrc, body_len, fill=0):
    """A plaintext packet of 8 + body_len bytes: an RTCP header with the sender SSRC, then filler.  (The
    SRTCP layer reads only the version bits and bytes 4..7; the framing inside is RTCP ingress's.)"""
    return bytes([0x80, 201, 0, (body_len + 4) // 4 & 255]) + ssrc.to_bytes(4, "big") + \
        bytes((fill + 7 * k) & 255 for k in range(body_len))


class Table:
    """One transport's receive state: 16 slots [in_use, ssrc, latest, mask] and the six counters."""

    def __init__(self):
        self.slots = [[0, 0, 0, 0] for _ in range(SSRCS)]
        self.accepted = self.auth_failures = self.replays = self.malformed = self.unencrypted = self.no_slot = 0

    def step(self, parsed, auth):
        """parsed: MALFORMED, UNENCRYPTED or (ssrc, index); auth: a callable -> bool, called only at step 5."""
        if parsed == MALFORMED:
            self.malformed += 1
            return MALFORMED
        if parsed == UNENCRYPTED:
            self.unencrypted += 1
            return UNENCRYPTED
        ssrc, index = parsed
        slot = next((s for s in self.slots if s[0] and s[1] == ssrc), None)
        if slot is not None and index <= slot[2]:
            if slot[2] - index >= WINDOW:
                self.replays += 1
                return REPLAY_OLD
            if (slot[3] >> (slot[2] - index)) & 1:
                self.replays += 1
                return REPLAY_DUP
        if slot is None and all(s[0] for s in self.slots):
            self.no_slot += 1
            return NO_SLOT
        if not auth():
            self.auth_failures += 1
            return AUTH
        if slot is None:
            slot = next(s for s in self.slots if not s[0])
            slot[:] = [1, ssrc, index, 1]
        elif index > slot[2]:
            sh = index - slot[2]
            slot[3] = ((slot[3] << sh) & M64 if sh < 64 else 0) | 1
            slot[2] = index
        else:
            slot[3] |= 1 << (slot[2] - index)
        self.accepted += 1
        return OK

    def as_tuple(self):
        """As Engine.transport_srtcp returns it."""
        return ([tuple(s) for s in self.slots],
                (self.accepted, self.auth_failures, self.replays, self.malformed, self.unencrypted, self.no_slot))


def parse(arena, off, ln, tag):
    """Steps 1 to 3 -> MALFORMED, UNENCRYPTED or (ssrc, index)."""
    if off % 16 or off + ln > len(arena) or ln < 8 + 4 + tag:
        return MALFORMED
    d = arena[off:off + ln]
    if d[0] >> 6 != 2:
        return MALFORMED
    w = int.from_bytes(d[-4:] if tag == 16 else d[-14:-10], "big")
    if not w >> 31:
        return UNENCRYPTED
    return int.from_bytes(d[4:8], "big"), w & 0x7FFFFFFF


class PySrtcpRx:
    """The engine's SRTCP receive side restated: add_transport() in handle order, then unprotect() per call."""

    def __init__(self, aes=None):
        self.aes = aes or OpenSSLOpen()
        self.keys = []    # per transport (master key, master salt, profile)
        self.sess = []
        self.tables = []

    def add_transport(self, mk, ms, prof):
        self.keys.append((mk, ms, prof))
        self.sess.append(session_rtcp(self.aes, mk, ms, prof))
        self.tables.append(Table())
        return len(self.keys) - 1

    def reset(self, t):
        self.tables[t] = Table()

    def open(self, t, pkt, ssrc, index):
        """Step 5 -> the plaintext, or None."""
        key, salt, auth = self.sess[t]
        if self.keys[t][2] == GCM:
            aad = bytes(pkt[:8]) + ((1 << 31) | index).to_bytes(4, "big")
            pt = self.aes.gcm_open(key, gcm_iv(salt, ssrc, index), aad, pkt[8:-20], pkt[-20:-4])
            return None if pt is None else bytes(pkt[:8]) + pt
        m = bytes(pkt[:-10])
        if not hmac.compare_digest(hmac.new(auth, m, hashlib.sha1).digest()[:10], bytes(pkt[-10:])):
            return None
        body = m[8:-4]
        ks = cm_keystream(self.aes, key, salt, ssrc, index, len(body))
        return m[:8] + bytes(a ^ b for a, b in zip(body, ks))

    def unprotect(self, pkts, arena):
        """pkts: (transport, off, len) per datagram -> (results [(ssrc, index, status, len)],
        {datagram: plaintext} of the accepted ones)."""
        arena = bytes(arena)
        res, plain = [], {}
        for i, (t, off, ln) in enumerate(pkts):
            if not 0 <= t < len(self.keys):
                res.append((0, 0, MALFORMED, 0))
                continue
            tag = tag_len(self.keys[t][2])
            p = parse(arena, off, ln, tag)
            got = []

            def auth(t=t, off=off, ln=ln, p=p, got=got):
                got.append(self.open(t, arena[off:off + ln], p[0], p[1]))
                return got[0] is not None

            st = self.tables[t].step(p, auth)
            if st == OK:
                plain[i] = got[0]
            ssrc, index = p if isinstance(p, tuple) else (0, 0)
            res.append((ssrc, index, st, ln - 4 - tag if st == OK else 0))
        return res, plain


class TxIndex:
    """Per (transport, SSRC): incremented before use, 31 bits."""

    def __init__(self):
        self.last = {}

    def next(self, t, ssrc):
        self.last[(t, ssrc)] = (self.last.get((t, ssrc), 0) + 1) & 0x7FFFFFFF
        return self.last[(t, ssrc)]


class Arena:
    """Datagrams laid out at 16-aligned offsets (or a forced one)."""

    def __init__(self):
        self.buf = bytearray()
        self.pkts = []  # (transport, off, len)

    def add(self, transport, data, misalign=0, length=None):
        off = (len(self.buf) + 15) // 16 * 16 + misalign
        self.buf += bytes(off - len(self.buf)) + bytes(data)
        self.pkts.append((transport, off, len(data) if length is None else length))
        return len(self.pkts) - 1

    def raws(self, abi):
        out = np.zeros(len(self.pkts), dtype=abi.SRTCP_RAW_DTYPE)
        for i, p in enumerate(self.pkts):
            out[i] = p
        return out


def make_keys(n=4, seed=77):
    """n transports' (master key, master salt, profile): AES-CM, GCM, AES-CM, GCM, ..."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        mk = rng.integers(0, 256, 16, dtype=np.uint8).tobytes()
        ms = rng.integers(0, 256, 14, dtype=np.uint8).tobytes()
        prof = GCM if k % 2 else AES_CM
        out.append((mk, ms[:12] if prof == GCM else ms, prof))
    return out


# ---- the composition test's traffic (tests/test_srtcp_gpu.py; its reject pattern is checked on the CPU with
# the restatement alone in tests/test_srtcp_cpu.py) ----
COMPOSE_SEED = 5
COMPOSE_TRANSPORTS = 4
COMPOSE_PER_TRANSPORT = 18  # datagrams each transport carries in the composition test


class Composer:
    """One subscriber transport's sender: seals compounds with indices 1.., about one in ten corrupted (one
    bit flipped anywhere in the datagram) or replayed (the previous datagram again).  Two draws per compound,
    whatever its length: the pattern depends on the seed and the count alone."""

    def __init__(self, aes, sess, prof, seed):
        self.aes, self.sess, self.prof = aes, sess, prof
        self.rng = np.random.default_rng(seed)
        self.index = 0
        self.last = None

    def seal(self, compound):
        r, where = self.rng.random(), self.rng.random()
        if r < 0.05 and self.last is not None:
            return self.last
        self.index += 1
        d = bytearray(seal(self.aes, self.sess, self.prof, compound, self.index))
        if r > 0.95:
            bit = int(where * 8 * len(d))
            d[bit // 8] ^= 1 << (bit % 8)
        self.last = bytes(d)
        return self.last
