#!/usr/bin/env python3
"""SRTP unprotect next to SRTP protect on configs[1], timed by GPU events.

For each profile (AES-CM, GCM) one engine at --rooms rooms: every 1-s raw
batch is protected on the host (one receive transport per publisher), then
lkf_unprotect_device -> lkf_ingest_device -> lkf_run -> lkf_protect run on the
same engine, whose DownTracks are bound to subscriber transports of the same
profile.  Over the batches after the first: lkf_unprotect_timing_window (the index,
crypto and commit kernels) and lkf_protect_timing_window (k_srtp_roc +
k_srtp_protect), each with the packets and bytes it covered, so the two
per-byte costs come from one process.  Every datagram must come back
LKF_SRTP_RX_OK.  With --corrupt P a share P of the datagrams gets one flipped
bit (the commit kernel's rare path) and the rejected count is reported instead.

Prints one JSON line per profile (and writes them to --out).
"""
import argparse
import ctypes as C
import hashlib
import hmac
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EPOCH = 1700000000 * 10**9


class Ctr:
    """AES-128-CTR from libcrypto (one call per packet: the host-side sealing is not what is measured)."""

    def __init__(self):
        c = C.CDLL("libcrypto.so.3")
        c.EVP_CIPHER_CTX_new.restype = C.c_void_p
        c.EVP_aes_128_ctr.restype = C.c_void_p
        c.EVP_EncryptInit_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_char_p]
        c.EVP_EncryptUpdate.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int), C.c_char_p, C.c_int]
        self.c, self.ctx, self.alg = c, c.EVP_CIPHER_CTX_new(), c.EVP_aes_128_ctr()
        self.out = C.create_string_buffer(1 << 16)
        self.n = C.c_int(0)

    def xor(self, key, iv16, data):
        if not data:
            return b""
        assert self.c.EVP_EncryptInit_ex(self.ctx, self.alg, None, key, iv16) == 1
        assert self.c.EVP_EncryptUpdate(self.ctx, self.out, C.byref(self.n), data, len(data)) == 1
        return self.out.raw[:self.n.value]


def seal_cm(ctr, sess, pkt, h, roc):
    key, salt, auth = sess
    seq = (pkt[2] << 8) | pkt[3]
    iv = int.from_bytes(salt + b"\0\0", "big") ^ (int.from_bytes(pkt[8:12], "big") << 64) ^ (((roc << 16) | seq) << 16)
    m = pkt[:h] + ctr.xor(key, iv.to_bytes(16, "big"), pkt[h:])
    return m + hmac.new(auth, m + roc.to_bytes(4, "big"), hashlib.sha1).digest()[:10]


def protect_batch(trace, b, keys, sess, senders, ctr, aes, rng, corrupt):
    """Batch b protected into a fresh 16-aligned arena -> (lkf_raw_pkt rows, arena bytes)."""
    from tests import srtp_lib
    from tests.srtp_rx_lib import Sender

    rp, n, ar, alen = trace.batch_raw(b)
    src = C.string_at(ar, alen) if alen else b""
    rows = np.zeros(n, dtype=[("arrival_ns", "<i8"), ("stream", "<u4"), ("off", "<u4"), ("len", "<u4"),
                              ("reserved", "<u4")])
    parts, off = [], 0
    for i in range(n):
        s, o, ln = int(rp[i].stream), int(rp[i].off), int(rp[i].len)
        pkt = src[o:o + ln]
        t, _, _, prof = keys[s]
        roc = senders.setdefault(s, Sender()).roc((pkt[2] << 8) | pkt[3])
        if prof == srtp_lib.GCM:
            data = srtp_lib.protect_gcm(aes, sess[t], pkt, roc)
        else:
            data = seal_cm(ctr, sess[t], pkt, srtp_lib.header_len(pkt), roc)
        if corrupt and rng.random() < corrupt:
            d = bytearray(data)
            bit = int(rng.integers(0, 8 * len(d)))
            d[bit // 8] ^= 1 << (bit % 8)
            data = bytes(d)
        rows[i] = (int(rp[i].arrival_ns), s, off, len(data), 0)
        pad = -len(data) % 16
        parts.append(data + bytes(pad))
        off += len(data) + pad
    return rows, b"".join(parts)


def run_profile(pkg, wl, args, prof_name):
    from tests import srtp_lib
    from tests import srtp_rx_lib as R

    gcm = prof_name == "gcm"
    trace = wl.Trace(2, duration_s=float(args.batches + 1), batch_s=1.0, rooms=args.rooms)
    nb = min(args.batches, trace.nbatches)
    eng = pkg.Engine.for_trace(trace, headroom=1.5)
    wl.load_topology(eng.api, eng.h, trace)
    wl.load_streams(eng.api, eng.h, trace)
    aes = R.OpenSSLOpen()
    keys = R.trace_keys(trace, 5, gcm_every=1 if gcm else 10**9)
    for k in R.transports_in_order(keys):
        assert eng.api["add_transport"](eng.h, C.byref(pkg.transport_params(k[1], k[2], k[3]))) == k[0]
    for s, k in keys.items():
        eng.set_stream_transport(s, k[0])
    srtp_lib.bind_transports(pkg, eng.api, eng.h, trace, 6, unbound_every=10**9, gcm_every=1 if gcm else 0)
    sess = {k[0]: srtp_lib.session(aes, k[1], k[2], k[3]) for k in keys.values()}
    senders, ctr, rng = {}, Ctr(), np.random.default_rng(9)
    dev = torch.device("cuda", 0)
    keep, pkts_in, bytes_in, rejected, pkts_out, bytes_out = [], 0, 0, 0, 0, 0
    for b in range(nb):
        rows, arena = protect_batch(trace, b, keys, sess, senders, ctr, aes, rng, args.corrupt)
        d_pk = torch.from_numpy(rows.view(np.uint8).copy()).to(dev)
        d_srtp = torch.zeros(len(arena) + 64, dtype=torch.uint8, device=dev)
        d_srtp[:len(arena)].copy_(torch.frombuffer(bytearray(arena), dtype=torch.uint8))
        d_out, d_plain = torch.zeros_like(d_pk), torch.zeros_like(d_srtp)
        torch.cuda.synchronize(dev)
        keep.append((d_pk, d_srtp, d_out, d_plain))
        p = lambda t: C.c_void_p(t.data_ptr())
        if args.events:
            wl.queue_events(eng.api, eng.h, trace, b)
        eng.unprotect_device(p(d_pk), len(rows), p(d_srtp), len(arena), p(d_out), p(d_plain))
        eng.ingest_device(p(d_out), len(rows), p(d_plain), len(arena))
        eng.run()
        assert eng.api["protect"](eng.h, EPOCH + b * 10**9) == 0
        eng.sync()
        res = eng.unprotect_results()
        bad = int((res["status"] != 0).sum())
        assert args.corrupt or bad == 0, "a clean datagram was rejected"
        del keep[:-1]
        if b == 0:  # the first batch warms the kernels up and is left out of the windows
            continue
        rejected += bad
        pkts_in += len(rows)
        bytes_in += int(rows["len"].sum())
        st = eng.stats()
        pkts_out += int(st["forwarded"])
        bytes_out += int(st["out_bytes"]) + (16 if gcm else 10) * int(st["forwarded"])
    nb -= 1
    un_ms, pr_ms = eng.unprotect_timing_window(nb), eng.protect_timing_window(nb)
    res = {
        "profile": prof_name, "rooms": args.rooms, "batches": nb, "streams": int(trace.nstreams),
        "corrupt": args.corrupt, "rejected": rejected,
        "unprotect_ms_per_batch": un_ms / nb, "unprotect_packets": pkts_in, "unprotect_bytes": bytes_in,
        "unprotect_packets_per_s": pkts_in / (un_ms / 1e3), "unprotect_bytes_per_s": bytes_in / (un_ms / 1e3),
        "unprotect_ns_per_byte": un_ms * 1e6 / bytes_in,
        "protect_ms_per_batch": pr_ms / nb, "protect_packets": pkts_out, "protect_bytes": bytes_out,
        "protect_packets_per_s": pkts_out / (pr_ms / 1e3), "protect_bytes_per_s": bytes_out / (pr_ms / 1e3),
        "protect_ns_per_byte": pr_ms * 1e6 / bytes_out,
    }
    eng.close()
    trace.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rooms", type=int, default=100)
    ap.add_argument("--batches", type=int, default=3, help="1-s batches, the first one unmeasured (at least 2)")
    ap.add_argument("--profiles", default="aes_cm,gcm")
    ap.add_argument("--corrupt", type=float, default=0.0)
    ap.add_argument("--events", action="store_true", help="queue the trace's scripted control ops as well")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    pkg = importlib.import_module("livekit-server_amd")
    wl = importlib.import_module("livekit-server_amd.workload")
    lines = []
    for prof in args.profiles.split(","):
        lines.append(json.dumps(run_profile(pkg, wl, args, prof)))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
