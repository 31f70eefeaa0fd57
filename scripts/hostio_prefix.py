#!/usr/bin/env python3
"""Host-fed configs[1] loop in wire and in prefix egress mode, one process.

The deployment shape of bench.py --host-io with the synchronous drain: pinned
host inputs and outputs, per step  submit(b); run(b); drain(batch b - 1)  so
the previous batch's output crosses PCIe while batch b computes.  After the
warm-up the loop runs in segments of --seg steps that alternate between
LKF_EGRESS_WIRE and LKF_EGRESS_PREFIX on one engine (the Forwarder state runs
on through all of them: it does not depend on the mode).  A segment is timed
from its first submit to the end of the drain of its last batch; between
segments the engine is synced, untimed.  Prints one JSON line with ms/step and
device -> host bytes/step of both modes (and writes it to --out).
"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rooms", type=int, default=100)
    ap.add_argument("--batch-s", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seg", type=int, default=4, help="steps per timed segment")
    ap.add_argument("--rounds", type=int, default=2, help="segments per mode")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    pkg = importlib.import_module("livekit-server_amd")
    wl = importlib.import_module("livekit-server_amd.workload")
    abi = pkg.abi
    nb = args.warmup + 2 * args.rounds * args.seg
    trace = wl.Trace(2, duration_s=nb * args.batch_s, batch_s=args.batch_s, rooms=args.rooms)
    eng = pkg.Engine.for_trace(trace)
    wl.load_topology(eng.api, eng.h, trace)

    # pinned host inputs (every batch) and outputs (one set per mode)
    hpk, har, meta = [], [], []
    for b in range(nb):
        pk, n, ar, alen = trace.batch(b)
        tp = torch.frombuffer(bytearray(C.string_at(pk, max(1, n) * 64)), dtype=torch.uint8).pin_memory()
        ta = torch.zeros(alen + 64, dtype=torch.uint8, pin_memory=True)
        if alen:
            ta[:alen].copy_(torch.from_numpy(np.ctypeslib.as_array(ar, shape=(alen,))))
        hpk.append(tp)
        har.append(ta)
        meta.append((n, alen))
    out_cap = int(trace.max_batch_tuples)
    ar_cap = int(trace.max_batch_out_bytes) + 16 * out_cap
    h_rec = torch.empty(out_cap * 48, dtype=torch.uint8, pin_memory=True)  # lkf_out (40 B) or lkf_pre (48 B)
    h_ar = torch.empty(ar_cap, dtype=torch.uint8, pin_memory=True)
    rec_p, ar_p = C.c_void_p(h_rec.data_ptr()), C.c_void_p(h_ar.data_ptr())

    def drain(mode, age):
        """-> device -> host bytes moved"""
        if mode == abi.LKF_EGRESS_PREFIX:
            nrec, nbytes = eng.drain_prefix_run_into(age, rec_p, out_cap, ar_p, ar_cap)
            return nrec * 48 + nbytes
        nrec, nbytes = eng.drain_run_into(age, rec_p, out_cap, ar_p, ar_cap)
        return nrec * 40 + nbytes

    def feed(b):
        wl.queue_events(eng.api, eng.h, trace, b)
        n, alen = meta[b]
        eng.submit(C.c_void_p(hpk[b].data_ptr()), n, C.c_void_p(har[b].data_ptr()), alen)
        eng.run()

    def segment(mode, b0, k):
        """k steps from batch b0 in `mode` -> (seconds, D2H bytes, H2D bytes)"""
        eng.set_egress(mode)
        eng.sync()
        d2h = h2d = 0
        t0 = time.perf_counter()
        for i in range(k):
            feed(b0 + i)
            h2d += meta[b0 + i][0] * 64 + meta[b0 + i][1]
            if i:
                d2h += drain(mode, 1)
        d2h += drain(mode, 0)
        return time.perf_counter() - t0, d2h, h2d

    modes = {"wire": abi.LKF_EGRESS_WIRE, "prefix": abi.LKF_EGRESS_PREFIX}
    # warm-up: both modes once (first-touch of the prefix buffers included)
    eng.set_egress(abi.LKF_EGRESS_PREFIX)
    b = 0
    for i in range(args.warmup):
        segment(modes["prefix" if i & 1 else "wire"], b, 1)
        b += 1
    res = {m: {"segments_ms_per_step": [], "d2h": 0, "h2d": 0, "s": 0.0} for m in modes}
    for r in range(args.rounds):
        for m in ("wire", "prefix"):
            s, d2h, h2d = segment(modes[m], b, args.seg)
            b += args.seg
            res[m]["segments_ms_per_step"].append(round(s * 1e3 / args.seg, 3))
            res[m]["d2h"] += d2h
            res[m]["h2d"] += h2d
            res[m]["s"] += s
    eng.sync()
    cum = eng.cumulative()
    eng.close()
    steps = args.rounds * args.seg
    line = {"workload": "configs[1] host-fed: %d rooms x 10 participants, %d DownTracks, %g s batches" % (
                args.rooms, trace.ndts, args.batch_s),
            "loop": "submit(b); run(b); drain_run(age 1), pinned host buffers, synchronous drains",
            "device": torch.cuda.get_device_name(0), "warmup": args.warmup, "steps_per_mode": steps,
            "forwarded_total": cum["forwarded"]}
    for m in modes:
        line[m] = {"ms_per_step": round(res[m]["s"] * 1e3 / steps, 3),
                   "segments_ms_per_step": res[m]["segments_ms_per_step"],
                   "d2h_bytes_per_step": res[m]["d2h"] // steps, "h2d_bytes_per_step": res[m]["h2d"] // steps}
    s = json.dumps(line)
    print(s)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
