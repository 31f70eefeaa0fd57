#!/usr/bin/env python3
"""What the ingress frame-rate calculators cost per ingest.

Workload: bench.py's headline shape, BASELINE.json configs[1] (100 rooms x 10
participants per GPU, VP8 3-layer simulcast + Opus, 2 % loss), one second of
media per batch, the raw datagrams resident in HBM.  The timed step is the
ingest alone: lkf_ingest_device and a wait for every stream of the engine (host
clock around work that ends in a device synchronise); the batch is then
forwarded untimed (lkf_run), so the engine stays in its steady state.

One engine per round, three phases in a row on the same engine and build:
  (a) nothing enabled                                   --warmup + --steps batches
  (b) every video stream enabled, while calculating     until an ingest completes no stream (at most --calc)
  (c) every video stream enabled, what can complete has --steps batches
(--off-only: phase (a) alone, for alternating runs against another library, LKF_LIB)
The phases follow each other on one engine because an engine's speed depends
on the hardware queues its streams get (bench.py next_engine), which would
confound two engines side by side; --rounds repeats the whole with a fresh
engine.  Per phase: min / median / max / p10 / p90 of the step in ms, and
whether median(c) - median(a) lies inside (a)'s own p10-p90 spread.

  python scripts/ingest_fps_bench.py [--rooms 100] [--steps 15] [--warmup 5] [--rounds 2] [--log profiles/ingest_fps_bench.log]

The kernel's own time comes from a run of its own under the profiler, with
only phases (b) and (c) (--profiled), and is read back with --stats-dir:
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o fps -- python scripts/ingest_fps_bench.py --profiled --steps 10
  python scripts/ingest_fps_bench.py --stats-dir OUT

--dd measures the dependency-descriptor calculator instead (k_ing_fps_dd,
lkf_stream_fps_enable_dd) on BASELINE.json configs[4], whose video streams are
the ones with a dependency descriptor (VP9 / AV1 SVC): --rooms then defaults to
200 (a tenth of the configuration, as one ingest of a second of its media), the
same three phases; add --dd to the --profiled and --stats-dir forms too.
"""
import argparse
import csv
import ctypes as C
import glob
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kernel_stats(d, dd=False):
    """k_ing_fps's (dd: k_ing_fps_dd's) row of rocprofv3's kernel statistics under d -> dict."""
    rows, name = [], "k_ing_fps_dd" if dd else "k_ing_fps"
    for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            rows += [r for r in csv.DictReader(f)
                     if name in r.get("Name", "") and (dd or "k_ing_fps_dd" not in r.get("Name", ""))]
    if not rows:
        raise SystemExit("no %s row in a *kernel_stats.csv under %s" % (name, d))
    r = rows[0]
    us = lambda k: round(float(r[k]) / 1e3, 2) if r.get(k) else None
    return dict(kernel=name, calls=int(r["Calls"]), total_us=us("TotalDurationNs"), avg_us=us("AverageNs"),
                min_us=us("MinNs"), max_us=us("MaxNs"))


def summary(v):
    s = sorted(v)
    q = lambda p: s[min(len(s) - 1, int(p * len(s)))]
    return dict(n=len(s), min=round(s[0], 4), p10=round(q(0.1), 4), median=round(statistics.median(s), 4),
                p90=round(q(0.9), 4), max=round(s[-1], 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rooms", type=int, default=0, help="default 100, with --dd 200")
    ap.add_argument("--dd", action="store_true", help="configs[4] and the dependency-descriptor calculator")
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calc", type=int, default=8, help="most batches of phase (b)")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--off-only", action="store_true",
                    help="phase (a) alone: also runs on a build without the calculators (a parent library)")
    ap.add_argument("--profiled", action="store_true", help="phases (b) and (c) only, one round (under rocprofv3)")
    ap.add_argument("--stats-dir", default="", help="read k_ing_fps's time from rocprofv3's output and exit")
    ap.add_argument("--log", default="")
    a = ap.parse_args()
    if a.stats_dir:
        print(json.dumps(kernel_stats(a.stats_dir, a.dd)))
        return
    a.rooms = a.rooms or (200 if a.dd else 100)

    import numpy as np
    import torch  # first: one HIP runtime in the process, as bench.py

    pkg = importlib.import_module("livekit-server_amd")
    wl = importlib.import_module("livekit-server_amd.workload")
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    na = 0 if a.profiled else a.warmup + a.steps
    nb = na if a.off_only else na + a.calc + a.steps
    trace = wl.Trace(5 if a.dd else 2, duration_s=nb * 1.0, batch_s=1.0, rooms=a.rooms)
    wl.events_at_batch_start(trace)
    dpk, dar, meta = [], [], []
    rsz = C.sizeof(pkg.abi.lkf_raw_pkt)
    for b in range(nb):
        pk, n, ar, alen = trace.batch_raw(b)
        dpk.append(torch.frombuffer(bytearray(C.string_at(pk, max(1, n) * rsz)), dtype=torch.uint8).to(dev))
        ta = torch.zeros(alen + 64, dtype=torch.uint8, device=dev)
        if alen:
            ta[:alen].copy_(torch.from_numpy(np.ctypeslib.as_array(ar, shape=(alen,))))
        dar.append(ta)
        meta.append((n, alen))
    torch.cuda.synchronize(dev)
    sp = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def step(eng, b):
        wl.queue_events(eng.api, eng.h, trace, b)
        n, alen = meta[b]
        eng.sync()
        t0 = time.perf_counter()
        eng.ingest_device(C.c_void_p(dpk[b].data_ptr()), n, C.c_void_p(dar[b].data_ptr()), alen)
        eng.sync()
        ms = (time.perf_counter() - t0) * 1e3
        eng.run(sp)  # (untimed: the batch is forwarded, the engine stays in its steady state)
        eng.sync()
        return ms

    rounds = []
    for rnd in range(1 if a.profiled else a.rounds):
        eng = pkg.Engine.for_trace(trace, device=0)
        try:
            wl.load_topology(eng.api, eng.h, trace)
            wl.load_streams(eng.api, eng.h, trace)
            pa = [step(eng, b) for b in range(na)][a.warmup:]
            if a.off_only:
                rounds.append(dict(round=rnd, datagrams_per_batch=int(np.median([m[0] for m in meta])),
                                   off_ms=summary(pa), off_batch_ms=[round(v, 4) for v in pa]))
                continue
            enable = eng.api["stream_fps_enable_dd" if a.dd else "stream_fps_enable"]
            on = [s for s in range(trace.nstreams) if enable(eng.h, s) == 0]
            pb, pc, done, b = [], [], 0, na
            while b < na + a.calc:  # (b): until an ingest completes nothing
                pb.append(step(eng, b))
                b += 1
                k = len(eng.ingest_fps_changed())
                done += k
                if not k and len(pb) > 1:
                    pc.append(pb.pop())  # (that ingest already belongs to (c))
                    break
            while len(pc) < a.steps and b < nb:
                pc.append(step(eng, b))
                b += 1
                done += len(eng.ingest_fps_changed())
            rec = dict(round=rnd, enabled=len(on), calculated=done, datagrams_per_batch=int(np.median([m[0] for m in meta])),
                       calculating_ms=summary(pb), calculated_ms=summary(pc))
            # (by batch: the trace's batches are not all the same work; off_batch_ms of an --off-only
            # run over the same batches is what a phase compares with)
            rec["first_batch"] = dict(calculating=na, calculated=na + len(pb))
            rec["calculating_batch_ms"] = [round(v, 4) for v in pb]
            rec["calculated_batch_ms"] = [round(v, 4) for v in pc]
            if pa:
                sa, sc = summary(pa), summary(pc)
                rec["off_ms"] = sa
                rec["calculated_minus_off_ms"] = round(sc["median"] - sa["median"], 4)
                rec["inside_off_spread"] = bool(sa["p10"] - sa["median"] <= sc["median"] - sa["median"] <= sa["p90"] - sa["median"])
            rounds.append(rec)
        finally:
            eng.close()
    out = dict(config="configs[4]" if a.dd else "configs[1]", rooms=a.rooms, steps=a.steps, warmup=a.warmup, profiled=a.profiled, rounds=rounds,
               version=pkg.load_library().lkf_version().decode())
    text = json.dumps(out)
    print(text)
    if a.log:
        with open(os.path.join(ROOT, a.log), "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
