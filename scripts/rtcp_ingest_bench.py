#!/usr/bin/env python3
"""What RTCP ingress costs per tick, on the GPU path and on the host path.

Workload: at configs[1]'s benched DownTrack count, one compound packet per
DownTrack: RR (one block for the DownTrack) + NACK with three pairs + SDES.
The engine holds that many DownTracks that have forwarded nothing (the
reports are then ignored by UpdateFromReceiverReport and the lookups find no
record, on both paths alike), so the figures are the cost of moving, parsing,
regrouping and dispatching the feedback, not of the statistics behind it.

  gpu path    lkf_rtcp_ingest + lkf_rtx_lookup_ingested
  host path   rtcp_in_bench --bench (rtcp_in_device.h compiled for the host,
              one thread, producing lkf_rtcp_fb[] / lkf_nack[]), then
              lkf_rtcp_feedback + lkf_rtx_lookup of those arrays

The two paths alternate tick by tick (a GPU tick, then a host tick: one parse
in the rtcp_in_bench child, timed inside it, plus the two struct calls).
Warm-up ticks first, then min / median / max of the timed ticks of each path
(wall clock around calls that return with their results on the host).  One
JSON line; --log appends it to a file under profiles/.

  python scripts/rtcp_ingest_bench.py [--dts N] [--ticks 500] [--warmup 20] [--log profiles/rtcp_ingest_bench.log]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch  # noqa: F401  (first: one HIP runtime in the process, as bench.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import rtcp_wire_lib as W  # noqa: E402


def benched_dts(workload):
    """The DownTrack count bench.py runs configs[1] at: config 2's default 100 rooms per GPU."""
    tr = workload.Trace(2, rooms=100, duration_s=1.0, batch_s=1.0)
    try:
        return int(tr.ndts)
    finally:
        tr.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dts", type=int, default=0)
    ap.add_argument("--ticks", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--log", default="")
    a = ap.parse_args()
    pkg = importlib.import_module("livekit-server_amd")
    workload = importlib.import_module("livekit-server_amd.workload")
    abi = pkg.abi
    n = a.dts or benched_dts(workload)

    eng = pkg.Engine(max_tracks=8, max_downtracks=n + 8, max_batch_pkts=1024, max_batch_arena=1 << 20,
                     max_out_pkts=1 << 16, max_out_bytes=1 << 24, max_batch_tuples=1 << 16)
    try:
        tp = abi.lkf_track_params()
        tp.kind, tp.clock_rate = abi.LKF_KIND_VIDEO, 90000
        track = eng.api["add_track"](eng.h, C.byref(tp))
        assert track >= 0, track
        dp = abi.lkf_downtrack_params()
        dp.track = track
        for i in range(n):
            dp.ssrc = 1000 + i
            assert eng.api["add_downtrack"](eng.h, C.byref(dp)) == i
        # the compounds, as rtcp_in_bench --bench builds them
        sd = W.sdes(1)
        parts, raws, off = [], np.zeros(n, dtype=abi.RTCP_RAW_DTYPE), 0
        for i in range(n):
            ssrc = 1000 + i
            c = W.compound(W.rr(ssrc ^ 0x5a5a, [W.report_block(ssrc, 1, i & 0xff, 5000 + i, i & 0x3ff)]),
                           W.nack(ssrc ^ 0x5a5a, ssrc, [(i & 0xffff, 5), ((i + 40) & 0xffff, 0),
                                                        ((i + 90) & 0xffff, 0x8000)]), sd)
            raws[i] = (i, off, len(c))
            parts.append(c)
            off += len(c)
        arena = np.frombuffer(b"".join(parts), dtype=np.uint8)
        now = 1700000000 * 10**9

        # the host path's arrays (what its parse produces), from one untimed call of the GPU path
        out, fb, fbo, refs, nn = eng.rtcp_ingest(raws, arena, now)
        rtx = eng.rtx_lookup_ingested(now)
        assert int(out["status"].max()) == 0 and len(fb) == n and nn == 6 * n
        ent = np.zeros(n, dtype=abi.RTCP_FB_DTYPE)
        ent[:] = fb
        nacks = eng.rtcp_ingested_nacks()
        rout = np.zeros(max(1, len(nacks)), dtype=abi.RTX_DTYPE)
        k = C.c_uint32()
        exe = os.path.join(ROOT, "livekit-server_amd", "lib", "rtcp_in_bench")
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "livekit-server_amd", "csrc"), "rtcp_in_bench"],
                       check=True)
        total = a.warmup + a.ticks
        parser = subprocess.Popen([exe, "--bench", str(n), str(total), "step"], stdin=subprocess.PIPE,
                                  stdout=subprocess.PIPE, text=True)
        # the two paths alternate tick by tick, so that drift hits both alike
        gpu, parse, calls = [], [], []
        try:
            for t in range(total):
                t0 = time.perf_counter()
                out, fb, fbo, refs, nn = eng.rtcp_ingest(raws, arena, now + 1 + 2 * t)
                rtx = eng.rtx_lookup_ingested(now + 1 + 2 * t)
                gpu.append((time.perf_counter() - t0) * 1e3)
                parser.stdin.write("\n")
                parser.stdin.flush()
                parse.append(float(parser.stdout.readline().split("=")[1]))  # (timed inside the program)
                t0 = time.perf_counter()
                eng.rtcp_feedback(ent, now + 2 + 2 * t)
                rc = eng.api["rtx_lookup"](eng.h, nacks.ctypes.data, len(nacks), now + 2 + 2 * t, rout.ctypes.data,
                                           len(rout), C.byref(k))
                calls.append((time.perf_counter() - t0) * 1e3)
                assert rc == 0
        finally:
            parser.stdin.close()
            parser.wait()
        g, ps, c = gpu[a.warmup:], parse[a.warmup:], calls[a.warmup:]
        host = [x + y for x, y in zip(ps, c)]  # a host tick: its parse and its two calls

        def mmm(v):
            return dict(min=round(min(v), 3), median=round(statistics.median(v), 3), max=round(max(v), 3))

        rec = dict(
            downtracks=n, ticks=a.ticks, warmup=a.warmup, gpu_ms=mmm(g), host_ms=mmm(host), host_parse_ms=mmm(ps),
            host_calls_ms=mmm(c),
            gpu_bytes_up=int(raws.nbytes + arena.nbytes),
            gpu_bytes_down=int(out.nbytes + fb.nbytes + fbo.nbytes + refs.nbytes + rtx.nbytes),
            host_bytes_up=int(ent.nbytes + nacks.nbytes),
            host_bytes_down=int(len(ent) * abi.RTCP_FB_RESULT_DTYPE.itemsize + int(k.value) * abi.RTX_DTYPE.itemsize),
            version=pkg.load_library().lkf_version().decode())
        text = json.dumps(rec)
        print(text)
        if a.log:
            with open(os.path.join(ROOT, a.log), "a") as f:
                f.write(text + "\n")
    finally:
        eng.close()


if __name__ == "__main__":
    main()
