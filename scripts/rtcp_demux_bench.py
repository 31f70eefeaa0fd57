#!/usr/bin/env python3
"""What routing subscribers' RTCP costs per tick, on the GPU and on the host.

Workload: at configs[1]'s benched DownTrack count, one sealed compound per
DownTrack per tick: RR (one block for the DownTrack) + NACK with three pairs +
SDES, from the subscriber's own SSRC.  --per-transport DownTracks share one
receive transport (one subscriber PeerConnection); every second transport is
AEAD_AES_128_GCM.  The engine holds that many DownTracks that have forwarded
nothing, as scripts/rtcp_ingest_bench.py does, so the figures are the cost of
opening, routing and dispatching the feedback, not of the statistics behind
it.  The datagrams of every tick are sealed afresh (lkf_srtcp_protect on the
same keys, untimed), so the replay check accepts them.

  gpu path    lkf_srtcp_unprotect(plain = NULL) + lkf_rtcp_demux_unprotected +
              lkf_rtcp_ingest_unprotected of its entries
  host path   lkf_srtcp_unprotect with the plaintext copied back, the walk and
              the table lookup in rtcp_dmx_bench --bench (rtcp_dmx_device.h
              compiled for the host, one thread, over compounds of the same
              shape, timed inside it), then the same ingest

The two paths alternate tick by tick.  Warm-up ticks first, then min / median
/ max of the timed ticks of each path (wall clock around calls that return
with their results on the host), and the device -> host bytes of one tick.
One JSON line; --log appends it to a file under profiles/.

  python scripts/rtcp_demux_bench.py [--dts N] [--per-transport 20] [--ticks 200] [--warmup 10] [--log profiles/rtcp_demux_bench.log]
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
from tests import srtcp_lib as L  # noqa: E402


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
    ap.add_argument("--per-transport", type=int, default=20)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--log", default="")
    a = ap.parse_args()
    pkg = importlib.import_module("livekit-server_amd")
    workload = importlib.import_module("livekit-server_amd.workload")
    abi = pkg.abi
    n = a.dts or benched_dts(workload)
    nt = (n + a.per_transport - 1) // a.per_transport

    eng = pkg.Engine(max_tracks=8, max_downtracks=n + 8, max_batch_pkts=1024, max_batch_arena=1 << 20,
                     max_out_pkts=1 << 16, max_out_bytes=1 << 24, max_batch_tuples=1 << 16)
    try:
        for t, (mk, ms, prof) in enumerate(L.make_keys(nt)):
            assert eng.api["add_transport"](eng.h, C.byref(pkg.transport_params(mk, ms, prof))) == t
        tp = abi.lkf_track_params()
        tp.kind, tp.clock_rate = abi.LKF_KIND_VIDEO, 90000
        track = eng.api["add_track"](eng.h, C.byref(tp))
        assert track >= 0, track
        dp = abi.lkf_downtrack_params()
        dp.track = track
        for i in range(n):
            dp.ssrc = 1000 + i
            assert eng.api["add_downtrack"](eng.h, C.byref(dp)) == i
            eng.set_downtrack_rtcp_transport(i, i % nt)
        # the compounds, as rtcp_dmx_bench --bench builds them: DownTrack i on transport i % nt
        parts, raws, off = [], np.zeros(n, dtype=abi.SRTCP_RAW_DTYPE), 0
        for i in range(n):
            ssrc, t = 1000 + i, i % nt
            c = W.compound(W.rr(0x70000000 + t, [W.report_block(ssrc, 1, i & 0xff, 5000 + i, i & 0x3ff)]),
                           W.nack(0x70000000 + t, ssrc, [(i & 0xffff, 5), ((i + 40) & 0xffff, 0),
                                                         ((i + 90) & 0xffff, 0x8000)]), W.sdes(0x70000000 + t))
            raws[i] = (t, off, len(c))
            parts.append(c)
            off += len(c)
        plain = np.frombuffer(b"".join(parts), dtype=np.uint8)
        now = 1700000000 * 10**9

        def sealed():
            """A tick's datagrams: the same compounds under the next SRTCP indices."""
            res, out = eng.srtcp_protect(raws, plain)
            rw = np.zeros(n, dtype=abi.SRTCP_RAW_DTYPE)
            rw["transport"], rw["off"], rw["len"] = raws["transport"], res["off"], res["len"]
            return rw, out

        # one untimed tick of the GPU path: what both paths must produce
        rw, ar = sealed()
        res, _ = eng.srtcp_unprotect(rw, ar, want_plain=False)
        assert int(res["status"].max()) == abi.LKF_SRTCP_RX_OK, res["status"].max()
        dres, entries = eng.rtcp_demux_unprotected()
        assert (dres["entries"] == 1).all() and (dres["unrouted"] == 0).all()
        assert (entries["dt"] == np.arange(n)).all() and (entries["dgram"] == np.arange(n)).all()
        out, fb, fbo, refs, nn = eng.rtcp_ingest_unprotected(entries, now)
        assert int(out["status"].max()) == 0 and len(fb) == n and nn == 6 * n
        ingest_down = int(out.nbytes + fb.nbytes + fbo.nbytes + refs.nbytes)
        host_entries = entries.copy()  # what the host walk yields for this workload

        exe = os.path.join(ROOT, "livekit-server_amd", "lib", "rtcp_dmx_bench")
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "livekit-server_amd", "csrc"), "rtcp_dmx_bench"],
                       check=True)
        total = a.warmup + a.ticks
        walker = subprocess.Popen([exe, "--bench", str(n), str(nt), str(total), "step"], stdin=subprocess.PIPE,
                                  stdout=subprocess.PIPE, text=True)
        gpu, walk, calls = [], [], []
        try:
            for t in range(total):
                rw, ar = sealed()
                t0 = time.perf_counter()
                eng.srtcp_unprotect(rw, ar, want_plain=False)
                _, ent = eng.rtcp_demux_unprotected()
                eng.rtcp_ingest_unprotected(ent, now + 1 + 2 * t)
                gpu.append((time.perf_counter() - t0) * 1e3)
                assert len(ent) == n
                rw, ar = sealed()
                t0 = time.perf_counter()
                eng.srtcp_unprotect(rw, ar, want_plain=True)
                t1 = time.perf_counter()
                walker.stdin.write("\n")
                walker.stdin.flush()
                walk.append(float(walker.stdout.readline().split("=")[1]))  # (timed inside the program)
                t2 = time.perf_counter()
                eng.rtcp_ingest_unprotected(host_entries, now + 2 + 2 * t)
                calls.append((t1 - t0 + time.perf_counter() - t2) * 1e3)
        finally:
            walker.stdin.close()
            walker.wait()
        g, ws, c = gpu[a.warmup:], walk[a.warmup:], calls[a.warmup:]
        host = [x + y for x, y in zip(ws, c)]  # a host tick: its two calls and its walk

        def mmm(v):
            return dict(min=round(min(v), 3), median=round(statistics.median(v), 3), max=round(max(v), 3))

        rec = dict(
            downtracks=n, transports=nt, ticks=a.ticks, warmup=a.warmup, datagram_bytes=int(len(ar)),
            gpu_ms=mmm(g), host_ms=mmm(host), host_walk_ms=mmm(ws), host_calls_ms=mmm(c),
            gpu_bytes_down=int(res.nbytes + dres.nbytes + entries.nbytes + ingest_down),
            host_bytes_down=int(res.nbytes + len(ar) + ingest_down),
            of_which_ingest_bytes_down=ingest_down,
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
