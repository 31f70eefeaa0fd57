#!/usr/bin/env python3
"""One RTCP tick over every DownTrack of configs[1], timed on the host.

After --batches 1-s batches at --rooms rooms: one lkf_rtcp_feedback with a
receiver report for every DownTrack, one lkf_rtcp_sender_reports and one
lkf_sender_delta_info, each as the median wall-clock time of --reps calls
after --warmup calls (time.perf_counter around the call: the calls wait for
their results, so the host time is the whole cost).  Each feedback call
acknowledges 32 more packets than the one before it, up to the highest
sequence number sent, so its reports are accepted and its intervals are not
empty.

The comparison, in the same process: the only way to read one interval's
statistics without these calls is lkf_sender_sninfo once per sequence number.
That is timed for the interval of one DownTrack (the packets of its last
batch) and scaled to every DownTrack's interval of that batch.

Prints one JSON line (and writes it to --out).
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch  # noqa: F401  (one HIP runtime per process: torch first)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EPOCH = 1700000000 * 10**9


def median_ms(fn, warmup, reps):
    for i in range(warmup):
        fn(i)
    ts = []
    for i in range(reps):
        t0 = time.perf_counter()
        fn(warmup + i)
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rooms", type=int, default=100)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    pkg = importlib.import_module("livekit-server_amd")
    wl = importlib.import_module("livekit-server_amd.workload")
    abi = pkg.abi
    # (one second more than is run: the generator's last batch is a short remainder)
    trace = wl.Trace(2, duration_s=float(args.batches + 1), batch_s=1.0, rooms=args.rooms)
    nb = min(args.batches, trace.nbatches)
    eng = pkg.Engine.for_trace(trace)
    wl.load_topology(eng.api, eng.h, trace)
    before = None
    for b in range(nb):
        if b == nb - 1:
            eng.sync()
            before = pkg.sender_stats(eng.api, eng.h, range(min(200, trace.ndts)))["ext_highest_sn"].astype(np.int64)
        wl.queue_events(eng.api, eng.h, trace, b)
        pk, n, ar, alen = trace.batch(b)
        eng.submit(pk, n, ar, alen)
        eng.run()
    eng.sync()
    forwarded = int(eng.stats()["forwarded"])

    ndts = trace.ndts
    dts = np.arange(ndts, dtype=np.int32)
    ss = pkg.sender_stats(eng.api, eng.h, dts)
    live = ss["initialized"] != 0
    start, high = ss["ext_start_sn"].astype(np.uint64), ss["ext_highest_sn"].astype(np.uint64)
    base = start & ~np.uint64(0xFFFF)
    calls = args.warmup + args.reps
    ent = np.zeros(ndts, dtype=abi.RTCP_FB_DTYPE)
    ent["dt"] = dts
    ent["flags"] = abi.LKF_FB_HAS_RR

    def feedback(i):  # call i acknowledges up to 32 * (calls - 1 - i) packets short of the highest
        back = np.minimum(np.uint64(32 * (calls - 1 - i)), high - start)
        ent["last_sequence_number"] = ((high - back - base) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        ent["jitter"] = 100 + i
        return eng.rtcp_feedback(ent, EPOCH + args.batches * 10**9 + i * 10**7)

    fb = median_ms(feedback, args.warmup, args.reps)
    last = feedback(calls - 1)
    ignored = int(((last["flags"] & abi.LKF_FB_IGNORED) != 0)[live].sum())

    req = np.zeros(ndts, dtype=abi.RTCP_SR_REQ_DTYPE)
    req["dt"] = dts
    sr = median_ms(lambda i: eng.rtcp_sender_reports(req, EPOCH + (args.batches + 1) * 10**9 + i * 10**7, wire=True),
                   args.warmup, args.reps)
    di = median_ms(lambda i: eng.sender_delta_info(dts), args.warmup, args.reps)

    # today's alternative: one lkf_sender_sninfo per sequence number of an interval.  Timed over the last-batch
    # interval of the DownTrack (of the first 200) that sent most in it; every DownTrack's last-batch interval
    # together holds as many sequence numbers as the batch forwarded packets (lkf_get_stats), so the whole
    # tick by this route costs that many calls.
    info = C.c_uint32()
    sent = high[:len(before)].astype(np.int64) - before
    one_dt = int(np.argmax(sent))
    lo, hi = int(before[one_dt]) + 1, int(high[one_dt])

    def by_sninfo(_):
        for esn in range(lo, hi + 1):
            rc = eng.api["sender_sninfo"](eng.h, one_dt, esn, C.byref(info))
            assert rc == 0, rc

    one = median_ms(by_sninfo, 1, 5)
    per_sn_ms = one[0] / max(1, hi - lo + 1)
    res = {
        "rooms": args.rooms, "downtracks": int(ndts), "downtracks_sending": int(live.sum()),
        "batches": args.batches, "reps": args.reps, "packets_acknowledged_per_feedback_call": 32,
        "rtcp_feedback_ms": {"median": fb[0], "min": fb[1], "max": fb[2]},
        "rtcp_feedback_ignored_in_last_call": ignored,
        "rtcp_sender_reports_ms": {"median": sr[0], "min": sr[1], "max": sr[2]},
        "sender_delta_info_ms": {"median": di[0], "min": di[1], "max": di[2]},
        "sninfo_interval_packets_one_downtrack": hi - lo + 1,
        "sninfo_one_downtrack_ms": {"median": one[0], "min": one[1], "max": one[2]},
        "sninfo_per_sequence_number_ms": per_sn_ms,
        "forwarded_in_last_batch": forwarded,
        "sninfo_all_downtracks_ms_extrapolated": per_sn_ms * forwarded,
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    eng.close()
    trace.close()


if __name__ == "__main__":
    main()
