"""bench.py's multi-GPU launcher, rehearsed on the CPU.

`python bench.py --gpus 2` with no torch.distributed environment must start
two ranks itself (the parent touches no GPU), shard the rooms, run the room
manager's summary all-gathers every 400 ms of media inside the loop, reduce
the time over ranks and print one line with n_gpus = 2.  `--dry-run` puts the
CPU oracle (tests/dryrun_engine.py) behind the engine methods and uses gloo,
so the launcher, the room plan, the gathers and the parity reduction are
exercised here; the forwarded totals of the two ranks must equal one process
forwarding all their rooms.
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args, timeout=300):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR",
                                                             "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(args), cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.parametrize("config,rooms", [(1, 1), (3, 1)])
def test_launcher_two_ranks_matches_one_process(config, rooms):
    common = ["--dry-run", "--full", "--config", str(config), "--steps", "2", "--warmup", "1", "--cpu-threads", "2"]
    two = _bench("--gpus", "2", "--rooms", str(rooms), *common)
    one = _bench("--gpus", "1", "--rooms", str(2 * rooms), "--no-cpu-baseline", *common)
    assert two["n_gpus"] == 2 and one["n_gpus"] == 1
    assert two["dry_run"] is True
    assert two["parity"] is True and two["parity_gate"]["parity_all_ranks"] is True
    assert two["forwarded_total"] == one["forwarded_total"] > 0
    c = two["collective"]
    assert c["update_ms"] == 400.0
    # 3 s of media: ticks at 0.4 .. 2.8 s, 5 of them after the 1-s warmup batch
    assert c["ticks"] == 7 and c["ticks_in_timed_region"] == 5
    assert c["rooms_gathered"] == 2 * rooms
    assert c["subscribers_gathered"] > 0
    if config == 3:  # the audio-heavy config ranks speakers
        assert c["rooms_with_speakers"] > 0
    cb = two["cpu_baseline"]
    assert cb["cores"] % 2 == 0 and cb["value"] > 0 and cb["per_rank_value"] > 0  # (threads used x 2 ranks)


def test_plain_run_dumps_last_step(tmp_path):
    """A plain run (no --full) leaves the CPU baseline and the parity gate out
    and, with --dump-outputs, writes the last timed step's records and wire
    bytes as float arrays, the same from run to run (here from the dry-run
    engine, which has the engine's drain call)."""
    import numpy as np
    args = ["--dry-run", "--gpus", "1", "--config", "1", "--steps", "2", "--warmup", "1"]
    a = _bench(*args, "--dump-outputs", str(tmp_path / "a"))
    b = _bench(*args, "--dump-outputs", str(tmp_path / "b"))
    assert a["steps"] == 2 and a["ms_per_step"] > 0
    assert a["cpu_baseline"] is None and a["parity"] is None and a["parity_gate"] is None
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["out_bytes.npy", "out_bytes_idx.npy", "out_records.npy", "out_records_idx.npy",
                     "out_totals.npy"]
    arrs = {n: np.load(tmp_path / "a" / n) for n in names}
    for n in names:
        assert arrs[n].dtype in (np.float32, np.float64), n
        assert np.array_equal(arrs[n], np.load(tmp_path / "b" / n)), n
    assert sum(x.nbytes for x in arrs.values()) <= 64 << 20
    nrec, nbytes = (int(x) for x in arrs["out_totals.npy"])
    assert 0 < nrec <= a["forwarded_total"]
    rec = arrs["out_records.npy"]
    assert rec.shape == (nrec, 9) and arrs["out_bytes.npy"].shape == (1, nbytes)
    assert 0 < (rec[:, 2] + rec[:, 5]).max() <= nbytes  # every record's out_off + out_len lies in the wire bytes


def test_steps_beyond_one_round_run_in_rounds():
    """--steps beyond bench.ROUND_STEPS (64) runs in rounds, each on a fresh
    engine over the same warmup batches and the timed batches after them: 65
    steps are a round of 32 and one of 33 (the uneven split), and forward what
    a 32-step run and a 33-step run forward together, with their tuples and
    bytes.  The parity gate checks the last, longer round."""
    args = ["--dry-run", "--full", "--no-cpu-baseline", "--gpus", "1", "--config", "1", "--warmup", "2"]
    a, b = _bench(*args, "--steps", "32"), _bench(*args, "--steps", "33")
    two = _bench(*args, "--steps", "65")
    assert (a["rounds"], b["rounds"], two["steps"], two["rounds"]) == (1, 1, 65, 2)
    assert two["forwarded_total"] == a["forwarded_total"] + b["forwarded_total"] > 0
    # exact where the three runs see the same input: tuples, and the decide kernel's bytes (packet descriptors,
    # forwarded tuples, DownTracks); the payload bytes of the 32-step run's last batch are those of a trace that
    # ends one second sooner, so the totals may differ by less than one step's bytes
    tup, dec, byt = ([f(x) * x["steps"] for x in (a, b, two)] for f in (
        lambda x: x["tuples_per_step"], lambda x: x["roofline"]["kernels"][0]["algorithmic_bytes_per_launch"],
        lambda x: x["roofline"]["algorithmic_bytes_per_step"]))
    assert tup[2] == tup[0] + tup[1] and dec[2] == dec[0] + dec[1]
    assert abs(byt[2] - byt[0] - byt[1]) < a["roofline"]["algorithmic_bytes_per_step"]
    assert a["parity"] is True and b["parity"] is True and two["parity"] is True
    assert two["parity_gate"]["batches"] == 35 and two["parity_gate"]["forwarded_total"] == \
        b["parity_gate"]["forwarded_total"]
    assert set(two["round_ms_per_step"]) == {"min", "max"} and two["outside_steps_s"] >= 0


def test_dump_outputs_samples_large_output(tmp_path, abi, monkeypatch):
    """Beyond its caps --dump-outputs keeps a seeded sample: the records at
    out_records_idx and the runs of wire bytes that start at out_bytes_idx."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(bench, "DUMP_RECORDS", 100)
    monkeypatch.setattr(bench, "DUMP_CHUNKS", 8)
    monkeypatch.setattr(bench, "DUMP_CHUNK", 16)
    recs = np.zeros(1000, dtype=abi.OUT_DTYPE)
    recs["ext_sn"] = (1 << 40) + np.arange(1000)
    recs["layer"] = -1
    arena = (np.arange(10000) % 251).astype(np.uint8)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), recs, arena)
    got = {n[:-4]: np.load(tmp_path / "a" / n) for n in os.listdir(tmp_path / "a")}
    for n, a in got.items():
        assert np.array_equal(a, np.load(tmp_path / "b" / (n + ".npy"))), n
    assert got["out_totals"].tolist() == [1000.0, 10000.0]
    ri, bi = got["out_records_idx"].astype(np.int64), got["out_bytes_idx"].astype(np.int64)
    assert ri.shape == (100,) and np.all(np.diff(ri) >= 0) and 0 <= ri.min() and ri.max() < 1000
    assert got["out_records"].shape == (100, 9)
    assert np.array_equal(got["out_records"][:, 0], (1 << 40) + ri) and np.all(got["out_records"][:, 7] == -1)
    assert bi.shape == (8,) and 0 <= bi.min() and bi.max() + 16 <= 10000
    assert got["out_bytes"].dtype == np.float32
    assert np.array_equal(got["out_bytes"], (bi[:, None] + np.arange(16)) % 251)


def test_tick_times():
    sys.path.insert(0, ROOT)
    import bench
    assert bench.tick_times(0, 1.0, 400) == pytest.approx([0.4, 0.8])
    assert bench.tick_times(1, 1.0, 400) == pytest.approx([1.2, 1.6, 2.0])
    assert bench.tick_times(2, 1.0, 400) == pytest.approx([2.4, 2.8])
    assert bench.tick_times(0, 0.01, 400) == []
    assert bench.tick_times(39, 0.01, 400) == pytest.approx([0.4])
    assert bench.tick_times(3, 1.0, 0) == []
