"""Prefix egress without a GPU: the C-ABI of lkf_pre and the new entry points,
and the test-side model (tests/prefix_lib.py) against the oracle — for every
wire packet the oracle produces, "prefix ++ unchanged slice of the input that
ends at the end of the input payload" must rebuild it exactly."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import prefix_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["lkf_set_egress", "lkf_drain_prefix", "lkf_drain_prefix_run", "lkf_output_prefix_device"]

# (Trace args, Trace kwargs): the six traces of the prefix egress tests
TRACES = [
    ((2,), dict(duration_s=3, batch_s=1, rooms=3, seed=8, twcc=1)),
    ((1,), dict(duration_s=1, batch_s=1)),
    ((5,), dict(duration_s=2, batch_s=0.5, rooms=3, seed=9, twcc=2)),
    ((5,), dict(duration_s=2, batch_s=0.5, rooms=3, svc_dd=2, seed=61)),
    ((5,), dict(duration_s=2, batch_s=0.5, rooms=3, svc_dd=0, seed=5)),
    ((1,), dict(duration_s=0.2, batch_s=0.01)),
]


def test_lkf_pre_is_48_bytes(abi, tmp_path):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "include/lkfwd.h"
int main(void){printf("%zu %zu %zu %zu %zu %zu %d %d\n", sizeof(lkf_pre), offsetof(lkf_pre, pre_off),
 offsetof(lkf_pre, out_len), offsetof(lkf_pre, pre_len), offsetof(lkf_pre, tail_len), offsetof(lkf_pre, tail_src),
 LKF_EGRESS_WIRE, LKF_EGRESS_PREFIX);return 0;}
'''
    exe = str(tmp_path / "lkf_pre_size")
    with open(exe + ".c", "w") as f:
        f.write(src)
    subprocess.run(["gcc", "-I", ROOT, "-o", exe, exe + ".c"], check=True)
    got = list(map(int, subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()))
    d = abi.PRE_DTYPE
    assert got == [48, d.fields["pre_off"][1], d.fields["out_len"][1], d.fields["pre_len"][1],
                   d.fields["tail_len"][1], d.fields["tail_src"][1], abi.LKF_EGRESS_WIRE, abi.LKF_EGRESS_PREFIX]
    assert C.sizeof(abi.lkf_pre) == 48 == d.itemsize
    for name, (_, off) in ((k, (v[0], v[1])) for k, v in d.fields.items()):
        assert getattr(abi.lkf_pre, name).offset == off, name


def test_library_exports_prefix_entry_points(pkg):
    lib = os.path.join(ROOT, "livekit-server_amd", "lib", "liblkfwd.so")
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    exported = set(l.split()[-1] for l in out.splitlines() if l.strip())
    missing = [s for s in NEW_SYMBOLS if s not in exported]
    assert not missing, missing
    api = pkg.load_library().api
    for k in ("set_egress", "drain_prefix", "drain_prefix_run", "output_prefix_device"):
        assert k in api, k


def test_oracle_still_binds_without_prefix_entry_points(oracle):
    assert "set_egress" not in oracle.api and "drain" in oracle.api


@pytest.mark.parametrize("args,kw", TRACES, ids=[str(i) for i in range(len(TRACES))])
def test_model_rebuilds_oracle_wire(pkg, workload, abi, oracle, args, kw):
    tr = workload.Trace(*args, **kw)
    oh = oracle.create(500)
    records = max_pre = two_byte = 0
    try:
        workload.load_topology(oracle.api, oh, tr)
        for b in range(tr.nbatches):
            workload.queue_events(oracle.api, oh, tr, b)
            pk, n, ar, alen = tr.batch(b)
            dd = tr.batch_dd(b)[0] if tr.has_dd() else None
            oracle.run(oh, pk, n, ar, alen, dd)
            orec, owire = pkg.drain_arrays(oracle.api, oh)
            pkts = prefix_lib.pkts_array(pk, n)
            inp = prefix_lib.arena_array(ar, alen)
            pre, parena = prefix_lib.expected_prefix(tr, pkts, orec, owire)
            assert len(pre) == len(orec)
            if not len(pre):
                assert len(parena) == 0
                continue
            # layout rule
            r16 = prefix_lib.round16(pre["pre_len"].astype(np.int64))
            assert np.array_equal(pre["pre_off"].astype(np.int64), np.cumsum(r16) - r16)
            assert len(parena) == int(r16.sum()) and (pre["pre_off"] % 16 == 0).all()
            assert np.array_equal(pre["pre_len"].astype(np.int64) + pre["tail_len"], orec["out_len"].astype(np.int64))
            # the tail is an unchanged slice of the input that ends at the payload's end
            p = pkts[pre["pkt"]]
            end = p["arena_off"].astype(np.int64) + p["payload_off"] + p["payload_len"]
            assert np.array_equal(pre["tail_src"].astype(np.int64) + pre["tail_len"], end)
            assert (pre["tail_src"].astype(np.int64) >= p["arena_off"].astype(np.int64) + p["payload_off"]).all()
            assert int(end.max()) <= alen
            wire = prefix_lib.reassemble(pre, parena, inp)
            assert wire.shape == owire.shape
            if not np.array_equal(wire, owire):
                bad = int(np.nonzero(wire != owire)[0][0])
                r = int(np.searchsorted(orec["out_off"], bad, side="right") - 1)
                raise AssertionError("batch %d: tail differs from the input slice at wire byte %d (record %d: %s)" % (
                    b, bad, r, pre[r]))
            records += len(pre)
            max_pre = max(max_pre, int(pre["pre_len"].max()))
            ext = owire[orec["out_off"].astype(np.int64) + 12 + 4 * (owire[orec["out_off"].astype(np.int64)] & 15)]
            hasx = (owire[orec["out_off"].astype(np.int64)] & 0x10) != 0
            two_byte += int(np.count_nonzero(hasx & (ext == 0x10)))
    finally:
        oracle.destroy(oh)
        tr.close()
    assert records > 0
    print("records %d max prefix %d two-byte profile %d" % (records, max_pre, two_byte))
    assert max_pre <= 352
