"""The engine's pure host pieces on the CPU (no GPU, no HIP runtime).

livekit-server_amd/csrc/host_unit.cpp is a stand-alone program built with the
host compiler and the address + undefined-behaviour sanitizers.  It tests
DevBuf (dev_buf.h) over a malloc-backed fake of the two allocation functions
(floors, no reallocation below the capacity, a failed grow leaving the buffer
empty and retried, move-assignment freeing once, allocations == frees, a
scratch family shared by calls of opposite shapes settling on one size), the
control-op CSR (ctl_csr.h) against std::stable_sort by (lane, at_pkt), and the
control calls' handle-list check (handles.h: range, repeats under each policy,
inactive handles, strides, the first offender deciding the code).  Each
case runs as its own test; a sanitizer report fails the case it occurs in.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "livekit-server_amd", "csrc")
EXE = os.path.join(ROOT, "livekit-server_amd", "lib", "host_unit")


def _names():
    subprocess.run(["make", "-s", "-C", CSRC, "host_unit"], check=True)  # (up to date after build(): a no-op)
    out = subprocess.run([EXE, "--list"], check=True, capture_output=True, text=True).stdout
    return [x for x in out.split() if x]


NAMES = _names()


def test_host_unit_inventory():
    assert sum(n.startswith("devbuf_") for n in NAMES) >= 6
    assert sum(n.startswith("csr_") for n in NAMES) >= 7
    assert sum(n.startswith("handles_") for n in NAMES) >= 9
    for nl in ("200", "300", "70000"):  # one, two and three radix passes
        assert "csr_nl_" + nl in NAMES


@pytest.mark.parametrize("name", NAMES)
def test_host_unit(name):
    r = subprocess.run([EXE, name], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert ("PASS " + name) in r.stdout
