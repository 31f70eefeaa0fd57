"""RTCP demultiplexing on the CPU: no GPU, no HIP runtime.

livekit-server_amd/csrc/rtcp_dmx_unit.cpp is a stand-alone program built with
the host compiler and the address + undefined-behaviour sanitizers over
rtcp_dmx_device.h, the destination-SSRC walk and the routing-table lookup the
kernel k_rtcp_dmx_mark compiles.  It walks every datagram from a heap block of
exactly its length and keeps the bitmap rows in a block of exactly their
words, so an over-read or a stray bit trips the sanitizer.  Its named cases
run one test each; its --replay mode demultiplexes seeded random and mutated
compounds (truncation, version flips, length edits, inflated REMB counts)
whose every result field and entry must equal tests/rtcp_demux_lib.PyRtcpDemux,
the restatement written from include/lkfwd.h.  The seeds the GPU tests use are
vetted here with the restatement alone.  The rest checks the ABI structs
against a C program, the ctypes mirror and the exported symbols.

(The LKF_EINVAL paths need an engine, and an engine needs a device:
tests/test_rtcp_demux_gpu.py covers them.)
"""
import ctypes as C
import os
import subprocess

import pytest

from tests import rtcp_demux_lib as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "livekit-server_amd", "csrc")
EXE = os.path.join(ROOT, "livekit-server_amd", "lib", "rtcp_dmx_unit")


def _names():
    subprocess.run(["make", "-s", "-C", CSRC, "rtcp_dmx_unit"], check=True)
    out = subprocess.run([EXE, "--list"], check=True, capture_output=True, text=True).stdout
    return [x for x in out.split() if x]


NAMES = _names()
INVENTORY = ("empty", "rr_blocks", "sr_blocks_then_sender", "nack_twcc_pli_media", "rrr_sli_media", "rrr_sli_short",
             "fir_entries", "remb_list", "others_none", "duplicate_ssrc_one_entry", "malformed_after_valid",
             "unrouted_other_transport", "same_ssrc_two_transports", "highest_handle_wins", "bitmap_word_boundaries",
             "order_by_dt_then_dgram", "find_edges")


def test_unit_inventory():
    for want in INVENTORY:
        assert want in NAMES, want


@pytest.mark.parametrize("name", NAMES)
def test_unit(name):
    r = subprocess.run([EXE, name], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert ("PASS " + name) in r.stdout


# ---- --replay against the restatement ---------------------------------------------------
def _topology_with_duplicates():
    """The tests' topology plus DownTracks that repeat a key of transports 3 and 5 (a higher handle, which
    wins) and inactive or unbound ones (which the table does not hold)."""
    topo = D.topology()
    rows = [(dt, ssrc, t, True) for dt, ssrc, t in topo]
    by = D.ssrcs_by_transport(topo)
    nxt = len(rows)
    for t in (3, 5, 5):
        rows.append((nxt, by[t][nxt % len(by[t])], t, True))
        nxt += 1
    rows.append((nxt, by[4][0], 4, False))      # removed: the lower handle keeps the key
    rows.append((nxt + 1, 0x7777, -1, True))    # unbound
    return topo, rows


SEEDS = (1, 2, 3)


@pytest.mark.parametrize("seed", SEEDS)
def test_replay_equals_restatement(seed):
    topo, rows = _topology_with_duplicates()
    table = D.build_table(rows)
    assert len(table) == D.NDTS  # the duplicates replaced, nothing added
    dgrams = D.random_datagrams(seed, 340, topo)
    want_res, want_entries = D.PyRtcpDemux.call(table, dgrams)
    D.assert_shares(want_res)
    dup_winners = sorted(table.values())[-3:]
    script = "".join("d %d %d %d\n" % (t, ssrc, dt) for dt, ssrc, t, active in rows if active and t >= 0)
    # in three calls, so that the datagram indices restart
    cuts = (0, 100, 101, len(dgrams))
    for a, b in zip(cuts, cuts[1:]):
        script += "".join("g %d %s\n" % (t, d.hex() or "-") for t, d in dgrams[a:b]) + "run\n"
    r = subprocess.run([EXE, "--replay"], input=script, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = r.stdout.splitlines()
    assert len(got) == len(dgrams) + 3
    at, seen = 0, set()
    for a, b in zip(cuts, cuts[1:]):
        res, entries = D.PyRtcpDemux.call(table, dgrams[a:b])
        assert res == want_res[a:b]
        for i, w in enumerate(res):
            assert got[at + i] == "r status=%d dests=%d unrouted=%d entries=%d" % w, (seed, a + i, dgrams[a + i][1].hex())
        assert got[at + b - a] == "x " + (",".join("%d:%d" % e for e in entries) or "-"), (seed, a)
        assert sum(w[3] for w in res) == len(entries)
        seen |= set(d for d, _ in entries)
        at += b - a + 1
    assert len(want_entries) == sum(w[3] for w in want_res)
    assert seen & set(dup_winners), "no datagram reached a DownTrack that won a duplicate key"


def test_gpu_seed_keeps_its_shares():
    """The random trace of tests/test_rtcp_demux_gpu.py, with the restatement alone."""
    topo = D.topology()
    table = D.build_table([(dt, ssrc, t, True) for dt, ssrc, t in topo])
    assert len(table) == D.NDTS == 171
    assert [sum(1 for _, _, t in topo if t == k) for k in range(6)] == list(D.COUNTS)
    assert any(dt > dt2 and s < s2 for dt, s, t in topo for dt2, s2, t2 in topo if t == t2 == 3)  # handle != SSRC order
    both = set(s for _, s, t in topo if t == 4) & set(s for _, s, t in topo if t == 5)
    assert len(both) == 65
    dgrams = D.random_datagrams(D.GPU_SEED, D.GPU_N, topo)
    res, entries = D.PyRtcpDemux.call(table, dgrams)
    D.assert_shares(res)
    assert entries == sorted(entries) and len(set(entries)) == len(entries)
    for t in (3, 4, 5):  # bits in every word of the wide transports' bitmap rows
        rank = {dt: k for k, (s, dt) in enumerate(sorted((s, dt) for (tt, s), dt in table.items() if tt == t))}
        words = set(rank[d] // 32 for d, i in entries if dgrams[i][0] == t)
        assert words == set(range((D.COUNTS[t] + 31) // 32)), (t, words)


# ---- ABI ------------------------------------------------------------------------------------
def test_struct_sizes(abi, tmp_path):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "include/lkfwd.h"
int main(void){printf("%zu %zu %zu %zu %zu\n", sizeof(lkf_rtcp_dmx_result), sizeof(lkf_rtcp_entry),
 offsetof(lkf_rtcp_dmx_result, dests), offsetof(lkf_rtcp_dmx_result, unrouted), offsetof(lkf_rtcp_dmx_result, entries));
 printf("%d %d %d\n", LKF_RTCP_DMX_OK, LKF_RTCP_DMX_EMPTY, LKF_RTCP_DMX_MALFORMED);return 0;}
'''
    exe = str(tmp_path / "lkf_rtcp_dmx_sizes")
    with open(exe + ".c", "w") as f:
        f.write(src)
    subprocess.run(["gcc", "-I", ROOT, "-o", exe, exe + ".c"], check=True)
    lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()
    py = [C.sizeof(abi.lkf_rtcp_dmx_result), C.sizeof(abi.lkf_rtcp_entry), abi.lkf_rtcp_dmx_result.dests.offset,
          abi.lkf_rtcp_dmx_result.unrouted.offset, abi.lkf_rtcp_dmx_result.entries.offset]
    assert list(map(int, lines[0].split())) == py == [16, 8, 4, 8, 12]
    assert list(map(int, lines[1].split())) == [abi.LKF_RTCP_DMX_OK, abi.LKF_RTCP_DMX_EMPTY,
                                                abi.LKF_RTCP_DMX_MALFORMED] == [D.DMX_OK, D.DMX_EMPTY, D.DMX_MALFORMED]
    assert abi.RTCP_DMX_RESULT_DTYPE.itemsize == 16
    assert [abi.RTCP_DMX_RESULT_DTYPE.fields[f][1] for f in ("status", "dests", "unrouted", "entries")] == [0, 4, 8, 12]


def test_symbols_exported_and_bound(pkg):
    names = ("set_downtrack_rtcp_transport", "rtcp_demux", "rtcp_demux_unprotected")
    for so in ("liblkfwd.so", "liblkfwd_checked.so"):
        lib = os.path.join(ROOT, "livekit-server_amd", "lib", so)
        out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
        exported = set(l.split()[-1] for l in out.splitlines() if l.strip())
        for s in names:
            assert "lkf_" + s in exported, (so, s)
    api = pkg.abi.bind_engine_api(pkg.load_library(), "lkf_")
    for k in names:
        assert k in api, k
        assert callable(getattr(pkg.Engine, k))
