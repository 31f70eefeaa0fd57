"""RTCP ingress on the CPU: no GPU, no HIP runtime.

livekit-server_amd/csrc/rtcp_in_unit.cpp is a stand-alone program built with
the host compiler and the address + undefined-behaviour sanitizers over
rtcp_in_device.h, the scalar parse (framing walk, per-type size checks, NACK
pair expansion) the kernels k_rtcp_in_count / k_rtcp_in_write compile.  It
parses every compound packet from a heap block of exactly its length, so an
over-read trips the sanitizer.  Its named cases run one test each; its
--replay mode parses seeded random and mutated compounds (truncation, byte
flips in headers, length edits) whose every field must equal
tests/rtcp_wire_lib.PyRtcpIn, the restatement written from include/lkfwd.h.
The rest checks the ABI structs against a C program, the ctypes mirror and the
exported symbols.
"""
import ctypes as C
import os
import random
import subprocess

import pytest

from tests import rtcp_wire_lib as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "livekit-server_amd", "csrc")
EXE = os.path.join(ROOT, "livekit-server_amd", "lib", "rtcp_in_unit")
SSRC = 0x5EED0001


def _names():
    subprocess.run(["make", "-s", "-C", CSRC, "rtcp_in_unit"], check=True)
    out = subprocess.run([EXE, "--list"], check=True, capture_output=True, text=True).stdout
    return [x for x in out.split() if x]


NAMES = _names()
INVENTORY = ("empty", "three_bytes", "bad_version", "length_past_end", "rr_rc0", "rr_rc1", "rr_rc31",
             "rr_truncated_block", "two_rr", "rr_two_matching_blocks", "sr_matching_block_ignored", "nack_blp0",
             "nack_blp_ffff", "nack_pid_wrap", "nack_no_pairs", "fir_bad_remainder", "remb_bad_id",
             "remb_numssrc_beyond", "twcc_16_bytes", "twcc_other_ssrc", "unknown_pt_skipped", "malformed_after_valid")


def test_unit_inventory():
    for want in INVENTORY:
        assert want in NAMES, want


@pytest.mark.parametrize("name", NAMES)
def test_unit(name):
    r = subprocess.run([EXE, name], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert ("PASS " + name) in r.stdout


# ---- --replay against the restatement ---------------------------------------------------
def random_packet(rnd, ssrc):
    other = ssrc ^ rnd.randrange(1, 1 << 16)
    who = lambda: ssrc if rnd.random() < 0.6 else other  # noqa: E731
    k = rnd.randrange(13)
    if k == 0:
        blocks = [W.report_block(who(), rnd.randrange(256), rnd.randrange(1 << 24), rnd.randrange(1 << 32),
                                 rnd.randrange(1 << 32), rnd.randrange(1 << 32), rnd.randrange(1 << 32))
                  for _ in range(rnd.choice((0, 1, 1, 2, 3, 31)))]
        return W.rr(other, blocks, extension=b"\xca\xfe\xf0\x0d" if rnd.random() < 0.2 else b"")
    if k == 1:
        return W.sr(other, [W.report_block(who(), lsn=rnd.randrange(1 << 32)) for _ in range(rnd.randrange(3))])
    if k == 2:
        return W.sdes(other, bytes(rnd.randrange(97, 123) for _ in range(rnd.randrange(1, 12))))
    if k == 3:
        return W.bye(*[rnd.randrange(1 << 32) for _ in range(rnd.randrange(3))])
    if k in (4, 5):
        return W.nack(other, who(), [(rnd.choice((0, 65535, rnd.randrange(65536))),
                                      rnd.choice((0, 0xFFFF, 1, 0x8000, rnd.randrange(65536))))
                                     for _ in range(rnd.randrange(5))])
    if k == 6:
        return W.twcc(other, who(), bytes(rnd.randrange(256) for _ in range(4 * rnd.randrange(1, 6))))
    if k == 7:
        return W.pli(other, who())
    if k == 8:
        return W.fir(other, 0, [(who(), rnd.randrange(256)) for _ in range(rnd.randrange(3))])
    if k == 9:
        n = rnd.randrange(4)
        return W.remb(other, ssrcs=[rnd.randrange(1 << 32) for _ in range(n)],
                      ident=b"REMB" if rnd.random() < 0.8 else b"RAMB", num=n if rnd.random() < 0.8 else n + 1)
    if k == 10:
        return W.xr(other)
    if k == 11:  # feedback formats the engine skips
        return W._hdr(rnd.choice((2, 3, 5, 8)), rnd.choice((205, 206)), bytes(rnd.randrange(256) for _ in range(8)))
    return W.unknown(rnd.choice((192, 199, 204, 208, 255)), rnd.randrange(32),
                     bytes(rnd.randrange(256) for _ in range(4 * rnd.randrange(4))))


def mutate(rnd, data, starts):
    """Truncation, a byte flip inside a packet header, or a length edit."""
    b = bytearray(data)
    m = rnd.randrange(4)
    if m == 0 and b:
        del b[rnd.randrange(len(b)):]
    elif m == 1 and starts:
        at = rnd.choice(starts) + rnd.randrange(2)
        b[at] ^= 1 << rnd.randrange(8)
    elif m == 2 and starts:
        at = rnd.choice(starts) + 3
        b[at] = (b[at] + rnd.choice((-2, -1, 1, 2, 7))) & 0xFF
    else:
        b += bytes(rnd.randrange(256) for _ in range(rnd.randrange(1, 4)))
    return bytes(b)


def random_entries(seed, n=400):
    rnd = random.Random(seed)
    out = []
    for _ in range(n):
        pk = [random_packet(rnd, SSRC) for _ in range(rnd.randrange(1, 6))]
        data = W.compound(*pk)
        if rnd.random() < 0.5:
            starts, at = [], 0
            for p in pk:
                starts.append(at)
                at += len(p)
            data = mutate(rnd, data, starts)
            if rnd.random() < 0.3:
                data = mutate(rnd, data, [s for s in starts if s + 4 <= len(data)])
        out.append(data)
    return out


def _expected_line(p):
    fb = ",".join("%d:%d:%d:%d:%d:%d:%d:%d:%d:%d" % (f["last_sequence_number"], f["total_lost"], f["jitter"],
                                                     f["last_sender_report"], f["delay"], f["fraction_lost"],
                                                     f["flags"], f["nacks"], f["plis"], f["firs"]) for f in p.fb)
    return "e status=%d reports=%d nacks=%d plis=%d firs=%d fb=%s sns=%s refs=%s" % (
        p.status, p.reports, p.nacks, p.plis, p.firs, fb or "-", ",".join(map(str, p.sns)) or "-",
        ",".join("%d:%d:%d" % r for r in p.refs) or "-")


SEEDS = (1, 2, 3)


@pytest.mark.parametrize("seed", SEEDS)
def test_replay_equals_restatement(seed):
    entries = random_entries(seed)
    want = [W.PyRtcpIn.parse(d, SSRC) for d in entries]
    # precondition, from the restatement alone: both outcomes are well represented
    ok = sum(p.status == W.IN_OK for p in want)
    assert ok * 4 >= len(want) and (len(want) - ok) * 4 >= len(want), (ok, len(want))
    assert any(p.reports > 1 for p in want) and any(p.nacks > 17 for p in want) and any(p.refs for p in want)
    script = "".join("e %d %s\n" % (SSRC, d.hex() or "-") for d in entries)
    r = subprocess.run([EXE, "--replay"], input=script, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = r.stdout.splitlines()
    assert len(got) == len(want)
    for i, (g, p) in enumerate(zip(got, want)):
        assert g == _expected_line(p), (seed, i, entries[i].hex())


def test_nack_pairs_round_trip():
    """The test marshaller's pairing keeps the order of any list, repeats and wraps included."""
    rnd = random.Random(9)
    for _ in range(200):
        base = rnd.choice((0, 65530, rnd.randrange(65536)))
        sns = [(base + rnd.randrange(-20, 40)) & 0xFFFF for _ in range(rnd.randrange(12))]
        p = W.PyRtcpIn.parse(W.nack(1, 2, W.nack_pairs(sns)), 2)
        assert p.status == W.IN_OK and p.sns == sns


# ---- ABI ------------------------------------------------------------------------------------
def test_struct_sizes(abi, tmp_path):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "include/lkfwd.h"
int main(void){printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(lkf_rtcp_raw), sizeof(lkf_rtcp_in_result),
 sizeof(lkf_rtcp_ref), offsetof(lkf_rtcp_in_result, pli_layer), offsetof(lkf_rtcp_in_result, ref_count),
 offsetof(lkf_rtcp_raw, len), offsetof(lkf_rtcp_ref, off));
 printf("%d %d %d %d\n", LKF_RTCP_IN_OK, LKF_RTCP_IN_MALFORMED, LKF_RTCP_REF_REMB, LKF_RTCP_REF_TWCC);return 0;}
'''
    exe = str(tmp_path / "lkf_rtcp_in_sizes")
    with open(exe + ".c", "w") as f:
        f.write(src)
    subprocess.run(["gcc", "-I", ROOT, "-o", exe, exe + ".c"], check=True)
    lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()
    py = [C.sizeof(abi.lkf_rtcp_raw), C.sizeof(abi.lkf_rtcp_in_result), C.sizeof(abi.lkf_rtcp_ref),
          abi.lkf_rtcp_in_result.pli_layer.offset, abi.lkf_rtcp_in_result.ref_count.offset,
          abi.lkf_rtcp_raw.len.offset, abi.lkf_rtcp_ref.off.offset]
    assert list(map(int, lines[0].split())) == py == [12, 48, 16, 36, 44, 8, 8]
    assert list(map(int, lines[1].split())) == [abi.LKF_RTCP_IN_OK, abi.LKF_RTCP_IN_MALFORMED,
                                                abi.LKF_RTCP_REF_REMB, abi.LKF_RTCP_REF_TWCC]
    assert [abi.RTCP_RAW_DTYPE.itemsize, abi.RTCP_IN_RESULT_DTYPE.itemsize, abi.RTCP_REF_DTYPE.itemsize] == [12, 48, 16]
    assert abi.RTCP_IN_RESULT_DTYPE.fields["pli_layer"][1] == 36


def test_symbols_exported_and_bound(pkg):
    lib = os.path.join(ROOT, "livekit-server_amd", "lib", "liblkfwd.so")
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    exported = set(l.split()[-1] for l in out.splitlines() if l.strip())
    for s in ("lkf_rtcp_ingest", "lkf_rtcp_ingested_nacks", "lkf_rtx_lookup_ingested"):
        assert s in exported, s
    api = pkg.abi.bind_engine_api(pkg.load_library(), "lkf_")
    for k in ("rtcp_ingest", "rtcp_ingested_nacks", "rtx_lookup_ingested"):
        assert k in api, k
    for m in ("rtcp_ingest", "rtcp_ingested_nacks", "rtx_lookup_ingested"):
        assert callable(getattr(pkg.Engine, m))
