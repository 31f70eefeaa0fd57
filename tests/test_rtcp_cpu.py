"""The DownTrack RTCP loop on the CPU: no GPU, no HIP runtime.

livekit-server_amd/csrc/rtcp_unit.cpp is a stand-alone program built with the
host compiler and the address + undefined-behaviour sanitizers over
rtcp_device.h, the scalar semantics the kernels of rtcp_kernels.hip run.  Its
named cases run one test each; its --replay mode runs seeded random scripts
(packets, receiver reports, sender reports, deltas, counter adds) whose every
result and every state word must equal tests/rtcp_lib.PyRtcp's, double bits
included.  The rest checks the ABI structs against a C program and the
exported symbols.
"""
import ctypes as C
import os
import random
import struct
import subprocess

import pytest

from tests import rtcp_lib
from tests.rtcp_lib import PyRtcp, parse_kv
from tests.test_sender_cpu import M64, PySender

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "livekit-server_amd", "csrc")
EXE = os.path.join(ROOT, "livekit-server_amd", "lib", "rtcp_unit")
T0 = 1700000000 * 10**9


def _names():
    subprocess.run(["make", "-s", "-C", CSRC, "rtcp_unit"], check=True)
    out = subprocess.run([EXE, "--list"], check=True, capture_output=True, text=True).stdout
    return [x for x in out.split() if x]


NAMES = _names()
INVENTORY = ("ntp_zero", "ntp_half", "ntp_round_up", "ntp_round_trip", "rtt_no_lsr", "rtt_wrong_lsr", "rtt_before",
             "rtt_value", "rr_sn_wrap", "rr_lost_wrap", "rr_before_start", "rr_out_of_order", "rr_uninitialized",
             "rr_closed", "interval_0", "interval_1", "interval_63", "interval_64", "interval_65", "interval_4096",
             "interval_4097", "interval_70000", "interval_empty_divergence", "sr_first", "sr_repair", "sr_clock_skew",
             "sr_primary_zero", "sr_wire", "delta_nil_before_rr", "delta_expected_zero", "delta_lost_clamped",
             "delta_negative_clamped")


def test_rtcp_unit_inventory():
    for want in INVENTORY:
        assert want in NAMES, want


@pytest.mark.parametrize("name", NAMES)
def test_rtcp_unit(name):
    r = subprocess.run([EXE, name], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert ("PASS " + name) in r.stdout


def test_sender_report_wire_bytes():
    """The 28 bytes of a unit case parse back to the record's fields."""
    r = subprocess.run([EXE, "sr_wire"], capture_output=True, text=True, check=True)
    lines = dict(l.split(None, 1) for l in r.stdout.splitlines() if l.startswith(("wire", "record")))
    wire = bytes(int(x, 16) for x in lines["wire"].split())
    ntp, rtp, packets, octets = map(int, lines["record"].split())
    assert len(wire) == 28
    b0, pt, length, ssrc, wntp, wrtp, wpackets, woctets = struct.unpack(">BBHIQIII", wire)
    assert (b0, pt, length, ssrc) == (0x80, 200, 6, 0x11223344)  # V=2, P=0, RC=0; PT 200; 6 words follow the first
    assert (wntp, wrtp, wpackets, woctets) == (ntp, rtp, packets, octets)


# ---- the restatement's own closed form against the Go loop, one esn at a time ----
def test_pyrtcp_interval_closed_form_against_loop():
    rnd = random.Random(5)
    s = PySender(90000)
    s.ring = [(rnd.choice((0, 0, 100 + rnd.randrange(1000))), 12, rnd.randrange(8)) for _ in range(4096)]
    s.ring = [(p, h, f if p else 0) for p, h, f in s.ring]
    m = PyRtcp(s)
    ehsn = 70037
    for length in (0, 1, 63, 64, 65, 4096, 4097, 9000):
        for end in (ehsn + 1, ehsn + 6, ehsn - 10, ehsn - 4090, ehsn - 5000):
            got = m.interval_stats(end - length, end, ehsn)
            want = dict.fromkeys(rtcp_lib.IS_FIELDS, 0)
            for esn in range(end - length, end):
                off = rtcp_lib.s64(ehsn - esn)
                if off >= 4096 or off < 0:
                    want["packets_not_found"] += 1
                    continue
                size, hdr, fl = s.ring[esn & 4095]
                if size == 0:
                    want["packets_lost"] += 1
                elif fl & 2:
                    want["packets_padding"] += 1
                    want["bytes_padding"] += size
                    want["header_bytes_padding"] += hdr
                else:
                    want["packets"] += 1
                    want["bytes"] += size
                    want["header_bytes"] += hdr
                    want["packets_out_of_order"] += 1 if fl & 4 else 0
                want["frames"] += 1 if fl & 1 else 0
            assert got == want, (length, end)


# ---- --replay against PyRtcp ----------------------------------------------------
def _script(seed):
    """One random script: (lines for rtcp_unit --replay, expected output records)."""
    rnd = random.Random(seed)
    clock = rnd.choice((90000, 48000))
    s = PySender(clock)
    m = PyRtcp(s)
    lines = ["clock %d" % clock]
    expect = []
    t = T0 + rnd.randrange(10**9)
    esn = rnd.choice((rnd.randrange(1, 200), rnd.randrange(4097, 70000), (1 << 32) - rnd.randrange(300),
                      (rnd.randrange(1, 9) << 16) + rnd.randrange(65536)))
    ets = rnd.randrange(1 << 32)
    missing = []
    acked = 0
    lost_total = 0
    for _ in range(rnd.randrange(50, 401)):
        r = rnd.random()
        t += rnd.randrange(1, 40) * 10**6
        if r < 0.70:  # a packet
            k = rnd.random()
            pay = 0 if rnd.random() < 0.08 else rnd.randrange(100, 1200)
            if k < 0.05 and missing:  # a reordered one
                e = missing.pop(rnd.randrange(len(missing)))
                ts = (ets - rnd.randrange(3000)) & M64
            elif k < 0.07 and s.init:  # a duplicate
                e, ts = s.high_sn, ets
            else:
                gap = 1
                if k < 0.15:
                    gap = rnd.randrange(2, 10)
                elif k < 0.16:
                    gap = rnd.randrange(4097, 9000)
                missing.extend(range(esn + 1, esn + min(gap, 20)))
                esn += gap
                ets += rnd.choice((0, 3000, 3000, 960))
                e, ts = esn, ets
            args = (t, e, ts, int(rnd.random() < 0.3), rnd.randrange(12, 40), pay, rnd.choice((0, 0, 7)))
            lines.append("update %d %d %d %d %d %d %d" % args)
            if m.end_time == 0:
                s.update(args[0], args[1], args[2], bool(args[3]), args[4], args[5], args[6])
        elif r < 0.82:  # a receiver report: at, behind (stale) or ahead of the highest SN
            k = rnd.random()
            top = s.high_sn if s.init else esn
            if k < 0.6:
                ack = top - rnd.randrange(0, 5)
            elif k < 0.75:
                ack = acked - rnd.randrange(1, 50)
            elif k < 0.85:
                ack = top + rnd.randrange(1, 50)
            else:
                ack = top - rnd.randrange(0, 6000)
            ack = max(ack, 0)
            acked = max(acked, ack)
            lost_total += rnd.randrange(0, 3)
            lsr, dlsr = 0, rnd.randrange(0, 1 << 16)
            if m.sr_newest is not None and rnd.random() < 0.7:
                lsr = (m.sr_newest[0] >> 16) & 0xFFFFFFFF
                if rnd.random() < 0.15:
                    lsr ^= 1 << rnd.randrange(32)
                if rnd.random() < 0.1:
                    dlsr = rnd.randrange(1 << 20, 1 << 24)
            rr = (t, rtcp_lib.rr_lsn(ack, s.start_sn if s.init else esn), lost_total & 0xFFFFFFFF,
                  rnd.randrange(0, 5000), lsr, dlsr)
            lines.append("rr %d %d %d %d %d %d" % rr)
            rtt, flags = m.receiver_report(*rr)
            expect.append(("rr", dict(rtt=rtt, flags=flags)))
        elif r < 0.89:  # a sender report
            ccr = rnd.choice((0, 0, rnd.randrange(80000, 100000), rnd.randrange(1, 400000)))
            lines.append("sr %d %d" % (t, ccr))
            rep = m.sender_report(t, ccr)
            rep["wire"] = m.sender_report_wire(rep, 0x11223344).hex()
            expect.append(("sr", rep))
        elif r < 0.94:
            lines.append("delta")
            d = m.delta()
            expect.append(("delta", d))
        elif r < 0.995:
            c = (rnd.randrange(20), rnd.randrange(3), rnd.randrange(2))
            lines.append("nack %d %d %d" % c)
            m.counts(*c)
        else:
            lines.append("stop")
            m.stop()
    lines.append("reset")
    st = dict(m.sender_state())
    st.update(m.state())
    expect.append(("state", st))
    return lines, expect


def test_replay_against_pyrtcp():
    nscripts = 220
    lines, expect = [], []
    nops = {"rr": 0, "sr": 0, "delta": 0}
    seen = dict(ignored=0, overflow=0, rtt=0, repaired=0, delta_valid=0, lost=0, ooo=0, padding=0)
    for seed in range(nscripts):
        l, e = _script(1000 + seed)
        lines += l
        expect += e
    r = subprocess.run([EXE, "--replay"], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [parse_kv(x) for x in r.stdout.splitlines()]
    got = got[:-1]  # (the state printed at the end of input: the fresh DownTrack after the last reset)
    assert len(got) == len(expect)
    for i, ((gk, gv), (ek, ev)) in enumerate(zip(got, expect)):
        assert gk == ek, i
        if ek == "delta" and ev is None:
            assert gv["valid"] == 0, (i, gv)
            continue
        assert gv == ev, (i, ek, {k: (gv.get(k), ev.get(k)) for k in set(gv) | set(ev) if gv.get(k) != ev.get(k)})
        if ek in nops:
            nops[ek] += 1
        if ek == "rr":
            seen["ignored"] += bool(ev["flags"] & rtcp_lib.FB_IGNORED)
            seen["overflow"] += bool(ev["flags"] & rtcp_lib.FB_CACHE_OVERFLOW)
            seen["rtt"] += bool(ev["flags"] & rtcp_lib.FB_RTT_CHANGED)
        elif ek == "sr":
            seen["repaired"] += bool(ev["flags"] & rtcp_lib.SR_REPAIRED)
        elif ek == "delta":
            seen["delta_valid"] += 1
        elif ek == "state":
            seen["lost"] += ev["is_packets_lost"]
            seen["ooo"] += ev["is_packets_out_of_order"]
            seen["padding"] += ev["is_packets_padding"]
    # the scripts reach the branches they are meant to
    assert all(v > 0 for v in seen.values()), seen
    assert min(nops.values()) > 200, nops


# ---- ABI ---------------------------------------------------------------------------
NEW_STRUCTS = ("lkf_rtcp_sr_data", "lkf_interval_stats", "lkf_sender_snapshot", "lkf_sender_rtcp", "lkf_rtcp_fb",
               "lkf_rtcp_fb_result", "lkf_rtcp_sr_req", "lkf_rtcp_sr", "lkf_rtp_delta_info")


def test_struct_sizes_against_c(abi, tmp_path):
    src = '#include <stdio.h>\n#include "include/lkfwd.h"\nint main(void){\n'
    src += "".join('printf("%%zu\\n", sizeof(%s));\n' % n for n in NEW_STRUCTS) + "return 0;}\n"
    exe = str(tmp_path / "rtcp_sizes")
    with open(exe + ".c", "w") as f:
        f.write(src)
    subprocess.run(["gcc", "-I", ROOT, "-o", exe, exe + ".c"], check=True)
    sizes = list(map(int, subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()))
    assert sizes == [C.sizeof(getattr(abi, n)) for n in NEW_STRUCTS]
    assert C.sizeof(abi.lkf_sender_rtcp) == 384 == abi.SENDER_RTCP_DTYPE.itemsize
    assert abi.RTCP_FB_DTYPE.itemsize == C.sizeof(abi.lkf_rtcp_fb)
    assert abi.RTP_DELTA_INFO_DTYPE.itemsize == C.sizeof(abi.lkf_rtp_delta_info)


def test_engine_exports_rtcp_entry_points(pkg):
    lib = C.CDLL(pkg.LIB_PATH)  # dlopen only; no engine, no device work
    for sym in ("lkf_rtcp_feedback", "lkf_rtcp_sender_reports", "lkf_sender_delta_info", "lkf_sender_rtcp_get"):
        assert hasattr(lib, sym), sym
    api = pkg.load_library().api
    for k in ("rtcp_feedback", "rtcp_sender_reports", "sender_delta_info", "sender_rtcp_get"):
        assert k in api


def test_oracle_library_still_loads(oracle):
    """The oracle does not get these entry points; the binding skips them."""
    assert "rtcp_feedback" not in oracle.api
