"""The publisher RTCP loop on the CPU: no GPU, no HIP runtime.

livekit-server_amd/csrc/pub_rtcp_unit.cpp is a stand-alone program built with
the host compiler and the address + undefined-behaviour sanitizers over
pub_rtcp_device.h, the scalar semantics the k_pub_* kernels and k_nack_wire of
rtcp_kernels.hip run.  Its named cases run one test each; its --replay mode
runs seeded random scripts (the counters advancing, struct sender reports,
compound packets, reception report requests, clock steps) whose every result
and every state word must equal tests/pub_rtcp_lib.PyStreamRtcp's.  Every
compound is parsed in a heap block of its exact length.  The rest checks the
ABI structs against a C program and the exported symbols.
"""
import ctypes as C
import os
import random
import struct
import subprocess

import pytest

from tests import pub_rtcp_lib as P
from tests import rtcp_wire_lib as W
from tests.pub_rtcp_lib import PyStreamRtcp
from tests.rtcp_lib import bits, to_ntp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "livekit-server_amd", "csrc")
EXE = os.path.join(ROOT, "livekit-server_amd", "lib", "pub_rtcp_unit")
T0 = 1700000000 * 10**9


def _names():
    subprocess.run(["make", "-s", "-C", CSRC, "pub_rtcp_unit"], check=True)
    out = subprocess.run([EXE, "--list"], check=True, capture_output=True, text=True).stdout
    return [x for x in out.split() if x]


NAMES = _names()
INVENTORY = (
    # reception reports
    "rr_uninitialized", "rr_first_from_start", "rr_nothing_expected", "rr_3_of_20", "rr_proxy", "rr_loss_rate_one",
    "rr_negative_lost_clamped", "rr_expected_65536", "rr_expected_65537", "rr_total_lost_saturates", "rr_sequence_wrap",
    "rr_no_sr", "rr_dlsr", "rr_wire", "fraction_lost_report",
    # sender reports
    "sr_before_init", "sr_first", "sr_anachronous", "sr_rtp_forward_wrap", "sr_backwards_resets_first", "sr_clock_skew",
    "sr_first_time_earlier", "sr_first_time_not_later", "sr_adjust_too_big", "sr_after_window",
    "sr_samples_diff_negative",
    # compounds
    "compound_sr_alone", "compound_sr_sdes", "compound_two_srs", "compound_rr_only", "compound_foreign_ssrc",
    "compound_truncated_sr", "compound_len_0",
    # NACK wire
    "nack_wire_1", "nack_wire_17", "nack_wire_two_records")


def test_pub_rtcp_unit_inventory():
    for want in INVENTORY:
        assert want in NAMES, want


@pytest.mark.parametrize("name", NAMES)
def test_pub_rtcp_unit(name):
    r = subprocess.run([EXE, name], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert ("PASS " + name) in r.stdout


def test_receiver_report_wire_bytes():
    """The 32 bytes of a unit case parse back, field by field, to the record."""
    r = subprocess.run([EXE, "rr_wire"], capture_output=True, text=True, check=True)
    lines = dict(l.split(None, 1) for l in r.stdout.splitlines() if l.startswith(("wire", "record")))
    wire = bytes(int(x, 16) for x in lines["wire"].split())
    ssrc, frac, total, lsn, jitter, lsr, dlsr = map(int, lines["record"].split())
    assert len(wire) == 32
    b0, pt, length, sender, source, fl, wlsn, wjit, wlsr, wdlsr = struct.unpack(">BBHIIIIIII", wire)
    assert (b0, pt, length) == (0x81, 201, 7)  # V=2, P=0, RC=1; PT 201; 7 words follow the first
    assert sender == source == ssrc == 0x11223344
    assert (fl >> 24, fl & 0xFFFFFF, wlsn, wjit, wlsr, wdlsr) == (frac, total, lsn, jitter, lsr, dlsr)
    # ... and through the ingress restatement's parser, as a subscriber-side engine would read it
    p = W.PyRtcpIn.parse(wire, ssrc)
    assert p.status == W.IN_OK and p.reports == 1
    assert p.fb[0]["fraction_lost"] == frac and p.fb[0]["total_lost"] == total and p.fb[0]["delay"] == dlsr


def test_restatement_transcribes_fraction_lost_report():
    """TestFractionLostReport (buffer_test.go:221-263) on the restatement alone."""
    m = PyStreamRtcp(48000, 123)
    hot = dict(init=False, sn_start=0, ext_highest_sn=0, ts_start=0, packets_lost=0, jitter=0.0, first_time=0)
    now, last, got = T0, 0, []
    for i in range(15):
        if i == 1:
            now += 10**9
        if i == 0:
            hot.update(init=True, first_time=now)
        hot["ext_highest_sn"] = i
        if now - last < 10**9:
            continue
        last = now
        r = m.reception_report(hot, 55, now)
        if r["flags"]:
            got.append(r["fraction_lost"])
    assert got == [55, 55]


# ---- --replay against PyStreamRtcp -----------------------------------------------
def parse_kv(line):
    """One pub_rtcp_unit --replay output line -> (kind, {name: int}); the wire bytes stay a hex string."""
    kind, *toks = line.split()
    out = {}
    for t in toks:
        k, v = t.split("=")
        out[k] = v if k == "wire" else int(v)
    return kind, out


def _compound(rnd, ssrc, t, rtp_now):
    """A compound packet: mostly well formed with 0..2 sender reports, sometimes broken."""
    pk = []
    for _ in range(rnd.choice((1, 1, 1, 2, 0))):
        ntp = to_ntp(t - rnd.randrange(0, 40) * 10**6)
        blocks = [W.report_block(rnd.randrange(1 << 32))] * rnd.choice((0, 0, 1, 2))
        pk.append(W.sr(rnd.choice((ssrc, 0xdeadbeef)), blocks, ntp=ntp, rtp=(rtp_now + rnd.randrange(-2000, 2000)) & P.M32))
    extra = [W.sdes(ssrc), W.rr(ssrc, [W.report_block(5)]), W.bye(ssrc), W.xr(ssrc), W.pli(1, 2),
             W.nack(1, 2, [(7, 1)]), W.remb(1, ssrcs=(3,))]
    for _ in range(rnd.randrange(0, 3)):
        pk.insert(rnd.randrange(len(pk) + 1), rnd.choice(extra))
    data = W.compound(*pk)
    k = rnd.random()
    if k < 0.06 and data:
        data = data[:len(data) - rnd.randrange(1, 8)]  # cut short
    elif k < 0.10 and data:
        data = data[:-4] + bytes([data[-4] & 0x3F]) + data[-3:] if len(data) >= 4 else data  # a bad version at the end
    elif k < 0.14:
        bad = bytearray(W.sr(ssrc, ntp=to_ntp(t), rtp=rtp_now))
        bad[0] |= 1  # claims a report block it has no room for
        data += bytes(bad)
    elif k < 0.17:
        data = b""
    return data


def _script(seed):
    rnd = random.Random(seed)
    clock = rnd.choice((90000, 48000))
    ssrc = rnd.randrange(1, 1 << 32)
    m = PyStreamRtcp(clock, ssrc)
    hot = dict(init=False, sn_start=0, ext_highest_sn=0, ts_start=0, packets_lost=0, jitter=0.0, first_time=0)
    lines = ["stream %d %d" % (clock, ssrc)]
    expect = []
    t = T0 + rnd.randrange(10**9)
    ts0 = rnd.choice((rnd.randrange(1 << 32), (1 << 32) - rnd.randrange(1, 200000)))
    t_first = t
    skew = rnd.choice((1.0, 1.0, 1.0, 1.5, 0.7))  # the publisher's clock against the nominal rate
    late = rnd.choice((0, 0, rnd.randrange(1, 400) * 10**6, 301 * 10**9))  # how late the first packet was
    for _ in range(rnd.randrange(30, 160)):
        r = rnd.random()
        t += rnd.choice((rnd.randrange(1, 400) * 10**6, rnd.randrange(1, 400) * 10**6, rnd.randrange(1, 3000),
                         rnd.randrange(1, 90) * 10**9))
        rtp_now = (ts0 + int((t - t_first + late) * skew * clock // 10**9)) & P.M32
        if r < 0.40:  # packets
            if not hot["init"]:
                if rnd.random() < 0.3:
                    continue
                sn = rnd.choice((rnd.randrange(65536), 65535 - rnd.randrange(30)))
                t_first = t
                hot.update(init=True, sn_start=sn, ext_highest_sn=sn, ts_start=ts0, first_time=t)
                lines.append("init %d %d %d" % (t, sn, ts0))
            else:
                k = rnd.random()
                adv = rnd.randrange(1, 60) if k < 0.9 else rnd.choice((65536, 65537, 65535, 70000)) if k < 0.95 else 0
                lost = hot["packets_lost"]
                lost += rnd.randrange(0, min(adv, 50) + 1) if rnd.random() < 0.5 else 0
                if rnd.random() < 0.1:
                    lost -= rnd.randrange(0, 4)  # reordered packets fill holes (the uint64 may wrap below 0)
                if rnd.random() < 0.02:
                    lost += 1 << 24
                hot["ext_highest_sn"] += adv
                hot["packets_lost"] = lost & P.M64
                hot["jitter"] = rnd.choice((0.0, rnd.random() * 5000, rnd.random() * 1e10, 1e300))
                lines.append("adv %d %d %d" % (hot["ext_highest_sn"], hot["packets_lost"], bits(hot["jitter"])))
        elif r < 0.60:  # a struct sender report
            k = rnd.random()
            ntp = to_ntp(t - rnd.randrange(0, 40) * 10**6)
            rtp = rtp_now
            if k < 0.08 and m.sr_newest:
                ntp = m.sr_newest[0] - rnd.randrange(1, 1 << 33)  # anachronous
            elif k < 0.16:
                rtp = (rtp - rnd.randrange(1, 1 << 20)) & P.M32  # backwards
            elif k < 0.22:
                rtp = (rtp + rnd.randrange(1 << 20, 1 << 31)) & P.M32
            ntp &= P.M64
            lines.append("sr %d %d %d" % (t, rtp, ntp))
            fl, sntp, sext = m.sender_report(hot, rtp, ntp, t)
            expect.append(("sr", dict(flags=fl, ntp=sntp, rtp_ext=sext)))
        elif r < 0.75:  # a compound packet
            data = _compound(rnd, ssrc, t, rtp_now)
            lines.append("bytes %d %s" % (t, data.hex() or "-"))
            expect.append(("bytes", m.ingest(hot, data, t)))
        elif r < 0.985:  # a reception report
            proxy = rnd.choice((0, 0, rnd.randrange(256)))
            lines.append("rr %d %d" % (t, proxy))
            rep = m.reception_report(hot, proxy, t)
            rep["wire"] = m.wire(rep).hex()
            expect.append(("rr", rep))
        else:
            lines.append("close")
            m.closed = True
    lines.append("reset")
    expect.append(("state", m.state(hot)))
    return lines, expect


def test_replay_against_pystreamrtcp():
    nscripts = 200
    lines, expect = [], []
    for seed in range(nscripts):
        l, e = _script(3000 + seed)
        lines += l
        expect += e
    r = subprocess.run([EXE, "--replay"], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [parse_kv(x) for x in r.stdout.splitlines()]
    got = got[:-1]  # (the state printed at the end of input: the fresh stream after the last reset)
    assert len(got) == len(expect)
    nops = {"sr": 0, "bytes": 0, "rr": 0}
    seen = dict(uninit=0, anachronous=0, skew=0, reset_first=0, adjusted=0, too_big=0, closed=0, malformed=0,
                two_srs=0, rr_valid=0, rr_nil=0, dlsr=0, saturated=0, adjusted_state=0)
    for i, ((gk, gv), (ek, ev)) in enumerate(zip(got, expect)):
        assert gk == ek, i
        assert gv == ev, (i, ek, {k: (gv.get(k), ev.get(k)) for k in set(gv) | set(ev) if gv.get(k) != ev.get(k)})
        if ek in nops:
            nops[ek] += 1
        if ek in ("sr", "bytes"):
            fl = ev["flags"]
            seen["uninit"] += bool(fl & P.SSR_IGNORED_UNINIT)
            seen["anachronous"] += bool(fl & P.SSR_ANACHRONOUS)
            seen["skew"] += bool(fl & P.SSR_CLOCK_SKEW)
            seen["reset_first"] += bool(fl & P.SSR_RESET_FIRST)
            seen["adjusted"] += bool(fl & P.SSR_FIRST_TIME_ADJUSTED)
            seen["too_big"] += bool(fl & P.SSR_ADJUST_TOO_BIG)
            seen["closed"] += bool(fl & P.SSR_CLOSED)
        if ek == "bytes":
            seen["malformed"] += ev["status"] == P.IN_MALFORMED
            seen["two_srs"] += ev["n_sr"] == 2
        elif ek == "rr":
            seen["rr_valid" if ev["flags"] else "rr_nil"] += 1
            seen["dlsr"] += ev["delay"] > 0
            seen["saturated"] += ev["total_lost"] == 0xFFFFFF
        elif ek == "state":
            seen["adjusted_state"] += ev["started"] and ev["first_time"] != ev["start_time"]
    # the scripts reach the branches they are meant to
    assert all(v > 0 for v in seen.values()), seen
    assert min(nops.values()) > 200, nops


# ---- ABI ---------------------------------------------------------------------------
NEW_STRUCTS = ("lkf_stream_sr", "lkf_stream_sr_result", "lkf_stream_rr_req", "lkf_stream_rr", "lkf_stream_rtcp_raw",
               "lkf_stream_rtcp_entry", "lkf_stream_rtcp_in_result", "lkf_stream_rtcp_pkt", "lkf_stream_rtcp")


def test_struct_sizes_against_c(abi, tmp_path):
    src = '#include <stdio.h>\n#include "include/lkfwd.h"\nint main(void){\n'
    src += "".join('printf("%%zu\\n", sizeof(%s));\n' % n for n in NEW_STRUCTS) + "return 0;}\n"
    exe = str(tmp_path / "pub_rtcp_sizes")
    with open(exe + ".c", "w") as f:
        f.write(src)
    subprocess.run(["gcc", "-I", ROOT, "-o", exe, exe + ".c"], check=True)
    sizes = list(map(int, subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()))
    assert sizes == [C.sizeof(getattr(abi, n)) for n in NEW_STRUCTS]
    assert sizes == [16, 24, 8, 40, 12, 8, 32, 16, 112]
    for n, d in (("lkf_stream_sr", abi.STREAM_SR_DTYPE), ("lkf_stream_sr_result", abi.STREAM_SR_RESULT_DTYPE),
                 ("lkf_stream_rr_req", abi.STREAM_RR_REQ_DTYPE), ("lkf_stream_rr", abi.STREAM_RR_DTYPE),
                 ("lkf_stream_rtcp_raw", abi.STREAM_RTCP_RAW_DTYPE), ("lkf_stream_rtcp_entry", abi.STREAM_RTCP_ENTRY_DTYPE),
                 ("lkf_stream_rtcp_in_result", abi.STREAM_RTCP_IN_RESULT_DTYPE),
                 ("lkf_stream_rtcp_pkt", abi.STREAM_RTCP_PKT_DTYPE), ("lkf_stream_rtcp", abi.STREAM_RTCP_DTYPE)):
        assert d.itemsize == C.sizeof(getattr(abi, n)), n


def test_engine_exports_publisher_rtcp_entry_points(pkg):
    lib = C.CDLL(pkg.LIB_PATH)  # dlopen only; no engine, no device work
    names = ("stream_sender_reports", "stream_receiver_reports", "stream_rtcp_ingest", "stream_rtcp_ingest_unprotected",
             "ingest_nacks_wire", "stream_rtcp_get")
    for k in names:
        assert hasattr(lib, "lkf_" + k), k
    api = pkg.load_library().api
    for k in names:
        assert k in api


def test_oracle_library_still_loads(oracle):
    """The oracle does not get these entry points; the binding skips them."""
    assert "stream_sender_reports" not in oracle.api
