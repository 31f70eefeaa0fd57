"""The dependency-descriptor frame-rate calculator on the CPU: no GPU, no HIP
runtime.

tests/fps_dd_lib.PyFpsDD restates buffer/fps.go:319-570 the way the Go is
written (sorted lists, frame records).  Here it runs the scenarios of the
reference's own TestFpsDD (fps_test.go:232-326: the same createFrames
generator, feeding order and SetMaxLayer call) under the reference's own
+-10 % bound (verifyFps), and it is the yardstick for
livekit-server_amd/csrc/fps_dd_unit.cpp: a stand-alone program built with the
host compiler, -ffp-contract=off and the address + undefined-behaviour
sanitizers over fps_dd_device.h (the masks-and-slots restatement k_ing_fps_dd
runs, the wave behind its 256-entry scalar stand-in).  The program prints its
whole state after every script line; every line must equal PyFpsDD's, on the
reference scenarios, on edge scripts and on seeded random scripts whose
parameters are chosen so that PyFpsDD completes on at least half of them
(asserted here: a test where nothing ever calculates cannot pass).

The dependency-descriptor writer of fps_dd_lib is checked against the reader
tests/test_dd_wide_cpu.py already has.
"""
import os
import random
import subprocess

import pytest

from tests import fps_dd_lib as D
from tests.fps_dd_lib import PyFpsDD
from tests.test_dd_wide_cpu import read_dd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "livekit-server_amd", "csrc")
EXE = os.path.join(ROOT, "livekit-server_amd", "lib", "fps_dd_unit")
CLOCK = 90000

# a script: [("M", spatial, temporal) | ("P", fn, ts, spatial, temporal, [diffs])]


def run_model(script, clock=CLOCK):
    """-> (the model after the script, its unit line after every op)."""
    m, lines = PyFpsDD(clock), []
    for op in script:
        if op[0] == "M":
            m.set_max_layer(op[1], op[2])
            lines.append(m.unit_line(False))
        else:
            lines.append(m.unit_line(m.packet(*op[1:])))
    return m, lines


@pytest.fixture(scope="module")
def unit():
    subprocess.run(["make", "-s", "-C", CSRC, "fps_dd_unit"], check=True)

    def run(scripts, tmp_path):
        """scripts: [script] -> per script, the program's lines."""
        path = os.path.join(str(tmp_path), "scripts.txt")
        with open(path, "w") as f:
            for sc in scripts:
                f.write("S %d\n" % CLOCK)
                for op in sc:
                    if op[0] == "M":
                        f.write("M %d %d\n" % op[1:])
                    else:
                        f.write("P %d %d %d %d %d %s\n" % (op[1], op[2], op[3], op[4], len(op[5]),
                                                           " ".join("%d" % d for d in op[5])))
        r = subprocess.run([EXE, path], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        out, cur = [], None
        for line in r.stdout.splitlines():
            if line == "S":
                cur = []
                out.append(cur)
            else:
                cur.append(line)
        assert len(out) == len(scripts)
        return out

    return run


def check(unit, scripts, tmp_path):
    got = unit(scripts, tmp_path)
    models = []
    for k, (sc, lines) in enumerate(zip(scripts, got)):
        m, want = run_model(sc)
        assert len(lines) == len(want), k
        for i, (a, b) in enumerate(zip(lines, want)):
            assert a == b, (k, i, sc[i], a, b)
        models.append(m)
    return models


# ---- the reference's TestFpsDD ------------------------------------------------
REF_CASES = {
    "normal": (12345678, 100, ((5.1, 10.1, 16), (5.1, 10.1, 16), (8, 15, 30.1)), True),
    "frame number and timestamp wrap": ((1 << 31) - 10, (1 << 15) - 10, ((7.5, 15, 30),) * 3, True),
    "vp8": (12345678, 100, ((7.5, 15), (7.5, 15), (15, 30)), False),
    "packet lost and duplicate": (12345678, 100, ((7.5, 15, 30),) * 3, True),
}


def ref_script(name):
    start_ts, start_fn, fps, dep = REF_CASES[name]
    frames = D.create_frames(start_fn, start_ts, 500, fps, dep)
    if name == "packet lost and duplicate":
        for fs in frames:
            for j in range(5, 130):
                if j % 2 == 0:
                    fs[j] = fs[j - 1]
    script = [("M", len(fps) - 1, len(fps[0]) - 1)]
    for fs in frames:  # (all of spatial 0, then all of spatial 1, ...: the reference's feeding order)
        script += [("P", fn, ts, s, t, list(diffs)) for fn, ts, s, t, diffs in fs]
    return script, fps


def verify_fps(fps, m):
    for s, row in enumerate(fps):
        for want, got in zip(row, m.rates[s]):
            assert want * 0.9 <= got <= want * 1.1, (s, row, m.rates[s])


@pytest.mark.parametrize("name", sorted(REF_CASES))
def test_reference_scenarios(name):
    script, fps = ref_script(name)
    m, _ = run_model(script)
    assert m.completed and m.calculated
    verify_fps(fps, m)


def test_host_program_on_reference_scenarios(unit, tmp_path):
    scripts = [ref_script(n)[0] for n in sorted(REF_CASES)]
    models = check(unit, scripts, tmp_path)
    assert all(m.calculated for m in models)


# ---- edge scripts ---------------------------------------------------------------
T3 = (0, 2, 1, 2)


def l1t3(start_fn, start_ts, n, step=3000, pattern=T3):
    """One spatial layer, the pattern's temporal layers; a frame depends on the
    latest earlier frame of a temporal layer not above its own."""
    out, latest = [], {}
    for i in range(n):
        t = pattern[i % len(pattern)]
        fn = (start_fn + i) & 0xFFFF
        dep = [latest[u] for u in latest if u <= t]
        diffs = [(fn - max(dep, key=lambda f: (f - start_fn) & 0xFFFF)) & 0xFFFF] if dep else []
        out.append(("P", fn, (start_ts + i * step) & 0xFFFFFFFF, 0, t, diffs))
        latest[t] = fn
    return out


def edge_scripts():
    e = {}
    # the plain compares stall every chain at the 16-bit wrap (slot 20): rates only after the window ran out
    e["wrap inside the window"] = [("M", 0, 2)] + l1t3(65516, 5000, 420)
    sc = l1t3(1000, 7, 30)
    sc += l1t3(1000 + 30 + 300, 7 + 30 * 3000, 200)  # the first of these resets, the next is the new base
    e["jump of 256 or more"] = [("M", 0, 2)] + sc
    sc = l1t3(500, 9000, 200)
    sc.insert(0, ("P", 450, 1, 0, 0, []))  # the base; 500 is then slot 50
    sc.insert(40, ("P", 440, 2, 0, 0, [1]))  # before the base: ignored
    sc.insert(60, ("P", 450, 3, 0, 0, [1]))  # the base again: ignored
    sc.insert(80, ("P", (450 + 0x8001) & 0xFFFF, 4, 0, 1, [1]))  # more than half the ring ahead: ignored
    e["jump backwards"] = [("M", 0, 2)] + sc
    sc = l1t3(2000, 100, 200)
    for k in (20, 21, 22, 23, 50):
        op = sc[k]
        sc[k] = op[:5] + (op[5] + [4096, 15, 300],)  # older than the second frame, and before the base
    e["a diff older than the second frame"] = [("M", 0, 2)] + sc
    sc = l1t3(3000, 100, 220)
    held = sc.pop(24)  # a temporal-0 frame arrives 9 frames late: every chain through it waits, then goes on
    sc.insert(33, held)
    e["a chain gap that later fills"] = [("M", 0, 2)] + sc
    sc = l1t3(3000, 100, 420)
    del sc[24]  # ... and one that never fills: the chains stall until the window runs out
    e["a chain gap that never fills"] = [("M", 0, 2)] + sc
    e["temporal 3"] = [("M", 0, 3)] + l1t3(100, 100, 250, pattern=(0, 3, 2, 3, 1, 3, 2, 3))
    e["temporal 3 unseen"] = l1t3(100, 100, 250)  # default max layer (2, 3): spatial 1 and 2 never seen
    e["zero timestamp difference"] = [("M", 0, 2)] + l1t3(100, 777, 200, step=0)
    e["timestamp wrap"] = [("M", 0, 2)] + l1t3(100, (1 << 32) - 50 * 3000, 250)
    sc = l1t3(100, 100, 60)
    sc.insert(10, ("P", 5000, 1, 3, 0, [1]))  # spatial 3
    sc.insert(11, ("P", 5001, 1, 0, 4, [1]))  # temporal 4
    sc.insert(12, ("P", 112, 1, -1, 0, [1]))  # an invalid spatial layer is layer 0
    e["layers out of range"] = [("M", 0, 2)] + sc
    e["max layer beyond the arrays"] = [("M", 3, 2)] + l1t3(100, 100, 200) + [("M", 0, 2)] + l1t3(300, 600100, 10)
    return e


def test_edge_scripts_do_what_they_say():
    """The model alone: each edge script reaches the behaviour it is named for."""
    e = edge_scripts()
    done = lambda n: run_model(e[n])[0]
    m = done("wrap inside the window")
    assert m.calculated and m.resets >= 2
    assert not run_model(e["wrap inside the window"][:250])[0].rates[0][0] > 0
    m = done("jump of 256 or more")
    assert m.resets >= 2 and m.calculated
    assert done("jump backwards").calculated
    assert done("a diff older than the second frame").calculated
    assert done("a chain gap that later fills").calculated
    m = done("a chain gap that never fills")
    assert m.calculated and m.resets >= 2  # (only after the window ran out and the calculator started again)
    m = done("temporal 3")
    assert not m.calculated and m.rates[0][3] == 0 and m.rates[0][2] > 0
    m = done("temporal 3 unseen")
    assert not m.calculated and m.rates[0][2] > 0  # (spatial 1: nothing below it calculated in its own row)
    m = done("zero timestamp difference")
    assert not m.calculated and all(r == 0 for r in m.rates[0])
    assert done("timestamp wrap").resets >= 0
    assert done("layers out of range").rates[0][0] >= 0
    m = done("max layer beyond the arrays")
    assert m.calculated and m.resets >= 1  # never with (3, 2), at once with (0, 2)


def test_host_program_on_edge_scripts(unit, tmp_path):
    e = edge_scripts()
    check(unit, [e[n] for n in sorted(e)], tmp_path)


# ---- random scripts -------------------------------------------------------------
def random_script(rng):
    ns, nt = rng.choice((1, 1, 2, 3)), rng.choice((1, 2, 3, 3))
    pattern = ((0,), (0, 1), T3)[nt - 1]
    start_fn = rng.choice((rng.randrange(65536), 65536 - rng.randrange(1, 300), 100))
    ts = rng.choice((rng.randrange(1 << 32), (1 << 32) - rng.randrange(1, 400000), 12345))
    step = rng.choice((3000, 3000, 1500, 6000))
    p_loss, p_dup, p_swap, p_extra = rng.choice(((0, 0, 0, 0.1), (0.004, 0.02, 0.02, 0.1), (0.01, 0.05, 0.05, 0.3)))
    script = [("M", ns - 1, nt - 1)]
    if rng.random() < 0.1:
        script = []  # the default max layer
    latest, fn = {}, start_fn
    units = rng.randrange(60, 200)
    jump_at = rng.randrange(units) if rng.random() < 0.15 else -1
    for u in range(units):
        if u == jump_at:
            fn = (fn + rng.choice((256, 300, 5000, 40000, 65536 - 20))) & 0xFFFF
        t = pattern[u % len(pattern)]
        for s in range(ns):
            diffs = []
            dep = [latest[(s, v)] for v in range(t + 1) if (s, v) in latest]
            if dep:
                diffs.append(min((fn - f) & 0xFFFF for f in dep))
            if s > 0 and (s - 1, t) in latest and rng.random() < 0.8:
                diffs.append((fn - latest[(s - 1, t)]) & 0xFFFF)
            while rng.random() < p_extra:
                diffs.append(rng.choice((1, 2, rng.randrange(1, 40), rng.randrange(1, 4097), 4096)))
            diffs = [d for d in diffs if 1 <= d <= 4096]
            rng.shuffle(diffs)
            latest[(s, t)] = fn
            op = ("P", fn, (ts + u * step) & 0xFFFFFFFF, s, t, diffs)
            fn = (fn + 1) & 0xFFFF
            if rng.random() < p_loss:
                continue
            script.append(op)
            if rng.random() < p_dup:
                script.append(rng.choice(script[-8:]))
            if rng.random() < p_swap and len(script) > 3:
                script[-1], script[-2] = script[-2], script[-1]
    return script


def test_host_program_on_random_scripts(unit, tmp_path):
    rng = random.Random(20261021)
    scripts = [random_script(rng) for _ in range(400)]
    assert all(1 <= d <= 4096 for sc in scripts for op in sc if op[0] == "P" for d in op[5])
    models = check(unit, scripts, tmp_path)
    done = sum(1 for m in models if m.calculated)
    assert 2 * done >= len(scripts), (done, len(scripts))
    # ... and not everything: resets, stalls and long diff lists are in there too
    assert done < len(scripts) and any(m.resets >= 2 for m in models)
    assert any(len(op[5]) > 8 for sc in scripts for op in sc if op[0] == "P")


# ---- the writer -----------------------------------------------------------------
def test_writer_reads_back():
    st = D.l3t3_structure(61)  # (template ids wrap past 63)
    d = D.descriptor(st.template_id(4), 0x1234, structure=st)
    got_st, out = read_dd(d, None)
    assert got_st["offset"] == 61 and got_st["ndt"] == 9 and got_st["ntmpl"] == 9 and got_st["chains"] == 0
    assert got_st["tmpl_fd"] == [len(t[3]) for t in st.templates]
    assert out["tmpl"] == 4 and out["custom_fd"] is None
    # three bytes when nothing is custom
    d = D.descriptor(st.template_id(8), 77)
    assert len(d) == 3 and read_dd(d, got_st)[1]["tmpl"] == 8
    assert (d[0] & 0x3F, (d[1] << 8) | d[2]) == (st.template_id(8), 77)
    # an active mask and custom frame diffs, short and long lists, every nibble count
    for diffs in ([1], [16, 17, 256, 257, 4096], list(range(1, 12)), [4096] * 20):
        d = D.descriptor(st.template_id(2), 9, active_mask=0x3F, ndt=9, custom_fdiffs=diffs)
        _, out = read_dd(d, got_st)
        assert out["tmpl"] == 2 and out["custom_fd"] == len(diffs)
    d3 = D.descriptor(st.template_id(2), 9, custom_fdiffs=[1, 2], fdiff_nibbles=3)
    assert read_dd(d3, got_st)[1]["custom_fd"] == 2
    assert len(d3) > len(D.descriptor(st.template_id(2), 9, custom_fdiffs=[1, 2]))
    # chains and resolutions
    st2 = D.Structure(3, [(0, 0, [D.SWITCH] * 3, []), (0, 0, [D.SWITCH] * 3, [4]), (0, 1, [0, 1, 3], [2]),
                          (0, 2, [0, 0, 1], [1])], 3, protected_by=[0, 0, 0], chain_diffs=[[0], [4], [2], [1]])
    got2, _ = read_dd(D.descriptor(3, 1, structure=st2), None)
    assert got2["chains"] == 1 and got2["ntmpl"] == 4 and got2["tmpl_fd"] == [0, 1, 1, 1]
    assert st2.max_layer(0b001) == (0, 0) and st2.max_layer(0b111) == (0, 2) and st.max_layer(0x3F) == (1, 2)


def test_rtp_extension_forms():
    short = D.rtp_ext(0x11223344, 7, 9, 5, b"\x80\x00\x01", b"pay")
    assert short[0] == 0x90 and short[12:16] == b"\xbe\xde\x00\x01" and short[16] == 0x52 and short.endswith(b"pay")
    long_ = D.rtp_ext(0x11223344, 7, 9, 5, bytes(range(20)), b"pay")
    assert long_[12:14] == b"\x10\x00" and long_[16:18] == bytes([5, 20]) and long_[18:38] == bytes(range(20))
    assert (len(long_) - 3 - 16) % 4 == 0
    assert D.rtp_ext(1, 2, 3, 5, None, b"pay")[0] == 0x80
