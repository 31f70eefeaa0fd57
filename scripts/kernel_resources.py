#!/usr/bin/env python3
"""Per-kernel resource figures of the engine's HIP kernels, from the compiler.

Compiles every kernel file of livekit-server_amd/csrc for gfx950 with
-Rpass-analysis=kernel-resource-usage (device side only, nothing is linked or
run, so it needs no GPU) and reads the remarks: one row per kernel with VGPRs,
AGPRs, SGPRs, scratch bytes per lane, SGPR / VGPR spill counts, LDS bytes per
workgroup and occupancy in waves per SIMD.

  python scripts/kernel_resources.py                 # -> profiles/kernel_resources.json + a table on stdout
  python scripts/kernel_resources.py --flags=-DLKF_CHECKED=1 --out /tmp/checked.json
  python scripts/kernel_resources.py --csrc <other tree>/livekit-server_amd/csrc --out parent.json
  python scripts/kernel_resources.py --diff parent.json   # rows that differ from another report
"""
import argparse
import hashlib
import json
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = [  # remark text -> key
    ("TotalSGPRs", "sgprs"),
    ("VGPRs", "vgprs"),
    ("AGPRs", "agprs"),
    ("ScratchSize [bytes/lane]", "scratch"),
    ("Occupancy [waves/SIMD]", "occupancy"),
    ("SGPRs Spill", "sgpr_spills"),
    ("VGPRs Spill", "vgpr_spills"),
    ("LDS Size [bytes/block]", "lds"),
]
COLS = ["vgprs", "agprs", "sgprs", "scratch", "sgpr_spills", "vgpr_spills", "lds", "occupancy"]


def sources_sha(csrc):
    """The digest bench.py's kernel_sources_sha() computes, for the tree at csrc."""
    h = hashlib.sha256()
    files = sorted(f for f in os.listdir(csrc) if f.endswith((".hip", ".h", ".cpp")) or f == "Makefile")
    for f in files + ["../../include/lkfwd.h"]:
        p = os.path.join(csrc, f)
        if os.path.exists(p):
            h.update(f.encode())
            h.update(open(p, "rb").read())
    return h.hexdigest()[:16]


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
        return out.split("\n")[: len(names)]
    except (OSError, subprocess.CalledProcessError):
        return list(names)


def short_name(dem):
    """'void k_emit<96>(EmitArgs)' -> 'k_emit<96>'."""
    s = re.sub(r"^void\s+", "", dem).replace("(anonymous namespace)::", "")
    depth = 0
    for i, ch in enumerate(s):
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            return s[:i]
    return s


def remarks_of(hipcc, arch, csrc, src, flags):
    cmd = [hipcc, "-O3", "-std=c++17", "--offload-arch=" + arch, "-ffp-contract=off", "--cuda-device-only", "-c",
           "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull, src] + flags
    r = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stderr)
        raise SystemExit("%s: the compiler failed" % src)
    rows, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: .*?Function Name: (\S+)", line)
        if m:
            cur = {"file": src, "symbol": m.group(1)}
            rows.append(cur)
            continue
        if cur is None or "remark:" not in line:
            continue
        text = line.split("remark:", 1)[1]
        for label, key in FIELDS:
            m = re.search(r"\s" + re.escape(label) + r": (\d+)", text)
            if m:
                cur[key] = int(m.group(1))
                break
    return rows


def table(rows):
    out = ["| kernel | VGPRs | AGPRs | SGPRs | scratch B/lane | SGPR spills | VGPR spills | LDS B | waves/SIMD |",
           "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        out.append("| `%s` | %s |" % (r["kernel"], " | ".join(str(r.get(c, "")) for c in COLS)))
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--csrc", default=os.path.join(ROOT, "livekit-server_amd", "csrc"))
    ap.add_argument("--hipcc", default=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    ap.add_argument("--arch", default="gfx950")
    ap.add_argument("--flags", default="", help="extra compiler flags (e.g. -DLKF_CHECKED=1)")
    ap.add_argument("--files", default="", help="comma-separated kernel files (default: every *.hip)")
    ap.add_argument("--only", default="", help="print only kernels whose name contains this")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kernel_resources.json"))
    ap.add_argument("--diff", default="", help="another report: print the rows that differ from it")
    args = ap.parse_args()

    csrc = os.path.abspath(args.csrc)
    files = [f for f in args.files.split(",") if f] or sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))
    flags = args.flags.split()
    with ThreadPoolExecutor(max_workers=min(8, len(files))) as ex:
        parts = list(ex.map(lambda f: remarks_of(args.hipcc, args.arch, csrc, f, flags), files))
    rows = [r for p in parts for r in p]
    for r, d in zip(rows, demangle([r["symbol"] for r in rows])):
        r["kernel"] = short_name(d)
    rows.sort(key=lambda r: (r["file"], r["kernel"]))
    report = {"kernel_sources_sha": sources_sha(csrc), "arch": args.arch, "flags": flags, "kernels": rows}
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    shown = [r for r in rows if args.only in r["kernel"]]
    print(table(shown))
    if args.diff:
        other = {(r["file"], r["kernel"]): r for r in json.load(open(args.diff))["kernels"]}
        print("\nchanged against %s (%s):" % (args.diff, json.load(open(args.diff))["kernel_sources_sha"]))
        for r in rows:
            o = other.get((r["file"], r["kernel"]))
            if o is None:
                print("  new      %s" % r["kernel"])
                continue
            ch = ["%s %s -> %s" % (c, o.get(c), r.get(c)) for c in COLS if o.get(c) != r.get(c)]
            if ch:
                print("  %-28s %s" % (r["kernel"], ", ".join(ch)))


if __name__ == "__main__":
    main()
