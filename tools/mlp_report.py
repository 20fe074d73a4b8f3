#!/usr/bin/env python3
"""Memory-level parallelism of the flat pool kernel's sweep, read from the compiler's own assembly.

Compiles the pool kernels as tools/spill_report.py does (same builds, same flags) and counts, per build and per MARKED
REGION of the kernel,

  loads   vector-memory loads (global_load_* / buffer_load_* / flat_load_*; scratch reloads are not counted)
  waits   s_waitcnt instructions that carry a vmcnt field -- a wave stands still there until loads have come back
  inner   those of them that stand between the region's first and last load (a wait in front of the first load does
          not serialise the region's loads; it can still hold the wave until an older load -- stage 0's prefetch -- is home)
  insts   instructions

and per build the instruction count of the probe side (everything outside the router's code).  A region lies between
two marker comments the device code plants with `asm volatile("; <name>-begin")` / `-end`; a function that is inlined
several times leaves several copies, whose figures are summed (`copies` says how many):

  polr-sweep-keys      flat_sweep phase 1 on the plain path (no selection vector, no validity column on a deeper
                       stage): the pops and the key gathers of ALL deeper stages.  waits = 0 means that no gather waits
                       for another one.
  polr-sweep-tables    flat_sweep phase 2: the bit words of all perfect-table stages (LDS or global memory)
  polr-sweep-sel-keys  phase 1 with a selection vector and / or validity columns: all rows, ONE wait, all keys and
                       validity bytes
  polr-stage0-slow     the lane-per-tuple step of stage 0 (selection, validity or an unaligned tail)

    python tools/mlp_report.py                 # all builds, a table
    python tools/mlp_report.py --build k4      # one build
    python tools/mlp_report.py --csrc DIR      # another copy of the device sources (e.g. an older revision)
    python tools/mlp_report.py --json out.json

No GPU needed: this is a cross-compile.
"""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spill_report  # noqa: E402  (builds, flags, function splitting)

REGIONS = ["polr-sweep-keys", "polr-sweep-tables", "polr-sweep-sel-keys", "polr-stage0-slow"]
PLAIN_REGIONS = ["polr-sweep-keys", "polr-sweep-tables"]  # (no wait on vmcnt allowed inside)
SEL_REGION = "polr-sweep-sel-keys"

VMEM_LOAD = re.compile(r"^\s*(global_load_|buffer_load_|flat_load_)")
VM_WAIT = re.compile(r"^\s*s_waitcnt\b.*\bvmcnt\(")
INST = re.compile(r"^\s+[a-z][a-z0-9_]*\b")  # (directives begin with '.', labels at column 0, comments with ';')


def is_inst(line):
    return bool(INST.match(line)) and not line.lstrip().startswith((".", ";"))


def compile_asm(build, tmpdir, flags, csrc):
    src, defs = spill_report.BUILDS[build]
    dst = os.path.join(tmpdir, build + ".s")
    cmd = [spill_report.hipcc()] + flags + defs + ["--cuda-device-only", "-S", os.path.join(csrc, src), "-o", dst]
    subprocess.check_call(cmd, stderr=subprocess.DEVNULL)
    return dst


def report_file(path):
    text = open(path).read()
    meta = spill_report.parse_metadata(text)
    rows = []
    for name, body in spill_report.split_functions(text):
        if name not in meta:
            continue
        regions = {r: dict(copies=0, loads=0, waits=0, inner=0, insts=0) for r in REGIONS}
        open_regions = set()
        pending = {r: None for r in REGIONS}  # waits since the copy's last load (None: no load yet in this copy)
        in_router = False
        probe_insts = 0
        for l in body:
            if spill_report.ROUTER_ENTRY.match(l):
                in_router = True
            if spill_report.ROUTER_END in l:
                in_router = False
            marker = False
            for r in REGIONS:
                if r + "-begin" in l:
                    open_regions.add(r)
                    regions[r]["copies"] += 1
                    pending[r] = None
                    marker = True
                elif r + "-end" in l:
                    open_regions.discard(r)
                    marker = True
            if marker or not is_inst(l):
                continue
            if not in_router:
                probe_insts += 1
            for r in open_regions:
                regions[r]["insts"] += 1
                if VMEM_LOAD.match(l):
                    regions[r]["loads"] += 1
                    regions[r]["inner"] += pending[r] or 0
                    pending[r] = 0
                elif VM_WAIT.match(l):
                    regions[r]["waits"] += 1
                    if pending[r] is not None:
                        pending[r] += 1
        rows.append(dict(kernel=name, probe_insts=probe_insts, regions=regions))
    return rows


def report(builds, tmpdir=None, csrc=None):
    own = tmpdir is None
    if own:
        tmpdir = tempfile.mkdtemp(prefix="polr_mlp_")
    try:
        flags = spill_report.make_flags()
        csrc = csrc or os.path.join(spill_report.PKG, "csrc")
        return {b: report_file(compile_asm(b, tmpdir, flags, csrc)) for b in builds}
    finally:
        if own:
            shutil.rmtree(tmpdir, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--build", action="append", choices=sorted(spill_report.BUILDS), help="builds to cover (default: all)")
    ap.add_argument("--csrc", help="directory of the device sources (default: duckdb-polr_amd/csrc)")
    ap.add_argument("--json", help="also write the figures to this file")
    a = ap.parse_args()
    if not spill_report.have_hipcc():
        sys.exit("hipcc not found")
    res = report(a.build or list(spill_report.BUILDS), csrc=a.csrc)
    print("%-6s %-20s %6s %6s %6s %6s %6s  kernel" % ("build", "region", "copies", "loads", "waits", "inner", "insts"))
    for b, rows in res.items():
        for r in rows:
            print("%-6s %-20s %6s %6s %6s %6s %6d  %s" % (b, "(probe side)", "", "", "", "", r["probe_insts"], r["kernel"]))
            for reg in REGIONS:
                f = r["regions"][reg]
                if f["copies"]:
                    print("%-6s %-20s %6d %6d %6d %6d %6d" % (b, reg, f["copies"], f["loads"], f["waits"], f["inner"], f["insts"]))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
