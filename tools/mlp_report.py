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

A second table covers what a probe wave does AROUND a unit (UNIT_REGIONS; scalar loads and waits on lgkmcnt count here too):

  polr-path-switch     flat_load_stages: the K stage records of another join order.  inner = 0: every record is asked
                       for before the first is waited for; words = the dwords asked for.
  polr-poll            polr_pool_look (the flat kernel's peek behind a unit's source): the adds of the tickets it lacks, their
                       waits, then ONE load with a lane per word and its wait; the generic kernels have no such region
  polr-arrive          pool_arrive: ret.at = returning counter atomics (one per copy: lane p adds counter p),
                       ret.wt = waits on vmcnt between it and the arrival add

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

# what a probe wave does AROUND a unit (a list of its own: the sweep's regions above are counted as before)
UNIT_REGIONS = ["polr-path-switch", "polr-poll", "polr-arrive"]
SWITCH_REGION, POLL_REGION, ARRIVE_REGION = UNIT_REGIONS

SMEM_LOAD = re.compile(r"^\s*s_load_dword(x(\d+))?\b")
VMEM_LOAD_W = re.compile(r"^\s*(?:global|buffer|flat)_load_dword(x(\d+))?\b")
ANY_WAIT = re.compile(r"^\s*s_waitcnt\b.*\b(vmcnt|lgkmcnt)\(")
ATOMIC = re.compile(r"^\s*global_atomic_\w+\s+(.*)$")

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


def unit_report_file(path):
    """The UNIT_REGIONS of every kernel in an assembly file: per region (summed over its copies)

      copies    how often the region was inlined
      loads     memory loads, scalar (s_load_*) or vector          words   dwords they ask for
      waits     s_waitcnt on vmcnt or lgkmcnt inside the region    inner   ... between a copy's first and last load
      ret_atomics  returning atomics (the counter adds of an arrival)
      ret_waits    vmcnt waits between a copy's first returning atomic and the next atomic that returns nothing (the
                   arrival add)

    A copy ends at its end marker; an arrival's copy also ends at its arrival add (the compiler lays the block with the
    end marker out wherever it likes, the add always follows the counter adds)."""
    text = open(path).read()
    meta = spill_report.parse_metadata(text)
    rows = []
    for name, body in spill_report.split_functions(text):
        if name not in meta:
            continue
        regions = {r: dict(copies=0, loads=0, words=0, waits=0, inner=0, ret_atomics=0, ret_waits=0) for r in UNIT_REGIONS}
        state = {}  # open region -> {"pending": waits since its last load or None, "after_ret": bool}
        for l in body:
            marker = False
            for r in UNIT_REGIONS:
                if r + "-begin" in l:
                    regions[r]["copies"] += 1
                    state[r] = dict(pending=None, after_ret=False)
                    marker = True
                elif r + "-end" in l:
                    state.pop(r, None)
                    marker = True
            if marker or not is_inst(l):
                continue
            for r in list(state):
                f, st = regions[r], state[r]
                m = SMEM_LOAD.match(l) or VMEM_LOAD_W.match(l)
                a = ATOMIC.match(l)
                if m:
                    f["loads"] += 1
                    f["words"] += int(m.group(2) or 1)
                    f["inner"] += st["pending"] or 0
                    st["pending"] = 0
                elif a and re.search(r"\bsc0\b", a.group(1)):
                    f["ret_atomics"] += 1
                    st["after_ret"] = True
                elif a:
                    if r == ARRIVE_REGION:
                        state.pop(r)
                elif ANY_WAIT.match(l):
                    f["waits"] += 1
                    if st["pending"] is not None:
                        st["pending"] += 1
                    if st["after_ret"] and VM_WAIT.match(l):
                        f["ret_waits"] += 1
        rows.append(dict(kernel=name, regions=regions))
    return rows


def unit_report(builds, tmpdir=None, csrc=None):
    """{build: rows of unit_report_file} -- compiles like report(); an assembly file already in tmpdir is read, not rebuilt"""
    own = tmpdir is None
    if own:
        tmpdir = tempfile.mkdtemp(prefix="polr_mlp_")
    try:
        flags = spill_report.make_flags()
        csrc = csrc or os.path.join(spill_report.PKG, "csrc")
        out = {}
        for b in builds:
            asm = os.path.join(tmpdir, b + ".s")
            out[b] = unit_report_file(asm if os.path.exists(asm) else compile_asm(b, tmpdir, flags, csrc))
        return out
    finally:
        if own:
            shutil.rmtree(tmpdir, ignore_errors=True)


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
    tmpdir = tempfile.mkdtemp(prefix="polr_mlp_")
    try:
        res = report(a.build or list(spill_report.BUILDS), tmpdir=tmpdir, csrc=a.csrc)
        units = unit_report(a.build or list(spill_report.BUILDS), tmpdir=tmpdir, csrc=a.csrc)
    finally:
        shutil.rmtree(tmpdir, ignore_errors=True)
    print("%-6s %-20s %6s %6s %6s %6s %6s  kernel" % ("build", "region", "copies", "loads", "waits", "inner", "insts"))
    for b, rows in res.items():
        for r in rows:
            print("%-6s %-20s %6s %6s %6s %6s %6d  %s" % (b, "(probe side)", "", "", "", "", r["probe_insts"], r["kernel"]))
            for reg in REGIONS:
                f = r["regions"][reg]
                if f["copies"]:
                    print("%-6s %-20s %6d %6d %6d %6d %6d" % (b, reg, f["copies"], f["loads"], f["waits"], f["inner"], f["insts"]))
    print()
    print("around a unit (join-order switch, the look for the next unit, arrival):")
    print("%-6s %-20s %6s %6s %6s %6s %6s %6s %6s  kernel" % ("build", "region", "copies", "loads", "words", "waits", "inner", "ret.at", "ret.wt"))
    for b, rows in units.items():
        for r in rows:
            first = True
            for reg in UNIT_REGIONS:
                f = r["regions"][reg]
                if f["copies"]:
                    print("%-6s %-20s %6d %6d %6d %6d %6d %6d %6d  %s" % (b, reg, f["copies"], f["loads"], f["words"], f["waits"], f["inner"],
                                                                       f["ret_atomics"], f["ret_waits"], r["kernel"] if first else ""))
                    first = False
    if a.json:
        for b in res:
            for row, urow in zip(res[b], units[b]):
                row["unit_regions"] = urow["regions"]
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
