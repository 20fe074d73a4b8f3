#!/usr/bin/env python3
"""Register and spill figures of the pool kernels, read from the compiler's own assembly.

Compiles duckdb-polr_amd/csrc/polr_pool.hip (flat pipeline: K = 2 / 4 / 6 / 8, counting and emitting) and
polr_poolg.hip (generic pipeline: POLR_EXT 0 and 1) to gfx950 assembly with the Makefile's flags, into a temporary
directory, and prints per kernel

  vgpr_count, vgpr_spill_count, sgpr_spill_count, private segment bytes      (the code object's metadata)
  spill instructions on the probe side / in the router's one-off code / in the router's STEP LOOP

A spill instruction is one the compiler marks "Folded Spill" or "Folded Reload" (a store to / load from scratch
memory).  The router's code begins at the `s_setprio 3` of pool_router_wave and ends at its "polr-router-end" marker
comment (where there is none: at the end of the kernel); inside it the step loop (wait, absorb, route, verify,
publish, rehearse) lies between the two marker comments polr_pool_router plants ("polr-router-steps-begin" / "-end").
Functions the kernel calls are executed once per step: all their spill instructions count for the step loop.

    python tools/spill_report.py                 # all builds, a table
    python tools/spill_report.py --build k4      # one build
    python tools/spill_report.py --json out.json

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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "duckdb-polr_amd")

BUILDS = {}
for _k in (2, 4, 6, 8):
    BUILDS["k%d" % _k] = ("polr_pool.hip", ["-DPOLR_K=%d" % _k, "-DPOLR_FLAT_EMIT=0"])
    BUILDS["e_k%d" % _k] = ("polr_pool.hip", ["-DPOLR_K=%d" % _k, "-DPOLR_FLAT_EMIT=1"])
BUILDS["g"] = ("polr_poolg.hip", ["-DPOLR_EXT=0"])
BUILDS["g_x"] = ("polr_poolg.hip", ["-DPOLR_EXT=1"])
# ... and the builds that fold into a fused ungrouped aggregate sink instead of writing row ids (the shipped shape of the fold)
BUILDS["g_a"] = ("polr_poolg.hip", ["-DPOLR_EXT=0", "-DPOLR_FUSE_AGG=2"])
BUILDS["g_ax"] = ("polr_poolg.hip", ["-DPOLR_EXT=1", "-DPOLR_FUSE_AGG=2"])
# ... and the measurement build of the fold's other shape (make fuseagg-ab)
BUILDS["g_a1"] = ("polr_poolg.hip", ["-DPOLR_EXT=0", "-DPOLR_FUSE_AGG=1"])
BUILDS["g_ax1"] = ("polr_poolg.hip", ["-DPOLR_EXT=1", "-DPOLR_FUSE_AGG=1"])
# ... and the dictionary encoder's kernels (no router: only the first five columns say something)
BUILDS["dict"] = ("polr_dict.hip", [])

ROUTER_ENTRY = re.compile(r"^\s*s_setprio\s+3\b")
STEPS_BEGIN = "polr-router-steps-begin"
STEPS_END = "polr-router-steps-end"
ROUTER_END = "polr-router-end"  # (absent in older sources: the router then runs to the end of the kernel)
SPILL = re.compile(r"Folded (Spill|Reload)")


def hipcc():
    return os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def have_hipcc():
    exe = hipcc()
    return os.path.isfile(exe) and os.access(exe, os.X_OK)


def make_flags():
    """HIPFLAGS exactly as the Makefile passes them."""
    out = subprocess.check_output(["make", "-s", "--no-print-directory", "-C", PKG, "hipflags"], text=True)
    return out.split()


def compile_asm(build, tmpdir, flags=None):
    src, defs = BUILDS[build]
    dst = os.path.join(tmpdir, build + ".s")
    cmd = [hipcc()] + (flags or make_flags()) + defs + ["--cuda-device-only", "-S", os.path.join(PKG, "csrc", src), "-o", dst]
    subprocess.check_call(cmd, stderr=subprocess.DEVNULL)
    return dst


def parse_metadata(text):
    """{kernel symbol: {vgpr_count, vgpr_spill_count, sgpr_spill_count, private_segment}} from .amdgpu_metadata"""
    kernels = {}
    m = re.search(r"\.amdgpu_metadata\n(.*?)\.end_amdgpu_metadata", text, re.S)
    if not m:
        return kernels
    # one list item of amdhsa.kernels per kernel: it begins "  - ." at the list's own indentation (its arguments are
    # list items too, deeper)
    for item in re.split(r"(?m)^  - (?=\.)", m.group(1))[1:]:
        cur = {}
        for key, val in re.findall(r"(?m)^\s*\.(name|vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s*(\S+)\s*$",
                                   item):
            if key == "name":
                # (arguments have names as well, indented deeper; the kernel's own comes last in the item)
                cur["name"] = val
            else:
                cur["private_segment" if key == "private_segment_fixed_size" else key] = int(val)
        if "name" in cur and "vgpr_count" in cur:
            kernels[cur["name"]] = cur
    return kernels


def split_functions(text):
    """[(symbol, [lines])] for every function body (label .. .Lfunc_endN)"""
    funcs = []
    types = set(re.findall(r"^\s*\.type\s+([^\s,]+),@function", text, re.M))
    name, body = None, []
    for line in text.splitlines():
        m = re.match(r"^([A-Za-z_$.][\w$.]*):", line)
        if m and m.group(1) in types and name is None:
            name, body = m.group(1), []
            continue
        if name is not None:
            if re.match(r"^\.Lfunc_end\d+:", line):
                funcs.append((name, body))
                name = None
            else:
                body.append(line)
    return funcs


def report_file(path):
    text = open(path).read()
    meta = parse_metadata(text)
    funcs = split_functions(text)
    callee_spills = sum(sum(1 for l in body if SPILL.search(l)) for name, body in funcs if name not in meta)
    callees = [name for name, _ in funcs if name not in meta]
    rows = []
    for name, body in funcs:
        if name not in meta:
            continue
        probe = once = steps = 0
        in_router = in_steps = False
        saw_steps = False
        for l in body:
            if ROUTER_ENTRY.match(l):
                in_router = True
            if ROUTER_END in l:
                in_router = False
            if STEPS_BEGIN in l:
                in_steps = saw_steps = True
            if STEPS_END in l:
                in_steps = False
            if SPILL.search(l):
                if not in_router:
                    probe += 1
                elif in_steps or not saw_steps:
                    steps += 1  # (no markers: the whole router counts as its step loop)
                else:
                    once += 1
        row = dict(meta[name])
        row.update(kernel=name, probe_spills=probe, router_once_spills=once, router_step_spills=steps + callee_spills,
                   callees=callees)
        rows.append(row)
    return rows


def report(builds, tmpdir=None):
    own = tmpdir is None
    if own:
        tmpdir = tempfile.mkdtemp(prefix="polr_spill_")
    try:
        flags = make_flags()
        out = {}
        for b in builds:
            out[b] = report_file(compile_asm(b, tmpdir, flags))
        return out
    finally:
        if own:
            shutil.rmtree(tmpdir, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--build", action="append", choices=sorted(BUILDS), help="builds to cover (default: all)")
    ap.add_argument("--json", help="also write the figures to this file")
    a = ap.parse_args()
    if not have_hipcc():
        sys.exit("hipcc not found")
    res = report(a.build or list(BUILDS))
    print("%-6s %5s %6s %6s %8s | %6s %7s %7s  kernel" % ("build", "vgpr", "vspill", "sspill", "private", "probe", "r.once", "r.step"))
    for b, rows in res.items():
        for r in rows:
            print("%-6s %5d %6d %6d %7dB | %6d %7d %7d  %s" % (b, r["vgpr_count"], r["vgpr_spill_count"], r["sgpr_spill_count"],
                                                                r["private_segment"], r["probe_spills"], r["router_once_spills"],
                                                                r["router_step_spills"], r["kernel"]))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
