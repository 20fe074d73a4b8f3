"""The plan of a pool launch, the part that needs no GPU: duckdb-polr_amd/csrc/polr_pool_plan.h as a stand-alone host
program (tests/poolplan/pool_plan_main.cpp: known answers of grid, ring and unit sizing, the effect of every tuning
field, the invariants the device code relies on over a sweep of shapes, and how a round is cut into units), built with the address +
undefined-behaviour sanitizers and run directly."""
import os
import re
import subprocess

import common

SRC = os.path.join(common.ROOT, "tests", "poolplan", "pool_plan_main.cpp")
HEADER = os.path.join(common.ROOT, "duckdb-polr_amd", "csrc", "polr_pool_plan.h")


def test_plan_program_under_sanitizers(tmp_path):
    assert os.path.isfile(HEADER), "duckdb-polr_amd/csrc/polr_pool_plan.h is missing"
    exe = str(tmp_path / "pool_plan")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            SRC, "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(run.stdout)
    assert run.returncode == 0, (run.stdout[-4000:], run.stderr[-4000:])
    assert "runtime error" not in run.stderr, run.stderr[-4000:]
    lines = run.stdout.strip().splitlines()
    assert lines[-1] == "ok" and not [l for l in lines if "FAILED" in l]
    # every row of the table, every input that must be refused, every tuning field, the whole sweep
    assert "known answers: 13 rows, 4 refused" in lines
    m = re.match(r"tuning answers: (\d+) checks", lines[1])
    assert m and int(m.group(1)) == 27, lines[1]
    m = re.match(r"invariants: (\d+) plans, (\d+) refused", lines[2])
    assert m and int(m.group(1)) + int(m.group(2)) == 2 * 2 * 4 * 4 * 8 * 16 * 8, lines[2]
    assert int(m.group(1)) > 0 and int(m.group(2)) > 0
    # how a round is cut into units: the known answers, and the whole table tests/test_pool_units.py reads
    assert "unit answers: 22 rows" in lines
    assert "unit table: %d lines" % (15 * 4 * 3 * 2 * 2 * 4) in lines
    assert len([l for l in lines if l.startswith("unit ") and " -> " in l]) == 15 * 4 * 3 * 2 * 2 * 4


def test_the_plan_header_needs_no_hip():
    """plain g++, <stdint.h> and the public header only: what lets the program above exist"""
    text = open(HEADER).read()
    includes = re.findall(r'^\s*#\s*include\s+[<"]([^>"]+)[>"]', text, re.M)
    assert sorted(includes) == sorted(["stdint.h", "../../include/polr_hip.h"]), includes
    # the constants the plan shares with the device code are defined once, here
    csrc = os.path.dirname(HEADER)
    for name in ["POLR_POOL_RINGS", "POLR_POOL_HI_TUPLES", "POLR_POOL_HI_UNIT", "POLR_SLOTS", "POLR_RES_TIMEOUT_TICKS"]:
        where = [f for f in sorted(os.listdir(csrc)) if f.endswith((".h", ".hip"))
                 and re.search(r"^\s*#\s*define\s+%s\b" % name, open(os.path.join(csrc, f)).read(), re.M)]
        assert where == ["polr_pool_plan.h"], (name, where)
