"""What polr_pipeline_create decides, the part that needs no GPU: duckdb-polr_amd/csrc/polr_pipeline_plan.h as a
stand-alone host program (tests/pipeplan/pipe_plan_main.cpp: known answers for tuple slots, multiplicities, the flat
kernel and its LDS tables, every refusal with its code and whole message, and the invariants the device code relies on
over a seeded sweep of random valid pipelines), built plain and with the address + undefined-behaviour sanitizers, and
run directly."""
import os
import re
import subprocess

import pytest

import common

SRC = os.path.join(common.ROOT, "tests", "pipeplan", "pipe_plan_main.cpp")
CSRC = os.path.join(common.ROOT, "duckdb-polr_amd", "csrc")
HEADER = os.path.join(CSRC, "polr_pipeline_plan.h")

# the CHECK()s each group of the program passes through, counted by hand from its source
GROUPS = [
    ("slots", 3 + 5 + 4 + 2 + 3 + 1),
    ("mult and unique", 2 + 1 + 2 + (1 + 5 + 1 + 1)),
    # (flat_of() is a CHECK of its own: every call counts twice)
    ("flat", (2 + 1) + (2 + 2 + 1) + 2 + 2 + 2 + 2 + 4 * 2 + 5 * 2 + 2 + 2 * 2 + (2 + 1)),
    ("lds tables", (1 + 6) + (1 + 2) + (1 + 3) + 2 * 2 + (1 + 2) + 6 * 2 + 13 * 2),
    # limits, descriptors, paths, columns, and the order of the passes: refused or accepted, one CHECK per input
    ("refusals", 7 + 9 + 5 + 21 + 3),
]


@pytest.mark.parametrize("sanitize", [None, "address,undefined"], ids=["plain", "asan-ubsan"])
def test_plan_program(tmp_path, sanitize):
    assert os.path.isfile(HEADER), "duckdb-polr_amd/csrc/polr_pipeline_plan.h is missing"
    exe = str(tmp_path / "pipe_plan")
    flags = ["-fsanitize=" + sanitize, "-fno-sanitize-recover=all"] if sanitize else []
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall"] + flags + [SRC, "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(run.stdout)
    assert run.returncode == 0, (run.stdout[-4000:], run.stderr[-4000:])
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-4000:]
    lines = run.stdout.strip().splitlines()
    assert lines[-1] == "ok" and not [l for l in lines if "FAILED" in l]
    assert lines[:len(GROUPS)] == ["%s: %d checks" % g for g in GROUPS]
    m = re.match(r"invariants: (\d+) plans, (\d+) flat, (\d+) emitting, (\d+) with multiplicities, (\d+) LDS tables, "
                 r"(\d+) shared$", lines[len(GROUPS)])
    assert m, lines[len(GROUPS)]
    plans, flat, emit, mult, tables, shared = [int(g) for g in m.groups()]
    # the sweep reaches every kind of plan the invariants speak about
    assert plans == 4000
    assert 0 < emit < flat < plans and mult > 0 and tables > 0 and shared > 0


def test_the_plan_header_needs_no_hip():
    """plain g++, standard headers and the public header only: what lets the program above exist"""
    text = open(HEADER).read()
    includes = re.findall(r'^\s*#\s*include\s+[<"]([^>"]+)[>"]', text, re.M)
    assert not [i for i in includes if i.startswith("hip/")], includes
    assert [i for i in includes if '/' in i or i.startswith("polr_")] == ["../../include/polr_hip.h"], includes
    # the constants the plan shares with the device structs are defined once, here
    for name in ["POLR_KMAX", "POLR_PMAX", "POLR_NKEYS", "POLR_NPREDS"]:
        where = [f for f in sorted(os.listdir(CSRC)) if f.endswith((".h", ".hip"))
                 and re.search(r"^\s*#\s*define\s+%s\b" % name, open(os.path.join(CSRC, f)).read(), re.M)]
        assert where == ["polr_pipeline_plan.h"], (name, where)
    where = [f for f in sorted(os.listdir(CSRC)) if f.endswith((".h", ".hip"))
             and re.search(r"\bKIND_PERFECT\s*=", open(os.path.join(CSRC, f)).read())]
    assert where == ["polr_pipeline_plan.h"], where
    # ... and tied to the ABI's limits by the compiler
    for pair in ["POLR_KMAX == POLR_MAX_JOINS", "POLR_PMAX == POLR_MAX_PATHS", "POLR_NKEYS == POLR_MAX_KEYS",
                 "POLR_NPREDS == POLR_MAX_PREDS"]:
        assert "static_assert(" + pair in text, pair
