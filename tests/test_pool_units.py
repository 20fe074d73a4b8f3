"""tests/poolunits.py, the Python restatement of how a round is cut into units, against the device library's own function
(polr_pool_unit_size, duckdb-polr_amd/csrc/polr_pool_plan.h): every line of the table the plan program prints
(tests/poolplan/pool_plan_main.cpp, built without sanitizers here; tests/test_pool_plan.py runs it under them).  No GPU."""
import os
import re
import subprocess

import pytest

import common
import poolunits

SRC = os.path.join(common.ROOT, "tests", "poolplan", "pool_plan_main.cpp")
LINE = re.compile(r"^unit (\d+) (\d+) (\d+) (\d+) (\d+) (\d+) (\d+) -> (\d+) (\d+)$")


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("poolunits") / "pool_plan")
    build = subprocess.run(["g++", "-std=c++17", "-O1", SRC, "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout[-4000:], run.stderr[-4000:])
    rows = [tuple(int(v) for v in m.groups()) for m in map(LINE.match, run.stdout.splitlines()) if m]
    assert "unit table: %d lines" % len(rows) in run.stdout.splitlines() and len(rows) > 1000
    return rows


def test_restatement_equals_every_line_of_the_table(table):
    for t, waves, active, gran, hi_tuples, units_x, hi_unit, unit, n_units in table:
        got = poolunits.unit_size(t, waves, active, gran, hi_tuples, units_x, hi_unit)
        assert got == (unit, n_units), (t, waves, active, gran, hi_tuples, units_x, hi_unit)
    # the table reaches both sides of every rule
    units = {r[7] for r in table}
    assert {64, 320, 512, 1024, 2560, 65536} <= units
    assert any(r[0] <= r[4] for r in table) and any(r[0] > r[4] for r in table)


def test_the_router_composes_the_same_two_expressions():
    """the routers' polr_pool_size_units (polr_pool_device.h) keeps the small-round branch of its own, because it picks the
    round's queue there; everything else must be the two expressions the host program checks: no arithmetic of its own"""
    text = open(os.path.join(common.ROOT, "duckdb-polr_amd", "csrc", "polr_pool_device.h")).read()
    m = re.search(r"void polr_pool_size_units\([^)]*\)\s*\{(.*?)\n\}", text, re.S)
    assert m
    body = re.sub(r"//[^\n]*", "", m.group(1))
    assert "if (tuples <= hi_tuples)" in body and "r.unit = hi_unit;" in body
    assert "r.unit = polr_pool_big_unit(tuples, pool_waves, n_exec, gran, units_x);" in body
    assert "r.n_units = polr_pool_units_of(tuples, r.unit);" in body
    assert not re.search(r"[/%&*+-]", body.replace("&r", "")), body


def test_source_rows_for_gives_the_unit_it_names(table):
    """for every plan of the table (probe waves, gran, units_x, hi_tuples, hi_unit) and one executor: a source of
    source_rows_for(unit) rows, and one 300 rows shorter, runs in units of `unit`; one row more does not (below the cap)"""
    plans = sorted({(r[1], r[3], r[4], r[5], r[6]) for r in table})
    checked = 0
    for waves, gran, hi_tuples, units_x, hi_unit in plans:
        info = {"pool_waves": waves, "gran": gran, "hi_tuples": hi_tuples, "units_x": units_x, "hi_unit": hi_unit}
        for unit in (gran, 2 * gran, 1024, 1536, 2560, 4096, 8192, 65536):
            target = max(16, units_x * waves)
            if unit % gran or target * unit - 300 <= hi_tuples:  # (not a unit of this kernel / a small round)
                continue
            rows = poolunits.source_rows_for(unit, info, units_x)
            checked += 1
            assert poolunits.unit_of(rows, info) == unit and poolunits.unit_of(rows - 300, info) == unit
            if unit > 300:
                assert poolunits.unit_size(rows - 300, waves, 1, gran, hi_tuples, units_x, hi_unit)[1] == target
            if unit < 65536:
                assert poolunits.unit_of(rows + 1, info) == unit + gran
            else:
                assert poolunits.unit_of(rows + 70000, info) == 65536
    assert checked > 300
    with pytest.raises(AssertionError):
        poolunits.source_rows_for(2560, dict(info, units_x=1), 4)
