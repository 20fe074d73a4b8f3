"""Aggregates whose argument is `left OP right` (polr_out_aggregate*_expr), CPU part.

tests/golden/expr_aggregates.json holds the REFERENCE's answers (tests/golden/make_golden_expr_agg.py): SSB flight 1 as
shipped, SSB-skew Q4.1's GROUP BY over sums of a difference / sum / product, the query it refuses when the measures are
UINTEGER, and (probe column, build payload column) pairs with NULLs.  Here: the oracle's join rows plus exact Python integer
arithmetic reproduce every value; a Python model of the range rule -- each non-NULL row's exact result must lie in the type the
binder gave the expression -- reproduces which queries the reference refused; header, library and binding agree on the three
new entry points.  The GPU part is tests/test_gpu_expr_aggregates.py."""
import ctypes as C
import json
import operator
import os
import re

import numpy as np
import pytest

import common
from common import orc, workloads
from polr_amd import capi

GOLD = json.load(open(os.path.join(common.GOLDEN, "expr_aggregates.json")))
OPS = {"+": operator.add, "-": operator.sub, "*": operator.mul}
SQL_DTYPE = {"TINYINT": np.int8, "UTINYINT": np.uint8, "SMALLINT": np.int16, "USMALLINT": np.uint16, "INTEGER": np.int32,
             "UINTEGER": np.uint32, "BIGINT": np.int64}
NAMES = ["polr_out_aggregate_expr", "polr_out_aggregate_grouped_expr", "polr_out_aggregate_hashed_expr"]


def expr_values(op, left, lvalid, right, rvalid, sql_type):
    """the model of the reference's projection: -> (the non-NULL in-range results as Python ints, rows out of range).
    A row with a NULL operand has a NULL argument and cannot overflow; every other row's exact result must lie in the
    result type (TryAddOperator / TrySubtractOperator / TryMultiplyOperator)."""
    info = np.iinfo(SQL_DTYPE[sql_type])
    lo, hi = int(info.min), int(info.max)
    lv = [True] * len(left) if lvalid is None else lvalid.tolist()
    rv = [True] * len(right) if rvalid is None else rvalid.tolist()
    vals, out_of_range = [], 0
    for x, xo, y, yo in zip(left.tolist(), lv, right.tolist(), rv):
        if not (xo and yo):
            continue
        r = OPS[op](int(x), int(y))
        if r < lo or r > hi:
            out_of_range += 1
        else:
            vals.append(r)
    return vals, out_of_range


def py_agg(fn, vals):
    if fn == "count":
        return len(vals)
    return {"sum": sum, "min": min, "max": max}[fn](vals) if vals else None


# ---- SSB flight 1 ----------------------------------------------------------------------------------------------------------
def flight1_rows(wl, name):
    """oracle: pushed-down scan filter -> join -> output rows of query `name`"""
    q = workloads.ssb_flight1_query(wl, name)
    names = list(q["probe"]["cols"].keys())
    cols = list(q["probe"]["cols"].values())
    sel, offs = orc.scan_filter(cols, [(names.index(c), op, v) for c, op, v in q["probe"]["filter"]])
    pcols, pvalid, joins = common.oracle_joins(q)
    res = orc.run_pipeline(pcols, joins, [[0]], routing="default_path", sel=sel, chunk_offsets=offs)
    return q, sel, res["out_rows"]


@pytest.mark.parametrize("name", ["q1.1", "q1.2", "q1.3"])
def test_oracle_flight1_matches_reference(name):
    g = GOLD["flight1"]
    wl = workloads.ssb_flight1()
    q, sel, rows = flight1_rows(wl, name)
    want = g["queries"][name]
    assert q["sql_where"] == want["sql_where"]
    assert len(sel) == want["filtered_rows"]
    assert len(rows) >= 1, "the query must select something at the fixture's scale"
    price, _ = orc.materialize_column(rows, 1, -1, wl["probe"]["cols"]["lo_extendedprice"], None)
    disc, _ = orc.materialize_column(rows, 1, -1, wl["probe"]["cols"]["lo_discount"], None)
    vals, oor = expr_values("*", price, None, disc, None, g["typeof"])
    assert oor == 0
    got = [py_agg(fn, vals) for fn in g["aggregates"][:4]] + [len(rows)]
    assert got == want["values"]


def test_flight1_date_columns_follow_the_day_index():
    d = workloads.ssb_flight1()["date_full"]
    assert np.array_equal(d["d_yearmonthnum"] // 100, d["d_year"])
    month, week = d["d_yearmonthnum"] % 100, d["d_weeknuminyear"]
    assert month.min() == 1 and month.max() == 12 and week.min() == 1 and week.max() in (52, 53)
    same_year = d["d_year"][1:] == d["d_year"][:-1]
    assert np.all(np.diff(month.astype(int))[same_year] >= 0) and np.all(np.diff(week.astype(int))[same_year] >= 0)


# ---- SSB-skew Q4.1, GROUP BY d_year, c_nation -----------------------------------------------------------------------------------
def q41_columns():
    wl = workloads.ssb_skew_q41(sf=0.2)
    pcols, pvalid, joins = common.oracle_joins(wl)
    k = len(joins)
    rows = orc.run_pipeline(pcols, joins, [list(range(k))], routing="default_path")["out_rows"]
    rev, _ = orc.materialize_column(rows, k, -1, wl["probe"]["cols"]["lo_revenue"], None)
    sup, _ = orc.materialize_column(rows, k, -1, wl["probe"]["cols"]["lo_supplycost"], None)
    nat, _ = orc.materialize_column(rows, k, 0, wl["joins"][0]["payload"]["c_nation"], None)
    yr, _ = orc.materialize_column(rows, k, 3, wl["joins"][3]["payload"]["d_year"], None)
    return rev, sup, yr, nat


def q41_exprs():
    """[(fn, op)] of the fixture's aggregate columns, e.g. "sum(-)" """
    return [re.match(r"(\w+)\((.)\)", c).groups() for c in GOLD["q41"]["columns"][3:]]


def test_oracle_q41_expressions_match_reference():
    g = GOLD["q41"]
    rev, sup, yr, nat = q41_columns()
    groups = {}
    for i, key in enumerate(zip(yr.tolist(), nat.tolist())):
        groups.setdefault(key, []).append(i)
    got = []
    for key in sorted(groups):
        idx = np.asarray(groups[key])
        row = [key[0], key[1], len(idx)]
        for fn, op in q41_exprs():
            vals, oor = expr_values(op, rev[idx], None, sup[idx], None, g["typeof"][op])
            assert oor == 0
            row.append(py_agg(fn, vals))
        got.append(row)
    assert got == g["rows"]
    assert any(r[4] < 0 for r in g["rows"]), "negative differences: signed results are exercised"


def test_range_model_reproduces_what_the_reference_refused():
    """measures declared INTEGER: every row in range, the reference answered; declared UINTEGER (what the arrays are): the
    differences below zero are out of range, the reference refused the query"""
    rev, sup, _, _ = q41_columns()
    for op in "-+*":
        assert expr_values(op, rev, None, sup, None, GOLD["q41"]["typeof"][op])[1] == 0
    err = GOLD["q41_error"]
    n_bad = expr_values("-", rev, None, sup, None, err["typeof"]["-"])[1]
    assert n_bad == int((rev.astype(np.int64) < sup.astype(np.int64)).sum()) and n_bad > 0
    assert err["exit_status"] == 3 and "Overflow in subtraction" in err["stderr"]
    assert expr_values("+", rev, None, sup, None, err["typeof"]["+"])[1] == 0


# ---- NULLs and mixed sources: star_skew_nulls ---------------------------------------------------------------------------------
def nulls_scenario():
    wl = workloads.star_skew(n_fact=60_000, with_nulls=True)
    pcols, pvalid, joins = common.oracle_joins(wl)
    k = len(joins)
    rows = orc.run_pipeline(pcols, joins, [list(range(k))], routing="default_path", probe_valid=pvalid)["out_rows"]
    return wl, k, rows


def test_oracle_null_pairs_match_reference():
    wl, k, rows = nulls_scenario()
    assert len(GOLD["nulls"]) >= 3
    refused = 0
    for pair in GOLD["nulls"]:
        j = wl["joins"][pair["join"]]
        left, lv = orc.materialize_column(rows, k, -1, wl["probe"]["cols"][pair["probe_col"]],
                                          wl["probe"].get("valid", {}).get(pair["probe_col"]))
        right, rv = orc.materialize_column(rows, k, pair["join"], j["payload"][pair["build_col"]],
                                           j.get("payload_valid", {}).get(pair["build_col"]))
        assert rv is not None and not rv.all(), "the pair has NULLs on the build side"
        for op, g in pair["exprs"].items():
            if g.get("unsupported"):
                assert g["typeof"] not in SQL_DTYPE
                continue
            vals, oor = expr_values(op, left, lv, right, rv, g["typeof"])
            if "stderr" in g:  # the reference refused it
                assert oor > 0 and g["exit_status"] == 3 and "Overflow in" in g["stderr"]
                refused += 1
                continue
            assert oor == 0
            assert len(rows) == g["count_star"]
            assert {fn: py_agg(fn, vals) for fn in ("count", "sum", "min", "max")} == \
                {fn: g[fn] for fn in ("count", "sum", "min", "max")}, (pair, op)
            assert g["count"] < g["count_star"]
    assert refused >= 1


# ---- the three entry points -------------------------------------------------------------------------------------------------
def test_header_library_and_binding_have_the_expression_entry_points():
    text = open(os.path.join(common.ROOT, "include", "polr_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = capi.load()
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, code), "include/polr_hip.h does not declare %s" % n
        assert hasattr(lib, n), "libpolr_hip.so does not export %s" % n
        assert n in capi.EXPORTS
        assert getattr(lib, n).argtypes is not None
        assert hasattr(capi.Output, n[len("polr_out_"):])
    assert lib.polr_abi_version() == 1  # (additive: the ABI version stays)
    assert re.search(r"POLR_E_RANGE\s*=\s*-7\b", code) and capi.E_RANGE == -7
    m = re.search(r"enum\s*\{\s*POLR_ARG_COLUMN\s*=\s*0,\s*POLR_ARG_ADD\s*=\s*1,\s*POLR_ARG_SUB\s*=\s*2,\s*POLR_ARG_MUL\s*=\s*3\s*\}", code)
    assert m and capi.ARG == {"column": 0, "+": 1, "-": 2, "*": 3}
    # the struct as the header lays it out: 4 + 4 + 8 + 8 + 4 + 4 bytes
    assert C.sizeof(capi.AggExpr) == 32 and capi.AggExpr.result_width.offset == 24


def test_null_handles_are_refused_without_a_device():
    lib = capi.load()
    n = C.c_uint64(7)
    assert lib.polr_out_aggregate_expr(None, None, None, 1, None, C.byref(n)) == capi.E_INVALID
    assert lib.polr_out_aggregate_grouped_expr(None, None, None, 1, None, 1, None, 1, None, C.byref(n)) == capi.E_INVALID
    assert lib.polr_out_aggregate_hashed_expr(None, None, None, 1, None, 1, 1, None, None, None, None, None, 0, None,
                                              C.byref(n)) == capi.E_INVALID
    assert n.value == 7
