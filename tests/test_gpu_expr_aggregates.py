"""Aggregates whose argument is `left OP right` on the device: polr_out_aggregate_expr, _grouped_expr, _hashed_expr.

Reads tests/golden/expr_aggregates.json (the REFERENCE's answers, tests/golden/make_golden_expr_agg.py) and never the
reference: SSB flight 1 end to end, SSB-skew Q4.1 through both GROUP BY sinks and the query the reference refuses, the
NULL / mixed-source pairs; then a type x operator matrix against exact Python over the row ids of the three probe engines
of tests/test_gpu_sink_matrix.py, the plain-column form against the existing entry points, and the refusals.

POLR_E_RANGE counts (row, aggregate) arguments: a call with four aggregates over one expression that is out of range for N
rows reports 4 N."""
import ctypes as C
import json
import operator
import os
import re

import numpy as np
import pytest

import common
from common import workloads
from polr_amd import capi
from test_gpu_sink_matrix import ENGINES, INT_TYPES, Star

pytestmark = pytest.mark.gpu

GOLD = json.load(open(os.path.join(common.GOLDEN, "expr_aggregates.json")))
OPS = {"+": operator.add, "-": operator.sub, "*": operator.mul}
SQL_DTYPE = {"TINYINT": np.int8, "UTINYINT": np.uint8, "SMALLINT": np.int16, "USMALLINT": np.uint16, "INTEGER": np.int32,
             "UINTEGER": np.uint32, "BIGINT": np.int64}
SENTINEL = 0x5A


def expr_values(op, left, lvalid, right, rvalid, dtype):
    """exact Python: (the non-NULL in-range results, the rows out of range of dtype)"""
    info = np.iinfo(dtype)
    lo, hi = int(info.min), int(info.max)
    vals, bad = [], 0
    for x, xo, y, yo in zip(left.tolist(), lvalid.tolist(), right.tolist(), rvalid.tolist()):
        if xo and yo:
            r = OPS[op](int(x), int(y))
            if lo <= r <= hi:
                vals.append(r)
            else:
                bad += 1
    return vals, bad


def py_agg(fn, vals):
    if fn == "count":
        return len(vals)
    return {"sum": sum, "min": min, "max": max}[fn](vals) if vals else None


# ---- SSB flight 1 end to end -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["q1.1", "q1.2", "q1.3"])
def test_device_flight1_matches_reference(gpu_ctx, name):
    """polr_pipeline_scan_filter -> resident run -> polr_out_aggregate_expr: SUM(lo_extendedprice * lo_discount) as shipped,
    with MIN / MAX / COUNT of the same product and COUNT(*); only the five values leave the GPU"""
    g = GOLD["flight1"]
    want = g["queries"][name]
    q = workloads.ssb_flight1_query(workloads.ssb_flight1(), name)
    names = list(q["probe"]["cols"].keys())
    cols = list(q["probe"]["cols"].values())
    joins = capi.build_joins(gpu_ctx, q, auto=True)
    pipe = capi.Pipeline(gpu_ctx, cols, len(cols[0]), joins, [[0]])
    n_sel, n_chunks = pipe.scan_filter([(names.index(c), op, v) for c, op, v in q["probe"]["filter"]])
    assert n_sel == want["filtered_rows"]
    out = capi.Output(pipe, 1024, 8192)
    mpx = capi.DeviceMultiplexer(pipe, "default_path")
    mpx.use_scan_chunks()
    capi.run_resident([mpx], [(0, n_chunks)], out=out, reset=True, finish=True)
    mpx.finish()
    left, right = (-1, names.index("lo_extendedprice")), (-1, names.index("lo_discount"))
    rtype = SQL_DTYPE[g["typeof"]]
    specs = [(fn, "*", left, right, rtype) for fn in g["aggregates"][:4]] + [("count_star", "column", left, None, None)]
    assert out.aggregate_expr(specs) == want["values"]
    mpx.close()
    pipe.close()


# ---- SSB-skew Q4.1: both GROUP BY sinks, and the query the reference refuses --------------------------------------------------------
def _q41_specs(cols, rtype_of):
    specs = []
    for c in GOLD["q41"]["columns"][3:]:
        fn, op = re.match(r"(\w+)\((.)\)", c).groups()
        specs.append((fn, op, cols[0], cols[1], rtype_of[op]))
    return specs


def test_device_q41_expressions_grouped_and_hashed(gpu_ctx):
    g = GOLD["q41"]
    wl = workloads.ssb_skew_q41(sf=0.2)
    joins = capi.build_joins(gpu_ctx, wl, auto=True)
    names = list(wl["probe"]["cols"].keys())
    cols = list(wl["probe"]["cols"].values())
    rev, sup = wl["probe"]["cols"]["lo_revenue"], wl["probe"]["cols"]["lo_supplycost"]
    # the measures twice: as the workload has them (UINTEGER) and as the fixture's query declares them (INTEGER)
    cols += [rev.astype(np.int32), sup.astype(np.int32)]
    u_cols = [(-1, names.index("lo_revenue")), (-1, names.index("lo_supplycost"))]
    i_cols = [(-1, len(names)), (-1, len(names) + 1)]
    n = len(cols[0])
    paths = np.asarray(common.load_golden("ssb_skew_q41")["paths"], dtype=np.int32)
    pipe = capi.Pipeline(gpu_ctx, cols, n, joins, paths)
    out = capi.Output(pipe, 1024, 8192)
    mpx = capi.DeviceMultiplexer(pipe, "adaptive_reinit")
    capi.run_resident([mpx], [(0, (n + 1023) // 1024)], out=out, reset=True, finish=True)
    mpx.finish()
    want = {(r[0], r[1]): r[2:] for r in g["rows"]}
    years = sorted({r[0] for r in g["rows"]})
    y0, ny = years[0], years[-1] - years[0] + 1
    keys = [(3, 0, y0, ny), (0, 0, 0, 25)]  # d_year (payload 0 of join 3), c_nation (payload 0 of join 0)
    assert g["operand_type"] == "INTEGER"
    specs = [("count_star", "column", i_cols[0], None, None)] + _q41_specs(i_cols, {o: SQL_DTYPE[t] for o, t in g["typeof"].items()})
    vals, counts, dropped = out.aggregate_grouped_expr(keys, specs)
    assert dropped == 0
    seen = 0
    for gi, v in enumerate(vals):
        key = (y0 + gi // 25, gi % 25)
        if key in want:
            assert v == want[key], key
            seen += 1
        else:
            assert v[0] == 0 and v[1] is None and v[4] == 0
    assert seen == len(want)
    hashed = out.aggregate_hashed_expr([(3, 0), (0, 0)], specs, 1024)
    assert hashed == want
    # ---- the UINTEGER declaration: what the arrays are, and what the reference refuses ("Overflow in subtraction") ----
    err = GOLD["q41_error"]
    assert err["exit_status"] == 3 and "Overflow in subtraction" in err["stderr"] and err["operand_type"] == "UINTEGER"
    ids = out.fetch_ids()
    r_out, s_out = rev[ids[:, 0]].astype(np.int64), sup[ids[:, 0]].astype(np.int64)
    n_bad = int((r_out < s_out).sum())
    assert n_bad > 0
    uspecs = [("count_star", "column", u_cols[0], None, None)] + _q41_specs(u_cols, {o: SQL_DTYPE[t] for o, t in err["typeof"].items()})
    n_minus = sum(1 for s in uspecs if s[1] == "-")
    for call in (lambda k: out.aggregate_grouped_expr(k, uspecs), lambda k: out.aggregate_hashed_expr([x[:2] for x in k], uspecs, 1024)):
        for k in (keys, [(3, 0, y0, 1), (0, 0, 0, 25)]):  # (rows a narrow domain drops are checked all the same)
            with pytest.raises(capi.PolrError) as e:
                call(k)
            assert e.value.code == capi.E_RANGE and e.value.count == n_minus * n_bad
            assert "aggregate 1" in str(e.value)  # (the first aggregate with a row out of range: sum(-))
    # ... and every result buffer still holds what the caller wrote
    na, n_groups = len(uspecs), ny * 25
    sa = capi.make_agg_exprs(uspecs)
    ka = (capi.GroupKey * 2)()
    for i, (sj, sc, mn, nv) in enumerate(keys):
        ka[i].src_join, ka[i].src_col, ka[i].min_value, ka[i].n_values = sj, sc, mn, nv
    res = (capi.AggValue * (n_groups * na))()
    C.memset(res, SENTINEL, C.sizeof(res))
    dropped, oor = C.c_uint64(77), C.c_uint64(0)
    rc = gpu_ctx.L.polr_out_aggregate_grouped_expr(out.h, None, ka, 2, sa, na, res, n_groups, C.byref(dropped), C.byref(oor))
    assert rc == capi.E_RANGE and oor.value == n_minus * n_bad and dropped.value == 77
    assert bytes(res) == bytes([SENTINEL]) * C.sizeof(res)
    res = (capi.AggValue * (1024 * na))()
    C.memset(res, SENTINEL, C.sizeof(res))
    gkeys = np.full((1024, 2), -3, np.int64)
    gnulls = np.full(1024, 0xABCD, np.uint32)
    arena = np.full(64, SENTINEL, np.uint8)
    n_g, used, oor = C.c_uint64(55), C.c_uint64(0), C.c_uint64(0)
    rc = gpu_ctx.L.polr_out_aggregate_hashed_expr(out.h, None, ka, 2, sa, na, 1024, gkeys.ctypes.data, gnulls.ctypes.data, res,
                                                  C.byref(n_g), arena.ctypes.data, 64, C.byref(used), C.byref(oor))
    assert rc == capi.E_RANGE and oor.value == n_minus * n_bad and n_g.value == 55
    assert bytes(res) == bytes([SENTINEL]) * C.sizeof(res)
    assert (gkeys == -3).all() and (gnulls == 0xABCD).all() and (arena == SENTINEL).all()
    res1 = (capi.AggValue * na)()
    C.memset(res1, SENTINEL, C.sizeof(res1))
    rc = gpu_ctx.L.polr_out_aggregate_expr(out.h, None, sa, na, res1, C.byref(oor))
    assert rc == capi.E_RANGE and oor.value == n_minus * n_bad and bytes(res1) == bytes([SENTINEL]) * C.sizeof(res1)
    # the sums in range (+ and * of UINTEGER) are answered under the same declaration
    ok_specs = [s for s in uspecs if s[1] != "-"]
    got = out.aggregate_expr(ok_specs)
    assert got == [len(ids), sum((r_out + s_out).tolist()), sum((r_out * s_out).tolist())]
    mpx.close()
    pipe.close()


# ---- NULLs and mixed sources ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("routing", ["adaptive_reinit", "default_path"])
def test_device_null_pairs_match_reference(gpu_ctx, routing):
    from test_gpu_probe import gpu_pipeline, scenario_paths
    wl = workloads.star_skew(n_fact=60_000, with_nulls=True)
    pipe, joins, n = gpu_pipeline(gpu_ctx, wl, scenario_paths(wl, "each_last_once"))
    out = capi.Output(pipe, 1024, 8192)
    mpx = capi.DeviceMultiplexer(pipe, routing)
    mpx.run_resident(0, (n + 1023) // 1024, out=out)
    mpx.finish()
    pnames = list(wl["probe"]["cols"].keys())
    checked = refused = 0
    for pair in GOLD["nulls"]:
        left = (-1, pnames.index(pair["probe_col"]))
        right = (pair["join"], list(wl["joins"][pair["join"]]["payload"].keys()).index(pair["build_col"]))
        for op, g in pair["exprs"].items():
            if g.get("unsupported"):
                continue
            specs = [("count_star", "column", left, None, None)] + [(fn, op, left, right, SQL_DTYPE[g["typeof"]])
                                                                    for fn in ("count", "sum", "min", "max")]
            if "stderr" in g:  # the reference refused the expression: so does the device
                with pytest.raises(capi.PolrError) as e:
                    out.aggregate_expr(specs)
                assert e.value.code == capi.E_RANGE and e.value.count > 0 and e.value.count % 4 == 0
                refused += 1
                continue
            want = [g["count_star"], g["count"], g["sum"], g["min"], g["max"]]
            assert out.aggregate_expr(specs) == want, (pair, op)
            # the operands the other way round: a build column on the left, the probe column on the right
            if op == "*":
                flipped = [specs[0]] + [(fn, op, right, left, rt) for fn, _, _, _, rt in specs[1:]]
                assert out.aggregate_expr(flipped) == want
            checked += 1
    assert checked >= 6 and refused >= 1
    mpx.close()
    pipe.close()


# ---- type x operator matrix against exact Python, over the row ids of every engine ----------------------------------------------------
def result_type(t1, t2):
    """the narrowest integer type that holds every value of both operand types (signed if they differ in signedness)"""
    a, b = np.dtype(t1), np.dtype(t2)
    if a.kind == b.kind:
        return a if a.itemsize >= b.itemsize else b
    s, u = (a, b) if a.kind == "i" else (b, a)
    return np.dtype("int%d" % (8 * min(8, max(s.itemsize, 2 * u.itemsize))))


def small_columns(rng, n, prefix):
    """one column per integer type with values whose sums, differences and products stay inside every result type of
    result_type(): unsigned 0..11, signed -11..11 (11 * 11 = 121 < 127); ~10 % NULLs"""
    cols = {}
    for dt in INT_TYPES:
        lo = 0 if np.dtype(dt).kind == "u" else -11
        cols["%s_%s" % (prefix, np.dtype(dt).name)] = rng.integers(lo, 12, n).astype(dt)
    return cols, {c: (rng.random(n) > 0.1).astype(np.uint8) for c in cols}


def full_columns(rng, n, prefix):
    """the full range of every type, NULLs as above (test_gpu_sink_matrix.typed_columns without the unsupported kinds)"""
    from test_gpu_sink_matrix import full_range
    cols = {"%s_%s" % (prefix, np.dtype(dt).name): full_range(rng, dt, n) for dt in INT_TYPES}
    return cols, {c: (rng.random(n) > 0.1).astype(np.uint8) for c in cols}


MATRIX = [(eng, kind) for eng in ENGINES for kind in ("small", "full")]


@pytest.mark.parametrize("engine,kind", MATRIX, ids=["%s-%s" % m for m in MATRIX])
def test_expression_matrix(gpu_ctx, engine, kind):
    """every pair of operand types x { +, -, * }: left operand a probe column, right a payload column of join 0 (two row-id
    slots), and both from join 1 (one slot, its row id read once); result type = result_type().  small: nothing is out of
    range -- but the negative differences of two unsigned columns -- and COUNT / SUM / MIN / MAX equal exact Python; full: the
    exact number of arguments out of range, or the values where none is.  One pair in seven also goes through both GROUP BY sinks, grouped by fk1 with a domain that drops rows."""
    extra = small_columns if kind == "small" else full_columns
    s = Star(n=6000, seed=70 + MATRIX.index((engine, kind)), extra=extra, flat=engine == "flat").run(gpu_ctx, engine)
    fk1 = s.values(-1, 1)[0].astype(np.int64)
    n_range = n_values = 0
    for i1, t1 in enumerate(INT_TYPES):
        for i2, t2 in enumerate(INT_TYPES):
            rt = result_type(t1, t2)
            for src1, src2 in (("p", "b0"), ("b1", "b1")):
                left, right = s.col("%s_%s" % (src1, np.dtype(t1).name)), s.col("%s_%s" % (src2, np.dtype(t2).name))
                (lv, lok), (rv, rok) = s.values(*left), s.values(*right)
                for op in "+-*":
                    vals, bad = expr_values(op, lv, lok, rv, rok, rt)
                    specs = [(fn, op, left, right, rt) for fn in ("count", "sum", "min", "max")]
                    tag = (np.dtype(t1).name, op, np.dtype(t2).name, src1)
                    if bad:
                        # (small values: only a difference of two unsigned columns can leave its -- unsigned -- result type)
                        assert kind == "full" or (op == "-" and np.dtype(t1).kind == "u" and np.dtype(t2).kind == "u"), tag
                        with pytest.raises(capi.PolrError) as e:
                            s.out.aggregate_expr(specs)
                        assert e.value.code == capi.E_RANGE and e.value.count == 4 * bad, tag
                        n_range += 1
                    else:
                        assert s.out.aggregate_expr(specs) == [py_agg(fn, vals) for fn, *_ in specs], tag
                        n_values += 1
                    if (i1 * len(INT_TYPES) + i2) % 7 != "+-*".index(op) or src1 != "p":
                        continue
                    # both GROUP BY sinks: grouped by fk1 over [0, 500) -- about half of the rows are dropped -- and hashed
                    gspecs = [("count_star", "column", left, None, None)] + specs
                    want = {}
                    for k in ([] if bad else sorted(set(fk1.tolist()))):
                        m = fk1 == k
                        gv, gbad = expr_values(op, lv[m], lok[m], rv[m], rok[m], rt)
                        want[(k,)] = [int(m.sum())] + [py_agg(fn, gv) for fn, *_ in specs]
                    if bad:
                        for call in (lambda: s.out.aggregate_grouped_expr([(-1, 1, 0, 500)], gspecs),
                                     lambda: s.out.aggregate_hashed_expr([(-1, 1)], gspecs, 2048)):
                            with pytest.raises(capi.PolrError) as e:
                                call()
                            assert e.value.code == capi.E_RANGE and e.value.count == 4 * bad, tag
                        continue
                    gvals, _, dropped = s.out.aggregate_grouped_expr([(-1, 1, 0, 500)], gspecs)
                    assert dropped == int((fk1 >= 500).sum()) and dropped > 0
                    for k in range(500):
                        assert gvals[k] == want.get((k,), [0, 0, None, None, None]), (tag, k)
                    assert s.out.aggregate_hashed_expr([(-1, 1)], gspecs, 2048) == want, tag
    assert n_values > 0 and n_range > 0
    if kind == "small":  # every pair of types and every operator was answered, but for unsigned - unsigned
        n_uu = sum(1 for t in INT_TYPES if np.dtype(t).kind == "u") ** 2
        assert n_values >= 2 * (3 * len(INT_TYPES) ** 2 - n_uu)
    s.close()


# ---- POLR_ARG_COLUMN is the existing call ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ENGINES)
def test_column_form_equals_the_existing_entry_points(gpu_ctx, engine):
    s = Star(n=6000, seed=90 + ENGINES.index(engine), flat=engine == "flat").run(gpu_ctx, engine)
    for prefix in ("p", "b0", "b1"):
        for dt in INT_TYPES:
            c = s.col("%s_%s" % (prefix, np.dtype(dt).name))
            plain = [("count_star", -1, 0)] + [(fn, *c) for fn in ("count", "sum", "min", "max")]
            # (result type and right operand are ignored: garbage in both)
            expr = [("count_star", "column", (-1, 0), None, None)] + [(fn, "column", c, (9, 99), np.uint8) for fn in ("count", "sum", "min", "max")]
            assert s.out.aggregate_expr(expr) == s.out.aggregate(plain)
            assert s.out.aggregate_grouped_expr([(-1, 1, 0, 1000)], expr) == s.out.aggregate_grouped([(-1, 1, 0, 1000)], plain)
            assert s.out.aggregate_hashed_expr([(-1, 1)], expr, 2048) == s.out.aggregate_hashed([(-1, 1)], plain, 2048)
            assert s.out.aggregate_hashed_expr([(-1, 1)], expr, 2048) == s.out.aggregate_hashed_str([(-1, 1)], plain, 2048)
    s.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals(gpu_ctx):
    s = Star(n=6000, seed=99).run(gpu_ctx, "path")
    i8, u8, i32, u32, i64 = (s.col("p_" + t) for t in ("int8", "uint8", "int32", "uint32", "int64"))
    b_i32 = s.col("b0_int32")
    calls = [lambda sp: s.out.aggregate_expr(sp), lambda sp: s.out.aggregate_grouped_expr([(-1, 1, 0, 1000)], sp),
             lambda sp: s.out.aggregate_hashed_expr([(-1, 1)], sp, 2048)]

    def refused(specs, code):
        for call in calls:
            with pytest.raises(capi.PolrError) as e:
                call(specs)
            assert e.value.code == code, (specs, e.value)

    # a result type that cannot hold an operand type: narrower, unsigned for a signed operand, signed of the same width
    # for an unsigned operand
    for left, right, rt in ((i32, i8, np.int16), (i8, u8, np.uint8), (i8, u8, np.int8), (u32, b_i32, np.int32),
                            (i64, i8, np.int32), (u8, i32, np.uint32)):
        refused([("sum", "*", left, right, rt)], capi.E_INVALID)
    # ... while the narrowest type that does is taken
    assert s.out.aggregate_expr([("count", "+", i8, u8, np.int16)])[0] >= 0
    # a result width that is no integer type's; an unsigned 8-byte result
    sa = capi.make_agg_exprs([("sum", "+", i8, i8, np.int8)])
    sa[0].result_width = 3
    res, oor = (capi.AggValue * 1)(), C.c_uint64()
    assert gpu_ctx.L.polr_out_aggregate_expr(s.out.h, None, sa, 1, res, C.byref(oor)) == capi.E_INVALID
    refused([("sum", "+", u32, u32, np.uint64)], capi.E_UNSUPPORTED)
    # unsigned 8-byte and VARCHAR operands, on either side
    for bad in ("p_u64", "b0_v16", "b1_u64", "p_v16"):
        refused([("sum", "+", s.col(bad), i8, np.int64)], capi.E_UNSUPPORTED)
        refused([("min", "-", i8, s.col(bad), np.int64)], capi.E_UNSUPPORTED)
        refused([("max", "column", s.col(bad), None, None)], capi.E_UNSUPPORTED)
    # an unknown operator, an unknown function, a column out of range
    refused([("sum", 4, i8, i8, np.int8)], capi.E_INVALID)
    refused([(5, "+", i8, i8, np.int8)], capi.E_INVALID)
    refused([("sum", "+", i8, (-1, 999), np.int8)], capi.E_INVALID)
    refused([("sum", "+", (7, 0), i8, np.int8)], capi.E_INVALID)
    # more than 8 aggregates
    refused([("count", "+", i8, i8, np.int16)] * 9, capi.E_UNSUPPORTED)
    # (8 are taken; TINYINT + TINYINT over the full range leaves TINYINT, so the result type here is the wider one)
    assert len(s.out.aggregate_expr([("count", "+", i8, i8, np.int16)] * 8)) == 8
    s.close()


def test_hashed_expr_range_wins_over_group_overflow(gpu_ctx):
    """more groups than the 1024-slot minimum table holds, max_groups = 16: rows that find no slot are range-checked all the
    same, POLR_E_RANGE comes before the POLR_E_OVERFLOW of the groups, and nothing is written -- but *str_used, which the
    call zeroes before it starts, as polr_out_aggregate_hashed_str does"""
    s = Star(n=6000, seed=97, extra=full_columns).run(gpu_ctx, "path")
    gcols = [(-1, 1), s.col("p_int16")]
    fk1 = s.values(*gcols[0])[0].astype(np.int64)
    g1, ok1 = s.values(*gcols[1])
    pairs = np.stack([fk1, np.where(ok1, g1.astype(np.int64), 1 << 40)], axis=1)  # (NULL is a group value of its own)
    assert len(np.unique(pairs, axis=0)) > 1024
    ka = (capi.GroupKey * 2)()
    for i, (sj, sc) in enumerate(gcols):
        ka[i].src_join, ka[i].src_col = sj, sc
    max_groups = 16

    def call(left, right, op, rt):
        specs = [("count_star", "column", left, None, None)] + [(fn, op, left, right, rt) for fn in ("count", "sum", "min", "max")]
        res = (capi.AggValue * (max_groups * len(specs)))()
        C.memset(res, SENTINEL, C.sizeof(res))
        gkeys = np.full((max_groups, 2), -3, np.int64)
        gnulls = np.full(max_groups, 0xABCD, np.uint32)
        arena = np.full(64, SENTINEL, np.uint8)
        n_g, used, oor = C.c_uint64(55), C.c_uint64(66), C.c_uint64(77)
        rc = gpu_ctx.L.polr_out_aggregate_hashed_expr(s.out.h, None, ka, 2, capi.make_agg_exprs(specs), len(specs), max_groups,
                                                      gkeys.ctypes.data, gnulls.ctypes.data, res, C.byref(n_g), arena.ctypes.data,
                                                      64, C.byref(used), C.byref(oor))
        untouched = (bytes(res) == bytes([SENTINEL]) * C.sizeof(res) and (gkeys == -3).all() and (gnulls == 0xABCD).all()
                     and (arena == SENTINEL).all())
        return rc, oor.value, n_g.value, used.value, untouched

    left, right = s.col("p_int32"), s.col("b0_int32")
    (lv, lok), (rv, rok) = s.values(*left), s.values(*right)
    _, bad = expr_values("*", lv, lok, rv, rok, np.int32)
    assert bad > 0
    rc, oor, n_g, used, untouched = call(left, right, "*", np.int32)
    assert rc == capi.E_RANGE and oor == 4 * bad
    assert untouched and n_g == 55 and used == 0
    # the same output and groups, an expression that stays in range: the groups do not fit
    rc, oor, n_g, used, untouched = call(s.col("p_int8"), s.col("b0_int8"), "+", np.int16)
    assert rc == capi.E_OVERFLOW and oor == 0 and n_g > max_groups and untouched
    s.close()


def test_fused_sink_is_unchanged(gpu_ctx):
    """polr_out_fuse_grouped takes polr_agg_spec -- plain columns -- as before, and answers as polr_out_aggregate_grouped_expr
    does for the column form over the emitted row ids"""
    s = Star(n=6000, seed=101, extra=small_columns, flat=True).run(gpu_ctx, "flat")
    assert gpu_ctx.L.polr_out_fuse_grouped.argtypes == [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    c = s.col("p_int32")
    keys = [(-1, 1, 0, 1000)]
    plain = [("count_star", -1, 0), ("sum", *c), ("count", *c)]
    want = s.out.aggregate_grouped_expr(keys, [("count_star", "column", (-1, 0), None, None), ("sum", "column", c, None, None),
                                               ("count", "column", c, None, None)])
    fused = capi.Output(s.pipe, 1024, 8192)
    fused.fuse_grouped(keys, plain)
    fused.reset()
    gpu_ctx.sync()
    m = capi.DeviceMultiplexer(s.pipe, "default_path")
    capi.run_resident([m], [(0, (6000 + 1023) // 1024)], out=fused, reset=True, finish=True)
    m.finish()
    got = fused.fused_result()
    assert got[0] == want[0] and got[2] == want[2]
    with pytest.raises(capi.PolrError) as e:  # MIN stays outside the fused sink
        capi.Output(s.pipe, 1024, 8192).fuse_grouped(keys, [("min", *c)])
    assert e.value.code == capi.E_UNSUPPORTED
    m.close()
    fused.close()
    s.close()
