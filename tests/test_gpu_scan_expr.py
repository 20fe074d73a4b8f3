"""Filter expressions in the device source scan (polr_pipeline_scan_filter_expr: OR / NOT trees, IN lists, LIKE) against the
tests' own evaluator (tests/scanexpr.py: three-valued logic in numpy, LIKE through a bytes regular expression), which
tests/test_scan_expr_golden.py pins against the reference engine.  Selections, counts and chunk boundaries are compared
exactly; a NULL row's cell is never read."""
import json
import os

import numpy as np
import pytest

import common
import scanexpr
import scanstr
from joinref import Join, Ref
from polr_amd import capi
from scanexpr import LIKE_PATTERNS, LIKE_STRINGS, chunks_of, passing

pytestmark = pytest.mark.gpu

S = 1  # the VARCHAR column of the pipelines below: (pk INTEGER, s VARCHAR, ...)


def make_pipe(ctx, values, n_blocks=1, extra=(), extra_valid=(), heaps=True, joins=None, pk=None, **cell_args):
    """probe table (pk, s, *extra) with one join on pk (build keys 0..99) unless `joins` says otherwise; pipe.cols: the
    columns as scanexpr.evaluate takes them"""
    n = len(values)
    cells, valid, blocks = scanstr.cells(values, n_blocks, **cell_args)
    pk = (np.arange(n, dtype=np.int32) % 128) if pk is None else pk
    joins = joins or [Join(np.arange(100, dtype=np.int32), 0)]
    hts = [j.device(ctx) for j in joins]
    cols = [pk, cells] + list(extra)
    extra_valid = list(extra_valid) or [None] * len(extra)
    pipe = capi.Pipeline(ctx, cols, n, [(h, [(-1, j.src)]) for h, j in zip(hts, joins)], [list(range(len(joins)))],
                         probe_valid=[None, valid] + extra_valid)
    if heaps:
        pipe.set_probe_heaps(S, blocks)
    pipe._test_keep = (hts, cols, blocks)
    pipe.cols = {0: (pk, None), S: values}
    pipe.cols.update({2 + i: (c, v) for i, (c, v) in enumerate(zip(extra, extra_valid))})
    pipe.n = n
    return pipe


def check(pipe, want, V, what):
    sel, offs = pipe.fetch_scan()
    want_offs = chunks_of(want, pipe.n, V)
    assert pipe.scan == (len(want), len(want_offs) - 1), what
    assert np.array_equal(sel, want), what
    assert np.array_equal(offs, want_offs), what


def scan_and_check(pipe, expr, V=1024, lip_joins=0):
    pipe.scan_filter_expr(expr, vector_size=V, lip_joins=lip_joins)
    check(pipe, passing(expr, pipe.cols, pipe.n), V, expr)


@pytest.mark.parametrize("nulls", [False, True], ids=["no-nulls", "nulls"])
def test_like_matrix(gpu_ctx, nulls):
    """3 x 1024 + 1 rows cycling through the string set (inline cells with garbage padding, the heap in two blocks): every
    pattern of the edge set as LIKE and as NOT LIKE; with 1-in-7 NULLs whose cells hold the inline string "abab", which
    every pattern matches either as LIKE or as NOT LIKE -- a scan that read NULL cells would pass rows it must not"""
    n = 3 * 1024 + 1
    values = [LIKE_STRINGS[(i * 5 + i // len(LIKE_STRINGS)) % len(LIKE_STRINGS)] for i in range(n)]
    if nulls:
        values = [None if i % 7 == 3 else v for i, v in enumerate(values)]
    assert {v for v in values if v is not None} == set(LIKE_STRINGS)
    pipe = make_pipe(gpu_ctx, values, n_blocks=2, dirty_seed=11, null_cell=b"abab")
    for p in LIKE_PATTERNS:
        scan_and_check(pipe, ("like", S, p))
        n_like = pipe.scan[0]
        scan_and_check(pipe, ("not", ("like", S, p)))
        assert n_like + pipe.scan[0] == sum(v is not None for v in values), p
    pipe.close()


def grid_pipe(ctx, n=2500):
    """s and two integer columns, each with NULLs of its own, so that every combination of TRUE / FALSE / NULL of
    (s = 'Japan', a < 50, b IN ...) occurs"""
    rng = np.random.default_rng(3)
    names = [b"Japan", b"Jap", b"Japanese", b"(voice: English version)", None]
    values = [names[int(x)] for x in rng.integers(0, len(names), n)]
    a = rng.integers(0, 100, n).astype(np.int32)
    b = rng.integers(-5, 5, n).astype(np.int64)
    av, bv = (rng.random(n) > 0.3).astype(np.uint8), (rng.random(n) > 0.3).astype(np.uint8)
    return make_pipe(ctx, values, extra=[a, b], extra_valid=[av, bv], null_cell=b"Japan")


def test_three_valued_logic(gpu_ctx):
    """the four Kleene cases on rows where they differ from a two-valued reading, IS NULL OR ..., a 64-node program of
    depth 32"""
    pipe = grid_pipe(gpu_ctx)
    x, y = ("cmp", S, "=", b"Japan"), ("cmp", 2, "<", 50)
    for e in (("not", x), ("and", x, y), ("or", x, y), ("not", ("and", x, y)), ("not", ("or", x, y)),
              ("or", ("cmp", S, "is null"), ("like", S, b"%voice%")), ("and", ("cmp", 2, "is not null"), ("not", y)),
              ("or", ("not", x), ("cmp", 3, "is null"), ("and", y, ("in", 3, [-5, 0, 4])))):
        scan_and_check(pipe, e)
    # NULL AND FALSE = FALSE, NULL OR TRUE = TRUE; NULL AND TRUE = NULL, NULL OR FALSE = NULL, NOT NULL = NULL: rows
    # with s NULL pass NOT (x AND y) exactly when y is FALSE, and x OR y exactly when y is TRUE
    a, av = pipe.cols[2]
    s_null = np.array([v is None for v in pipe.cols[S]])
    pipe.scan_filter_expr(("not", ("and", x, y)))
    sel, _ = pipe.fetch_scan()
    assert np.array_equal(sel[s_null[sel]], np.nonzero(s_null & (av == 1) & (a >= 50))[0])
    pipe.scan_filter_expr(("or", x, y))
    sel, _ = pipe.fetch_scan()
    assert np.array_equal(sel[s_null[sel]], np.nonzero(s_null & (av == 1) & (a < 50))[0])
    assert (s_null & (av == 0)).sum() > 20 and (s_null & (av == 1) & (a >= 50)).sum() > 20
    # 32 leaves pushed before the first operator: depth 32, 64 nodes with the NOT on top
    leaves = [("cmp", 2, ("<", ">=")[i % 2], 10 + 2 * i) if i % 3 == 0 else
              ("in", 3, [i % 5 - 2, 4]) if i % 3 == 1 else
              ("like", S, (b"Jap%", b"%n", b"%voice%", b"_ap")[i % 4]) for i in range(32)]
    e = leaves[-1]
    for i in range(30, -1, -1):
        e = (("and", "or")[i % 2], leaves[i], e)
    e = ("not", e)
    nodes, _ = capi.flatten_filter_expr(e)
    assert len(nodes) == capi.MAX_FILTER_NODES and [nd[0] for nd in nodes[:32]].count("cmp") == 11
    scan_and_check(pipe, e)
    assert 0 < pipe.scan[0] < pipe.n
    pipe.close()


def test_in_lists(gpu_ctx):
    """IN and NOT IN with 1, 8 and 64 members: VARCHAR (inline and heap members), signed and unsigned integers"""
    n = 4000
    rng = np.random.default_rng(8)
    values = scanstr.fixture_column(31, n)
    distinct = sorted({v for v in values if v is not None}, key=lambda v: (len(v) > 12, v))
    u = rng.integers(0, 200, n).astype(np.uint32)
    i64 = rng.integers(-100, 100, n).astype(np.int64)
    pipe = make_pipe(gpu_ctx, values, n_blocks=2, extra=[u, i64], extra_valid=[None, (rng.random(n) > 0.2).astype(np.uint8)])
    for m in (1, 8, 64):
        members = distinct[:m // 2] + distinct[-(m - m // 2):]  # short ones and long ones
        assert len(members) == m and (m == 1 or len(members[0]) <= 12 < len(members[-1]))
        for e in (("in", S, members), ("in", 2, list(range(3, 3 + 2 * m, 2))), ("in", 3, list(range(-m, m, 2)))):
            scan_and_check(pipe, e)
            assert 0 < pipe.scan[0] < n, e
            scan_and_check(pipe, ("not", e))
    scan_and_check(pipe, ("in", S, [b"no such string", b""]))
    pipe.close()


@pytest.mark.parametrize("V", [64, 1000, 2048])
def test_vector_shapes(gpu_ctx, V):
    """2 V + 1 rows (the last vector holds one row): a program nothing passes, one everything passes, no program at all,
    and one in between"""
    n = 2 * V + 1
    values = [LIKE_STRINGS[(i * 7 + i // 64) % len(LIKE_STRINGS)] for i in range(n)]
    pipe = make_pipe(gpu_ctx, values, n_blocks=2)
    scan_and_check(pipe, ("and", ("like", S, b"a%"), ("not", ("like", S, b"a%"))), V)
    assert pipe.scan == (0, 0)
    scan_and_check(pipe, ("or", ("like", S, b"%_%"), ("cmp", S, "=", b"")), V)
    assert pipe.scan == (n, 3)
    scan_and_check(pipe, None, V)
    assert pipe.scan == (n, 3)
    scan_and_check(pipe, ("or", ("like", S, b"%(USA)%"), ("in", S, [b"ab", scanstr._S40])), V)
    assert 0 < pipe.scan[0] < n
    scan_and_check(pipe, ("cmp", S, "=", values[-1]), V)
    assert pipe.fetch_scan()[0][-1] == n - 1  # the one row of the last vector
    pipe.close()


def test_and_only_programs_equal_the_existing_scans(gpu_ctx):
    """AND-only programs against scan_filter / scan_filter_str on the same pipeline, with LIP as well"""
    n = 6000
    rng = np.random.default_rng(42)
    values = scanstr.fixture_column(7, n)
    i1 = rng.integers(0, 100, n).astype(np.int32)
    i2 = rng.integers(-2**40, 2**40, n).astype(np.int64)
    i2v = (rng.random(n) > 0.1).astype(np.uint8)
    pk = rng.integers(0, 200, n).astype(np.int32)
    pipe = make_pipe(gpu_ctx, values, n_blocks=2, extra=[i1, i2], extra_valid=[None, i2v], pk=pk,
                     joins=[Join(np.arange(0, 200, 2, dtype=np.int32), 0)])
    cases = [
        [(2, "<", 80)],
        [(2, "<", 80), (3, ">=", -2**39), (3, "is not null", None)],
        [(S, ">=", b"J"), (S, "<", "日本".encode()), (2, "<", 80), (S, "is not null", None)],
        [(S, "=", b"Japan")],
        [(S, "is null", None), (3, "<>", 0)],
    ]
    for filters in cases:
        for lip in (0, 1):
            pipe.scan_filter(filters, lip_joins=lip)
            want, want_scan = pipe.fetch_scan(), pipe.scan
            leaves = [("cmp", c, op, const) for c, op, const in filters]
            pipe.scan_filter_expr(leaves[0] if len(leaves) == 1 else ("and",) + tuple(leaves), lip_joins=lip)
            got = pipe.fetch_scan()
            assert pipe.scan == want_scan and 0 < want_scan[0] < n, (filters, lip)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (filters, lip)
    pipe.close()


GOLD = json.load(open(os.path.join(common.ROOT, "tests", "golden", "scan_expr.json"), encoding="utf-8"))


def test_fixture_of_the_reference_engine(gpu_ctx):
    """every query of tests/golden/scan_expr.json: count and SHA-1 of the row ids the reference engine returned"""
    values = scanstr.fixture_column(GOLD["seed"], GOLD["n_rows"])
    assert scanstr.column_digest(values) == GOLD["column_sha1"]
    ints, ivalid = scanexpr.fixture_int(GOLD["int_seed"], GOLD["n_rows"])
    pipe = make_pipe(gpu_ctx, values, n_blocks=2, extra=[ints], extra_valid=[ivalid])
    for q in GOLD["queries"]:
        pipe.scan_filter_expr(scanexpr.bind(q["expr"], {"s": S, "i": 2}))
        sel, _ = pipe.fetch_scan()
        assert scanstr.rows_digest(sel) == {"count": q["count"], "sha1": q["sha1"]}, q["where"]
    pipe.close()


def test_expression_scan_feeds_a_resident_run(gpu_ctx):
    """expression scan -> polr_mpx_use_scan_chunks -> a resident run of a two-join star: COUNT(*) against joinref.Ref over
    the expected rows; then a plain scan_filter and a run, then an expression scan again: each result is its own (the
    pass-bit buffer and the settling leak nothing between scans)"""
    n = 8000
    rng = np.random.default_rng(5)
    values = scanstr.fixture_column(99, n)
    k0, k1 = rng.integers(0, 300, n).astype(np.int32), rng.integers(0, 50, n).astype(np.int32)
    joins = [Join(rng.permutation(np.arange(0, 300, 2, dtype=np.int32)), 0), Join(np.arange(0, 40, dtype=np.int32), 2)]
    pipe = make_pipe(gpu_ctx, values, n_blocks=2, extra=[k1], extra_valid=[None], pk=k0, joins=joins)
    m = capi.DeviceMultiplexer(pipe, "default_path")
    first = ("or", ("like", S, b"%a%"), ("in", S, [b"Tokyo", "日本語".encode()]))
    steps = [("expr", first), ("plain", [(2, "<", 25)]), ("expr", ("not", ("like", S, b"%a%"))), ("expr", first)]
    seen = []
    for kind, f in steps:
        if kind == "expr":
            n_sel, n_chunks = pipe.scan_filter_expr(f)
            want = passing(f, pipe.cols, n)
        else:
            n_sel, n_chunks = pipe.scan_filter(f)
            want = np.nonzero(k1 < 25)[0].astype(np.uint32)
        check(pipe, want, 1024, f)
        m.use_scan_chunks()
        capi.run_resident([m], [(0, n_chunks)], reset=True, finish=True)
        counts = Ref([k0, None, k1], None, joins, want).stage_counts([0, 1])
        assert counts[-1] > 20
        assert m.finish()["stage_out"][0] == counts, f
        seen.append(counts[-1])
    assert seen[0] == seen[3] and len(set(seen[:3])) == 3
    m.close()
    pipe.close()


def test_refusals_leave_the_previous_scan(gpu_ctx):
    """every POLR_E_INVALID / POLR_E_UNSUPPORTED of the contract; after each, fetch_scan returns the scan before it"""
    n = 3000
    values = [LIKE_STRINGS[i % len(LIKE_STRINGS)] for i in range(n)]
    i1 = (np.arange(n, dtype=np.int32) * 7) % 100
    u1 = ((np.arange(n) * 3) % 50).astype(np.uint32)
    more = [np.arange(n, dtype=np.int64) for _ in range(7)]
    pipe = make_pipe(gpu_ctx, values, n_blocks=2, extra=[i1, u1] + more)
    n_cols = 4 + len(more)
    first = ("or", ("cmp", 2, "<", 10), ("like", S, b"%(USA)%"))
    pipe.scan_filter_expr(first, vector_size=64)
    want = passing(first, pipe.cols, n)
    check(pipe, want, 64, "first")
    EQ, IS_NULL = capi.CMP["="], capi.CMP["is null"]
    k5, AND, NOT = (5, None, 0), ("and", 0, 0, 0, 0), ("not", 0, 0, 0, 0)
    leaf = ("cmp", 2, EQ, 0, 1)
    I, U = capi.E_INVALID, capi.E_UNSUPPORTED
    refused = [
        ("NOT on an empty stack", [NOT], [], I),
        ("AND with one operand", [leaf, AND], [k5], I),
        ("two values left", [leaf, leaf], [k5], I),
        ("unknown kind", [(6, 2, EQ, 0, 1)], [k5], I),
        ("unknown op", [("cmp", 2, 8, 0, 1)], [k5], I),
        ("a value range outside values", [("in", 2, 0, 0, 2)], [k5], I),
        ("a column out of range", [("cmp", n_cols, EQ, 0, 1)], [k5], I),
        ("bytes against an integer column", [leaf], [(0, b"x", 1)], I),
        ("a length without bytes", [("cmp", S, EQ, 0, 1)], [(0, None, 5)], I),
        ("LIKE on an integer column", [("like", 2, 0, 0, 1)], [k5], I),
        ("IN without members", [("in", S, 0, 0, 0)], [(0, b"x", 1)], I),
        ("a negative constant against an unsigned column", [("cmp", 3, EQ, 0, 1)], [(-1, None, 0)], I),
        ("65 nodes", [leaf] * 32 + [AND] * 31 + [NOT] * 2, [k5], U),
        ("depth 33", [leaf] * 33 + [AND] * 32, [k5], U),
        ("65 values", [leaf], [k5] * 65, U),
        ("16385 bytes", [("in", S, 0, 0, 5)], [(0, b"y" * 4096, 4096)] * 4 + [(0, b"z", 1)], U),
        ("a constant of 4097 bytes", [("cmp", S, EQ, 0, 1)], [(0, b"y" * 4097, 4097)], U),
        ("9 distinct columns", [("cmp", 2 + i, EQ, 0, 1) for i in range(9)] + [AND] * 8, [k5], U),
        ("a NUL byte in a pattern", [("like", S, 0, 0, 1)], [(0, b"a\0%", 3)], U),
    ]
    for what, nodes, vals, code in refused:
        with pytest.raises(capi.PolrError) as e:
            pipe.scan_filter_expr_raw(nodes, vals, vector_size=64)
        assert e.value.code == code, what
        check(pipe, want, 64, what)
    for what, kw, code in (("a LIP join that does not exist", {"lip_joins": 2}, I), ("vector size 1", {"vector_size": 1}, I)):
        with pytest.raises(capi.PolrError) as e:
            pipe.scan_filter_expr_raw([leaf], [k5], **kw)
        assert e.value.code == code, what
        check(pipe, want, 64, what)
    # not refusals: the limits themselves
    pipe.scan_filter_expr_raw([leaf] * 32 + [AND] * 31 + [NOT], [k5], vector_size=64)
    check(pipe, np.nonzero(i1 != 5)[0].astype(np.uint32), 64, "64 nodes, depth 32")
    pipe.scan_filter_expr_raw([("in", S, 0, 0, 4)], [(0, b"y" * 4096, 4096)] * 4, vector_size=64)
    assert pipe.scan == (0, 0)
    scan_and_check(pipe, ("and",) + tuple(("cmp", c, ">=", 5) for c in range(3, 11)), 64)  # 8 distinct columns
    assert 0 < pipe.scan[0] < n
    pipe.scan_filter_expr_raw([("cmp", S, EQ, 0, 1)], [(0, None, 0)], vector_size=64)
    check(pipe, passing(("cmp", S, "=", b""), pipe.cols, n), 64, "the empty string")
    pipe.close()


def test_heap_that_never_came(gpu_ctx):
    """a column the library uploaded, one non-NULL cell of 13 bytes, no heap: POLR_E_INVALID before a pointer is followed,
    the scan before it in place; the same column is accepted when that row is NULL"""
    n = 2000
    long_row = 1234
    for null_it in (False, True):
        values = [(b"a", b"twelve bytes", b"abc")[i % 3] for i in range(n)]
        values[long_row] = None if null_it else b"thirteen byte"
        host = np.frombuffer(b"thirteen byte", np.uint8).copy()
        cell = np.zeros(16, np.uint8)
        cell[0:4] = np.frombuffer(np.uint32(13).tobytes(), np.uint8)
        cell[4:8] = host[:4]
        cell[8:16] = np.frombuffer(np.uint64(host.ctypes.data).tobytes(), np.uint8)
        pipe = make_pipe(gpu_ctx, values, heaps=False, null_cell=cell.view("V16")[0])
        before = ("cmp", 0, "<", 64)
        scan_and_check(pipe, before)
        e1, e2 = ("or", ("like", S, b"%teen%"), ("cmp", 0, "=", 3)), ("in", S, [b"thirteen byte", b"abc"])
        if null_it:
            scan_and_check(pipe, e1)
            scan_and_check(pipe, e2)
            assert pipe.scan[0] == sum(v == b"abc" for v in values)
        else:
            for e in (e1, e2):
                with pytest.raises(capi.PolrError) as err:
                    pipe.scan_filter_expr(e)
                assert err.value.code == capi.E_INVALID and "heap" in str(err.value)
                check(pipe, passing(before, pipe.cols, n), 1024, "after the refusal")
            scan_and_check(pipe, ("or", ("cmp", S, "is null"), ("cmp", 0, "=", 3)))  # (reads no cell: accepted)
        pipe.close()
