"""Pushed-down VARCHAR comparisons in the device source scan (polr_pipeline_scan_filter_str) against Python's bytes
comparison -- memcmp over the shorter length, the shorter string first on a tie: the order of the reference's
StringComparisonOperators, pinned against the reference engine itself by tests/test_scan_varchar_golden.py.  Selections,
counts and chunk boundaries are compared exactly; a NULL row passes no comparison and its cell is never read."""
import json
import os

import numpy as np
import pytest

import common
import scanstr
from joinref import Join, Ref
from polr_amd import capi
from scanstr import EDGES, OPS, chunks_of, passing

pytestmark = pytest.mark.gpu

S = 1  # the VARCHAR column of the pipelines below: (pk INTEGER, s VARCHAR, ...)


def make_pipe(ctx, values, n_blocks=1, extra=(), extra_valid=(), heaps=True, joins=None, pk=None, **cell_args):
    """probe table (pk, s, *extra) with one join on pk (build keys 0..99) unless `joins` says otherwise"""
    n = len(values)
    cells, valid, blocks = scanstr.cells(values, n_blocks, **cell_args)
    pk = (np.arange(n, dtype=np.int32) % 128) if pk is None else pk
    joins = joins or [Join(np.arange(100, dtype=np.int32), 0)]
    hts = [j.device(ctx) for j in joins]
    cols = [pk, cells] + list(extra)
    pipe = capi.Pipeline(ctx, cols, n, [(h, [(-1, j.src)]) for h, j in zip(hts, joins)], [list(range(len(joins)))],
                         probe_valid=[None, valid] + list(extra_valid))
    if heaps:
        pipe.set_probe_heaps(S, blocks)
    pipe._test_keep = (hts, cols, blocks)
    return pipe


def check(pipe, n, want, V, what):
    sel, offs = pipe.fetch_scan()
    want_offs = chunks_of(want, n, V)
    assert pipe.scan == (len(want), len(want_offs) - 1), what
    assert np.array_equal(sel, want), what
    assert np.array_equal(offs, want_offs), what


def scan_and_check(pipe, values, filters, V=1024):
    """filters: [(op, constant)] on column S"""
    pipe.scan_filter([(S, op, c) for op, c in filters], vector_size=V)
    check(pipe, len(values), passing(values, filters), V, filters)


@pytest.mark.parametrize("nulls", [False, True], ids=["no-nulls", "nulls"])
def test_semantics_matrix(gpu_ctx, nulls):
    """3 x 1024 + 1 rows cycling through the edge set (inline cells with garbage padding, the heap in two blocks): every
    constant of the set x six operators; with 1-in-7 NULLs (whose cells hold the inline string "ab") also IS [NOT] NULL"""
    n = 3 * 1024 + 1
    values = [EDGES[(i * 5 + i // len(EDGES)) % len(EDGES)] for i in range(n)]
    if nulls:
        values = [None if i % 7 == 3 else v for i, v in enumerate(values)]
    assert {v for v in values if v is not None} == set(EDGES)
    pipe = make_pipe(gpu_ctx, values, n_blocks=2, dirty_seed=11)
    for c in EDGES:
        for op in OPS:
            scan_and_check(pipe, values, [(op, c)])
    if nulls:
        for f in ([("is null", None)], [("is not null", None)]):
            pipe.scan_filter_str_raw([(S, op, 0, None, 0) for op, _ in f])
            check(pipe, n, passing(values, f), 1024, f)
        scan_and_check(pipe, values, [("is not null", None), ("<>", b"ab")])
        scan_and_check(pipe, values, [("is null", None), ("<>", b"ab")])  # (nothing: 0 chunks)
        assert pipe.scan == (0, 0)
    pipe.close()


def test_null_cells_are_not_read(gpu_ctx):
    """an inline-only column without a heap whose NULL rows hold inline cells equal to the constant"""
    n = 2500
    values = [None if i % 3 == 0 else (b"Japan", b"Jap", b"Japanese", b"")[i % 4] for i in range(n)]
    pipe = make_pipe(gpu_ctx, values, heaps=False, null_cell=b"Japan")
    for op in ("=", "<>", "<=", ">="):
        scan_and_check(pipe, values, [(op, b"Japan")])
        sel, _ = pipe.fetch_scan()
        assert not any(values[r] is None for r in sel.tolist()), op
    pipe.close()


GOLD = json.load(open(os.path.join(common.ROOT, "tests", "golden", "scan_varchar.json"), encoding="utf-8"))


def test_fixture_of_the_reference_engine(gpu_ctx):
    """every query of tests/golden/scan_varchar.json: constant comparisons, LIKE 'x%' / prefix() through like_pushdown,
    range conjunctions -- count and SHA-1 of the row ids the reference engine returned"""
    from test_scan_varchar_golden import filters_of
    values = scanstr.fixture_column(GOLD["seed"], GOLD["n_rows"])
    assert scanstr.column_digest(values) == GOLD["column_sha1"]
    pipe = make_pipe(gpu_ctx, values, n_blocks=2)
    for q in GOLD["queries"]:
        pipe.scan_filter([(S, op, c) for op, c in filters_of(q)])
        sel, _ = pipe.fetch_scan()
        assert scanstr.rows_digest(sel) == {"count": q["count"], "sha1": q["sha1"]}, q["where"]
    pipe.close()


def test_mixed_varchar_integer_and_lip(gpu_ctx):
    """two VARCHAR columns (a range on one, = on the other), two integer filters and LIP on the join in one call against
    the intersection computed in numpy and Python; then 8 filters in one call"""
    n = 6000
    rng = np.random.default_rng(42)
    s1 = scanstr.fixture_column(7, n)
    names = [b"(voice)", b"(voice: English version)", b"(uncredited)", b"", None]
    s2 = [names[int(x)] for x in rng.integers(0, len(names), n)]
    c2, v2, b2 = scanstr.cells(s2, 1, null_cell=b"(voice: English version)"[:12])
    i1 = rng.integers(0, 100, n).astype(np.int32)
    i2 = rng.integers(-2**40, 2**40, n).astype(np.int64)
    i2v = (rng.random(n) > 0.1).astype(np.uint8)
    pk = rng.integers(0, 200, n).astype(np.int32)
    bk = np.arange(0, 200, 2, dtype=np.int32)
    pipe = make_pipe(gpu_ctx, s1, n_blocks=2, extra=[c2, i1, i2], extra_valid=[v2, None, i2v], pk=pk, joins=[Join(bk, 0)])
    pipe.set_probe_heaps(2, b2)
    str_f1 = [(">=", b"J"), ("<", "日本".encode())]
    str_f2 = [("=", b"(voice: English version)")]
    ok = np.zeros(n, bool)
    ok[np.intersect1d(passing(s1, str_f1), passing(s2, str_f2))] = True
    ok &= (i1 < 80) & (i2 >= -2**39) & i2v.astype(bool)
    filters = [(S, op, c) for op, c in str_f1] + [(3, "<", 80), (2, "=", str_f2[0][1]), (4, ">=", -2**39)]
    pipe.scan_filter(filters)
    check(pipe, n, np.nonzero(ok)[0].astype(np.uint32), 1024, "no LIP")
    pipe.scan_filter(filters, lip_joins=1)
    want = np.nonzero(ok & np.isin(pk, bk))[0].astype(np.uint32)
    assert 20 < len(want) < ok.sum()
    check(pipe, n, want, 1024, "LIP")
    eight = filters + [(S, "is not null", None), (2, "<>", b""), (S, "<>", b"Japan")]
    assert len(eight) == 8
    pipe.scan_filter(eight, lip_joins=1)
    ok8 = ok & np.isin(pk, bk)
    ok8[[i for i, v in enumerate(s1) if v == b"Japan"]] = False
    check(pipe, n, np.nonzero(ok8)[0].astype(np.uint32), 1024, "8 filters")
    pipe.close()


@pytest.mark.parametrize("V", [2, 65536])
def test_vector_edges(gpu_ctx, V):
    """vector_size 2 and 65536 over 2 V + 1 rows: a filter nothing passes (0 chunks), one everything passes, one in between"""
    n = 2 * V + 1
    values = [EDGES[(i * 7 + i // 64) % len(EDGES)] for i in range(n)]
    pipe = make_pipe(gpu_ctx, values, n_blocks=2)
    scan_and_check(pipe, values, [("=", b"no such string")], V)
    assert pipe.scan == (0, 0)
    scan_and_check(pipe, values, [(">=", b"")], V)
    assert pipe.scan == (n, 3)
    scan_and_check(pipe, values, [(">", EDGES[12]), ("<=", b"\x80")], V)
    assert 0 < pipe.scan[0] < n
    pipe.close()


def test_like_range_feeds_a_resident_run(gpu_ctx):
    """scan with a LIKE range -> polr_mpx_use_scan_chunks -> one resident run of a two-join star: COUNT(*) against
    joinref.Ref over the expected rows; a re-scan with another pattern and a second run"""
    n = 8000
    rng = np.random.default_rng(5)
    values = scanstr.fixture_column(99, n)
    k0, k1 = rng.integers(0, 300, n).astype(np.int32), rng.integers(0, 50, n).astype(np.int32)
    joins = [Join(rng.permutation(np.arange(0, 300, 2, dtype=np.int32)), 0), Join(np.arange(0, 40, dtype=np.int32), 2)]
    pipe = make_pipe(gpu_ctx, values, n_blocks=2, extra=[k1], extra_valid=[None], pk=k0, joins=joins)
    m = capi.DeviceMultiplexer(pipe, "default_path")
    for pattern in (b"Jap%", "日本%".encode()):
        f = capi.like_pushdown(pattern)
        want = passing(values, f)
        n_sel, n_chunks = pipe.scan_filter([(S, op, c) for op, c in f])
        check(pipe, n, want, 1024, pattern)
        m.use_scan_chunks()
        capi.run_resident([m], [(0, n_chunks)], reset=True, finish=True)
        ref = Ref([k0, None, k1], None, joins, want)
        counts = ref.stage_counts([0, 1])
        assert counts[-1] > 20
        assert m.finish()["stage_out"][0] == counts, pattern
    m.close()
    pipe.close()


def test_refusals_leave_the_previous_scan(gpu_ctx):
    """every refusal of the contract, and 9 filters; after each, fetch_scan returns the scan before it"""
    n = 3000
    values = [EDGES[i % len(EDGES)] for i in range(n)]
    i1 = (np.arange(n, dtype=np.int32) * 7) % 100
    pipe = make_pipe(gpu_ctx, values, n_blocks=2, extra=[i1], extra_valid=[None])
    first = [(2, "<", 50), (S, ">=", b"ab")]
    pipe.scan_filter(first, vector_size=64)
    want = np.intersect1d(passing(values, [(">=", b"ab")]), np.nonzero(i1 < 50)[0]).astype(np.uint32)
    check(pipe, n, want, 64, "first")
    EQ = capi.CMP["="]
    refused = [
        ("a length without bytes", [(S, EQ, 0, None, 5)], capi.E_INVALID),
        ("bytes against an integer column", [(2, EQ, 0, b"x", 1)], capi.E_INVALID),
        ("bytes with IS NULL against an integer column", [(2, capi.CMP["is null"], 0, b"x", 1)], capi.E_INVALID),
        ("POLR_CMP_STR_EQ", [(S, 8, 0, b"x", 1)], capi.E_INVALID),
        ("a code above IS NOT NULL", [(S, 9, 0, b"x", 1)], capi.E_INVALID),
        ("a column out of range", [(3, EQ, 0, b"x", 1)], capi.E_INVALID),
        ("a constant of 4097 bytes", [(S, EQ, 0, b"y" * 4097, 4097)], capi.E_UNSUPPORTED),
        ("9 filters", [(S, EQ, 0, b"ab", 2)] * 9, capi.E_UNSUPPORTED),
    ]
    for what, filters, code in refused:
        with pytest.raises(capi.PolrError) as e:
            pipe.scan_filter_str_raw(filters, vector_size=64)
        assert e.value.code == code, what
        check(pipe, n, want, 64, what)
    # not refusals: no bytes and no length is the empty string; 4096 bytes; with no 16-byte column the integer scan
    pipe.scan_filter_str_raw([(S, EQ, 0, None, 0)], vector_size=64)
    check(pipe, n, passing(values, [("=", b"")]), 64, "empty constant")
    assert pipe.scan[0] == sum(v == b"" for v in values) > 0
    scan_and_check(pipe, values, [("<", EDGES[-1] + b"y" * (4096 - 300))], 64)
    pipe.scan_filter_str_raw([(2, capi.CMP["<"], 50, None, 0)], vector_size=64)
    check(pipe, n, np.nonzero(i1 < 50)[0].astype(np.uint32), 64, "integer only")
    pipe.close()


def test_heap_that_never_came(gpu_ctx):
    """a column the library uploaded, one non-NULL cell longer than 12 bytes, no heap: POLR_E_INVALID before a pointer is
    followed, the scan before it in place; the same column is accepted when that row is NULL"""
    n = 2000
    long_row = 1234
    for null_it in (False, True):
        values = [(b"a", b"twelve bytes", b"abc")[i % 3] for i in range(n)]
        values[long_row] = None if null_it else b"a string of 25 bytes here"
        host = np.frombuffer(b"a string of 25 bytes here", np.uint8).copy()
        cell = np.zeros(16, np.uint8)
        cell[0:4] = np.frombuffer(np.uint32(25).tobytes(), np.uint8)
        cell[4:8] = host[:4]
        cell[8:16] = np.frombuffer(np.uint64(host.ctypes.data).tobytes(), np.uint8)
        pipe = make_pipe(gpu_ctx, values, heaps=False, null_cell=cell.view("V16")[0])
        if not null_it:
            raw = pipe._test_keep[1][1].view(np.uint8).reshape(-1, 16)
            assert bytes(raw[long_row, 0:4]) == np.uint32(25).tobytes()  # (scanstr.cells wrote the long form)
        pipe.scan_filter([(0, "<", 64)])
        want = np.nonzero(np.arange(n) % 128 < 64)[0].astype(np.uint32)
        check(pipe, n, want, 1024, "integer scan")
        if null_it:
            scan_and_check(pipe, values, [(">=", b"a string")])
            scan_and_check(pipe, values, [("=", b"a string of 25 bytes here")])
            assert pipe.scan == (0, 0)
        else:
            with pytest.raises(capi.PolrError) as e:
                pipe.scan_filter([(S, ">=", b"a string")])
            assert e.value.code == capi.E_INVALID and "heap" in str(e.value)
            check(pipe, n, want, 1024, "after the refusal")
            pipe.scan_filter_str_raw([(S, capi.CMP["is not null"], 0, None, 0)])  # (reads no cell: accepted)
            assert pipe.scan[0] == n
        pipe.close()
