"""The pass bits of the device source scan: every entry point (polr_pipeline_scan_filter, _lip, _str, _expr) evaluates a row
once, keeps the ballot of every 64-row step -- ceil(V / 64) words per vector -- and writes the selection from those words.
Checked here: the word layout at its edges (rows and vector sizes around 64, the last vector cut by the table's end, an empty
table), one pipeline whose scans change entry point and words-per-vector, and refusals that must leave the installed scan.

The reference is never the device: the rows come from tests/scanexpr.py (which evaluates integer and VARCHAR leaves alike;
tests/scanstr.py and the oracle's scan_filter are held against it where they apply), LIP membership from np.isin, the
chunk boundaries from scanstr.chunks_of."""
import ctypes as C

import numpy as np
import pytest

import scanexpr
import scanstr
from common import orc
from joinref import Join
from polr_amd import capi

pytestmark = pytest.mark.gpu

PK, I, S, BLK = 0, 1, 2, 3  # the table: (pk INTEGER, i INTEGER with NULLs, s VARCHAR: inline and heap cells, NULLs, blk INTEGER)
BUILD_KEYS = np.arange(0, 32, 2, dtype=np.int32)  # the 16-key build side: LIP keeps the rows whose pk is even
WORDS = [b"Japan", b"Jap", b"Japanese-language (heap cell)", b"Jaq", b"J", b"Tokyo", b"twelve bytes", b"twelve bytes!",
         b"Japan: a string of more than twelve bytes", b"", b"Jamaica"]
assert sum(len(w) > 12 for w in WORDS) >= 3

FILTER_SETS = {
    "none": [],
    "int": [(I, "<", 50)],
    "int+notnull": [(I, ">=", 20), (I, "is not null", None)],
    "like-range": [(S, ">=", b"Jap"), (S, "<", b"Jaq")],
}


class Table:
    def __init__(self, ctx, n, string_nulls=True):
        r = np.arange(n)
        self.n = n
        self.pk = ((r * 7 + r // 64) % 32).astype(np.int32)
        self.i = ((r * 37 + r // 100) % 100).astype(np.int32)
        self.ivalid = (r % 5 != 2).astype(np.uint8)
        self.blk = ((r // 100) % 3).astype(np.int32)  # constant over every 100-row vector
        self.s = [None if string_nulls and x % 7 == 3 else WORDS[(x * 5 + x // 11) % len(WORDS)] for x in range(n)]
        cells, svalid, blocks = scanstr.cells(self.s, 2, null_cell=b"Japan", dirty_seed=n + 1)
        self.join = Join(BUILD_KEYS, PK)
        self.ht = self.join.device(ctx)
        self.keep = (cells, blocks)
        self.pipe = capi.Pipeline(ctx, [self.pk, self.i, cells, self.blk], n, [(self.ht, [(-1, PK)])], [[0]],
                                  probe_valid=[None, self.ivalid, svalid, None])
        self.pipe.set_probe_heaps(S, blocks)
        self.cols = {PK: (self.pk, None), I: (self.i, self.ivalid), S: self.s, BLK: (self.blk, None)}
        self.member = np.isin(self.pk, BUILD_KEYS)

    def want_rows(self, filters, lip):
        """the rows the AND of `filters` keeps (and LIP on join 0): scanexpr; the same from scanstr / the oracle where
        the filter set is theirs to evaluate"""
        ok = np.ones(self.n, bool)
        for f in filters:
            ok &= scanexpr.evaluate(("cmp",) + tuple(f), self.cols)[0]
        if filters and all(c == S for c, _, _ in filters):
            assert np.array_equal(np.nonzero(ok)[0], scanstr.passing(self.s, [(op, c) for _, op, c in filters]))
        if all(c != S for c, _, _ in filters) and self.n:
            # (column S is not the oracle's to read: pk stands in its place)
            osel, _ = orc.scan_filter([self.pk, self.i, self.pk, self.blk], filters, valids=[None, self.ivalid, None, None])
            assert np.array_equal(np.nonzero(ok)[0], osel)
        if lip:
            ok &= self.member
        return np.nonzero(ok)[0].astype(np.uint32)

    def check(self, want, V, what):
        sel, offs = self.pipe.fetch_scan()
        want_offs = scanstr.chunks_of(want, self.n, V)
        assert self.pipe.scan == (len(want), len(want_offs) - 1), what
        assert np.array_equal(sel, want), what
        assert np.array_equal(offs, want_offs), what
        return sel, offs

    def close(self):
        self.pipe.close()
        self.ht.close()


def as_program(filters):
    leaves = [("cmp", c, op, const) for c, op, const in filters]
    return None if not leaves else leaves[0] if len(leaves) == 1 else ("and",) + tuple(leaves)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 129, 1000, 4097])
def test_word_layout_edges(gpu_ctx, n):
    """every filter set, without and with LIP, at every vector size: through scan_filter (the integer entry point, or the
    VARCHAR one for the LIKE range) and through scan_filter_expr with the same AND program -- both equal the reference in
    n_selected, n_chunks, sel and offs, hence each other"""
    t = Table(gpu_ctx, n)
    for name, filters in FILTER_SETS.items():
        for lip in (0, 1):
            want = t.want_rows(filters, lip)
            for V in (2, 64, 65, 100, 1024):
                what = (name, lip, V)
                t.pipe.scan_filter(filters, vector_size=V, lip_joins=lip)
                a = t.check(want, V, what)
                scan_a = t.pipe.scan
                t.pipe.scan_filter_expr(as_program(filters), vector_size=V, lip_joins=lip)
                b = t.check(want, V, what)
                assert t.pipe.scan == scan_a and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), what
            if n >= 1000 and (filters or lip):
                assert 0 < len(want) < n, (name, lip)
    t.close()


def test_one_pipeline_changing_scans(gpu_ctx):
    """expression scan at V = 64 (one word per vector), integer scan at V = 1024 (16 words), VARCHAR scan at V = 2 that keeps
    every row (2049 vectors of one word), integer scan at V = 100 (two words) that leaves two vectors of three empty, the
    first scan again: the pass-bit buffer grows, is re-used with another words-per-vector, and no scan reads a word of the
    one before"""
    n = 4097
    t = Table(gpu_ctx, n, string_nulls=False)
    first = ("or", ("cmp", I, "<", 10), ("and", ("cmp", S, ">=", b"Jap"), ("cmp", S, "<", b"Jaq")))
    every = [(S, ">=", b""), (S, "<", b"\xff\xff")]
    steps = [
        ("expr", first, 64, scanexpr.passing(first, t.cols, n)),
        ("int", [(I, "<", 50)], 1024, t.want_rows([(I, "<", 50)], 0)),
        ("str", every, 2, t.want_rows(every, 0)),
        ("int", [(BLK, "=", 1)], 100, t.want_rows([(BLK, "=", 1)], 0)),
        ("expr", first, 64, scanexpr.passing(first, t.cols, n)),
    ]
    assert len(steps[2][3]) == n and 0 < len(steps[0][3]) < n and np.array_equal(steps[3][3], np.nonzero(t.blk == 1)[0])
    for kind, f, V, want in steps:
        if kind == "expr":
            t.pipe.scan_filter_expr(f, vector_size=V)
        else:
            t.pipe.scan_filter(f, vector_size=V)
        t.check(want, V, (kind, V))
    t.close()


def test_refusals_keep_the_result(gpu_ctx):
    """a column out of range, vector size 1 and a LIP mask beyond the pipeline's one join, through each entry point (the mask:
    through the three that take one): each raises, and fetch_scan still returns the scan before"""
    n = 1000
    t = Table(gpu_ctx, n)
    good = [(I, "<", 50), (S, ">=", b"Jap")]
    t.pipe.scan_filter(good, vector_size=64, lip_joins=1)
    want = t.want_rows(good, 1)
    assert 0 < len(want) < n
    t.check(want, 64, "the good scan")
    L, h = t.pipe.ctx.L, t.pipe.h

    def plain(filters, vector_size):  # polr_pipeline_scan_filter itself: the binding's scan_filter calls _lip
        arr = (capi.ScanFilter * len(filters))()
        for x, (col, op, const) in enumerate(filters):
            arr[x].col, arr[x].op, arr[x].constant = col, capi.CMP[op], const
        ns, nc = C.c_uint64(), C.c_uint64()
        t.pipe.ctx.check(L.polr_pipeline_scan_filter(h, None, arr, len(filters), vector_size, C.byref(ns), C.byref(nc)))

    ok_int, ok_str, ok_expr = [(I, "<", 50)], [(S, "=", b"Japan")], ("cmp", I, "<", 50)
    refused = [
        ("plain: column", lambda: plain([(BLK + 1, "<", 50)], 64)),
        ("plain: vector size", lambda: plain(ok_int, 1)),
        ("lip: column", lambda: t.pipe.scan_filter([(BLK + 1, "<", 50)], vector_size=64)),
        ("lip: vector size", lambda: t.pipe.scan_filter(ok_int, vector_size=1)),
        ("lip: mask", lambda: t.pipe.scan_filter(ok_int, vector_size=64, lip_joins=2)),
        ("str: column", lambda: t.pipe.scan_filter([(BLK + 1, "=", b"Japan")], vector_size=64)),
        ("str: vector size", lambda: t.pipe.scan_filter(ok_str, vector_size=1)),
        ("str: mask", lambda: t.pipe.scan_filter(ok_str, vector_size=64, lip_joins=2)),
        ("expr: column", lambda: t.pipe.scan_filter_expr(("cmp", BLK + 1, "<", 50), vector_size=64)),
        ("expr: vector size", lambda: t.pipe.scan_filter_expr(ok_expr, vector_size=1)),
        ("expr: mask", lambda: t.pipe.scan_filter_expr(ok_expr, vector_size=64, lip_joins=2)),
    ]
    for what, call in refused:
        with pytest.raises(capi.PolrError) as e:
            call()
        assert e.value.code == capi.E_INVALID, what
        t.check(want, 64, what)  # (pipe.scan, the binding's record of the last good call, is the good scan's still)
    t.close()
