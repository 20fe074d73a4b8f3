"""Dictionary codes of VARCHAR PROBE columns (polr_pipeline_encode_dictionary / polr_pipeline_fetch_dictionary[_codes];
Pipeline.encode_dictionary / .dictionary / .dictionary_strings), over all rows and over the selection in force
(POLR_DICT_SELECTED), and the consumers of the code column.  The reference of every comparison is Python over the inputs: a
dict over bytes in table-row order for first-appearance codes, sorted(set(...)) for sorted codes, numpy for the joins -- never
a second call of the library.  Columns are made as in the build-side dictionary tests: NULL rows whose cells hold garbage
lengths and pointers, dirty inline padding, the heap in two blocks."""
import ctypes as C

import numpy as np
import pytest

from polr_amd import capi
from test_gpu_dictionary_sorted import ALL_EDGES, live_bytes, mixed_values, refused
from test_gpu_group_varchar import dirty_padding
from test_gpu_sink_matrix import MAX_WAVE_CHUNKS, string_blocks

pytestmark = pytest.mark.gpu

SORTED, NULL_INVALID, SELECTED = capi.DICT_SORTED, capi.DICT_NULL_INVALID, capi.DICT_SELECTED
ROWS = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097]
DISTINCT = [1, 2, 1024, 1025, 2049]  # one sort tile, one merge pass, two merge passes (tiles of 1024 values)
N_TABLE = 4097
SELECTIONS = [0, 1, 63, 64, 65, 1025]


# ---- inputs and references -----------------------------------------------------------------------------------------------------
def make_column(n, d, seed, null_share=0.08):
    """n rows over d distinct values (the edge strings first), every value at least once where n allows, shuffled; about 8 %
    NULL rows -> (string per row, validity per row)"""
    rng = np.random.default_rng(seed)
    values = mixed_values(d)
    pick = np.concatenate([np.arange(min(d, n)), rng.integers(0, max(d, 1), max(n - d, 0))])[:n]
    pick = pick[rng.permutation(n)] if n else pick
    strs = [values[i] for i in pick.tolist()]
    valid = (rng.random(n) >= null_share).astype(np.uint8)
    return strs, valid


def py_codes(strs, valid, rows=None, sorted_=False):
    """the dictionary and the codes of the table rows `rows` (None: all): (words, code per table row -- len(words) for a
    NULL row and for a row that takes no part --, has_null)"""
    part = np.zeros(len(strs), bool)
    part[slice(None) if rows is None else np.asarray(rows, dtype=np.int64)] = True
    taking = [(s, bool(ok)) if p else None for s, ok, p in zip(strs, valid.tolist(), part.tolist())]
    if sorted_:
        words = sorted(set(t[0] for t in taking if t and t[1]))
        index = {w: i for i, w in enumerate(words)}
    else:
        index = {}
        for t in taking:  # (table-row order: first appearance is the lowest table row)
            if t and t[1]:
                index.setdefault(t[0], len(index))
        words = list(index)
    codes = [index[t[0]] if t and t[1] else len(words) for t in taking]
    return words, codes, int(any(t is not None and not t[1] for t in taking))


class Probe:
    """probe (pk, VARCHAR columns ...) x one perfect join that every probe row passes exactly once.  columns: [(strings,
    validity or None)]; heaps=False: no heap is handed over"""

    def __init__(self, ctx, columns, n, seed=5, blocks=2, heaps=True):
        self.n = n
        self.ht = capi.HashTable.from_columns(ctx, [np.arange(4, dtype=np.int32)])
        assert self.ht.finalize_perfect(0, 3)
        cols, pv, self.heaps = [(np.arange(n) % 4).astype(np.int32)], [None], []
        for i, (strs, valid) in enumerate(columns):
            v = np.ones(n, np.uint8) if valid is None else valid
            cells, heap = string_blocks(strs, v, blocks, seed + i)
            dirty_padding(cells, strs, v, np.random.default_rng(seed + 100 + i))
            cols.append(cells)
            pv.append(valid)
            self.heaps.append(heap)
        self.n_cols = len(cols)
        self.pipe = capi.Pipeline(ctx, cols, n, [(self.ht, [(-1, 0)])], [[0]], probe_valid=pv)
        if heaps:
            self.set_heaps()

    def set_heaps(self):
        for i, heap in enumerate(self.heaps):
            self.pipe.set_probe_heaps(1 + i, heap)

    def column(self, col):
        """probe column `col` by TABLE ROW, whatever was selected: (values, validity) -- the selection is lifted, every row is
        emitted once and the column materialised"""
        self.pipe.set_selection(None)
        if self.n == 0:
            return np.zeros(0, np.uint32), np.zeros(0, np.uint8)
        out = capi.Output(self.pipe, 1024, self.n // 1024 + 1 + MAX_WAVE_CHUNKS)
        self.pipe.probe_rounds([(0, self.n, 0, 1)], out=out)
        ids = out.fetch_ids()
        assert sorted(ids[:, 0].tolist()) == list(range(self.n))
        assert out._col_width(-1, col) == 4
        got, ok = out.materialize(-1, col, np.uint32)
        vals, okrow = np.zeros(self.n, np.uint32), np.zeros(self.n, np.uint8)
        vals[ids[:, 0]] = got
        okrow[ids[:, 0]] = ok
        out.close()
        return vals, okrow

    def close(self):
        self.pipe.close()
        self.ht.close()


# ---- 1. codes over all rows ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sorted_", [False, True], ids=["first", "sorted"])
@pytest.mark.parametrize("n,d", [(n, min(n, 37)) for n in ROWS] + [(2 * d + 7, d) for d in DISTINCT])
def test_codes_over_all_rows(gpu_ctx, n, d, sorted_):
    """the dictionary is the Python one, the code of every table row is the index of its string in it (a NULL row: n_codes),
    the counts are exact, the column is 4 bytes wide and has no validity array"""
    before = live_bytes()
    strs, valid = make_column(n, d, 1000 + n + d)
    p = Probe(gpu_ctx, [(strs, valid)], n)
    words, codes, has_null = py_codes(strs, valid, sorted_=sorted_)
    assert p.pipe.encode_dictionary(1, sorted=sorted_) == (2, len(words), has_null)
    assert p.pipe.dictionary(2) == words
    got, ok = p.column(2)
    assert got.tolist() == codes and ok.all()
    p.close()
    assert live_bytes() == before


def test_the_string_edges(gpu_ctx):
    """the empty string, 12 and 13 bytes, a shared 8-byte prefix, an embedded NUL, bytes 0x80 and 0xFF, each twice, with
    dirty padding, a heap in two blocks and NULL rows whose cells hold garbage pointers"""
    values = list(dict.fromkeys(ALL_EDGES + [b"", b"x" * 12, b"x" * 13, b"prefix8.", b"prefix8.a", b"prefix8.b" + b"c" * 20,
                                             b"prefix8.b" + b"c" * 19 + b"d", b"nul\0in", b"nul\0io", b"nul", b"\x80", b"\xff", b"\x80\xff"]))
    rng = np.random.default_rng(77)
    strs = [values[i] for i in rng.permutation(np.repeat(np.arange(len(values)), 2)).tolist()] + [b"never read"] * 9
    valid = np.array([1] * (2 * len(values)) + [0] * 9, np.uint8)
    order = rng.permutation(len(strs))
    strs, valid = [strs[i] for i in order.tolist()], valid[order]
    for sorted_ in (False, True):
        p = Probe(gpu_ctx, [(strs, valid)], len(strs))
        words, codes, has_null = py_codes(strs, valid, sorted_=sorted_)
        assert len(words) == len(values) and has_null == 1
        assert p.pipe.encode_dictionary(1, sorted=sorted_) == (2, len(words), 1)
        assert p.pipe.dictionary(2) == words
        assert p.column(2)[0].tolist() == codes
        p.close()


def vector_column(values, pick, valid):
    """string cells of values[pick[r]] per row without a Python loop over the rows: one template cell per value (equal
    strings share their heap bytes), garbage in the NULL rows"""
    tmpl, heap = string_blocks(values, np.ones(len(values), np.uint8), 2, 3)
    cells = tmpl[pick].copy()
    raw = cells.view(np.uint8).reshape(-1, 16)
    raw[valid == 0] = 0xEE  # (length 0xEEEEEEEE, pointer 0xEEEE...: never read)
    return cells, heap


def test_more_rows_than_one_trip_of_the_insert_grid(gpu_ctx):
    """600 001 rows of 5 distinct values (a trip of the insert grid covers CUs x 8 x 256 rows: 524 288 on 256 CUs): over all
    rows, and through a shuffled selection of 540 000 positions"""
    before = live_bytes()
    n, values = 600_001, [b"delta-delta-delta-delta", b"", b"alpha", b"charlie-13-by", b"bravo"]
    rng = np.random.default_rng(9)
    pick = rng.integers(0, 5, n)
    pick[:5] = [3, 3, 0, 4, 1]
    valid = (rng.random(n) >= 0.05).astype(np.uint8)
    valid[:5] = 1
    ht = capi.HashTable.from_columns(gpu_ctx, [np.arange(4, dtype=np.int32)])
    assert ht.finalize_perfect(0, 3)
    cells, heap = vector_column(values, pick, valid)
    pipe = capi.Pipeline(gpu_ctx, [(np.arange(n) % 4).astype(np.int32), cells, cells], n, [(ht, [(-1, 0)])], [[0]], probe_valid=[None, valid, valid])
    pipe.set_probe_heaps(1, heap)
    pipe.set_probe_heaps(2, heap)
    # first appearance over all rows: 3, 0, 4, 1, then 2 wherever it comes first
    first = {}
    for v in pick[valid == 1][:1000].tolist():
        first.setdefault(v, len(first))
    assert len(first) == 5
    assert pipe.encode_dictionary(1) == (3, 5, 1)
    assert pipe.dictionary(3) == [values[v] for v in first]
    want_all = np.where(valid == 1, np.array([first[v] for v in range(5)])[pick], 5)
    # sorted codes through a shuffled selection
    sel = rng.permutation(n)[:540_000].astype(np.uint32)
    pipe.set_selection(sel)
    assert pipe.encode_dictionary(2, sorted=True, selected=True) == (4, 5, 1)
    assert pipe.dictionary(4) == sorted(values)
    rank = np.array([sorted(values).index(v) for v in values])
    part = np.zeros(n, bool)
    part[sel] = True
    want_sel = np.where((valid == 1) & part, rank[pick], 5)
    pipe.set_selection(None)
    out = capi.Output(pipe, 1024, n // 1024 + 1 + MAX_WAVE_CHUNKS)
    pipe.probe_rounds([(0, n, 0, 1)], out=out)
    rows = out.fetch_ids()[:, 0]
    assert np.array_equal(out.materialize(-1, 3, np.uint32)[0], want_all[rows])
    assert np.array_equal(out.materialize(-1, 4, np.uint32)[0], want_sel[rows])
    out.close()
    pipe.close()
    ht.close()
    assert live_bytes() == before


# ---- 2. POLR_DICT_SELECTED -------------------------------------------------------------------------------------------------------
_TABLE = {}


def table():
    """4097 rows over 23 values with NULLs; the same strings once more without a validity array (the NULL rows hold a
    string of their own there).  Made once, shared, left unchanged."""
    if not _TABLE:
        strs, valid = make_column(N_TABLE, 23, 4242)
        _TABLE["strs"], _TABLE["valid"] = strs, valid
        _TABLE["full"] = [s if ok else b"was null" for s, ok in zip(strs, valid.tolist())]
    return _TABLE["strs"], _TABLE["valid"], _TABLE["full"]


def selection(n_sel, order, seed=1):
    rows = np.sort(np.random.default_rng(seed + n_sel).permutation(N_TABLE)[:n_sel]).astype(np.uint32)
    if order == "descending":
        rows = rows[::-1].copy()
    elif order == "shuffled":
        rows = rows[np.random.default_rng(seed + 7).permutation(n_sel)]
    return rows


def lowest_row_in_a_high_lane(strs, valid, sel):
    """some wave of the insert (64 consecutive positions) holds a string twice, its lowest table row in the higher lane"""
    for w in range(0, len(sel), 64):
        seen = {}
        for r in sel[w:w + 64].tolist():
            if valid[r]:
                if strs[r] in seen and r < seen[strs[r]]:
                    return True
                seen[strs[r]] = min(r, seen.get(strs[r], r))
    return False


@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
@pytest.mark.parametrize("n_sel", SELECTIONS)
def test_selected_rows_only(gpu_ctx, n_sel, order):
    """n_codes, has_null and first appearance speak of the selected rows, whatever the order of the selection; a row outside
    it holds n_codes; with NULL_INVALID the code column's validity is `valid AND selected`, also for a source without a
    validity array, and column_stats counts exactly those rows"""
    before = live_bytes()
    strs, valid, full = table()
    sel = selection(n_sel, order)
    if order != "ascending" and n_sel >= 63:
        assert lowest_row_in_a_high_lane(strs, valid, sel)
    p = Probe(gpu_ctx, [(strs, valid), (strs, valid), (full, None)], N_TABLE)
    p.pipe.set_selection(sel)
    # first appearance, no validity array: the unselected rows are seen to hold n_codes
    words, codes, has_null = py_codes(strs, valid, sel)
    assert p.pipe.encode_dictionary(1, selected=True) == (4, len(words), has_null)
    # sorted codes with NULL_INVALID, of a source with and of one without a validity array
    swords, scodes, _ = py_codes(strs, valid, sel, sorted_=True)
    assert p.pipe.encode_dictionary(2, sorted=True, null_invalid=True, selected=True) == (5, len(swords), has_null)
    fwords, fcodes, _ = py_codes(full, np.ones(N_TABLE, np.uint8), sel, sorted_=True)
    assert p.pipe.encode_dictionary(3, sorted=True, null_invalid=True, selected=True) == (6, len(fwords), 0)
    assert (p.pipe.dictionary(4), p.pipe.dictionary(5), p.pipe.dictionary(6)) == (words, swords, fwords)
    part = np.zeros(N_TABLE, bool)
    part[sel] = True
    st = p.pipe.column_stats([5, 6])
    assert [s["n_valid"] for s in st] == [int((part & (valid == 1)).sum()), n_sel]
    if st[0]["n_valid"]:
        assert (st[0]["min_value"], st[0]["max_value"]) == (0, len(swords) - 1)
    got, ok = p.column(4)
    assert got.tolist() == codes and ok.all()
    got, ok = p.column(5)  # (a NULL cell is materialised as zero)
    assert np.array_equal(ok.astype(bool), part & (valid == 1))
    assert got.tolist() == [c if o else 0 for c, o in zip(scodes, ok.tolist())]
    got, ok = p.column(6)
    assert np.array_equal(ok.astype(bool), part)
    assert got.tolist() == [c if o else 0 for c, o in zip(fcodes, ok.tolist())]
    p.close()
    assert live_bytes() == before


def test_a_row_listed_twice_counts_once_and_all_rows_selected_is_the_unselected_answer(gpu_ctx):
    strs, valid, _full = table()
    rng = np.random.default_rng(31)
    p = Probe(gpu_ctx, [(strs, valid)] * 4, N_TABLE)
    # 300 rows, every one listed twice and some three times, shuffled
    rows = rng.permutation(N_TABLE)[:300]
    sel = rng.permutation(np.concatenate([rows, rows, rows[:40]])).astype(np.uint32)
    p.pipe.set_selection(sel)
    for col, sorted_ in ((1, False), (2, True)):
        words, codes, has_null = py_codes(strs, valid, rows, sorted_=sorted_)
        assert p.pipe.encode_dictionary(col, sorted=sorted_, selected=True) == (4 + col, len(words), has_null)
        assert p.pipe.dictionary(4 + col) == words
    # every row selected, in any order: what the call without the flag returns
    p.pipe.set_selection(rng.permutation(N_TABLE).astype(np.uint32))
    words, codes_all, has_null = py_codes(strs, valid)
    assert p.pipe.encode_dictionary(3, selected=True) == (7, len(words), has_null)
    assert p.pipe.encode_dictionary(4) == (8, len(words), has_null)  # (without the flag the selection plays no part)
    assert p.pipe.dictionary(7) == p.pipe.dictionary(8) == words
    for col, sorted_ in ((1, False), (2, True)):
        assert p.column(4 + col)[0].tolist() == py_codes(strs, valid, rows, sorted_=sorted_)[1]
    assert p.column(7)[0].tolist() == p.column(8)[0].tolist() == codes_all
    # with no selection in force the flag means all rows (the selection was lifted by column())
    strs2 = strs[:100]
    q = Probe(gpu_ctx, [(strs2, valid[:100])], 100)
    w2, c2, h2 = py_codes(strs2, valid[:100])
    assert q.pipe.encode_dictionary(1, selected=True, null_invalid=True) == (2, len(w2), h2)
    got, ok = q.column(2)
    assert np.array_equal(ok, valid[:100]) and got.tolist() == [c if o else 0 for c, o in zip(c2, valid[:100].tolist())]
    q.close()
    p.close()


def test_has_null_speaks_of_the_selected_rows(gpu_ctx):
    strs, valid, _full = table()
    assert not valid.all()
    p = Probe(gpu_ctx, [(strs, valid)], N_TABLE)
    sel = np.nonzero(valid)[0][::-3].astype(np.uint32).copy()  # no NULL row among them, descending
    p.pipe.set_selection(sel)
    words, codes, has_null = py_codes(strs, valid, sel)
    assert has_null == 0
    assert p.pipe.encode_dictionary(1, selected=True) == (2, len(words), 0)
    assert p.column(2)[0].tolist() == codes
    p.close()


# ---- 3. the consumers ------------------------------------------------------------------------------------------------------------
NAMES = [b"comedy", b"documentary-feature", b"", b"drama", b"drama-series-13", b"zz", b"action"]


def consumer_probe(rng, n=20_000):
    pick = rng.integers(0, len(NAMES), n)
    valid = (rng.random(n) >= 0.1).astype(np.uint8)
    f = rng.integers(0, 1000, n).astype(np.int32)
    return pick, valid, f


def run_pool(pipe, out, n_chunks, scan):
    mpx = capi.DeviceMultiplexer(pipe, "adaptive_reinit")
    if scan:
        mpx.use_scan_chunks()
    capi.run_resident([mpx], [(0, n_chunks)], out=out, reset=True, finish=True)
    mpx.finish()
    mpx.close()


@pytest.mark.parametrize("shape", ["star", "fanout"])
def test_consumers_of_the_code_column(gpu_ctx, shape):
    """star: two perfect joins (the flat kernel, fuse_grouped); fanout: one hash join whose keys repeat (the generic kernel).
    MIN / MAX / COUNT of the code column through the fused ungrouped sink equal aggregate_string and aggregate of an emitting
    run over the same rows, and Python's min / max; GROUP BY the code column equals GROUP BY the string column"""
    before = live_bytes()
    rng = np.random.default_rng(500 + len(shape))
    n = 20_000
    pick, valid, f = consumer_probe(rng, n)
    strs = [NAMES[i] for i in pick.tolist()]
    cells, heap = string_blocks(strs, valid, 2, 11)
    k1 = rng.integers(0, 50, n).astype(np.int32)
    k2 = rng.integers(0, 33, n).astype(np.int32)
    if shape == "star":
        h1 = capi.HashTable.from_columns(gpu_ctx, [np.arange(40, dtype=np.int32)])
        h2 = capi.HashTable.from_columns(gpu_ctx, [np.arange(30, dtype=np.int32)])
        assert h1.finalize_perfect(0, 39) and h2.finalize_perfect(0, 29)
        joins, paths = [(h1, [(-1, 0)]), (h2, [(-1, 1)])], [[0, 1], [1, 0]]
        mult = ((k1 < 40) & (k2 < 30)).astype(np.int64)
    else:
        bkeys = rng.integers(0, 45, 120).astype(np.int32)  # repeated keys: a probe row finds 0 to several build rows
        h1 = capi.HashTable.from_columns(gpu_ctx, [bkeys])
        h1.finalize_hash()
        joins, paths = [(h1, [(-1, 0)])], [[0]]
        mult = np.bincount(bkeys, minlength=50)[k1].astype(np.int64)
    pipe = capi.Pipeline(gpu_ctx, [k1, k2, f, cells, cells], n, joins, paths, probe_valid=[None, None, None, valid, valid])
    pipe.set_probe_heaps(3, heap)
    pipe.set_probe_heaps(4, heap)
    assert pipe.launch_info()["flat"] == (1 if shape == "star" else 0)
    n_sel, n_chunks = pipe.scan_filter([(2, "<", 400)])
    passed = f < 400
    assert n_sel == int(passed.sum())
    words = sorted(set(s for s, ok, p in zip(strs, valid.tolist(), passed.tolist()) if ok and p))
    has_null = int((passed & (valid == 0)).any())
    assert len(words) == 7 and has_null == 1
    assert pipe.encode_dictionary(3, sorted=True, null_invalid=True, selected=True) == (5, 7, 1)
    assert pipe.encode_dictionary(4, sorted=True, selected=True) == (6, 7, 1)  # (no validity: NULL is the code 7)
    # what Python says of the result rows
    weight = np.where(passed, mult, 0)
    live = [(s, w) for s, ok, w in zip(strs, valid.tolist(), weight.tolist()) if ok and w]
    want_min, want_max, want_count = min(s for s, _ in live), max(s for s, _ in live), sum(w for _, w in live)
    by_str = {}
    for s, ok, w in zip(strs, valid.tolist(), weight.tolist()):
        if w:
            by_str[s if ok else None] = by_str.get(s if ok else None, 0) + w
    assert None in by_str and len(by_str) == 8
    # the fused ungrouped sink: one pool launch, nothing written
    fused = capi.Output(pipe, 1024, 1)
    fused.fuse_aggregate([("min", -1, 5), ("max", -1, 5), ("count", -1, 5), ("count_star", -1, 0)])
    run_pool(pipe, fused, n_chunks, True)
    lo, hi, cnt, star = fused.fused_aggregate_result()
    assert pipe.dictionary_strings(5, [lo, hi]) == [want_min, want_max]
    assert (cnt, star) == (want_count, int(weight.sum())) and fused.stats()[0] == 0
    fused.close()
    # an emitting run over the same rows: the string sink, the integer sink, the grouped sinks
    out = capi.Output(pipe, 1024, int(weight.sum()) // 1024 + 1 + MAX_WAVE_CHUNKS)
    run_pool(pipe, out, n_chunks, True)
    assert out.stats()[0] == int(weight.sum())
    assert (out.aggregate_string("min", -1, 3), out.aggregate_string("max", -1, 3)) == (want_min, want_max)
    assert out.aggregate([("min", -1, 5), ("max", -1, 5), ("count", -1, 5)]) == [lo, hi, cnt]
    hashed = out.aggregate_hashed_str([(-1, 3)], [("count_star", -1, 0)], 64)
    assert {k[0]: v[0] for k, v in hashed.items()} == by_str
    vals, _counts, dropped = out.aggregate_grouped([(-1, 6, 0, 8)], [("count_star", -1, 0)])
    groups = [words[c] if c < 7 else None for c in range(8)]  # index order: ORDER BY the string, NULL last
    assert dropped == 0 and {g: v[0] for g, v in zip(groups, vals)} == by_str
    assert groups[:7] == sorted(k for k in by_str if k is not None)
    vals, _counts, dropped = out.aggregate_grouped([(-1, 5, 0, 7)], [("count_star", -1, 0)])
    assert dropped == by_str[None] and {g: v[0] for g, v in zip(groups[:7], vals)} == {k: v for k, v in by_str.items() if k is not None}
    out.close()
    if shape == "star":  # the fused GROUP BY sink, by the code column
        fg = capi.Output(pipe, 1024, 64)
        fg.fuse_grouped([(-1, 6, 0, 8)], [("count_star", -1, 0)])
        run_pool(pipe, fg, n_chunks, True)
        vals, _counts, dropped = fg.fused_result()
        assert dropped == 0 and {g: v[0] for g, v in zip(groups, vals)} == by_str
        fg.close()
    # a scan-filter expression on the code column (a subset of the selection the codes were made for)
    n_sel2, _ = pipe.scan_filter_expr(("and", ("cmp", 2, "<", 400), ("cmp", 5, "<", 3)))
    rank = {w: i for i, w in enumerate(words)}
    assert n_sel2 == sum(1 for s, ok, p in zip(strs, valid.tolist(), passed.tolist()) if ok and p and rank[s] < 3)
    pipe.close()
    for h, _ in joins:
        h.close()
    assert live_bytes() == before


# ---- 4. handles made before the call, refusals ------------------------------------------------------------------------------------
def test_handles_made_before_the_call_run_on(gpu_ctx):
    strs, valid, _full = table()
    p = Probe(gpu_ctx, [(strs, valid)], N_TABLE)
    sel = selection(1025, "shuffled")
    p.pipe.set_selection(sel)
    out = capi.Output(p.pipe, 1024, 2 + MAX_WAVE_CHUNKS)
    mpx = capi.DeviceMultiplexer(p.pipe, "adaptive_reinit")

    def row_set():
        out.reset()
        capi.run_resident([mpx], [(0, 2)], out=out, reset=True, finish=True)
        mpx.finish()
        pool = sorted(out.fetch_ids()[:, 0].tolist())
        out.reset()
        p.pipe.probe_rounds([(0, 1025, 0, 1)], out=out)
        return pool, sorted(out.fetch_ids()[:, 0].tolist()), out.aggregate_string("min", -1, 1)

    first = row_set()
    assert first[0] == first[1] == sorted(sel.tolist())
    words, _codes, has_null = py_codes(strs, valid, sel, sorted_=True)
    assert p.pipe.encode_dictionary(1, sorted=True, null_invalid=True, selected=True) == (2, len(words), has_null)
    assert row_set() == first
    assert out.aggregate([("min", -1, 2)]) == [words.index(first[2])]  # (and the old output reads the new column)
    mpx.close()
    out.close()
    p.close()


def test_refusals_leave_the_pipeline_as_it_was(gpu_ctx):
    """every refusal, the heap-never-came one included: no column is appended (column_stats of the next index stays
    refused), nothing stays allocated; the corrected call gets the index the first one would have got"""
    strs, valid, _full = table()
    assert any(ok and len(s) > 12 for s, ok in zip(strs, valid.tolist()))
    p = Probe(gpu_ctx, [(strs, valid)], N_TABLE, heaps=False)
    live = live_bytes()

    def untouched():
        return refused(p.pipe.column_stats, [p.n_cols]) == capi.E_INVALID and live_bytes() == live

    assert untouched()
    for flags in (0, SORTED, SELECTED, SORTED | NULL_INVALID | SELECTED):
        assert refused(p.pipe.encode_dictionary, 1, flags=flags) == capi.E_INVALID  # long cells, the heap never came
        assert untouched()
    with pytest.raises(capi.PolrError, match="polr_pipeline_set_probe_heaps"):
        p.pipe.encode_dictionary(1)
    # ... and through a selection, in any order, that names such rows (the guard reads the selected rows only)
    long_rows = [r for r, (s, ok) in enumerate(zip(strs, valid.tolist())) if ok and len(s) > 12][:70]
    p.pipe.set_selection(np.array(long_rows[::-1] + [0, 1, 2], np.uint32))
    live = live_bytes()  # (the uploaded selection)
    for flags in (SELECTED, SORTED | NULL_INVALID | SELECTED):
        assert refused(p.pipe.encode_dictionary, 1, flags=flags) == capi.E_INVALID
        assert untouched()
    for flags in (8, 16, 1 << 31, 0xFFFFFFF8):
        assert refused(p.pipe.encode_dictionary, 1, flags=flags) == capi.E_INVALID    # an undefined flag
    assert refused(p.pipe.encode_dictionary, 2) == capi.E_INVALID                     # no such column
    assert refused(p.pipe.encode_dictionary, 0, sorted=True) == capi.E_INVALID        # a 4-byte column
    assert refused(p.pipe.dictionary, 1) == capi.E_INVALID                            # no dictionary yet
    assert refused(p.pipe.dictionary_strings, 1, [0]) == capi.E_INVALID
    assert untouched()
    p.set_heaps()
    p.pipe.set_selection(None)
    live = live_bytes()
    words, _codes, has_null = py_codes(strs, valid)
    assert p.pipe.encode_dictionary(1) == (2, len(words), has_null)
    # (the scratch is gone: the codes, a cell per code and one more 24-byte column descriptor stay)
    assert live_bytes() == live + 4 * N_TABLE + 16 * len(words) + 24
    live = live_bytes()
    assert refused(p.pipe.encode_dictionary, 1, sorted=True) == capi.E_INVALID         # encoded already
    with pytest.raises(capi.PolrError, match=r"encoded already \(code column 2\)"):
        p.pipe.encode_dictionary(1, selected=True)
    assert refused(p.pipe.encode_dictionary, 2) == capi.E_INVALID                      # a code column as source
    assert refused(p.pipe.column_stats, [3]) == capi.E_INVALID and live_bytes() == live
    assert p.pipe.column_stats([2])[0]["n_valid"] == N_TABLE  # (no NULL_INVALID: no validity array)
    # the build-side call still refuses the new bit
    ht = capi.HashTable.from_columns(gpu_ctx, [np.arange(3, dtype=np.int32)], [capi.string_cells([b"a", b"b", b"a"])[0]])
    assert refused(ht.encode_dictionary, 0, flags=SELECTED) == capi.E_INVALID
    assert ht.encode_dictionary(0) == (1, 2, 0)
    ht.close()
    p.close()


# ---- 5. the fetch calls --------------------------------------------------------------------------------------------------------
def raw_fetch(pipe, code_col, codes, n_offsets, str_cap):
    """polr_pipeline_fetch_dictionary (codes None) / _codes as the C ABI has them, into sentinel-filled buffers ->
    (rc, str_used, offsets, arena)"""
    offs = np.full(max(n_offsets, 1), 0xABABABABABABABAB, np.uint64)
    arena = np.full(max(str_cap, 1), 0xEE, np.uint8)
    used = C.c_uint64(77)
    L = pipe.ctx.L
    if codes is None:
        rc = L.polr_pipeline_fetch_dictionary(pipe.h, code_col, None, offs.ctypes.data, n_offsets, arena.ctypes.data, str_cap, C.byref(used))
    else:
        codes = np.ascontiguousarray(codes, np.uint32)
        rc = L.polr_pipeline_fetch_dictionary_codes(pipe.h, code_col, None, codes.ctypes.data, len(codes), offs.ctypes.data,
                                                    arena.ctypes.data, str_cap, C.byref(used))
    return rc, used.value, offs, arena


def records(arena, offs, n):
    raw = arena.tobytes()
    out = []
    for at in offs[:n].tolist():
        ln = int.from_bytes(raw[at:at + 4], "little")
        out.append(raw[at + 4:at + 4 + ln])
    return out


def test_fetch_the_dictionary_and_listed_codes(gpu_ctx):
    strs, valid, _full = table()
    p = Probe(gpu_ctx, [(strs, valid)], N_TABLE)
    words = py_codes(strs, valid, sorted_=True)[0]
    nc = len(words)
    assert p.pipe.encode_dictionary(1, sorted=True)[1] == nc
    need = sum(4 + len(w) for w in words)
    for n_offsets, cap in ((nc, need - 1), (nc - 1, need), (0, 0)):  # too small, then one retry with the size reported
        rc, used, offs, arena = raw_fetch(p.pipe, 2, None, n_offsets, cap)
        assert rc == capi.E_OVERFLOW and used == need and (offs == 0xABABABABABABABAB).all() and (arena == 0xEE).all()
    rc, used, offs, arena = raw_fetch(p.pipe, 2, None, nc, used)
    assert rc == capi.OK and used == need and records(arena, offs, nc) == words
    listed = [nc - 1, 0, 0, 3, nc - 1, 3, 3]  # duplicates, any order
    need = sum(4 + len(words[c]) for c in listed)
    rc, used, offs, arena = raw_fetch(p.pipe, 2, listed, len(listed), need - 1)
    assert rc == capi.E_OVERFLOW and used == need and (offs == 0xABABABABABABABAB).all() and (arena == 0xEE).all()
    rc, used, offs, arena = raw_fetch(p.pipe, 2, listed, len(listed), used)
    assert rc == capi.OK and used == need and records(arena, offs, len(listed)) == [words[c] for c in listed]
    assert p.pipe.dictionary_strings(2, listed, str_cap=1) == [words[c] for c in listed]  # (the binding's one retry)
    assert p.pipe.dictionary(2, str_cap=1) == words
    assert raw_fetch(p.pipe, 2, [], 0, 0)[:2] == (capi.OK, 0)
    for bad in ([nc], [0, 1, nc, 2], [0xFFFFFFFF]):  # the NULL code is not a string
        rc, used, offs, arena = raw_fetch(p.pipe, 2, bad, len(bad), 4096)
        assert rc == capi.E_INVALID and used == 77 and (offs == 0xABABABABABABABAB).all() and (arena == 0xEE).all()
    assert raw_fetch(p.pipe, 1, None, nc, 4096)[0] == capi.E_INVALID  # not a code column
    assert raw_fetch(p.pipe, 1, [0], 1, 4096)[0] == capi.E_INVALID
    p.close()


# ---- 6. a pipeline made from an output ---------------------------------------------------------------------------------------
def test_a_pipeline_from_an_output_encodes_and_runs_fused(gpu_ctx):
    """library-owned cells and a packed heap: the second stage's VARCHAR source column is encoded, COUNT(*) / MIN / MAX are
    folded in one pool launch, and a third stage carries the code column on as a plain 4-byte column"""
    before = live_bytes()
    strs, valid, _full = table()
    p = Probe(gpu_ctx, [(strs, valid)], N_TABLE)
    sel = selection(1025, "ascending")
    p.pipe.set_selection(sel)
    out = capi.Output(p.pipe, 1024, 2 + MAX_WAVE_CHUNKS)
    p.pipe.probe_rounds([(0, 1025, 0, 1)], out=out)
    rows = out.fetch_ids()[:, 0]  # (row r of the new pipeline is output row r)
    keys2 = np.array([0, 2, 2, 3], np.int32)  # pk 1 finds nothing, pk 2 twice
    h2 = capi.HashTable.from_columns(gpu_ctx, [keys2])
    h2.finalize_hash()
    pipe2 = capi.Pipeline.from_output(out, [(-1, 0), (-1, 1)], [(h2, [(-1, 0)])], [[0]])
    out.close()
    p.close()
    s2 = [strs[r] for r in rows.tolist()]
    v2 = valid[rows]
    words, codes, has_null = py_codes(s2, v2, sorted_=True)
    assert pipe2.encode_dictionary(1, sorted=True, null_invalid=True, selected=True) == (2, len(words), has_null)
    assert pipe2.dictionary(2) == words
    mult = np.array([1, 0, 2, 1])[rows % 4]
    live = [s for s, ok, m in zip(s2, v2.tolist(), mult.tolist()) if ok and m]
    fused = capi.Output(pipe2, 1024, 1)
    fused.fuse_aggregate([("count_star", -1, 0), ("min", -1, 2), ("max", -1, 2), ("count", -1, 2)])
    run_pool(pipe2, fused, 2, False)
    star, lo, hi, cnt = fused.fused_aggregate_result()
    assert star == int(mult.sum()) and cnt == int(mult[v2 == 1].sum())
    assert pipe2.dictionary_strings(2, [lo, hi]) == [min(live), max(live)]
    fused.close()
    # carried forward: codes and validity, not the strings
    out2 = capi.Output(pipe2, 1024, 2 + MAX_WAVE_CHUNKS)
    pipe2.probe_rounds([(0, 1025, 0, 1)], out=out2)
    rows2 = out2.fetch_ids()[:, 0]
    h3 = capi.HashTable.from_columns(gpu_ctx, [np.arange(4, dtype=np.int32)])
    assert h3.finalize_perfect(0, 3)
    pipe3 = capi.Pipeline.from_output(out2, [(-1, 0), (-1, 2)], [(h3, [(-1, 0)])], [[0]])
    st = pipe3.column_stats([1])[0]
    assert st["n_valid"] == int(v2[rows2].sum()) and (st["min_value"], st["max_value"]) == (lo, hi)
    assert refused(pipe3.dictionary, 1) == capi.E_INVALID and refused(pipe3.encode_dictionary, 1) == capi.E_INVALID
    for h in (pipe3, out2, pipe2, h3, h2):
        h.close()
    assert live_bytes() == before
