"""Dictionary codes for VARCHAR build columns (polr_ht_encode_dictionary / polr_ht_fetch_dictionary, HashTable.encode_dictionary
/ .dictionary) and the grouped and fused sinks over them.  Everything is exact integer / byte equality against Python over
the inputs: a `dict` for the first-appearance codes, the numpy join of tests/joinref.py, Python ints for the aggregates, the
reference-run fixture for Q4.1 -- never anything the code under test computed.  Engines as in tests/test_gpu_group_varchar.py:

  path     the path kernel (probe_rounds) over a repeated-key hash table
  generic  the generic pool (run_resident) over the same table
  flat     the emitting flat pool (run_resident) over a perfect table (encoded before finalize_perfect)
"""
import ctypes as C

import numpy as np
import pytest

import common
import strref
from joinref import Join, Ref, device_rows, sort_rows
from polr_amd import capi
from test_gpu_group_varchar import ALL_AGGS, EDGES, big_values, dirty_padding, distinct_strings, string_pool
from test_gpu_sink_matrix import MAX_WAVE_CHUNKS, py_agg, string_blocks

pytestmark = pytest.mark.gpu

ENGINES = ["path", "generic", "flat"]
G_MIN, G_N = 10, 5  # domain of the integer group column b_g


def py_dictionary(strs, valid):
    """first-appearance codes: ([string per code], [code per row]); NULL rows get n_codes"""
    d = {}
    for s, ok in zip(strs, valid):
        if ok:
            d.setdefault(s, len(d))
    return list(d), [d[s] if ok else len(d) for s, ok in zip(strs, valid)]


class DictBank:
    """probe (pk, p_i int16, p_big int64) x one join (repeated-key hash table; perfect for `flat`; 3 % NULL keys) with payload
    (b_s VARCHAR, b_s2 VARCHAR, b_i int32, b_big int64, b_g int32 without NULLs).  The VARCHAR columns: 8 % NULLs whose cells
    hold garbage, dirty inline padding, heap in three blocks (heaps=False: no heap is handed over).  The table is uploaded by
    the constructor; encode() / finish() do the rest, so that a test can put refused calls in between."""
    PROBE = {"p_i": 1, "p_big": 2}
    BUILD = {"b_s": 0, "b_s2": 1, "b_i": 2, "b_big": 3, "b_g": 4}
    N_PAYLOAD = 5

    def __init__(self, ctx, engine, seed, n=20_000, nb=3000, b_strs=None, b_valid=None, heaps=True, cap=64):
        rng = np.random.default_rng(seed)
        self.ctx, self.engine, self.n, self.nb, self.cap = ctx, engine, n, nb, cap
        if engine == "flat":
            bk = rng.permutation(np.arange(0, nb, dtype=np.int32))
        else:
            bk = rng.permutation(np.repeat(np.arange(0, nb, 2, dtype=np.int32), 2))
        kvalid = (rng.random(nb) > 0.03).astype(np.uint8)
        self.join = Join(bk, 0, (0, nb - 1) if engine == "flat" else None, valid=kvalid)
        self.pk = rng.integers(-nb // 30, nb + nb // 30, n).astype(np.int32)
        pool = string_pool(rng)
        assert pool[:len(EDGES)] == EDGES
        self.cols = {"p_i": rng.integers(-3, 4, n).astype(np.int16), "p_big": big_values(rng, n),
                     "b_s": b_strs if b_strs is not None else [pool[i] for i in rng.integers(0, 40, nb)],
                     "b_s2": [pool[i] for i in rng.integers(10, 30, nb)],
                     "b_i": rng.choice(np.array([-(1 << 31), -1, 0, 1, (1 << 31) - 1], np.int32), nb),
                     "b_big": big_values(rng, nb), "b_g": rng.integers(G_MIN, G_MIN + G_N, nb).astype(np.int32)}
        self.valid = {c: (rng.random(len(v)) > 0.08).astype(np.uint8) for c, v in self.cols.items()}
        self.valid["b_g"] = np.ones(nb, np.uint8)
        if b_valid is not None:
            self.valid["b_s"] = b_valid
        cells, heap = string_blocks(self.cols["b_s"], self.valid["b_s"], 3, seed + 1)
        cells2, heap2 = string_blocks(self.cols["b_s2"], self.valid["b_s2"], 3, seed + 2)
        dirty_padding(cells, self.cols["b_s"], self.valid["b_s"], rng)
        dirty_padding(cells2, self.cols["b_s2"], self.valid["b_s2"], rng)
        self.keep = (cells, heap, cells2, heap2)  # (host heaps stay alive as long as the bank)
        self.ht = capi.HashTable.from_columns(ctx, [bk], [cells, cells2, self.cols["b_i"], self.cols["b_big"], self.cols["b_g"]],
                                              key_valid=[kvalid],
                                              payload_valid=[self.valid[c] for c in ("b_s", "b_s2", "b_i", "b_big")] + [None])
        if heaps:
            self.set_heaps()
        self.pipe = self.out = None

    def set_heaps(self):
        self.ht.set_payload_heaps(0, self.keep[1])
        self.ht.set_payload_heaps(1, self.keep[3])

    def finalize(self):
        if self.engine == "flat":
            assert self.ht.finalize_perfect(0, self.nb - 1)
        else:
            self.ht.finalize_hash()

    def finish(self):
        """finalize, run the join on the bank's engine, check the row set"""
        self.finalize()
        n = self.n
        self.pipe = capi.Pipeline(self.ctx, [self.pk, self.cols["p_i"], self.cols["p_big"]], n, [(self.ht, [(-1, 0)])], [[0]],
                                  probe_valid=[None] + [self.valid[c] for c in ("p_i", "p_big")])
        assert self.pipe.launch_info(True)["flat"] == int(self.engine == "flat")  # which engine emits the row ids
        self.rows = sort_rows(Ref([self.pk], None, [self.join]).rows())
        assert len(self.rows) > n // 2
        self.out = capi.Output(self.pipe, self.cap, len(self.rows) // self.cap + 1 + MAX_WAVE_CHUNKS)
        if self.engine == "path":
            self.pipe.probe_rounds([(0, n, 0, 1)], out=self.out)
        else:
            mx = capi.DeviceMultiplexer(self.pipe, "default_path")
            capi.run_resident([mx], [(0, (n + 1023) // 1024)], out=self.out, reset=True, finish=True)
            mx.finish()
            mx.close()
        self.dev_rows = device_rows(self.out.fetch_ids(), [self.join])  # (in the order the sinks and materialize see them)
        assert np.array_equal(sort_rows(self.dev_rows), self.rows)
        return self

    def col(self, name):
        return (-1, self.PROBE[name]) if name in self.PROBE else (0, self.BUILD[name])

    def column(self, name):
        """(python values, validity) of a column over the reference's join rows"""
        r = self.rows[:, 0] if name in self.PROBE else self.rows[:, 1]
        v = self.cols[name]
        vals = [v[i] for i in r.tolist()] if isinstance(v, list) else v[r].tolist()
        return vals, self.valid[name][r].astype(bool).tolist()

    def want(self, group_names, specs):
        """exact Python GROUP BY: {key tuple (bytes / int / None): [aggregate values]}"""
        keys = [self.column(c) for c in group_names]
        members = {}
        for i in range(len(self.rows)):
            members.setdefault(tuple(v[i] if ok[i] else None for v, ok in keys), []).append(i)
        aggs = {}
        for fn, name in specs:
            if name is not None and name not in aggs:
                v, ok = self.column(name)
                aggs[name] = (np.array(v, dtype=object), np.array(ok, dtype=bool))
        return {key: [len(idx) if fn == "count_star" else py_agg(fn, aggs[name][0][idx], aggs[name][1][idx]) for fn, name in specs]
                for key, idx in members.items()}

    def specs(self, specs):
        return [(fn, -1, 0) if name is None else (fn, *self.col(name)) for fn, name in specs]

    def close(self):
        if self.out:
            self.out.close()
        if self.pipe:
            self.pipe.close()
        self.ht.close()


def check_cells(vals, domains, decode, want, n_aggs):
    """every cell of a grouped result over mixed-radix `domains` against the Python groups: decode(index tuple) -> key"""
    seen = 0
    for g, v in enumerate(vals):
        idx, rest = [], g
        for nv in reversed(domains):
            idx.append(rest % nv)
            rest //= nv
        key = decode(tuple(reversed(idx)))
        if key in want:
            assert v == want[key], key
            seen += 1
        else:
            assert v[0] == 0, key  # (COUNT(*) of a group no row fell into)
    assert seen == len(want)
    assert len(vals[0]) == n_aggs


# ---- 1. codes and dictionary on the three engines ------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ENGINES)
def test_codes_and_dictionary(gpu_ctx, engine):
    """a build column over the string edges (inline / heap boundary, shared 12-byte prefixes, last-byte differences, empty
    string, \\0 and 0xFF bytes), 8 % NULLs with garbage cells, dirty padding, heap in three blocks: the dictionary is the
    Python first-appearance list, and the code column gathered over the join result is the Python code of every output row's
    build row (NULL -> n_codes)"""
    b = DictBank(gpu_ctx, engine, seed=700 + ENGINES.index(engine))
    words, codes = py_dictionary(b.cols["b_s"], b.valid["b_s"])
    assert set(EDGES) <= set(words) and not b.valid["b_s"].all()
    info = b.ht.info()
    code_col, n_codes, has_null = b.ht.encode_dictionary(0)
    assert (code_col, n_codes, has_null) == (DictBank.N_PAYLOAD, len(words), 1)
    assert b.ht.info()["kind"] == info["kind"] == 0
    assert b.ht.dictionary(code_col) == words
    assert b.ht.dictionary(code_col, str_cap=1) == words  # (the binding's one retry)
    b.finish()
    assert b.ht.dictionary(code_col) == words  # (finalizing keeps the dictionary)
    assert b.out._col_width(0, code_col) == 4
    got, ok = b.out.materialize(0, code_col, np.uint32)
    assert ok.all()  # (no validity array: NULL is a code)
    assert got.tolist() == [codes[r] for r in b.dev_rows[:, 1].tolist()]
    assert n_codes in got.tolist()  # (NULL rows are in the join result)
    b.close()


# ---- 2. the perfect-hash sink keyed by (code column, integer column) -------------------------------------------------------
@pytest.mark.parametrize("engine", ENGINES)
def test_grouped_sink_on_codes(gpu_ctx, engine):
    """aggregate_grouped keyed by (code column, b_g): with n_values = n_codes + has_null NULL is a group of its own and the
    cells are exact Python grouping by (bytes-or-None, int) for eight aggregates (sums beyond int64), nothing dropped; with
    n_values = n_codes the NULL rows are counted in `dropped` and the other groups are unchanged.  The same groups as
    aggregate_hashed_str over the VARCHAR column itself on the same output."""
    b = DictBank(gpu_ctx, engine, seed=710 + ENGINES.index(engine))
    words, _codes = py_dictionary(b.cols["b_s"], b.valid["b_s"])
    code_col, n_codes, has_null = b.ht.encode_dictionary(0)
    assert (n_codes, has_null) == (len(words), 1)
    b.finish()
    want = b.want(["b_s", "b_g"], ALL_AGGS)
    assert any(k[0] is None for k in want) and any(v[2] is not None and abs(v[2]) > (1 << 64) for v in want.values())
    specs = b.specs(ALL_AGGS)
    g_col = b.col("b_g")[1]
    vals, _counts, dropped = b.out.aggregate_grouped([(0, code_col, 0, n_codes + has_null), (0, g_col, G_MIN, G_N)], specs)
    assert dropped == 0
    check_cells(vals, [n_codes + 1, G_N], lambda i: (words[i[0]] if i[0] < n_codes else None, G_MIN + i[1]), want, len(specs))
    vals, _counts, dropped = b.out.aggregate_grouped([(0, code_col, 0, n_codes), (0, g_col, G_MIN, G_N)], specs)
    assert dropped == sum(v[0] for k, v in want.items() if k[0] is None) > 0
    check_cells(vals, [n_codes, G_N], lambda i: (words[i[0]], G_MIN + i[1]), {k: v for k, v in want.items() if k[0] is not None},
                len(specs))
    assert b.out.aggregate_hashed_str([b.col("b_s"), b.col("b_g")], specs, max(1024, 2 * len(want))) == want
    # ... and the general hash sink takes the code column as the integer column it is
    hashed = b.out.aggregate_hashed([(0, code_col), (0, g_col)], specs, max(1024, 2 * len(want)))
    assert {(words[k[0]] if k[0] < n_codes else None, k[1]): v for k, v in hashed.items()} == want
    b.close()


# ---- 3. two VARCHAR columns of one table, both encoded, + an integer column (the Q3 shape) ----------------------------------
@pytest.mark.parametrize("engine", ENGINES)
def test_two_encoded_columns_and_an_integer(gpu_ctx, engine):
    b = DictBank(gpu_ctx, engine, seed=720 + ENGINES.index(engine))
    w1, _ = py_dictionary(b.cols["b_s"], b.valid["b_s"])
    w2, _ = py_dictionary(b.cols["b_s2"], b.valid["b_s2"])
    c2 = b.ht.encode_dictionary(1)  # (the second column first: code columns are appended in call order)
    c1 = b.ht.encode_dictionary(0)
    assert c2 == (DictBank.N_PAYLOAD, len(w2), 1) and c1 == (DictBank.N_PAYLOAD + 1, len(w1), 1)
    assert b.ht.dictionary(c1[0]) == w1 and b.ht.dictionary(c2[0]) == w2
    b.finish()
    want = b.want(["b_s", "b_s2", "b_g"], ALL_AGGS)
    assert any(k[0] is None and k[1] is None for k in want)
    specs = b.specs(ALL_AGGS)
    domains = [len(w1) + 1, len(w2) + 1, G_N]
    vals, _counts, dropped = b.out.aggregate_grouped([(0, c1[0], 0, domains[0]), (0, c2[0], 0, domains[1]),
                                                      (0, b.col("b_g")[1], G_MIN, G_N)], specs)
    assert dropped == 0
    check_cells(vals, domains, lambda i: (w1[i[0]] if i[0] < len(w1) else None, w2[i[1]] if i[1] < len(w2) else None, G_MIN + i[2]),
                want, len(specs))
    b.close()


# ---- 4. SSB-skew Q4.1 with the real c_nation, fused, against the reference (tests/golden/ssb_q41_varchar.json) ------------------
@pytest.mark.parametrize("n_exec", [1, 16])
@pytest.mark.parametrize("run", ["rows", "rows_nulls"])
def test_q41_with_varchar_nation_fused_against_the_reference(gpu_ctx, run, n_exec):
    """c_nation goes up as string_t cells + heap, is dictionary-encoded on the customer build side, and the GROUP BY d_year,
    c_nation is fused into the flat pipeline's last join over the code column: no row id is written, the group cells are the
    reference's rows; a second pass doubles every sum"""
    from polr_amd import ssb_skew
    gold = common.load_golden("ssb_q41_varchar")
    want = {(r[0], None if r[1] is None else r[1].encode()): r[2] for r in gold[run]}
    assert len(want) == len(gold[run])
    wl = ssb_skew.workload("q4.1", **gold["shape"])
    inst = wl["instance"]
    m = inst.lineorder(0, inst.n_lo, cols=["lo_revenue", "lo_supplycost"])
    names = list(wl["probe"]["cols"].keys()) + ["lo_revenue", "lo_supplycost"]
    cols = list(wl["probe"]["cols"].values()) + [m["lo_revenue"], m["lo_supplycost"]]
    n = len(cols[0])
    cust = wl["joins"][0]
    assert cust["name"] == "customer" and wl["joins"][3]["name"] == "date"
    cust["strings"] = {"c_nation_name": strref.nation_names(cust["payload"]["c_nation"])}
    valid = np.ones(len(cust["keys"][0]), np.uint8)
    if run == "rows_nulls":
        assert gold["null_every"] == strref.NULL_EVERY
        valid = strref.nation_valid(cust["keys"][0])
        cust["strings_valid"] = {"c_nation_name": valid}
    cust["dictionary"] = ["c_nation_name"]
    joins = capi.build_joins(gpu_ctx, wl, auto=True)
    code_col, (n_codes, has_null) = capi.dictionary_payload_index(cust, "c_nation_name")
    words, _codes = py_dictionary(cust["strings"]["c_nation_name"], valid)
    assert code_col == capi.string_payload_index(cust, "c_nation_name") + 1
    assert (n_codes, has_null) == (len(words), int(run == "rows_nulls")) and joins[0][0].dictionary(code_col) == words
    assert {w for _y, w in want if w is not None} <= set(words)
    paths = np.asarray(common.load_golden("ssb_skew_sample")["cases"]["q4.1/3"]["paths"], dtype=np.int32)
    pipe = capi.Pipeline(gpu_ctx, cols, n, joins, paths)
    assert pipe.launch_info(True)["flat"] == 1
    years = sorted({y for y, _c in want})
    y0, ny = years[0], years[-1] - years[0] + 1
    nv = n_codes + has_null
    specs = [("count_star", -1, 0), ("sum", -1, names.index("lo_revenue")), ("sum", -1, names.index("lo_supplycost"))]
    out = capi.Output(pipe, 1024, 64)  # (no room for the row ids: none are written)
    out.fuse_grouped([(3, 0, y0, ny), (0, code_col, 0, nv)], specs)
    n_chunks = (n + 1023) // 1024
    mpxs = [capi.DeviceMultiplexer(pipe, "adaptive_reinit") for _ in range(n_exec)]
    ranges = [((e * n_chunks) // n_exec, ((e + 1) * n_chunks) // n_exec) for e in range(n_exec)]
    k = len(wl["joins"])
    for passes in (1, 2):
        capi.run_resident(mpxs, ranges, out=out, reset=True, finish=True)
        stats = capi.finish_many(mpxs)
        vals, _counts, dropped = out.fused_result()
        assert dropped == 0 and len(vals) == ny * nv
        got = {(y0 + g // nv, words[g % nv] if g % nv < n_codes else None): v[1] - v[2] for g, v in enumerate(vals) if v[0]}
        assert got == {key: passes * v for key, v in want.items()}
        assert all(v[1] is None for v in vals if not v[0])
        n_out = sum(sum(st["stage_out"][p][k - 1] for p in range(len(paths))) for st in stats)
        assert sum(v[0] for v in vals) == passes * n_out
        assert out.stats()[0] == 0  # nothing was emitted
    if run == "rows_nulls":
        assert any(key[1] is None for key in got)
    for m_ in mpxs:
        m_.close()
    out.close()
    pipe.close()
    for h, _ in joins:
        h.close()


# ---- 5. extremes ---------------------------------------------------------------------------------------------------------------
def encoded_codes(ctx, strs, valid, n_blocks=2):
    """encode one VARCHAR payload column of a perfect table keyed 0 .. n - 1 and read the codes back through a join that keeps
    every build row -> (n_codes, has_null, dictionary, codes by build row)"""
    n = len(strs)
    cells, heap = string_blocks(strs, valid, n_blocks, 5)
    ht = capi.HashTable.from_columns(ctx, [np.arange(n, dtype=np.int32)], [cells], payload_valid=[valid])
    ht.set_payload_heaps(0, heap)
    code_col, n_codes, has_null = ht.encode_dictionary(0)
    assert code_col == 1
    words = ht.dictionary(code_col)
    assert ht.finalize_perfect(0, n - 1)
    pk = np.arange(n, dtype=np.int32)
    pipe = capi.Pipeline(ctx, [pk], n, [(ht, [(-1, 0)])], [[0]])
    out = capi.Output(pipe, 1024, n // 1024 + 1 + MAX_WAVE_CHUNKS)
    pipe.probe_rounds([(0, n, 0, 1)], out=out)
    ids = out.fetch_ids()
    got, ok = out.materialize(0, code_col, np.uint32)
    assert len(ids) == n and ok.all()
    codes = np.full(n, -1, np.int64)
    codes[ids[:, 1]] = got  # (build id of a perfect table keyed 0 .. n - 1 = build row)
    out.close()
    pipe.close()
    ht.close()
    return n_codes, has_null, words, codes


def test_all_distinct(gpu_ctx):
    """50 000 different strings (tails that differ in the last bytes only): every row a code of its own, in row order"""
    n = 50_000
    strs = distinct_strings(n)
    n_codes, has_null, words, codes = encoded_codes(gpu_ctx, strs, np.ones(n, np.uint8))
    assert (n_codes, has_null) == (n, 0) and words == strs
    assert np.array_equal(codes, np.arange(n))


def test_one_value_on_every_row(gpu_ctx):
    """every lane on one slot: one code; with a second value at the very end: two, in order of appearance"""
    n = 50_000
    hot = b"UNITED STATES MINOR OUTLYING ISLANDS"
    n_codes, has_null, words, codes = encoded_codes(gpu_ctx, [hot] * n, np.ones(n, np.uint8))
    assert (n_codes, has_null, words) == (1, 0, [hot]) and not codes.any()
    n_codes, has_null, words, codes = encoded_codes(gpu_ctx, [hot] * (n - 1) + [hot[:-1]], np.ones(n, np.uint8))
    assert (n_codes, has_null, words) == (2, 0, [hot, hot[:-1]])
    assert not codes[:-1].any() and codes[-1] == 1


def test_all_null_and_the_empty_table(gpu_ctx):
    n = 5000
    n_codes, has_null, words, codes = encoded_codes(gpu_ctx, [b"never read"] * n, np.zeros(n, np.uint8))
    assert (n_codes, has_null, words) == (0, 1, []) and not codes.any()
    cells, heap = string_blocks([], np.zeros(0, np.uint8), 1)
    ht = capi.HashTable.from_columns(gpu_ctx, [np.zeros(0, np.int32)], [cells])
    assert ht.encode_dictionary(0) == (1, 0, 0)
    assert ht.dictionary(1) == []
    ht.finalize_hash()
    assert ht.info()["n_rows"] == 0
    ht.close()


# ---- 6. the contract -----------------------------------------------------------------------------------------------------------
def refused(call, *args):
    with pytest.raises(capi.PolrError) as e:
        call(*args)
    return e.value.code


def raw_fetch(ht, code_col, n_offsets, str_cap):
    """polr_ht_fetch_dictionary as the C ABI has it, into sentinel-filled buffers -> (rc, str_used, offsets, arena)"""
    offs = np.full(max(n_offsets, 1), 0xABABABABABABABAB, np.uint64)
    arena = np.full(max(str_cap, 1), 0xEE, np.uint8)
    used = C.c_uint64()
    rc = ht.ctx.L.polr_ht_fetch_dictionary(ht.h, code_col, None, offs.ctypes.data, n_offsets, arena.ctypes.data, str_cap, C.byref(used))
    return rc, used.value, offs, arena


@pytest.mark.parametrize("engine", ["path", "flat"])
def test_refusals_leave_the_table_as_it_was(gpu_ctx, engine):
    """every refusal returns its code and appends nothing: the next successful call still returns code_col = the number of
    payload columns uploaded, and info() is unchanged; after "the heap never came", setting the heap and encoding succeeds"""
    b = DictBank(gpu_ctx, engine, seed=730, heaps=False)
    info = b.ht.info()
    assert any(ok and len(s) > 12 for s, ok in zip(b.cols["b_s"], b.valid["b_s"]))
    assert refused(b.ht.encode_dictionary, 0) == capi.E_INVALID                    # long cells, the heap never came
    assert refused(b.ht.encode_dictionary, b.col("b_i")[1]) == capi.E_INVALID      # not a VARCHAR column
    assert refused(b.ht.encode_dictionary, DictBank.N_PAYLOAD) == capi.E_INVALID   # no such column
    assert refused(b.ht.dictionary, 0) == capi.E_INVALID                           # never encoded
    assert b.ht.info() == info
    b.set_heaps()
    words, codes = py_dictionary(b.cols["b_s"], b.valid["b_s"])
    assert b.ht.encode_dictionary(0) == (DictBank.N_PAYLOAD, len(words), 1)
    assert refused(b.ht.encode_dictionary, 0) == capi.E_INVALID                    # encoded already
    assert refused(b.ht.encode_dictionary, DictBank.N_PAYLOAD) == capi.E_INVALID   # a code column is not a VARCHAR column
    assert refused(b.ht.dictionary, 0) == capi.E_INVALID and refused(b.ht.dictionary, 1) == capi.E_INVALID  # not code columns
    b.finalize()
    assert refused(b.ht.encode_dictionary, 1) == capi.E_INVALID                    # finalized
    assert b.ht.dictionary(DictBank.N_PAYLOAD) == words
    assert refused(b.ht.dictionary, DictBank.N_PAYLOAD + 1) == capi.E_INVALID      # nothing was appended by the refusals
    b.close()
    # an all-inline column needs no heap
    short = [s[:12] for s in b.cols["b_s"]]
    b = DictBank(gpu_ctx, engine, seed=730, heaps=False, b_strs=short)
    assert b.ht.encode_dictionary(0) == (DictBank.N_PAYLOAD, len(py_dictionary(short, b.valid["b_s"])[0]), 1)
    assert b.ht.dictionary(DictBank.N_PAYLOAD) == py_dictionary(short, b.valid["b_s"])[0]
    b.close()


def test_fetch_capacity_contract(gpu_ctx):
    """str_cap one byte short, or one offset short: POLR_E_OVERFLOW with *str_used exact and nothing written; the retry with
    *str_used succeeds"""
    b = DictBank(gpu_ctx, "path", seed=740)
    words, _ = py_dictionary(b.cols["b_s"], b.valid["b_s"])
    code_col, n_codes, _ = b.ht.encode_dictionary(0)
    need = sum(4 + len(w) for w in words)
    for n_offsets, cap in ((n_codes, need - 1), (n_codes - 1, need), (0, 0)):
        rc, used, offs, arena = raw_fetch(b.ht, code_col, n_offsets, cap)
        assert rc == capi.E_OVERFLOW and used == need
        assert (offs == 0xABABABABABABABAB).all() and (arena == 0xEE).all()  # nothing half-written
    rc, used, offs, arena = raw_fetch(b.ht, code_col, n_codes + 3, used + 5)
    assert rc == capi.OK and used == need
    assert (offs[n_codes:] == 0xABABABABABABABAB).all() and (arena[need:] == 0xEE).all()
    raw, at = arena.tobytes(), 0
    for c, w in enumerate(words):  # records {u32 length, bytes}, code after code
        assert int(offs[c]) == at and int.from_bytes(raw[at:at + 4], "little") == len(w) and raw[at + 4:at + 4 + len(w)] == w
        at += 4 + len(w)
    b.close()


@pytest.mark.parametrize("engine", ["path", "flat"])
def test_the_code_column_travels_as_an_ordinary_payload_column(gpu_ctx, engine):
    """polr_ht_export of an encoded, finalized table: its buffers are at least 4 bytes per slot of the code column larger than
    those of the same table without the encoding; a table made from its metadata carries the codes but not the strings"""
    plain = DictBank(gpu_ctx, engine, seed=750)
    enc = DictBank(gpu_ctx, engine, seed=750)
    code_col, _n, _h = enc.ht.encode_dictionary(0)
    plain.finalize()
    enc.finalize()
    slots = enc.ht.info()["capacity"] if engine == "flat" else enc.nb
    meta, bufs = enc.ht.export()
    _meta0, bufs0 = plain.ht.export()
    assert sum(s for _p, s in bufs) >= sum(s for _p, s in bufs0) + 4 * slots
    assert len(bufs) > len(bufs0)
    like = capi.HashTable.alloc_like(gpu_ctx, meta)
    assert like.info()["kind"] == enc.ht.info()["kind"]
    assert len(like.export()[1]) == len(bufs)
    assert refused(like.dictionary, code_col) == capi.E_INVALID
    like.close()
    plain.close()
    enc.close()


def test_a_table_is_never_given_more_columns_than_export_carries(gpu_ctx):
    """polr_ht_export describes at most 62 payload columns: the 62nd column may be a code column, a 63rd is refused with the
    table untouched"""
    strs = [b"a", b"b" * 20, b"a", b"c"]
    cells, heap = string_blocks(strs, np.ones(4, np.uint8), 1)
    for n_int, ok in ((60, True), (61, False)):
        ht = capi.HashTable.from_columns(gpu_ctx, [np.arange(4, dtype=np.int32)], [cells] + [np.arange(4, dtype=np.uint8)] * n_int)
        ht.set_payload_heaps(0, heap)
        if ok:
            assert ht.encode_dictionary(0) == (61, 3, 0)
            assert ht.dictionary(61) == [b"a", b"b" * 20, b"c"]
        else:
            assert refused(ht.encode_dictionary, 0) == capi.E_UNSUPPORTED
            assert refused(ht.dictionary, 62) == capi.E_INVALID
        ht.finalize_hash()
        assert len(ht.export()[1]) >= 61
        ht.close()


# ---- 7. nothing else moved -----------------------------------------------------------------------------------------------------
def test_a_table_that_was_never_encoded_has_no_extra_column(gpu_ctx):
    b = DictBank(gpu_ctx, "path", seed=760).finish()
    assert b.out._col_width(0, DictBank.N_PAYLOAD - 1) == 4
    assert refused(b.out._col_width, 0, DictBank.N_PAYLOAD) == capi.E_INVALID
    b.close()
