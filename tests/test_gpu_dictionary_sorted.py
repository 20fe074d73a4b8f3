"""Order-preserving dictionary codes (polr_ht_encode_dictionary_ex with POLR_DICT_SORTED / POLR_DICT_NULL_INVALID,
polr_ht_fetch_dictionary_codes; HashTable.encode_dictionary(sorted=, null_invalid=) / .dictionary_strings) and the sinks over
them.  The reference of every comparison is Python over the inputs -- sorted() / min() / max() on bytes, the numpy join of
tests/joinref.py, the reference-run fixture for Q4.1 -- never a second call of the library.  Columns are made as in
test_gpu_dictionary.DictBank: 8 % NULL rows whose cells hold garbage, dirty inline padding, heap in three blocks; every
value occurs 1 to 3 times, in shuffled rows."""
import ctypes as C
import gc

import numpy as np
import pytest

import common
import scanstr
import strref
from buildside import clone
from joinref import device_rows
from polr_amd import capi
from test_gpu_dictionary import G_MIN, G_N, DictBank, py_dictionary
from test_gpu_group_varchar import EDGES, dirty_padding, distinct_strings
from test_gpu_sink_matrix import MAX_WAVE_CHUNKS, string_blocks

pytestmark = pytest.mark.gpu

ENGINES = ["path", "generic", "flat"]
SORTED, NULL_INVALID = capi.DICT_SORTED, capi.DICT_NULL_INVALID
TILE = 1024  # POLR_DICT_SORT_TILE of polr_dict.hip: inside 64 .. 4096, so the sizes below straddle it and its multiples
SIZES = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 6149, 20497, 40000]
PREFIX_K = (3, 7, 8, 11, 12, 13, 40)
ALL_EDGES = list(dict.fromkeys(EDGES + scanstr.EDGES))


def live_bytes():
    gc.collect()
    return capi.device_bytes_live()


def download(ptr, nbytes):
    """device memory -> uint8 array"""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = np.zeros(nbytes, np.uint8)
    assert hip.hipMemcpy(out.ctypes.data, ptr, nbytes, 2) == 0
    return out


def refused(call, *args, **kw):
    with pytest.raises(capi.PolrError) as e:
        call(*args, **kw)
    return e.value.code


def mixed_values(d):
    """d different strings of three kinds: the edge sets, the shared-prefix family b"P" * k + b"%07d" % i (differences inside
    bytes 4..7 of long cells, behind the 8-byte key, across the 12 / 13 inline boundary), distinct_strings"""
    out = ALL_EDGES[:d]
    n_family = (d - len(out)) // 2
    out = out + [b"P" * PREFIX_K[i % len(PREFIX_K)] + b"%07d" % (i // len(PREFIX_K)) for i in range(n_family)]
    out = out + distinct_strings(d - len(out))
    assert len(out) == d == len(set(out))
    return out


def make_rows(values, seed, n_null=None):
    """every value 1 to 3 times and 8 % NULL rows (at least one), shuffled -> (string per row, validity per row)"""
    rng = np.random.default_rng(seed)
    rows = [v for v, k in zip(values, rng.integers(1, 4, len(values)).tolist()) for _ in range(k)]
    if n_null is None:
        n_null = max(1, len(rows) * 8 // 92)
    strs = rows + [b"never read"] * n_null
    valid = np.array([1] * len(rows) + [0] * n_null, np.uint8)
    order = rng.permutation(len(strs))
    return [strs[i] for i in order.tolist()], valid[order]


def encoded(ctx, strs, valid, seed=5, **flags):
    """encode one VARCHAR payload column of a perfect table keyed 0 .. n - 1 and read the codes back through a join that keeps
    every build row -> (n_codes, has_null, dictionary, codes by build row, validity by build row)"""
    n = len(strs)
    cells, heap = string_blocks(strs, valid, 3, seed)
    dirty_padding(cells, strs, valid, np.random.default_rng(seed + 1))
    ht = capi.HashTable.from_columns(ctx, [np.arange(n, dtype=np.int32)], [cells], payload_valid=[valid])
    ht.set_payload_heaps(0, heap)
    code_col, n_codes, has_null = ht.encode_dictionary(0, **flags)
    assert code_col == 1
    words = ht.dictionary(code_col)
    assert ht.finalize_perfect(0, n - 1)
    pk = np.arange(n, dtype=np.int32)
    pipe = capi.Pipeline(ctx, [pk], n, [(ht, [(-1, 0)])], [[0]])
    out = capi.Output(pipe, 1024, n // 1024 + 1 + MAX_WAVE_CHUNKS)
    pipe.probe_rounds([(0, n, 0, 1)], out=out)
    ids = out.fetch_ids()
    got, ok = out.materialize(0, code_col, np.uint32)
    assert len(ids) == n
    codes = np.full(n, -1, np.int64)
    codes[ids[:, 1]] = got  # (build id of a perfect table keyed 0 .. n - 1 = build row)
    okrow = np.zeros(n, np.uint8)
    okrow[ids[:, 1]] = ok
    out.close()
    pipe.close()
    ht.close()
    return n_codes, has_null, words, codes, okrow


def check_sorted(values, strs, valid, n_codes, has_null, words, codes):
    want = sorted(values)
    assert (n_codes, has_null) == (len(want), int(not valid.all()))
    assert words == want
    index = {w: i for i, w in enumerate(want)}
    assert codes.tolist() == [index[s] if ok else len(want) for s, ok in zip(strs, valid.tolist())]


# ---- 1. the order at the sizes where the sort can go wrong ---------------------------------------------------------------------
@pytest.mark.parametrize("d", SIZES)
def test_codes_rise_with_the_strings(gpu_ctx, d):
    """d distinct non-NULL values: the dictionary is sorted(values), the code of every build row is the index of its string
    in that list (NULL rows: n_codes), the counts are exact"""
    before = live_bytes()
    values = mixed_values(d)
    strs, valid = make_rows(values, 100 + d, n_null=5 if d == 0 else None)
    n_codes, has_null, words, codes, ok = encoded(gpu_ctx, strs, valid, sorted=True)
    check_sorted(values, strs, valid, n_codes, has_null, words, codes)
    assert ok.all()  # (no NULL_INVALID: no validity array)
    assert live_bytes() == before


# ---- 2. prefix chains --------------------------------------------------------------------------------------------------------------
def test_prefix_chains(gpu_ctx):
    """b"\\0" * i and b"a" * i for i in 0 .. 20, each also with a trailing \\x00, \\x7f, \\x80, \\xff: every neighbouring pair of
    the sorted result differs by length only or in the last byte only"""
    values = list(dict.fromkeys(b * i + t for b in (b"\0", b"a") for i in range(21) for t in (b"", b"\x00", b"\x7f", b"\x80", b"\xff")))
    strs, valid = make_rows(values, 200)
    n_codes, has_null, words, codes, _ok = encoded(gpu_ctx, strs, valid, sorted=True)
    check_sorted(values, strs, valid, n_codes, has_null, words, codes)
    for a, b in zip(words, words[1:]):
        assert a < b


# ---- 3. the order of the rows plays no part --------------------------------------------------------------------------------------
def test_row_order_plays_no_part(gpu_ctx):
    values = mixed_values(3000)
    strs, valid = make_rows(values, 300)
    perm = np.random.default_rng(301).permutation(len(strs))
    strs2, valid2 = [strs[i] for i in perm.tolist()], valid[perm]
    a = encoded(gpu_ctx, strs, valid, seed=5, sorted=True)
    b = encoded(gpu_ctx, strs2, valid2, seed=9, sorted=True)  # (another heap layout and padding too)
    assert a[:3] == b[:3] == (len(values), 1, sorted(values))
    assert a[3][perm].tolist() == b[3].tolist()
    check_sorted(values, strs2, valid2, *b[:4])
    # first-appearance codes do depend on it: that is what the flag changes
    c = encoded(gpu_ctx, strs, valid)
    assert c[2] == py_dictionary(strs, valid)[0] != a[2]


# ---- 4. flags and refusals -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ["path", "flat"])
def test_flags_and_refusals(gpu_ctx, engine):
    """flags = 0 is the first-appearance call; an unknown bit is refused; every refusal of polr_ht_encode_dictionary is a
    refusal with SORTED too, the table as it was (payload count, info, device bytes); a corrected call succeeds"""
    b = DictBank(gpu_ctx, engine, seed=800, heaps=False)
    info = b.ht.info()
    words0, codes0 = py_dictionary(b.cols["b_s"], b.valid["b_s"])
    live = live_bytes()
    assert any(ok and len(s) > 12 for s, ok in zip(b.cols["b_s"], b.valid["b_s"]))
    assert refused(b.ht.encode_dictionary, 0, sorted=True) == capi.E_INVALID                  # long cells, the heap never came
    assert refused(b.ht.encode_dictionary, b.col("b_i")[1], sorted=True) == capi.E_INVALID    # a width-4 column
    assert refused(b.ht.encode_dictionary, DictBank.N_PAYLOAD, sorted=True) == capi.E_INVALID  # no such column
    b.set_heaps()
    live = live_bytes()
    for bad in (4, 8, 1 << 31, 7, 0xFFFFFFFF):
        assert refused(b.ht.encode_dictionary, 0, flags=bad) == capi.E_INVALID                # an unknown bit
    assert b.ht.info() == info and live_bytes() == live
    # flags = 0 through the new entry point: first appearance, bit for bit what the old call documents
    col, n, null = C.c_uint32(), C.c_uint32(), C.c_uint32()
    b.ctx.check(b.ctx.L.polr_ht_encode_dictionary_ex(b.ht.h, 0, 0, None, C.byref(col), C.byref(n), C.byref(null)))
    assert (col.value, n.value, null.value) == (DictBank.N_PAYLOAD, len(words0), 1)  # (nothing was appended by the refusals)
    b.ht._n_codes = {col.value: n.value}
    assert b.ht.dictionary(col.value) == words0
    info1, live = b.ht.info(), live_bytes()
    assert refused(b.ht.encode_dictionary, 0, sorted=True) == capi.E_INVALID                  # encoded already, by the other call
    assert refused(b.ht.encode_dictionary, 0) == capi.E_INVALID
    assert b.ht.info() == info1 and live_bytes() == live
    w2 = sorted(set(s for s, ok in zip(b.cols["b_s2"], b.valid["b_s2"]) if ok))
    assert b.ht.encode_dictionary(1, sorted=True) == (DictBank.N_PAYLOAD + 1, len(w2), 1)     # the corrected call
    assert b.ht.dictionary(DictBank.N_PAYLOAD + 1) == w2
    assert refused(b.ht.encode_dictionary, 1) == capi.E_INVALID                               # encoded already, by the new call
    assert refused(b.ht.encode_dictionary, 1, sorted=True) == capi.E_INVALID
    b.finish()
    got, ok = b.out.materialize(0, DictBank.N_PAYLOAD, np.uint32)
    assert got.tolist() == [codes0[r] for r in b.dev_rows[:, 1].tolist()] and ok.all()
    b.close()
    b = DictBank(gpu_ctx, engine, seed=800)
    b.finalize()
    info = b.ht.info()
    assert refused(b.ht.encode_dictionary, 0, sorted=True) == capi.E_INVALID                  # finalized
    assert refused(b.ht.encode_dictionary, 0, null_invalid=True) == capi.E_INVALID
    assert b.ht.info() == info
    b.close()


# ---- 5. NULL_INVALID -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("flags", [NULL_INVALID, SORTED | NULL_INVALID, SORTED, 0])
def test_null_invalid_gives_the_code_column_the_validity_of_its_source(gpu_ctx, engine, flags):
    b = DictBank(gpu_ctx, engine, seed=810)
    if flags & SORTED:
        words = sorted(set(s for s, ok in zip(b.cols["b_s"], b.valid["b_s"]) if ok))
        codes = [words.index(s) if ok else len(words) for s, ok in zip(b.cols["b_s"], b.valid["b_s"])]
    else:
        words, codes = py_dictionary(b.cols["b_s"], b.valid["b_s"])
    before = b.ht.info()["device_bytes"]
    code_col, n_codes, has_null = b.ht.encode_dictionary(0, flags=flags)
    assert (code_col, n_codes, has_null) == (DictBank.N_PAYLOAD, len(words), 1)
    grown = b.ht.info()["device_bytes"] - before
    assert grown == 4 * b.nb + 16 * n_codes + (b.nb if flags & NULL_INVALID else 0)  # (the copy is counted)
    assert b.ht.encode_dictionary(b.col("b_s2")[1], flags=flags)[0] == DictBank.N_PAYLOAD + 1  # (a second code column)
    b.finish()
    assert b.ht.dictionary(code_col) == words
    assert b.out._col_width(0, code_col) == 4
    if engine != "flat":  # the column as the table holds it, in build-row order: the cell of a NULL row is still n_codes
        data = b.ht.export()[1][-4 if flags & NULL_INVALID else -2]  # (.. codes [validity], codes of b_s2 [validity])
        assert data[1] == 4 * b.nb and download(data[0], data[1]).view(np.uint32).tolist() == codes
    got, ok = b.out.materialize(0, code_col, np.uint32)
    rows = b.dev_rows[:, 1]
    if flags & NULL_INVALID:  # (polr_out_materialize writes a NULL cell as zero, whatever the column)
        assert np.array_equal(ok, b.valid["b_s"][rows]) and not ok.all()
        assert got.tolist() == [codes[r] if b.valid["b_s"][r] else 0 for r in rows.tolist()]
    else:
        assert ok.all()
        assert got.tolist() == [codes[r] for r in rows.tolist()]
    b.close()


def test_a_column_without_validity_gets_none(gpu_ctx):
    strs = [b"b", b"a" * 20, b"b", b"c", b""]
    cells, heap = string_blocks(strs, np.ones(5, np.uint8), 1)
    n_buffers = []
    for null_invalid in (False, True):
        ht = capi.HashTable.from_columns(gpu_ctx, [np.arange(5, dtype=np.int32)], [cells])
        ht.set_payload_heaps(0, heap)
        before = ht.info()["device_bytes"]
        assert ht.encode_dictionary(0, sorted=True, null_invalid=null_invalid) == (1, 4, 0)
        assert ht.info()["device_bytes"] - before == 4 * 5 + 16 * 4
        assert ht.dictionary(1) == [b"", b"a" * 20, b"b", b"c"]
        ht.finalize_hash()
        n_buffers.append(len(ht.export()[1]))
        ht.close()
    assert n_buffers[0] == n_buffers[1]  # (no validity buffer either way)


# ---- 6. the sinks over sorted codes ----------------------------------------------------------------------------------------------
def sink_bank(ctx, engine, seed):
    """a DictBank whose b_s is NULL on every build row of group G_MIN + 2, encoded SORTED | NULL_INVALID"""
    probe = DictBank(ctx, engine, seed)
    b_valid = (probe.valid["b_s"].astype(bool) & (probe.cols["b_g"] != G_MIN + 2)).astype(np.uint8)
    probe.close()
    b = DictBank(ctx, engine, seed, b_valid=b_valid)
    assert np.array_equal(b.cols["b_g"], probe.cols["b_g"])
    words = sorted(set(s for s, ok in zip(b.cols["b_s"], b_valid) if ok))
    code_col, n_codes, has_null = b.ht.encode_dictionary(0, sorted=True, null_invalid=True)
    assert (code_col, n_codes, has_null) == (DictBank.N_PAYLOAD, len(words), 1)
    return b, words, code_col


def py_min_max(values, valid, groups=None):
    """{group: (min, max) of the non-NULL bytes, None when there is none}"""
    members = {}
    for i, (v, ok) in enumerate(zip(values, valid)):
        g = None if groups is None else groups[i]
        members.setdefault(g, [])
        if ok:
            members[g].append(v)
    return {g: (min(v), max(v)) if v else (None, None) for g, v in members.items()}


def grouped_min_max_by_g(b, ht, out, code_col):
    """MIN / MAX of the code column per b_g through the perfect-hash sink, mapped back to strings"""
    vals, _counts, dropped = out.aggregate_grouped([(0, b.col("b_g")[1], G_MIN, G_N)], [("min", 0, code_col), ("max", 0, code_col)])
    assert dropped == 0
    flat = [c for v in vals for c in v if c is not None]
    strings = iter(ht.dictionary_strings(code_col, flat, str_cap=16))
    return vals, {G_MIN + g: tuple(None if c is None else next(strings) for c in v) for g, v in enumerate(vals)}


@pytest.mark.parametrize("engine", ENGINES)
def test_min_max_of_a_varchar_through_the_integer_sinks(gpu_ctx, engine):
    b, words, code_col = sink_bank(gpu_ctx, engine, 820 + ENGINES.index(engine))
    b.finish()
    s, s_ok = b.column("b_s")
    # ungrouped
    lo, hi = py_min_max(s, s_ok)[None]
    got = b.out.aggregate([("min", 0, code_col), ("max", 0, code_col), ("count", 0, code_col)])
    assert (words[got[0]], words[got[1]]) == (lo, hi) and got[2] == sum(s_ok)
    assert b.ht.dictionary_strings(code_col, got[:2]) == [lo, hi]
    assert (b.out.aggregate_string("min", 0, b.col("b_s")[1]), b.out.aggregate_string("max", 0, b.col("b_s")[1])) == (lo, hi)
    # grouped by b_g (perfect-hash sink)
    g, _ = b.column("b_g")
    want = py_min_max(s, s_ok, g)
    assert want[G_MIN + 2] == (None, None) and len(want) == G_N
    vals, got_g = grouped_min_max_by_g(b, b.ht, b.out, code_col)
    assert got_g == want
    assert vals[2] == [None, None]  # (a group whose rows are all NULL)
    # grouped by p_i (hash sink; NULL is a group of its own)
    p, p_ok = b.column("p_i")
    want = py_min_max(s, s_ok, [v if ok else None for v, ok in zip(p, p_ok)])
    hashed = b.out.aggregate_hashed([b.col("p_i")], [("min", 0, code_col), ("max", 0, code_col)], 1024)
    flat = [c for v in hashed.values() for c in v if c is not None]
    strings = iter(b.ht.dictionary_strings(code_col, flat))
    assert {k[0]: tuple(None if c is None else next(strings) for c in v) for k, v in hashed.items()} == want
    assert None in want
    # the code column as a group key: the perfect-hash sink drops the NULL-key rows, the hash sink makes them a group
    _vals, _counts, dropped = b.out.aggregate_grouped([(0, code_col, 0, len(words))], [("count_star", -1, 0)])
    assert dropped == len(s_ok) - sum(s_ok) > 0
    by_code = b.out.aggregate_hashed([(0, code_col)], [("count_star", -1, 0)], 1024)
    assert by_code[(None,)] == [dropped] and len(by_code) == len(set(v for v, ok in zip(s, s_ok) if ok)) + 1
    b.close()


# ---- 7. ORDER BY against the reference -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", ["rows", "rows_nulls"])
def test_q41_group_index_order_is_the_order_by_of_the_reference(gpu_ctx, run):
    """the fused run of test_q41_with_varchar_nation_fused_against_the_reference with c_nation_name encoded SORTED: the
    result array read in index order (per year the NULL group moved from the back to the front: the reference sorts NULLS
    FIRST) IS the reference's ORDER BY d_year, c_nation answer, order included"""
    from polr_amd import ssb_skew
    gold = common.load_golden("ssb_q41_varchar")
    want = [(r[0], None if r[1] is None else r[1].encode(), r[2]) for r in gold[run]]
    names_in_gold = [w for _y, w, _v in want if w is not None]
    assert {b"UNITED ST", b"UNITED STATES", b"UNITED STATES MINOR OUTLYING ISLANDS"} <= set(names_in_gold)
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
        valid = strref.nation_valid(cust["keys"][0])
        cust["strings_valid"] = {"c_nation_name": valid}
    cust["dictionary"] = ["c_nation_name"]
    cust["dictionary_flags"] = {"c_nation_name": SORTED}
    joins = capi.build_joins(gpu_ctx, wl, auto=True)
    code_col, (n_codes, has_null) = capi.dictionary_payload_index(cust, "c_nation_name")
    words = sorted(set(s for s, ok in zip(cust["strings"]["c_nation_name"], valid) if ok))
    assert (n_codes, has_null) == (len(words), int(run == "rows_nulls")) and joins[0][0].dictionary(code_col) == words
    paths = np.asarray(common.load_golden("ssb_skew_sample")["cases"]["q4.1/3"]["paths"], dtype=np.int32)
    pipe = capi.Pipeline(gpu_ctx, cols, n, joins, paths)
    assert pipe.launch_info(True)["flat"] == 1
    years = sorted({y for y, _c, _v in want})
    y0, ny = years[0], years[-1] - years[0] + 1
    nv = n_codes + has_null
    specs = [("count_star", -1, 0), ("sum", -1, names.index("lo_revenue")), ("sum", -1, names.index("lo_supplycost"))]
    out = capi.Output(pipe, 1024, 64)
    out.fuse_grouped([(3, 0, y0, ny), (0, code_col, 0, nv)], specs)
    mpx = capi.DeviceMultiplexer(pipe, "adaptive_reinit")
    capi.run_resident([mpx], [(0, (n + 1023) // 1024)], out=out, reset=True, finish=True)
    capi.finish_many([mpx])
    vals, _counts, dropped = out.fused_result()
    assert dropped == 0 and len(vals) == ny * nv
    got = []
    for y in range(ny):
        year = vals[y * nv:(y + 1) * nv]
        order = ([n_codes] if has_null else []) + list(range(n_codes))  # NULL (the largest code) first
        got += [(y0 + y, words[c] if c < n_codes else None, year[c][1] - year[c][2]) for c in order if year[c][0]]
    assert got == want
    mpx.close()
    out.close()
    pipe.close()
    for h, _ in joins:
        h.close()


# ---- 8. polr_ht_fetch_dictionary_codes ---------------------------------------------------------------------------------------------
def raw_fetch_codes(ht, code_col, codes, str_cap):
    """polr_ht_fetch_dictionary_codes as the C ABI has it, into sentinel-filled buffers -> (rc, str_used, offsets, arena)"""
    codes = np.ascontiguousarray(codes, np.uint32)
    offs = np.full(max(len(codes), 1), 0xABABABABABABABAB, np.uint64)
    arena = np.full(max(str_cap, 1), 0xEE, np.uint8)
    used = C.c_uint64(77)
    rc = ht.ctx.L.polr_ht_fetch_dictionary_codes(ht.h, code_col, None, codes.ctypes.data, len(codes), offs.ctypes.data,
                                                 arena.ctypes.data, str_cap, C.byref(used))
    return rc, used.value, offs, arena


def test_fetch_listed_codes_and_a_cloned_table(gpu_ctx):
    b, words, code_col = sink_bank(gpu_ctx, "path", 830)
    n_codes = len(words)
    rng = np.random.default_rng(831)
    listed = rng.integers(0, n_codes, 50).tolist() + [n_codes - 1, 0, 0, n_codes - 1]  # duplicates, any order
    need = sum(4 + len(words[c]) for c in listed)
    for cap in (need - 1, 0):
        rc, used, offs, arena = raw_fetch_codes(b.ht, code_col, listed, cap)
        assert rc == capi.E_OVERFLOW and used == need
        assert (offs == 0xABABABABABABABAB).all() and (arena == 0xEE).all()  # nothing half-written
    rc, used, offs, arena = raw_fetch_codes(b.ht, code_col, listed, need + 5)
    assert rc == capi.OK and used == need and (arena[need:] == 0xEE).all()
    raw, at = arena.tobytes(), 0
    for i, c in enumerate(listed):  # records {u32 length, bytes}, in list order
        w = words[c]
        assert int(offs[i]) == at and int.from_bytes(raw[at:at + 4], "little") == len(w) and raw[at + 4:at + 4 + len(w)] == w
        at += 4 + len(w)
    assert b.ht.dictionary_strings(code_col, listed, str_cap=1) == [words[c] for c in listed]  # (the binding's one retry)
    assert raw_fetch_codes(b.ht, code_col, [], 0)[:2] == (capi.OK, 0) and b.ht.dictionary_strings(code_col, []) == []
    for bad in ([n_codes], [0, 1, n_codes, 2], [0xFFFFFFFF]):  # the NULL code is not a string
        rc, used, offs, arena = raw_fetch_codes(b.ht, code_col, bad, 4096)
        assert rc == capi.E_INVALID and used == 77 and (offs == 0xABABABABABABABAB).all() and (arena == 0xEE).all()
    assert refused(b.ht.dictionary_strings, 0, [0]) == capi.E_INVALID  # not a code column
    b.finish()
    assert b.ht.dictionary_strings(code_col, listed) == [words[c] for c in listed]  # (finalizing keeps the dictionary)
    vals, got_g = grouped_min_max_by_g(b, b.ht, b.out, code_col)
    s, s_ok = b.column("b_s")
    assert got_g == py_min_max(s, s_ok, b.column("b_g")[0])
    # a table made from the export: the codes and their validity, not the strings
    twin = clone(gpu_ctx, b.ht)
    assert refused(twin.dictionary_strings, code_col, [0]) == capi.E_INVALID
    assert refused(twin.dictionary, code_col) == capi.E_INVALID
    pipe = capi.Pipeline(gpu_ctx, [b.pk, b.cols["p_i"], b.cols["p_big"]], b.n, [(twin, [(-1, 0)])], [[0]],
                         probe_valid=[None] + [b.valid[c] for c in ("p_i", "p_big")])
    out = capi.Output(pipe, b.cap, len(b.rows) // b.cap + 1 + MAX_WAVE_CHUNKS)
    pipe.probe_rounds([(0, b.n, 0, 1)], out=out)
    rows = device_rows(out.fetch_ids(), [b.join])[:, 1]
    got, ok = out.materialize(0, code_col, np.uint32)
    index = {w: i for i, w in enumerate(words)}
    assert np.array_equal(ok, b.valid["b_s"][rows]) and not ok.all()  # (the validity array is carried)
    assert got.tolist() == [index[b.cols["b_s"][r]] if b.valid["b_s"][r] else 0 for r in rows.tolist()]  # (NULL cells: zero)
    twin_vals, _c, _d = out.aggregate_grouped([(0, b.col("b_g")[1], G_MIN, G_N)], [("min", 0, code_col), ("max", 0, code_col)])
    assert twin_vals == vals
    out.close()
    pipe.close()
    twin.close()
    b.close()


# ---- 9. nothing leaks --------------------------------------------------------------------------------------------------------------
def test_nothing_leaks(gpu_ctx):
    """the sort's scratch is gone when the call returns: what stays is the code column, its validity copy and one cell per
    code; closing every handle returns to the count before the test"""
    before = live_bytes()
    values = mixed_values(3 * TILE + 5)
    strs, valid = make_rows(values, 900)
    n = len(strs)
    cells, heap = string_blocks(strs, valid, 3, 5)
    ht = capi.HashTable.from_columns(gpu_ctx, [np.arange(n, dtype=np.int32)], [cells], payload_valid=[valid])
    ht.set_payload_heaps(0, heap)
    uploaded = live_bytes()
    assert refused(ht.encode_dictionary, 0, flags=SORTED | 4) == capi.E_INVALID
    assert refused(ht.encode_dictionary, 1, sorted=True) == capi.E_INVALID
    assert live_bytes() == uploaded
    assert ht.encode_dictionary(0, sorted=True, null_invalid=True) == (1, len(values), 1)
    assert live_bytes() == uploaded + 4 * n + n + 16 * len(values)
    assert ht.dictionary_strings(1, [0, len(values) - 1]) == [min(values), max(values)]
    assert live_bytes() == uploaded + 4 * n + n + 16 * len(values)
    ht.close()
    assert live_bytes() == before
