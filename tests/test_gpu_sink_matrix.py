"""Sink matrix: every entry point that turns emitted row ids into an answer -- the ungrouped aggregate, the perfect-hash and the
general GROUP BY, MIN / MAX over VARCHAR with its string heaps, and materialize -- against exact Python over the numpy join
result (tests/joinref.py), over the row ids of every probe engine.

The reference: aggregates as Python ints (SUM in unbounded precision, NULLs taking no part, SUM / MIN / MAX NULL over no
rows); strings as Python bytes (unsigned bytes, a proper prefix first: the reference's order).  Every case asserts
`launch_info(materialize)["flat"]` of its pipeline, so it records which engine produced the ids it aggregates:

  path     the path kernel (probe_rounds) over a repeated-key hash table (S16) and a perfect table
  generic  the generic pool (run_resident) over the same tables
  flat     the emitting flat pool (run_resident) over two perfect tables
"""
import ctypes as C

import numpy as np
import pytest

from joinref import Join, Ref, device_rows, sort_rows
from polr_amd import capi

pytestmark = pytest.mark.gpu

ENGINES = ["path", "generic", "flat"]
INT_TYPES = [np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.int64]
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
MAX_WAVE_CHUNKS = 8192  # one partially filled chunk per emitting wave (polr_out_create)


class DevBuf:
    """device memory from the HIP runtime the library runs on (hipMalloc / hipMemcpy, synchronous)"""
    hip = None

    def __init__(self, nbytes):
        if DevBuf.hip is None:
            DevBuf.hip = C.CDLL("libamdhip64.so")
            DevBuf.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        p = C.c_void_p()
        assert DevBuf.hip.hipMalloc(C.byref(p), C.c_size_t(max(nbytes, 1))) == 0
        self.ptr, self.nbytes = p.value, nbytes

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes == self.nbytes and DevBuf.hip.hipMemcpy(self.ptr, arr.ctypes.data, arr.nbytes, 1) == 0

    def download(self):
        out = np.zeros(self.nbytes, np.uint8)
        assert DevBuf.hip.hipMemcpy(out.ctypes.data, self.ptr, self.nbytes, 2) == 0
        return out

    def free(self):
        assert DevBuf.hip.hipFree(C.c_void_p(self.ptr)) == 0


# ---- one star join run through one engine ---------------------------------------------------------------------------------
def full_range(rng, dt, n):
    """values over the whole domain of dt, its min and max among them"""
    info = np.iinfo(dt)
    v = rng.integers(int(info.min), int(info.max), n, dtype=np.dtype(dt), endpoint=True)
    v[::53] = info.min
    v[7::53] = info.max
    return v


def typed_columns(rng, n, prefix):
    """one full-range column per integer type plus the unsupported kinds, each with ~10 % NULLs"""
    cols = {"%s_%s" % (prefix, np.dtype(dt).name): full_range(rng, dt, n) for dt in INT_TYPES}
    cols[prefix + "_u64"] = full_range(rng, np.uint64, n)
    cols[prefix + "_v16"] = rng.integers(0, 256, (n, 16), dtype=np.uint8).reshape(-1).view("V16")
    valid = {c: (rng.random(n) > 0.1).astype(np.uint8) for c in cols}
    return cols, valid


class Star:
    """probe columns (fk0, fk1, then extra columns) x join 0 (repeated-key hash table, or perfect for `flat`) x join 1
    (perfect); both joins carry the same extra columns as payload.  run(engine, cap) emits the join result."""

    def __init__(self, n=20_000, seed=0, extra=None, flat=False, n_b0=2000):
        rng = np.random.default_rng(seed)
        self.rng = rng
        extra = extra or (lambda r, m, p: typed_columns(r, m, p))
        if flat:
            k0 = np.arange(-n_b0 // 2, n_b0 - n_b0 // 2, dtype=np.int32)
            k0 = rng.permutation(k0[k0 % 13 != 5])
            perfect0 = (int(-(n_b0 // 2)), int(n_b0 - n_b0 // 2 - 1))
        else:
            base = rng.choice(np.arange(-10**6, 10**6, 11, dtype=np.int64), n_b0 // 2, replace=False)
            k0 = rng.permutation(np.repeat(base, 1 + np.arange(len(base)) % 3)[:n_b0]).astype(np.int32)
            perfect0 = None
        k1 = rng.permutation(np.arange(0, 1000, dtype=np.int32)[np.arange(1000) % 17 != 4])
        c0, v0 = extra(rng, len(k0), "b0")
        c1, v1 = extra(rng, len(k1), "b1")
        self.names0, self.names1 = list(c0), list(c1)
        self.joins = [Join(k0, 0, perfect0, None, list(c0.values()), [v0[c] for c in c0]),
                      Join(k1, 1, (0, 999), None, list(c1.values()), [v1[c] for c in c1])]
        fk0 = np.where(rng.random(n) < 0.85, rng.choice(k0, n), rng.integers(-10**6, 10**6, n)).astype(np.int32)
        fk1 = rng.integers(-20, 1020, n).astype(np.int32)
        cp, vp = extra(rng, n, "p")
        self.pnames = ["fk0", "fk1"] + list(cp)
        self.pcols = [fk0, fk1] + list(cp.values())
        self.pvalid = [(rng.random(n) > 0.02).astype(np.uint8), None] + [vp[c] for c in cp]
        self.pipe_cols = None  # (what the pipeline reads instead of pcols: device columns)
        self.flat = flat

    def col(self, name):
        """(src_join, src_col) of a column name"""
        if name in self.pnames:
            return -1, self.pnames.index(name)
        if name in self.names0:
            return 0, self.names0.index(name)
        return 1, self.names1.index(name)

    def run(self, ctx, engine, cap=1024, max_chunks=None):
        assert (engine == "flat") == self.flat
        n = len(self.pcols[0])
        self.ght = [j.device(ctx) for j in self.joins]
        self.pipe = capi.Pipeline(ctx, self.pipe_cols or self.pcols, n, [(h, [(-1, j.src)]) for h, j in zip(self.ght, self.joins)],
                                  [[0, 1]], probe_valid=self.pvalid)
        assert self.pipe.launch_info(True)["flat"] == int(engine == "flat")
        self.rows = sort_rows(Ref(self.pcols, self.pvalid, self.joins).rows())
        self.out = capi.Output(self.pipe, cap, max_chunks or (len(self.rows) + cap - 1) // cap + MAX_WAVE_CHUNKS)
        if engine == "path":
            self.pipe.probe_rounds([(0, n, 0, 1)], out=self.out)
        else:
            m = capi.DeviceMultiplexer(self.pipe, "default_path")
            capi.run_resident([m], [(0, (n + 1023) // 1024)], out=self.out, reset=True, finish=True)
            m.finish()
            m.close()
        n_rows, self.n_chunks, over = self.out.stats()
        assert not over and n_rows == len(self.rows)
        self.ids = self.out.fetch_ids()
        assert np.array_equal(sort_rows(device_rows(self.ids, self.joins)), self.rows)
        return self

    def values(self, sj, sc, rows=None):
        """(values, validity) of column (sj, sc) over the reference rows"""
        rows = self.rows if rows is None else rows
        if sj < 0:
            v = self.pvalid[sc]
            r = rows[:, 0]
            data = self.pcols[sc]
        else:
            j = self.joins[sj]
            v = j.payload_valid[sc]
            r = rows[:, 1 + sj]
            data = j.payload[sc]
        return data[r], (np.ones(len(r), bool) if v is None else v[r].astype(bool))

    def close(self):
        self.out.close()
        self.pipe.close()
        for h in self.ght:
            h.close()


def py_agg(fn, vals, valid):
    """the reference's aggregate over a column: exact Python ints"""
    if fn == "count_star":
        return len(vals)
    v = [int(x) for x, ok in zip(vals.tolist(), valid.tolist()) if ok]
    if fn == "count":
        return len(v)
    if not v:
        return None
    return {"sum": sum, "min": min, "max": max}[fn](v)


# ---- A. the ungrouped aggregate ---------------------------------------------------------------------------------------------
A_SHAPES = [(eng, cap) for eng in ENGINES for cap in (64, 65, 1000, 2048)]


@pytest.mark.parametrize("engine,cap", A_SHAPES, ids=["%s-%d" % s for s in A_SHAPES])
def test_aggregate_every_type_and_source(gpu_ctx, engine, cap):
    """COUNT(*) / COUNT / SUM / MIN / MAX over every integer type at its full range, from the probe row, a hash table's
    payload and a perfect table's re-ordered payload (pcols); 8 aggregates per call with the count field checked; 9 and
    uint64 / 16-byte columns refused"""
    s = Star(seed=10 + A_SHAPES.index((engine, cap)), flat=engine == "flat").run(gpu_ctx, engine, cap)
    if engine != "path":  # pool outputs: many partly filled chunks
        assert s.n_chunks > -(-len(s.rows) // cap)
    for prefix in ("p", "b0", "b1"):
        for dt in INT_TYPES:
            sj, sc = s.col("%s_%s" % (prefix, np.dtype(dt).name))
            vals, valid = s.values(sj, sc)
            specs = [("count_star", -1, 0), ("count", sj, sc), ("sum", sj, sc), ("min", sj, sc), ("max", sj, sc),
                     ("sum", sj, sc), ("count", sj, sc), ("max", sj, sc)]
            got = s.out.aggregate(specs)
            want = [py_agg(fn, vals, valid) for fn, _, _ in specs]
            assert got == want, "%s_%s" % (prefix, np.dtype(dt).name)
        # the count field of every aggregate: rows that took part
        res = (capi.AggValue * 2)()
        spec = (capi.AggSpec * 2)(capi.AggSpec(capi.AGG["count_star"], -1, 0), capi.AggSpec(capi.AGG["min"], sj, sc))
        gpu_ctx.check(gpu_ctx.L.polr_out_aggregate(s.out.h, None, spec, 2, res))
        assert res[0].count == len(vals) and res[1].count == int(valid.sum())
        for bad in ("u64", "v16"):
            with pytest.raises(capi.PolrError) as e:
                s.out.aggregate([("sum", *s.col("%s_%s" % (prefix, bad)))])
            assert e.value.code == capi.E_UNSUPPORTED
    with pytest.raises(capi.PolrError) as e:
        s.out.aggregate([("count_star", -1, 0)] * 9)
    assert e.value.code == capi.E_UNSUPPORTED
    s.close()


def _extreme_columns(rng, n, prefix):
    """int64 columns at the sentinels: runs of INT64_MIN (SUM below -2^64), of INT64_MAX (above 2^64), all zero"""
    lo = np.full(n, I64_MIN, np.int64)
    lo[::5] = rng.integers(-10, 10, len(lo[::5]))
    hi = np.full(n, I64_MAX, np.int64)
    hi[::7] = rng.integers(-10, 10, len(hi[::7]))
    cols = {prefix + "_min": lo, prefix + "_max": hi, prefix + "_zero": np.zeros(n, np.int64),
            prefix + "_only_min": np.full(n, I64_MIN, np.int64), prefix + "_only_max": np.full(n, I64_MAX, np.int64)}
    return cols, {c: (rng.random(n) > 0.05).astype(np.uint8) for c in cols}


@pytest.mark.parametrize("engine", ENGINES)
def test_aggregate_int64_sentinels(gpu_ctx, engine):
    """INT64_MIN / INT64_MAX are the kernel's MIN / MAX init values: MIN returns INT64_MIN and MAX INT64_MAX as values,
    sums leave the 64-bit range on both sides (high limb <= -2 and >= 1), SUM of zeros is 0, not NULL"""
    s = Star(seed=30 + ENGINES.index(engine), extra=_extreme_columns, flat=engine == "flat").run(gpu_ctx, engine)
    for prefix in ("p", "b0", "b1"):
        for c in ("min", "max", "zero", "only_min", "only_max"):
            sj, sc = s.col("%s_%s" % (prefix, c))
            vals, valid = s.values(sj, sc)
            specs = [(fn, sj, sc) for fn in ("count", "sum", "min", "max")]
            got = s.out.aggregate(specs)
            assert got == [py_agg(fn, vals, valid) for fn, _, _ in specs], "%s_%s" % (prefix, c)
            if c == "min":
                assert got[1] < -(1 << 64) and got[2] == I64_MIN
            if c == "max":
                assert got[1] > (1 << 64) and got[3] == I64_MAX
            if c == "zero":
                assert got[1] == 0
    s.close()


NULL_PATTERNS = ["none", "all", "every-other", "first-row", "last-row"]


@pytest.mark.parametrize("engine,pattern", [(e, p) for e in ENGINES for p in NULL_PATTERNS])
def test_aggregate_null_patterns(gpu_ctx, engine, pattern):
    """validity patterns over the output rows, on a device-resident probe column (POLR_COL_DEVICE) whose validity is
    written after the run: none NULL, all NULL (SUM / MIN / MAX NULL, COUNT 0), every other probe row, only the first or only the last
    output row's probe row valid"""
    s = Star(n=12_000, seed=40 + ENGINES.index(engine), flat=engine == "flat")
    n = len(s.pcols[0])
    x = full_range(np.random.default_rng(41), np.int64, n)
    dx, dv = DevBuf(8 * n), DevBuf(n)
    dx.upload(x)
    dv.upload(np.ones(n, np.uint8))
    s.pipe_cols = s.pcols + [capi.dev_col(dx.ptr, 8, True, dv.ptr)]
    s.pcols = s.pcols + [x]  # (the reference reads the host copy)
    s.pvalid = s.pvalid + [None]
    s.run(gpu_ctx, engine, 1000)
    valid = np.ones(n, np.uint8)
    if pattern == "all":
        valid[:] = 0
    elif pattern == "every-other":
        valid[1::2] = 0
    elif pattern in ("first-row", "last-row"):
        valid[:] = 0
        valid[s.ids[0 if pattern == "first-row" else -1, 0]] = 1
    gpu_ctx.sync()
    dv.upload(valid)
    col = len(s.pcols) - 1
    specs = [("count_star", -1, 0)] + [(fn, -1, col) for fn in ("count", "sum", "min", "max")]
    got = s.out.aggregate(specs)
    vals, ok = x[s.rows[:, 0]], valid[s.rows[:, 0]].astype(bool)
    assert got == [len(s.rows)] + [py_agg(fn, vals, ok) for fn, _, _ in specs[1:]]
    if pattern == "all":
        assert got[1:] == [0, None, None, None]
    elif pattern != "none" and pattern != "every-other":
        assert got[1] == int((valid[s.rows[:, 0]]).sum()) >= 1
    s.close()
    dx.free()
    dv.free()


def test_aggregate_empty_one_row_and_many_chunks(gpu_ctx):
    """0 output rows (COUNT 0, SUM / MIN / MAX NULL), 1 output row, and more 64-row chunks than the n_cus x 8 workgroups of
    the grid (the grid-stride loop takes several chunks per workgroup)"""
    rng = np.random.default_rng(50)
    j = Join(np.arange(0, 100, dtype=np.int32), 0, (0, 99), None, [np.arange(100, dtype=np.int64) * -(10**15)])
    ht = j.device(gpu_ctx)
    for n_match in (0, 1):
        pk = np.full(5000, 500, np.int32)
        pk[:n_match] = 42
        x = full_range(rng, np.int16, 5000)
        pipe = capi.Pipeline(gpu_ctx, [pk, x], 5000, [(ht, [(-1, 0)])], [[0]])
        assert pipe.launch_info(True)["flat"] == 1
        out = capi.Output(pipe, 64, 16)
        pipe.probe_rounds([(0, 5000, 0, 1)], out=out)
        got = out.aggregate([("count_star", -1, 0), ("sum", -1, 1), ("min", 0, 0), ("max", -1, 1)])
        assert got == ([0, None, None, None] if n_match == 0 else [1, int(x[0]), -42 * 10**15, int(x[0])])
        out.close()
        pipe.close()
    # many chunks: ~200k rows in 64-row chunks
    n = 200_000
    pk = rng.integers(0, 100, n).astype(np.int32)
    x = full_range(rng, np.int32, n)
    pipe = capi.Pipeline(gpu_ctx, [pk, x], n, [(ht, [(-1, 0)])], [[0]])
    li = pipe.launch_info(True)
    assert li["flat"] == 1
    out = capi.Output(pipe, 64, n // 64 + 64)
    pipe.probe_rounds([(0, n, 0, 1)], out=out)
    rows, chunks, over = out.stats()
    assert rows == n and not over and chunks > li["n_cus"] * 8
    got = out.aggregate([("count_star", -1, 0), ("sum", -1, 1), ("min", -1, 1), ("max", 0, 0)])
    assert got == [n, int(x.astype(np.int64).sum()), int(x.min()), -int(pk.min()) * 10**15]
    out.close()
    pipe.close()
    ht.close()


# ---- B. the perfect-hash GROUP BY --------------------------------------------------------------------------------------------
KEY_DOMAIN = (-3, 6)  # (min_value, n_values) of the small key columns: values in [-5, 4] (signed) or [0, 4] (unsigned)
WRAP = (I64_MIN + 5, 4)  # an int64 key whose out-of-domain values near INT64_MAX wrap the offset


def group_columns(rng, n, prefix):
    """key columns of every width and signedness over a small range, an int64 key near both ends of its domain, a
    wide int32 key, hashed-GROUP-BY keys (INT64_MIN / MAX, -1, 0, 1 and 1 + 2^32), a hot key; aggregated columns of
    large magnitude"""
    cols = {}
    for dt in INT_TYPES:
        lo = -5 if np.iinfo(dt).min < 0 else 0
        cols["%s_k_%s" % (prefix, np.dtype(dt).name)] = rng.integers(lo, 5, n).astype(dt)
    cols[prefix + "_wrap"] = np.where(rng.random(n) < 0.5, WRAP[0] + rng.integers(-2, 6, n),
                                      I64_MAX - rng.integers(0, 8, n)).astype(np.int64)
    cols[prefix + "_wide"] = rng.integers(-10, (1 << 18) + 10, n).astype(np.int32)
    specials = np.array([I64_MIN, I64_MAX, -1, 0, 1, 1 + (1 << 32), 1 << 32, -(1 << 32), I64_MIN + 1], dtype=np.int64)
    cols[prefix + "_h"] = rng.choice(specials, n)
    cols[prefix + "_hot"] = np.where(rng.random(n) < 0.9, 7, rng.integers(-10**9, 10**9, n)).astype(np.int32)
    big = rng.integers(1 << 61, I64_MAX, n, dtype=np.int64, endpoint=True)
    cols[prefix + "_big"] = np.where(rng.random(n) < 0.6, -big - 1, big)
    cols[prefix + "_i8"] = full_range(rng, np.int8, n)
    cols[prefix + "_u32"] = full_range(rng, np.uint32, n)
    valid = {c: (rng.random(n) > 0.05).astype(np.uint8) for c in cols}
    return cols, valid


def py_grouped(s, keys, specs):
    """perfect-hash GROUP BY over the reference rows -> (values[n_groups][n_aggs], dropped)"""
    n = len(s.rows)
    g = [0] * n
    ok = [True] * n
    n_groups = 1
    for sj, sc, mn, nv in keys:
        vals, valid = s.values(sj, sc)
        for i, (v, o) in enumerate(zip(vals.tolist(), valid.tolist())):
            off = int(v) - mn
            ok[i] = ok[i] and o and 0 <= off < nv
            g[i] = g[i] * nv + (off if ok[i] else 0)
        n_groups *= nv
    cols = [s.values(sj, sc) if fn != "count_star" else None for fn, sj, sc in specs]
    members = {}
    for i in range(n):
        if ok[i]:
            members.setdefault(g[i], []).append(i)
    want = [[0 if fn in ("count", "count_star") else None for fn, _, _ in specs] for _ in range(n_groups)]
    for q, idx in members.items():
        for a, (fn, _, _) in enumerate(specs):
            if fn == "count_star":
                want[q][a] = len(idx)
            else:
                vals, valid = cols[a]
                want[q][a] = py_agg(fn, vals[idx], valid[idx])
    return want, ok.count(False)


ALL_FNS = ["count_star", "count", "sum", "min", "max"]
B_SHAPES = {
    # name: ([(key column, min_value, n_values)], aggregated column, functions)
    "probe-1key": ([("p_k_int8",) + KEY_DOMAIN], "p_big", ALL_FNS),
    "3keys-every-source": ([("p_k_uint16",) + KEY_DOMAIN, ("b0_k_int32",) + KEY_DOMAIN, ("b1_k_uint8", -3, 5)], "b1_big",
                           ALL_FNS),
    "widths": ([("b0_k_uint32",) + KEY_DOMAIN, ("b1_k_int64",) + KEY_DOMAIN, ("p_k_int16", -5, 2)], "b0_i8", ALL_FNS),
    "cells-1024-lds": ([("p_k_int32", -5, 16), ("b1_k_uint8", -2, 16)], "b0_big", ["count_star", "sum", "min", "max"]),
    "cells-1025-global": ([("p_k_int8", -5, 5), ("b0_k_int16", -30, 41)], "b1_big", ALL_FNS),
    "int64-wrap": ([("p_wrap",) + WRAP], "p_big", ALL_FNS),
    "2^18-groups": ([("b1_wide", 0, 1 << 18)], "p_u32", ALL_FNS),
}
B_CASES = [(e, shape) for e in ENGINES for shape in B_SHAPES]


@pytest.mark.parametrize("engine,shape", B_CASES, ids=["%s-%s" % c for c in B_CASES])
def test_grouped(gpu_ctx, engine, shape):
    """perfect-hash GROUP BY: 1-3 keys of every width and signedness from the probe row and both kinds of table, negative
    min_value, all five functions over large int64 values (per-group high-limb sums go negative), cells exactly at the LDS
    limit (1024) and one past it, 2^18 groups, an int64 key whose offset wraps; dropped = NULL + out-of-domain keys"""
    key_names, agg_name, fns = B_SHAPES[shape]
    s = Star(n=15_000, seed=60 + B_CASES.index((engine, shape)), extra=group_columns, flat=engine == "flat")
    s.run(gpu_ctx, engine)
    keys = [s.col(c) + (mn, nv) for c, mn, nv in key_names]
    specs = [(fn, *s.col(agg_name)) if fn != "count_star" else (fn, -1, 0) for fn in fns]
    n_groups = int(np.prod([k[3] for k in keys]))
    cells = n_groups * len(specs)
    assert cells == {"cells-1024-lds": 1024, "cells-1025-global": 1025}.get(shape, cells)
    vals, counts, dropped = s.out.aggregate_grouped(keys, specs)
    want, want_dropped = py_grouped(s, keys, specs)
    assert dropped == want_dropped and dropped > 0
    if shape == "int64-wrap":  # rows near INT64_MAX exist; none landed in a group
        assert (s.values(*s.col("p_wrap"))[0] > 0).sum() > 100
    for q in range(n_groups):
        assert vals[q] == want[q], "group %d" % q
    assert sum(counts[q][0] for q in range(n_groups)) + dropped == len(s.rows)
    s.close()


def test_grouped_refusals(gpu_ctx):
    """an n_groups that is not the domain product and an empty domain: POLR_E_INVALID; a domain product above 2^20:
    POLR_E_UNSUPPORTED (nothing written to the results)"""
    s = Star(n=2000, seed=70, extra=group_columns).run(gpu_ctx, "path")
    L = gpu_ctx.L
    sj, sc = s.col("p_k_int8")
    spec = (capi.AggSpec * 1)(capi.AggSpec(0, -1, 0))
    res = (capi.AggValue * 64)()
    dropped = C.c_uint64()

    def call(key_list, n_groups):
        ka = (capi.GroupKey * len(key_list))()
        for i, (mn, nv) in enumerate(key_list):
            ka[i].src_join, ka[i].src_col, ka[i].min_value, ka[i].n_values = sj, sc, mn, nv
        return L.polr_out_aggregate_grouped(s.out.h, None, ka, len(key_list), spec, 1, res, n_groups, C.byref(dropped))

    assert call([(-5, 8)], 8) == capi.OK
    assert call([(-5, 8)], 9) == capi.E_INVALID
    assert call([(-5, 8), (0, 0)], 0) == capi.E_INVALID
    assert call([(0, 1 << 11), (0, 1 << 10)], 1 << 21) == capi.E_UNSUPPORTED
    s.close()


# ---- C. the general GROUP BY ---------------------------------------------------------------------------------------------------
def py_hashed(s, cols, specs):
    keys = [s.values(sj, sc) for sj, sc in cols]
    aggs = [s.values(sj, sc) if fn != "count_star" else None for fn, sj, sc in specs]
    members = {}
    for i in range(len(s.rows)):
        key = tuple(int(v[i]) if ok[i] else None for v, ok in keys)
        members.setdefault(key, []).append(i)
    want = {}
    for key, idx in members.items():
        want[key] = [len(idx) if fn == "count_star" else py_agg(fn, aggs[a][0][idx], aggs[a][1][idx])
                     for a, (fn, _, _) in enumerate(specs)]
    return want


C_SHAPES = {
    "specials": ["p_h"],
    "hi-bits-3": ["b1_h", "p_k_uint32", "b0_k_int8"],
    "widths": ["p_k_uint8", "b0_k_int16", "b1_k_uint16"],
    "widths-64": ["b0_k_int64", "b1_k_int32", "p_k_uint32"],
    "hot-group": ["p_hot"],
}
C_CASES = [(e, shape) for e in ENGINES for shape in C_SHAPES]


@pytest.mark.parametrize("engine,shape", C_CASES, ids=["%s-%s" % c for c in C_CASES])
def test_hashed(gpu_ctx, engine, shape):
    """general GROUP BY: 1-3 group columns of every width and signedness from the probe row and both kinds of table; NULL
    and 0 are two groups; INT64_MIN, INT64_MAX, -1, 0; 1 and 1 + 2^32 are two groups; a hot group of ~90 % of the rows
    (every lane of a workgroup races for one empty slot); the key set exactly, then every cell"""
    s = Star(n=15_000, seed=80 + C_CASES.index((engine, shape)), extra=group_columns, flat=engine == "flat")
    s.run(gpu_ctx, engine)
    cols = [s.col(c) for c in C_SHAPES[shape]]
    specs = [("count_star", -1, 0)] + [(fn, *s.col("b0_big")) for fn in ALL_FNS[1:]] + [("sum", *s.col("p_i8")),
                                                                                        ("max", *s.col("b1_u32"))]
    want = py_hashed(s, cols, specs)
    got = s.out.aggregate_hashed(cols, specs, max(1024, 2 * len(want)))
    assert set(got) == set(want)
    for key in want:
        assert got[key] == want[key], key
    if shape == "specials":
        assert {(None,), (0,), (1,), (1 + (1 << 32),), (I64_MIN,), (I64_MAX,), (-1,)} <= set(got)
    if shape == "hot-group":
        assert got[(7,)][0] > 0.8 * len(s.rows)
    s.close()


def test_hashed_capacity(gpu_ctx):
    """groups = rows (all distinct); exactly max_groups groups succeed, max_groups - 1 is POLR_E_OVERFLOW with n_groups >=
    max_groups - 1; max_groups above 2^24 is POLR_E_UNSUPPORTED; an empty output gives 0 groups"""
    rng = np.random.default_rng(90)
    n = 50_000
    j = Join(np.arange(0, n, dtype=np.int32), 0, (0, n - 1))
    ht = j.device(gpu_ctx)
    pk = rng.permutation(n).astype(np.int32)
    g = (pk.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)).view(np.int64)  # (a bijection: wide, sparse, distinct)
    assert len(np.unique(g)) == n
    pipe = capi.Pipeline(gpu_ctx, [pk, g], n, [(ht, [(-1, 0)])], [[0]])
    assert pipe.launch_info(True)["flat"] == 1
    out = capi.Output(pipe, 1024, n // 1024 + 1 + MAX_WAVE_CHUNKS)
    pipe.probe_rounds([(0, n, 0, 1)], out=out)
    got = out.aggregate_hashed([(-1, 1)], [("count_star", -1, 0), ("sum", -1, 1)], n)
    assert len(got) == n and all(v == [1, k[0]] for k, v in got.items()) and set(k[0] for k in got) == set(g.tolist())
    L = gpu_ctx.L
    ka = (capi.GroupKey * 1)()
    ka[0].src_join, ka[0].src_col = -1, 1
    sa = (capi.AggSpec * 1)(capi.AggSpec(0, -1, 0))
    keys = np.zeros((n, 1), np.int64)
    nulls = np.zeros(n, np.uint32)
    res = (capi.AggValue * n)()
    n_groups = C.c_uint64()
    rc = L.polr_out_aggregate_hashed(out.h, None, ka, 1, sa, 1, n - 1, keys.ctypes.data, nulls.ctypes.data, res,
                                     C.byref(n_groups))
    assert rc == capi.E_OVERFLOW and n_groups.value >= n - 1
    rc = L.polr_out_aggregate_hashed(out.h, None, ka, 1, sa, 1, (1 << 24) + 1, keys.ctypes.data, nulls.ctypes.data, res,
                                     C.byref(n_groups))
    assert rc == capi.E_UNSUPPORTED
    out.reset()
    assert out.aggregate_hashed([(-1, 1)], [("count_star", -1, 0)], 16) == {}
    out.close()
    pipe.close()
    ht.close()


# ---- D. the general GROUP BY against one run of the reference (tests/golden/hash_groupby.json) -----------------------------------
@pytest.mark.parametrize("engine", ["path", "generic"])
def test_hashed_against_the_reference(gpu_ctx, engine):
    """the fixture's inputs regenerated from its seed and shape; the device's groups against the reference's"""
    from common import load_golden
    from joinref import hashagg_inputs
    gold = load_golden("hash_groupby")
    fact, fact_valid, dim, dim_valid = hashagg_inputs(**gold["shape"])
    j = Join(dim["dk"], 0, None, None, [dim["g2"]], [dim_valid["g2"]])
    ht = j.device(gpu_ctx)
    pcols = [fact["fk"], fact["g1"], fact["x"]]
    pvalid = [None, fact_valid["g1"], fact_valid["x"]]
    n = len(pcols[0])
    pipe = capi.Pipeline(gpu_ctx, pcols, n, [(ht, [(-1, 0)])], [[0]], probe_valid=pvalid)
    assert pipe.launch_info(True)["flat"] == 0
    out = capi.Output(pipe, 1024, n // 1024 + 1 + MAX_WAVE_CHUNKS)
    if engine == "path":
        pipe.probe_rounds([(0, n, 0, 1)], out=out)
    else:
        m = capi.DeviceMultiplexer(pipe, "default_path")
        capi.run_resident([m], [(0, (n + 1023) // 1024)], out=out, reset=True, finish=True)
        m.finish()
        m.close()
    specs = [("count_star", -1, 0)] + [(fn, -1, 2) for fn in ("count", "sum", "min", "max")]
    got = out.aggregate_hashed([(-1, 1), (0, 0)], specs, 1024)
    want = {(r[0], r[1]): r[2:] for r in gold["rows"]}
    assert got == want
    out.close()
    pipe.close()
    ht.close()


# ---- E. string heaps and the string sink -------------------------------------------------------------------------------------
def string_blocks(values, valid, n_blocks, seed=0):
    """string_t cells for `values` (bytes) with the long ones spread over n_blocks heap blocks (separate host arrays, in
    turn); the cells of NULL rows hold arbitrary bytes -- length > 12 and any pointer -- as the reference leaves them"""
    rng = np.random.default_rng(seed)
    parts, sizes, loc = [[] for _ in range(n_blocks)], [0] * n_blocks, []
    n_long = 0
    for i, v in enumerate(values):
        if valid[i] and len(v) > 12:
            b = n_long % n_blocks
            n_long += 1
            loc.append((b, sizes[b]))
            parts[b].append(v)
            sizes[b] += len(v)
        else:
            loc.append(None)
    blocks = [np.frombuffer(b"".join(p) + b"\x00", np.uint8).copy() for p in parts]  # (+1: never empty)
    cells = np.zeros((len(values), 16), np.uint8)
    for i, v in enumerate(values):
        if not valid[i]:
            cells[i] = rng.integers(0, 256, 16)
            cells[i, 0:4] = np.frombuffer(np.uint32(13 + i % 5000).tobytes(), np.uint8)
            continue
        cells[i, 0:4] = np.frombuffer(np.uint32(len(v)).tobytes(), np.uint8)
        if len(v) <= 12:
            cells[i, 4:4 + len(v)] = np.frombuffer(v, np.uint8)
        else:
            b, off = loc[i]
            cells[i, 4:8] = np.frombuffer(v[:4], np.uint8)
            cells[i, 8:16] = np.frombuffer(np.uint64(blocks[b].ctypes.data + off).tobytes(), np.uint8)
    return cells.reshape(-1).view("V16"), blocks


LENGTHS = [0, 1, 4, 5, 11, 12, 13, 16, 100]
ALPHABET = [0x00, 0x01, 0x41, 0x7F, 0x80, 0xC3, 0xFE, 0xFF]


def random_strings(rng, n):
    """lengths 0..100 at the inline / heap edges over an alphabet with \\0 and bytes 0x80-0xFF: many shared prefixes"""
    lens = rng.choice(LENGTHS, n)
    vals = [bytes(rng.choice(ALPHABET, k).astype(np.uint8).tolist()) for k in lens]
    vals[:4] = [b"\xff" * 12, b"\xff" * 13, b"\x00" * 12, b"\x00" * 13]  # inline 12 vs heap 13, same first 12 bytes
    return vals


def _string_bank(ctx, side, engine, n_blocks, n=20_000, seed=0, all_null=False):
    """join 0 (repeated-key hash table, perfect for `flat`) with a VARCHAR payload, probe rows with a VARCHAR column; the
    heap of the `side` column goes up in n_blocks blocks: first without the last block (refused: a non-NULL long cell lies
    outside), then whole (accepted), then again (refused: already rebased) -> (pipe, out, rows, strings, valid, src)"""
    rng = np.random.default_rng(seed)
    if engine == "flat":
        bk = rng.permutation(np.arange(0, 3000, dtype=np.int32))
    else:
        bk = rng.permutation(np.repeat(np.arange(0, 3000, 2, dtype=np.int32), 2))
    j = Join(bk, 0, (0, 2999) if engine == "flat" else None)
    nb = len(bk)
    pk = rng.integers(-100, 3100, n).astype(np.int32)
    m = nb if side == "build" else n
    strs = random_strings(rng, m)
    valid = np.zeros(m, np.uint8) if all_null else (rng.random(m) > 0.15).astype(np.uint8)
    cells, blocks = string_blocks(strs, valid, n_blocks, seed)
    upload = blocks if all_null else blocks[:-1]
    if side == "build":
        ht = capi.HashTable.from_columns(ctx, [bk], [cells], payload_valid=[valid])
        if not all_null:
            with pytest.raises(capi.PolrError) as e:
                ht.set_payload_heaps(0, upload)
            assert e.value.code == capi.E_INVALID
        ht.set_payload_heaps(0, blocks)  # (against a library that reads NULL cells: refused here, before any kernel reads one)
        with pytest.raises(capi.PolrError) as e:
            ht.set_payload_heaps(0, blocks)
        assert e.value.code == capi.E_INVALID
        if engine == "flat":
            assert ht.finalize_perfect(0, 2999)
        else:
            ht.finalize_hash()
        pipe = capi.Pipeline(ctx, [pk], n, [(ht, [(-1, 0)])], [[0]])
        src = (0, 0)
    else:
        ht = j.device(ctx)
        pipe = capi.Pipeline(ctx, [pk, cells], n, [(ht, [(-1, 0)])], [[0]], probe_valid=[None, valid])
        if not all_null:
            with pytest.raises(capi.PolrError) as e:
                pipe.set_probe_heaps(1, upload)
            assert e.value.code == capi.E_INVALID
        pipe.set_probe_heaps(1, blocks)
        with pytest.raises(capi.PolrError) as e:
            pipe.set_probe_heaps(1, blocks)
        assert e.value.code == capi.E_INVALID
        src = (-1, 1)
    assert pipe.launch_info(True)["flat"] == int(engine == "flat")
    rows = sort_rows(Ref([pk], None, [j]).rows())
    out = capi.Output(pipe, 64, len(rows) // 64 + 1 + MAX_WAVE_CHUNKS)
    if engine == "path":
        pipe.probe_rounds([(0, n, 0, 1)], out=out)
    else:
        mx = capi.DeviceMultiplexer(pipe, "default_path")
        capi.run_resident([mx], [(0, (n + 1023) // 1024)], out=out, reset=True, finish=True)
        mx.finish()
        mx.close()
    assert np.array_equal(sort_rows(device_rows(out.fetch_ids(), [j])), rows)
    assert out.stats()[1] > 256  # more output chunks than the second pass has lanes
    taken = rows[:, 0] if side == "probe" else rows[:, 1]
    return pipe, out, ht, rows, [strs[r] for r in taken.tolist() if valid[r]], src, blocks


STRING_CASES = [("path", "probe", 2), ("path", "build", 3), ("generic", "build", 2), ("generic", "probe", 3),
                ("flat", "build", 3), ("flat", "probe", 2)]


@pytest.mark.parametrize("engine,side,n_blocks", STRING_CASES, ids=["%s-%s-%d" % c for c in STRING_CASES])
def test_string_heaps_and_minmax(gpu_ctx, engine, side, n_blocks):
    """multi-block heaps on the build side (hash table, perfect table: heap set before finalize_perfect) and the probe side;
    NULL cells with arbitrary bytes take no part; an upload refused for a cell outside the given ranges leaves the column
    as it was and a corrected retry succeeds; MIN / MAX against Python bytes over > 256 output chunks"""
    pipe, out, ht, rows, live, src, _blocks = _string_bank(gpu_ctx, side, engine, n_blocks,
                                                          seed=STRING_CASES.index((engine, side, n_blocks)))
    assert len(live) > 1000
    assert out.aggregate_string("min", *src) == min(live)
    assert out.aggregate_string("max", *src) == max(live)
    out.close()
    pipe.close()
    ht.close()


def test_string_sink_edges(gpu_ctx):
    """an all-NULL column is NULL; dst_cap below the winner's length: *len is the whole length and only dst_cap bytes are
    written"""
    pipe, out, ht, rows, live, src, _b = _string_bank(gpu_ctx, "probe", "path", 2, seed=9, all_null=True)
    assert live == [] and len(rows) > 0
    assert out.aggregate_string("min", *src) is None and out.aggregate_string("max", *src) is None
    out.close()
    pipe.close()
    ht.close()
    pipe, out, ht, rows, live, src, _b = _string_bank(gpu_ctx, "build", "path", 2, seed=10)
    want = max(live)
    assert len(want) > 5
    buf = C.create_string_buffer(b"\xaa" * 16, 16)
    n_len, null = C.c_uint32(), C.c_uint32()
    gpu_ctx.check(gpu_ctx.L.polr_out_aggregate_string(out.h, None, capi.AGG["max"], src[0], src[1], buf, 5, C.byref(n_len),
                                                      C.byref(null)))
    assert null.value == 0 and n_len.value == len(want)
    assert buf.raw[:5] == want[:5] and buf.raw[5:] == b"\xaa" * 11
    out.close()
    pipe.close()
    ht.close()


def test_string_heap_refuses_wrapping_pointers(gpu_ctx):
    """a non-NULL cell whose pointer + length passes 2^64 lies in no range: refused, whatever the range"""
    blocks = [np.zeros(64, np.uint8)]
    cells = np.zeros((3, 16), np.uint8)
    cells[:, 0] = 13
    cells[0, 8:16] = np.frombuffer(np.uint64(blocks[0].ctypes.data).tobytes(), np.uint8)
    cells[1, 8:16] = np.frombuffer(np.uint64(0xFFFFFFFFFFFFFFF9).tobytes(), np.uint8)
    cells[2, 8:16] = np.frombuffer(np.uint64(blocks[0].ctypes.data + 51).tobytes(), np.uint8)  # (51 + 13 = 64: inside)
    pk = np.arange(3, dtype=np.int32)
    ht = Join(pk, 0, (0, 2)).device(gpu_ctx)
    pipe = capi.Pipeline(gpu_ctx, [pk, cells.reshape(-1).view("V16")], 3, [(ht, [(-1, 0)])], [[0]])
    with pytest.raises(capi.PolrError) as e:
        pipe.set_probe_heaps(1, blocks)
    assert e.value.code == capi.E_INVALID
    with pytest.raises(capi.PolrError) as e:  # overlapping ranges
        pipe.set_probe_heaps(1, [blocks[0], blocks[0][8:]])
    assert e.value.code == capi.E_INVALID
    pipe.close()
    ht.close()


# ---- F. materialize ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ENGINES)
def test_materialize(gpu_ctx, engine):
    """every width (1, 2, 4, 8, 16; signed and unsigned) with NULLs, from the probe row, a hash table's payload and a perfect
    table's; to host memory and to device memory (POLR_COL_DEVICE, hipMalloc'ed); against a numpy gather over fetch_ids;
    a destination shorter than the output is refused"""
    s = Star(n=15_000, seed=100 + ENGINES.index(engine), flat=engine == "flat").run(gpu_ctx, engine, 1000)
    rows = device_rows(s.ids, s.joins)  # (device order)
    n = len(rows)
    L = gpu_ctx.L
    for prefix in ("p", "b0", "b1"):
        for name in [np.dtype(d).name for d in INT_TYPES] + ["u64", "v16"]:
            sj, sc = s.col("%s_%s" % (prefix, name))
            vals, valid = s.values(sj, sc, rows)
            dt = vals.dtype
            want = vals.copy()
            want.view(np.uint8).reshape(n, -1)[~valid] = 0  # (NULL rows come back as 0)
            data, v = s.out.materialize(sj, sc, dt)
            assert np.array_equal(v.astype(bool), valid), (prefix, name)
            assert data.tobytes() == want.tobytes(), (prefix, name)
            dd, dv = DevBuf(n * dt.itemsize), DevBuf(n)
            dv.upload(np.full(n, 7, np.uint8))
            gpu_ctx.check(L.polr_out_materialize(s.out.h, None, sj, sc, dd.ptr, dv.ptr, n, capi.COL_DEVICE))
            gpu_ctx.sync()
            assert dd.download().tobytes() == want.tobytes() and np.array_equal(dv.download().astype(bool), valid)
            dd.free()
            dv.free()
            buf = np.zeros(n * dt.itemsize, np.uint8)
            assert L.polr_out_materialize(s.out.h, None, sj, sc, buf.ctypes.data, None, n - 1, 0) == capi.E_INVALID
    s.close()
