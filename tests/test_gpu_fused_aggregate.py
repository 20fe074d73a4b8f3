"""The fused ungrouped aggregate sink of the generic pool kernel (polr_out_fuse_aggregate / polr_out_fused_aggregate_result):
COUNT(*) / COUNT / SUM / MIN / MAX folded into aggregate cells where the run would have written row ids.

The reference is this file's own evaluation -- numpy and Python ints over the join result of tests/joinref.py's Ref
(searchsorted, NULL never matching, the row set expanded join by join): NULL arguments take no part, COUNT is never NULL,
SUM / MIN / MAX over no rows are None, sums are exact (two numpy limbs recombined as Python ints).  A second witness, where a
case says so, is Output.aggregate over an emitting run of the same pipeline.  Every fused run writes into an output of ONE
chunk: a single row id written would overflow it, and out.stats() must report no rows."""
import ctypes as C

import numpy as np
import pytest

from joinref import Join, Ref
from polr_amd import capi
from test_gpu_sink_matrix import DevBuf

pytestmark = pytest.mark.gpu

INT_TYPES = [np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.int64]
SIZES = [0, 1, 63, 64, 65, 129, 4097]  # around the 64-lane batch, GEN_STEP = 128 and the 64-tuple unit granularity
KINDS = ["perfect", "unique", "run"]
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def typed_columns(rng, n, prefix):
    """one column per integer type over its whole range, the extremes present (where there are rows enough), ~10 % NULLs,
    plus a column whose every row is NULL"""
    cols, valid = {}, {}
    for dt in INT_TYPES:
        info = np.iinfo(dt)
        v = rng.integers(int(info.min), int(info.max), n, dtype=np.dtype(dt), endpoint=True)
        v[::5] = info.min
        v[2::5] = info.max
        name = "%s_%s" % (prefix, np.dtype(dt).name)
        cols[name] = v
        valid[name] = (rng.random(n) > 0.1).astype(np.uint8)
    cols[prefix + "_allnull"] = rng.integers(-5, 5, n).astype(np.int32)
    valid[prefix + "_allnull"] = np.zeros(n, np.uint8)
    return cols, valid


def build_side(rng, kind, run, n_keys=300):
    """keys of one build side: a perfect table (dense, with holes), a unique-key hash table, or a hash table whose every key
    repeats `run` times; hash tables have NULL keys among them"""
    if kind == "perfect":
        keys = rng.permutation(np.arange(0, n_keys, dtype=np.int32)[np.arange(n_keys) % 11 != 3])
        return keys, (0, n_keys - 1), None
    base = rng.choice(np.arange(-10**6, 10**6, 7, dtype=np.int64), n_keys if kind == "unique" else max(n_keys // run, 8), replace=False)
    keys = rng.permutation(np.repeat(base, 1 if kind == "unique" else run)).astype(np.int32)
    return keys, None, (rng.random(len(keys)) > 0.03).astype(np.uint8)


class Bank:
    """n probe rows x k joins keyed by probe columns fk0 .. fk(k-1); every build side and the probe table carry the typed
    columns.  kinds: one table kind per join."""

    def __init__(self, n, kinds, run=2, seed=0, hit=0.8):
        rng = np.random.default_rng(seed)
        self.n, self.k = n, len(kinds)
        self.joins, self.bnames = [], []
        fks, fkv = [], []
        for j, kind in enumerate(kinds):
            keys, perfect, kvalid = build_side(rng, kind, run)
            cols, valid = typed_columns(rng, len(keys), "b%d" % j)
            self.bnames.append(list(cols))
            self.joins.append(Join(keys, j, perfect, kvalid, list(cols.values()), [valid[c] for c in cols]))
            fk = np.where(rng.random(n) < hit, rng.choice(keys, n), rng.integers(-10**6, 10**6, n)).astype(np.int32)
            fks.append(fk)
            fkv.append((rng.random(n) > 0.03).astype(np.uint8))  # NULL join keys on the probe side
        cols, valid = typed_columns(rng, n, "p")
        self.pnames = ["fk%d" % j for j in range(self.k)] + list(cols)
        self.pcols = fks + list(cols.values())
        self.pvalid = fkv + [valid[c] for c in cols]
        self.paths = [list(range(self.k)), list(range(self.k))[::-1]] if self.k > 1 else [[0]]

    def col(self, name):
        if name in self.pnames:
            return -1, self.pnames.index(name)
        j = int(name[1])
        return j, self.bnames[j].index(name)

    def device(self, ctx):
        self.ght = [j.device(ctx) for j in self.joins]
        self.pipe = capi.Pipeline(ctx, self.pcols, self.n, [(h, [(-1, j.src)]) for h, j in zip(self.ght, self.joins)], self.paths,
                                  probe_valid=self.pvalid)
        return self.pipe

    def rows(self, sel=None):
        return Ref(self.pcols, self.pvalid, self.joins, sel).rows()

    def values(self, rows, sj, sc):
        if sj < 0:
            data, v, r = self.pcols[sc], self.pvalid[sc], rows[:, 0]
        else:
            data, v, r = self.joins[sj].payload[sc], self.joins[sj].payload_valid[sc], rows[:, 1 + sj]
        return data[r], (np.ones(len(r), bool) if v is None else v[r].astype(bool))

    def want(self, rows, specs):
        return [py_agg(fn, *self.values(rows, sj, sc)) if fn != "count_star" else len(rows) for fn, sj, sc in specs]

    def close(self):
        self.pipe.close()
        for h in self.ght:
            h.close()


def py_agg(fn, vals, valid):
    v = vals[valid]
    if fn == "count":
        return len(v)
    if len(v) == 0:
        return None
    if fn == "min":
        return int(v.min())
    if fn == "max":
        return int(v.max())
    # exact: the low 32 bits and the (signed) rest are summed apart -- each sum stays far inside 64 bits for these row
    # counts -- and recombined as Python ints
    w = v.astype(np.int64)
    return (int((w >> 32).sum()) << 32) + int((w & 0xFFFFFFFF).sum())


def eight_specs(bank, types):
    """8 aggregates at once over the probe table, the first and the last join's build side"""
    last = bank.k - 1
    t = [np.dtype(x).name for x in types]
    return [("count_star", -1, 0), ("sum",) + bank.col("p_" + t[0]), ("min",) + bank.col("b0_" + t[1]),
            ("max",) + bank.col("b%d_%s" % (last, t[2])), ("count",) + bank.col("b%d_%s" % (last, t[0])),
            ("sum",) + bank.col("b%d_%s" % (last, t[1])), ("min",) + bank.col("p_" + t[2]), ("sum",) + bank.col("b0_allnull")]


def run_pool(pipe, out, n_chunks, launch="resident", E=1, routing="adaptive_reinit", scan=False):
    """one pool run of the whole source into `out` (which is not reset here)"""
    if launch == "backpressure":
        routing, E = "backpressure", pipe.n_paths
    mpxs = [capi.DeviceMultiplexer(pipe, routing) for _ in range(E)]
    if scan:
        for m in mpxs:
            m.use_scan_chunks()
    ranges = [((e * n_chunks) // E, ((e + 1) * n_chunks) // E) for e in range(E)]
    if launch == "resident":
        capi.run_resident(mpxs, ranges, out=out, reset=True, finish=True)
    elif launch == "morsels":
        capi.run_resident_morsels(mpxs, 0, n_chunks, morsel_chunks=1, out=out, reset=True, finish=True)
    elif launch == "ranges":
        q = [(i * n_chunks) // (2 * E) for i in range(2 * E + 1)]
        capi.run_resident_ranges(mpxs, [[(q[e], q[e + 1]), (q[E + e], q[E + e + 1])] for e in range(E)], out=out, reset=True,
                                 finish=True)
    elif launch == "stealing":
        capi.run_resident_stealing(mpxs, ranges, 1, out=out, reset=True, finish=True)
    else:
        capi.run_backpressure(mpxs, 0, n_chunks, morsel_chunks=1, out=out)
    stats = capi.finish_many(mpxs)
    for m in mpxs:
        m.close()
    return sum(sum(st["stage_out"][p][pipe.k - 1] for p in range(pipe.n_paths)) for st in stats)


def fused(ctx, bank, specs, **kw):
    """the specs through the fused sink over one run of the whole table -> results"""
    out = capi.Output(bank.pipe, 64, 1)
    out.fuse_aggregate(specs)
    counted = run_pool(bank.pipe, out, (bank.n + 1023) // 1024, **kw)
    got = out.fused_aggregate_result()
    assert out.stats() == (0, 0, False)  # no row id was written, nothing overflowed
    out.close()
    return got, counted


# ---- sizes x joins x table kinds ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("n", SIZES)
def test_sizes_joins_and_table_kinds(gpu_ctx, n, k):
    """every probe size x 1, 2, 3 joins, with perfect, unique-key hash and run (every key twice) tables in every position in
    turn: 8 aggregates over the probe table, the first and the last join's build side, NULL arguments, NULL join keys, an
    all-NULL argument"""
    for r, first in enumerate(KINDS):
        kinds = [KINDS[(KINDS.index(first) + j) % 3] for j in range(k)]
        bank = Bank(n, kinds, run=2, seed=1000 * k + 10 * SIZES.index(n) + r, hit=0.9)
        bank.device(gpu_ctx)
        rows = bank.rows()
        specs = eight_specs(bank, INT_TYPES[2 * r:2 * r + 3])
        want = bank.want(rows, specs)
        got, counted = fused(gpu_ctx, bank, specs)
        assert counted == len(rows) and got == want, (kinds, got, want)
        assert got[7] is None  # SUM over an all-NULL argument
        if n >= 64:
            assert len(rows) > 0
        bank.close()


# ---- run lengths, work sharing -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("share_after", [16, None], ids=["share16", "default"])
@pytest.mark.parametrize("run", [1, 2, 64, 65, 300])
def test_run_lengths_and_work_sharing(gpu_ctx, run, share_after):
    """the last join's build keys repeat `run` times (300: a pending run long enough for a work-sharing split, the piece
    travelling as a CONT entry), after a unique-key join; with share_after = 16 and the default"""
    bank = Bank(4097 if run < 300 else 1500, ["unique", "run"], run=run, seed=run)
    bank.paths = [[0, 1]]
    bank.device(gpu_ctx)
    rows = bank.rows()
    assert len(rows) > 500 * run
    specs = eight_specs(bank, [np.int64, np.int32, np.uint16])
    want = bank.want(rows, specs)
    try:
        if share_after:
            gpu_ctx.set_pool_tuning(share_after=share_after)
        got, counted = fused(gpu_ctx, bank, specs, routing="default_path")
    finally:
        gpu_ctx.set_pool_tuning()
    assert counted == len(rows) and got == want
    bank.close()


# ---- widths and extremes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["p", "b0", "b1"])
def test_every_width_signed_and_unsigned(gpu_ctx, source):
    """COUNT / SUM / MIN / MAX over each of the seven integer types at its full range, the extremes among the rows, from the
    probe table, a hash table's and a perfect table's payload; the second witness: Output.aggregate over an emitting run"""
    bank = Bank(3000, ["run", "perfect"], run=3, seed=77)
    bank.device(gpu_ctx)
    rows = bank.rows()
    out = capi.Output(bank.pipe, 1024, len(rows) // 1024 + 1 + 8192)
    assert run_pool(bank.pipe, out, 3) == len(rows) == out.stats()[0]
    for dt in INT_TYPES:
        sj, sc = bank.col("%s_%s" % (source, np.dtype(dt).name))
        specs = [("count_star", -1, 0), ("count", sj, sc), ("sum", sj, sc), ("min", sj, sc), ("max", sj, sc)]
        want = bank.want(rows, specs)
        got, _ = fused(gpu_ctx, bank, specs)
        assert got == want == out.aggregate(specs), np.dtype(dt).name
        info = np.iinfo(dt)
        assert got[3] == int(info.min) and got[4] == int(info.max)  # the extremes took part
    out.close()
    bank.close()


def test_sum_beyond_64_bits(gpu_ctx):
    """an 8-byte column of INT64_MAX (and one of INT64_MIN) over a few thousand result rows: the exact SUM needs more than
    64 bits; mixed with a column that cancels to a small value"""
    n = 2000
    keys = np.arange(0, 100, dtype=np.int32)
    pay = [np.full(100, I64_MAX, np.int64), np.full(100, I64_MIN, np.int64)]
    j = Join(keys, 0, (0, 99), None, pay, [None, None])
    fk = (np.arange(n) % 100).astype(np.int32)
    x = np.where(np.arange(n) % 2 == 0, I64_MAX, I64_MIN).astype(np.int64)
    ht = j.device(gpu_ctx)
    pipe = capi.Pipeline(gpu_ctx, [fk, x], n, [(ht, [(-1, 0)])], [[0]])
    out = capi.Output(pipe, 64, 1)
    out.fuse_aggregate([("sum", 0, 0), ("sum", 0, 1), ("sum", -1, 1), ("min", 0, 1), ("max", 0, 0)])
    assert run_pool(pipe, out, 2) == n
    assert out.fused_aggregate_result() == [n * I64_MAX, n * I64_MIN, (n // 2) * (I64_MAX + I64_MIN), I64_MIN, I64_MAX]
    assert n * I64_MAX > 2 ** 64
    out.close()
    pipe.close()
    ht.close()


# ---- run kinds, executors, routing -------------------------------------------------------------------------------------------
LAUNCHES = [("resident", 1), ("resident", 4), ("ranges", 1), ("ranges", 4), ("morsels", 1), ("morsels", 4), ("stealing", 1),
            ("stealing", 4), ("backpressure", 0)]


@pytest.fixture(scope="module")
def shared_bank(gpu_ctx):
    bank = Bank(6000, ["unique", "run", "perfect"], run=3, seed=5)
    bank.device(gpu_ctx)
    bank.ref_rows = bank.rows()
    bank.specs = eight_specs(bank, [np.int32, np.int64, np.uint8])
    bank.ref_want = bank.want(bank.ref_rows, bank.specs)
    yield bank
    bank.close()


@pytest.mark.parametrize("launch,E", LAUNCHES, ids=["%s-%d" % x for x in LAUNCHES])
def test_run_kinds_and_executors(gpu_ctx, shared_bank, launch, E):
    """resident, ranges, morsels, stealing with 1 and 4 executors, and backpressure (one executor per join order): the
    results do not depend on who ran what"""
    got, counted = fused(gpu_ctx, shared_bank, shared_bank.specs, launch=launch, E=E)
    assert counted == len(shared_bank.ref_rows) > 3000 and got == shared_bank.ref_want


def test_routing_does_not_change_the_result(gpu_ctx, shared_bank):
    a, _ = fused(gpu_ctx, shared_bank, shared_bank.specs, routing="alternate")
    b, _ = fused(gpu_ctx, shared_bank, shared_bank.specs, routing="adaptive_reinit", E=4)
    assert a == b == shared_bank.ref_want


# ---- the EXT build: a non-equality condition, a packed two-column key ---------------------------------------------------------
def _brute(pk_cols, bk_cols, cond=None):
    """(probe row, build row) pairs whose key columns are equal (and cond(p, b) holds), by a dictionary"""
    index = {}
    for b, key in enumerate(zip(*[c.tolist() for c in bk_cols])):
        index.setdefault(key, []).append(b)
    pairs = [(p, b) for p, key in enumerate(zip(*[c.tolist() for c in pk_cols])) for b in index.get(key, ())
             if cond is None or cond(p, b)]
    return np.asarray(pairs, dtype=np.int64).reshape(-1, 2)


def test_non_equality_condition(gpu_ctx):
    """a join with `probe.x < build.y` beside its key: conditions are evaluated by the EXT build of the kernel"""
    rng = np.random.default_rng(3)
    n = 3000
    bk = rng.integers(0, 200, 900).astype(np.int32)  # repeated keys
    y = rng.integers(-1000, 1000, 900).astype(np.int32)
    z = rng.integers(I64_MIN, I64_MAX, 900, dtype=np.int64)
    fk = rng.integers(-20, 220, n).astype(np.int32)
    x = rng.integers(-1000, 1000, n).astype(np.int32)
    ht = capi.HashTable.from_columns(gpu_ctx, [bk], [y, z])
    ht.finalize_hash()
    ht.preds = [("<", (-1, 1), 0)]
    pipe = capi.Pipeline(gpu_ctx, [fk, x], n, [(ht, [(-1, 0)])], [[0]])
    pairs = _brute([fk], [bk], lambda p, b: x[p] < y[b])
    assert len(pairs) > 1000
    specs = [("count_star", -1, 0), ("sum", 0, 1), ("min", 0, 0), ("max", -1, 1), ("sum", -1, 1)]
    out = capi.Output(pipe, 64, 1)
    out.fuse_aggregate(specs)
    assert run_pool(pipe, out, 3) == len(pairs)
    zz, yy, xx = z[pairs[:, 1]], y[pairs[:, 1]], x[pairs[:, 0]]
    ones = np.ones(len(pairs), bool)
    assert out.fused_aggregate_result() == [len(pairs), py_agg("sum", zz, ones), int(yy.min()), int(xx.max()), py_agg("sum", xx, ones)]
    out.close()
    pipe.close()
    ht.close()


def test_packed_two_column_key(gpu_ctx):
    """a join keyed by (an 8-byte column, a 2-byte column): a composite key in packed form, fetched by the EXT build"""
    rng = np.random.default_rng(4)
    n = 3000
    b0 = rng.integers(10**12, 10**12 + 40, 500).astype(np.int64)
    b1 = rng.integers(-5, 5, 500).astype(np.int16)
    w = rng.integers(-30000, 30000, 500).astype(np.int16)
    p0 = rng.integers(10**12 - 3, 10**12 + 43, n).astype(np.int64)
    p1 = rng.integers(-6, 6, n).astype(np.int16)
    ht = capi.HashTable.from_columns(gpu_ctx, [b0, b1], [w])
    ht.finalize_hash()
    pipe = capi.Pipeline(gpu_ctx, [p0, p1], n, [(ht, [(-1, 0), (-1, 1)])], [[0]])
    pairs = _brute([p0, p1], [b0, b1])
    assert len(pairs) > 1000
    specs = [("count_star", -1, 0), ("sum", 0, 0), ("min", 0, 0), ("max", 0, 0), ("min", -1, 0)]
    out = capi.Output(pipe, 64, 1)
    out.fuse_aggregate(specs)
    assert run_pool(pipe, out, 3) == len(pairs)
    ww = w[pairs[:, 1]]
    assert out.fused_aggregate_result() == [len(pairs), int(ww.astype(np.int64).sum()), int(ww.min()), int(ww.max()),
                                            int(p0[pairs[:, 0]].min())]
    out.close()
    pipe.close()
    ht.close()


# ---- sources: a scan-filtered source, a host selection -----------------------------------------------------------------------
def test_scan_filtered_source_and_host_selection(gpu_ctx):
    bank = Bank(5000, ["unique", "run"], run=2, seed=9)
    bank.device(gpu_ctx)
    specs = eight_specs(bank, [np.int16, np.int64, np.uint32])
    f = bank.pnames.index("p_int8")
    _n, n_chunks = bank.pipe.scan_filter([(f, "<", 40)])
    sel, _ = bank.pipe.fetch_scan()
    rows = bank.rows(sel)
    out = capi.Output(bank.pipe, 64, 1)
    out.fuse_aggregate(specs)
    assert run_pool(bank.pipe, out, n_chunks, scan=True, E=2) == len(rows) > 200
    assert out.fused_aggregate_result() == bank.want(rows, specs)
    out.close()
    bank.close()
    bank = Bank(5000, ["perfect", "unique"], seed=10)
    bank.device(gpu_ctx)
    sel = np.nonzero(np.arange(5000) % 3 != 1)[0].astype(np.uint32)
    bank.pipe.set_selection(sel)
    rows = bank.rows(sel)
    out = capi.Output(bank.pipe, 64, 1)
    out.fuse_aggregate(specs)
    assert run_pool(bank.pipe, out, (len(sel) + 1023) // 1024) == len(rows) > 200
    assert out.fused_aggregate_result() == bank.want(rows, specs)
    out.close()
    bank.close()


# ---- a flat-eligible pipeline ------------------------------------------------------------------------------------------------
def test_flat_eligible_pipeline_runs_on_the_generic_kernel(gpu_ctx):
    """every join a perfect table keyed by a 4-byte probe column: emitting runs would take the flat kernel; with the sink
    attached the launch is the generic one, the results are right, and launch_info says what it said"""
    bank = Bank(5000, ["perfect", "perfect"], seed=11)
    bank.device(gpu_ctx)
    before = (bank.pipe.launch_info(False), bank.pipe.launch_info(True))
    assert before[1]["flat"] == 1
    rows = bank.rows()
    specs = eight_specs(bank, [np.int32, np.int8, np.int64])
    out = capi.Output(bank.pipe, 64, 1)
    m = capi.DeviceMultiplexer(bank.pipe, "adaptive_reinit")
    assert capi.pool_info([m], out)["flat"] == 1
    out.fuse_aggregate(specs)
    assert capi.pool_info([m], out)["flat"] == 0 and capi.pool_info([m])["flat"] == 1  # (counting runs stay flat)
    m.close()
    assert run_pool(bank.pipe, out, 5) == len(rows) > 1000
    assert out.fused_aggregate_result() == bank.want(rows, specs)
    assert (bank.pipe.launch_info(False), bank.pipe.launch_info(True)) == before
    out.close()
    bank.close()


# ---- lifecycle ---------------------------------------------------------------------------------------------------------------
def test_lifecycle_accumulate_reset_unfuse(gpu_ctx):
    live = capi.device_bytes_live()
    bank = Bank(3000, ["unique", "perfect"], seed=12)
    bank.device(gpu_ctx)
    rows = bank.rows()
    specs = [("count_star", -1, 0), ("sum",) + bank.col("b0_int64"), ("min",) + bank.col("p_int16"), ("max",) + bank.col("b1_uint8"),
             ("count",) + bank.col("p_int32")]
    want = bank.want(rows, specs)
    out = capi.Output(bank.pipe, 1024, 8192 + 8)
    out.fuse_aggregate(specs)
    # before any run: no rows
    assert out.fused_aggregate_result() == [0, None, None, None, 0]
    run_pool(bank.pipe, out, 3)
    assert out.fused_aggregate_result() == want
    assert out.fused_aggregate_result() == want  # read twice
    run_pool(bank.pipe, out, 3)  # two runs without a reset add up: counts and sums double, MIN / MAX stay
    assert out.fused_aggregate_result() == [2 * want[0], 2 * want[1], want[2], want[3], 2 * want[4]]
    # reset, then a run over an empty range: MIN is NULL, not a stale value (and not the 0 a memset would leave)
    out.reset()
    m = capi.DeviceMultiplexer(bank.pipe, "adaptive_reinit")
    capi.run_resident([m], [(0, 0)], out=out, reset=True, finish=True)
    m.finish()
    m.close()
    assert out.fused_aggregate_result() == [0, None, None, None, 0]
    run_pool(bank.pipe, out, 3)
    assert out.fused_aggregate_result() == want
    # un-fuse: row ids flow again, and the result call has nothing to read
    out.fuse_aggregate(None)
    out.reset()
    assert run_pool(bank.pipe, out, 3) == len(rows) == out.stats()[0]
    assert out.aggregate(specs) == want
    with pytest.raises(capi.PolrError) as e:
        gpu_ctx.check(gpu_ctx.L.polr_out_fused_aggregate_result(out.h, None, (capi.AggValue * 5)(), 5))
    assert e.value.code == capi.E_INVALID and "no fused aggregate sink" in str(e.value)
    out.fuse_aggregate(specs)  # attached again, then closed with the sink on
    out.close()
    bank.close()
    assert capi.device_bytes_live() == live


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals(gpu_ctx):
    rng = np.random.default_rng(13)
    n = 2000
    keys = rng.permutation(np.arange(0, 200, dtype=np.int32))
    pay = [rng.integers(0, 7, 200).astype(np.int32), rng.integers(0, 2**63, 200, dtype=np.uint64),
           rng.integers(0, 256, (200, 16), dtype=np.uint8).reshape(-1).view("V16")]
    j = Join(keys, 0, (0, 199), None, pay, [None] * 3)
    fk = rng.integers(0, 220, n).astype(np.int32)
    j2 = Join(np.arange(0, 210, dtype=np.int32), 0, (0, 209))
    ht, ht2 = j.device(gpu_ctx), j2.device(gpu_ctx)
    pipe = capi.Pipeline(gpu_ctx, [fk], n, [(ht, [(-1, 0)]), (ht2, [(-1, 0)])], [[0, 1], [1, 0]])
    rows = Ref([fk], None, [j, j2]).rows()
    out = capi.Output(pipe, 1024, 8200)
    specs = [("count_star", -1, 0), ("sum", 0, 0), ("min", -1, 0)]
    want = [len(rows), int(pay[0][rows[:, 1]].sum()), int(fk[rows[:, 0]].min())]

    def refused(code, call, text=None):
        with pytest.raises(capi.PolrError) as e:
            call()
        assert e.value.code == code, e.value
        assert text is None or text in str(e.value), e.value
        return str(e.value)

    # VARCHAR and unsigned 8-byte arguments: the rule and the words of polr_out_aggregate
    for bad in (1, 2):
        a = refused(capi.E_UNSUPPORTED, lambda: out.fuse_aggregate([("count_star", -1, 0), ("min", 0, bad)]))
        b = refused(capi.E_UNSUPPORTED, lambda: out.aggregate([("count_star", -1, 0), ("min", 0, bad)]))
        assert a == b and "aggregate 1: only integer columns of up to 8 bytes (signed if 8)" in a
    assert refused(capi.E_INVALID, lambda: out.fuse_aggregate([("sum", 0, 9)])) == refused(capi.E_INVALID, lambda: out.aggregate([("sum", 0, 9)]))
    refused(capi.E_UNSUPPORTED, lambda: out.fuse_aggregate([("count_star", -1, 0)] * 9), "at most 8 aggregates")
    refused(capi.E_INVALID, lambda: out.fuse_aggregate([(7, -1, 0)]), "unknown function 7")
    # the result call without a sink (nothing above attached one)
    refused(capi.E_INVALID, lambda: gpu_ctx.check(gpu_ctx.L.polr_out_fused_aggregate_result(out.h, None, (capi.AggValue * 3)(), 3)),
            "no fused aggregate sink")
    # both sinks on one output, either way round (the pipeline is flat: the grouped sink is accepted on its own)
    assert pipe.launch_info(True)["flat"] == 1
    out.fuse_grouped([(0, 0, 0, 7)], [("count_star", -1, 0)])
    refused(capi.E_INVALID, lambda: out.fuse_aggregate(specs), "already has a fused sink")
    out.fuse_grouped(None, None)
    out.fuse_aggregate(specs)
    refused(capi.E_INVALID, lambda: out.fuse_grouped([(0, 0, 0, 7)], [("count_star", -1, 0)]), "already has a fused sink")
    refused(capi.E_INVALID, lambda: out.fuse_aggregate(specs), "already has a fused sink")
    refused(capi.E_INVALID, lambda: gpu_ctx.check(gpu_ctx.L.polr_out_fused_aggregate_result(out.h, None, (capi.AggValue * 2)(), 2)),
            "results hold 2 aggregates, the sink 3")
    # the four entry points that launch the per-round path kernel: POLR_E_UNSUPPORTED, nothing enqueued
    m = capi.DeviceMultiplexer(pipe, "adaptive_reinit")
    refused(capi.E_UNSUPPORTED, lambda: pipe.probe_rounds([(0, n, 0, 1)], out=out), "only the pool launch fills")
    counts_dev = DevBuf(64)
    refused(capi.E_UNSUPPORTED, lambda: pipe.probe_rounds_async(capi.make_rounds([(0, n, 0, 1)]), 1, C.c_void_p(counts_dev.ptr), out=out),
            "fused aggregate sink")
    counts_dev.free()
    refused(capi.E_UNSUPPORTED, lambda: m.run(0, 2, out=out), "fused aggregate sink")
    refused(capi.E_UNSUPPORTED, lambda: capi.run_many([m], [(0, 2)], out=out), "fused aggregate sink")
    gpu_ctx.sync()
    assert out.fused_aggregate_result() == [0, None, None]  # nothing was folded
    m.close()
    # ... and a following pool run gives the right answer
    assert run_pool(pipe, out, 2) == len(rows)
    assert out.fused_aggregate_result() == want
    # the calls that read row ids: the output holds none
    assert out.stats() == (0, 0, False)
    no_ids = "no row ids"
    refused(capi.E_INVALID, lambda: out.fetch_ids(), no_ids)
    refused(capi.E_INVALID, lambda: out.materialize(0, 0, np.int32), no_ids)
    refused(capi.E_INVALID, lambda: out.materialize_strings(0, 2), no_ids)
    refused(capi.E_INVALID, lambda: out.aggregate(specs), no_ids)
    refused(capi.E_INVALID, lambda: capi.HashTable.from_output(out, [(-1, 0)]), no_ids)
    refused(capi.E_INVALID, lambda: capi.Pipeline.from_output(out, [(-1, 0)], [(ht, [(-1, 0)])], [[0]]), no_ids)
    assert out.fused_aggregate_result() == want  # the refusals left the cells alone
    out.close()
    pipe.close()
    ht.close()
    ht2.close()
