"""The pool kernels at every unit size, source form and tuning field.

How a round is cut into units depends on the probe waves of the launch (polr_pool_unit_size, polr_pool_plan.h): on a full
device every source of 20 000 to 200 000 rows runs the flat kernel in 512-tuple units and the generic one in 64-tuple
units.  Here the pool tuning (device_share = 16, units_x = 1) makes the pool small, `capi.pool_info` says how small, and
`poolunits.source_rows_for` sizes the source so that ONE executor's DEFAULT_PATH round -- its whole chunk range -- is cut
into units of a stated size; every one-executor case asserts that size through the restatement (tests/poolunits.py,
held against the library's own function by tests/test_pool_units.py) before it runs.  (DEFAULT_PATH sets "never route
again" with its first decision, so polr_router_route adds every remaining chunk of the range to that round:
polr_mpx_device.h, polr_routing.h DetermineNextPath.)  Units above 1024 tuples reach the flat kernel's chain of in-unit
prefetches, sweeps in the middle of a long source, queues at exactly flat_qcap<K>(), 16-bit unit positions above 32 767
and the cap of 65 536; the prefetch of the NEXT unit's first step is reached where a probe wave gets several units
(the x4 cases, see SEVERAL_UNITS, and two waves of the cap case).

All comparisons are exact, against tests/joinref.py's Ref (numpy searchsorted; per-position counts; the expanded row set)
-- for the one 17 M row case a boolean lookup table, for the generic bank (a join keyed by another join's payload) the
same expansion join by join -- and against the oracle where it takes the shape at a small size.  Unless a case says
otherwise a run is DEFAULT_PATH through run_resident, counting and emitting, with every join order of the bank as path 0
(rotations where k > 3)."""
import itertools

import numpy as np
import pytest

import poolunits
from common import orc
from joinref import Join, Ref, _key_case, _perfect_ranges, chunks_for, device_rows, sort_rows
from polr_amd import capi
from test_gpu_sink_matrix import DevBuf
from test_gpu_engine_matrix import (FUSED_AGGS_8, FUSED_AGGS_SMALL, FUSED_SHAPES, _fused_star, _fused_want, _perfect_join,
                                    _wrap_keys, oracle_check)

pytestmark = pytest.mark.gpu

SMALL_POOL = dict(device_share=16, units_x=1)  # the fewest probe waves the tuning allows; ONE unit per probe wave
# ... and four units per probe wave.  A round's units are dealt round-robin over the rings in one publish, and a wave
# takes its ring's tickets in order: with as many units as waves (units_x = 1) every wave gets exactly one unit, and its
# look for a next unit (polr_pool.hip, behind flat_run_source) finds none.  With units_x = 4 every ring holds four
# units per wave, so from a wave's first unit on that look finds the next unit of the same join order already queued
# and flat_prefetch_unit requests its first step -- every time, not by timing.
SEVERAL_UNITS = dict(device_share=16, units_x=4)
I32_MIN, I32_MAX = -2**31, 2**31 - 1


def _tiny_pipe(ctx):
    j = Join(np.arange(8, dtype=np.int32), 0, (0, 7))
    ht = j.device(ctx)
    pipe = capi.Pipeline(ctx, [np.arange(64, dtype=np.int32)], 64, [(ht, [(-1, 0)])], [[0]])
    return ht, pipe, capi.DeviceMultiplexer(pipe, "default_path")


@pytest.fixture(scope="module", autouse=True)
def tuning_left_at_defaults(gpu_ctx):
    """the module leaves the pool tuning of the session's context as it found it: a default-tuned pool_info at its end
    equals the one taken at its start"""
    ht, pipe, m = _tiny_pipe(gpu_ctx)
    before = capi.pool_info([m])
    yield before
    after = capi.pool_info([m])
    m.close()
    pipe.close()
    ht.close()
    assert after == before, (before, after)


def _orders(k):
    if k <= 3:
        return [list(p) for p in itertools.permutations(range(k))]
    return [[(r + i) % k for i in range(k)] for r in range(k)]


def _plan(ctx, joins, col_dtypes, n_exec=1, key_src=None):
    """pool_info of a counting and of an emitting run of this bank, from a pipeline over a 64-row source (the launch's
    shape does not depend on the source) -> (info counting, info emitting)"""
    ght = [j.device(ctx) for j in joins]
    key_src = key_src or [[(-1, j.src)] for j in joins]
    pipe = capi.Pipeline(ctx, [np.zeros(64, dt) for dt in col_dtypes], 64, list(zip(ght, key_src)), [list(range(len(joins)))])
    ms = [capi.DeviceMultiplexer(pipe, "default_path") for _ in range(n_exec)]
    out = capi.Output(pipe, 64, 16)
    infos = capi.pool_info(ms), capi.pool_info(ms, out)
    print("pool_info counting %s\npool_info emitting %s" % infos)
    out.close()
    for m in ms:
        m.close()
    pipe.close()
    for h in ght:
        h.close()
    return infos


def _rows_for(ctx, unit, joins, col_dtypes, flat_emit=True, key_src=None, units_x=1):
    """the source size, 300 rows short of a whole number of units, at which one executor's round runs in units of `unit`:
    units_x units for every probe wave"""
    ic, ie = _plan(ctx, joins, col_dtypes, key_src=key_src)
    assert ic["units_x"] == units_x and ic["share"] == 16
    rows = poolunits.source_rows_for(unit, ic, units_x) - 300
    assert poolunits.unit_of(rows, ic) == unit
    if unit > 300:
        assert -(-rows // unit) == units_x * ic["pool_waves"]
    if flat_emit:
        assert poolunits.unit_of(rows, ie) == unit, (ic, ie)
    return rows


def _want(ref):
    if not hasattr(ref, "want"):
        ref.want = sort_rows(ref.rows())
    return ref.want


def run_orders(ctx, joins, orders, unit, source, flat=(True, True), sel=None, chunk_size=1024, chunk_begin=0, caps=(1024,),
               emit_orders=None):
    """every order as path 0 of a pipeline of its own: run_resident counting and emitting with ONE executor over the chunks
    [chunk_begin, end).  source(order) -> (probe columns, validity, Ref).  flat: the kernel of counting / emitting runs;
    a flat run asserts that its round is cut into units of `unit` tuples"""
    ght = [j.device(ctx) for j in joins]
    for order in orders:
        pcols, pvalid, ref = source(order)
        paths = [order] + [o for o in orders if o != order]
        pipe = capi.Pipeline(ctx, pcols, ref.n, [(h, [(-1, j.src)]) for h, j in zip(ght, joins)], paths, probe_valid=pvalid)
        if sel is not None:
            pipe.set_selection(sel)
        n_src = len(sel) if sel is not None else ref.n
        n_chunks = (n_src + chunk_size - 1) // chunk_size
        round_rows = n_src - chunk_begin * chunk_size
        stage = ref.stage_counts(order)
        want = _want(ref)
        m = capi.DeviceMultiplexer(pipe, "default_path", chunk_size=chunk_size)
        for emit in (False, True):
            if emit and emit_orders is not None and order not in emit_orders:
                continue
            for cap in (caps if emit else (None,)):
                out = capi.Output(pipe, cap, chunks_for(len(want), cap)) if emit else None
                info = capi.pool_info([m], out)
                assert info["flat"] == pipe.launch_info(emit)["flat"] == int(flat[emit]), (order, emit)
                if info["flat"]:
                    assert info["gran"] == 512 and poolunits.unit_of(round_rows, info) == unit, (order, emit, info)
                else:
                    assert info["gran"] == 64
                capi.run_resident([m], [(chunk_begin, n_chunks)], out=out, reset=True, finish=True)
                st = m.finish()
                assert st["stage_out"][0] == stage, "order %s, emit %d, cap %s" % (order, emit, cap)
                assert sum(st["input_tuple_count_per_path"]) == round_rows
                if emit:
                    n_rows, n_used, over = out.stats()
                    assert not over and n_rows == len(want) and n_used >= -(-n_rows // cap)
                    assert np.array_equal(sort_rows(device_rows(out.fetch_ids(), joins)), want), "rows, order %s" % order
                    out.close()
        m.close()
        pipe.close()
    for h in ght:
        h.close()


# ---- data ---------------------------------------------------------------------------------------------------------------------
RANGES = [(-300, 699), (0, 499), (-1000, -1), (5, 1204), (-64, 63), (100, 355)]


def _col(rng, n, lo, hi, frac=0.9):
    """int32 probe keys: about `frac` of them inside [lo, hi] (hits, and misses where the table has holes), the rest on
    both sides of it; the type's minimum, maximum, 0 and -1 sprinkled in"""
    width = hi - lo + 1
    span = int(width / frac)
    lo2 = lo - (span - width) // 2
    c = rng.integers(lo2, lo2 + span, n)
    c[rng.integers(0, n, 64)] = np.resize([I32_MIN, I32_MAX, 0, -1], 64)
    return c.astype(np.int32)


def _flat_bank(rng, k):
    return [_perfect_join(rng, np.int32, lo, hi, hi - lo + 1, c) for c, (lo, hi) in enumerate(RANGES[:k])]  # ~63 % of the range


def _fixed(pcols, pvalid, joins, sel=None):
    ref = Ref(pcols, pvalid, joins, sel)
    return lambda order: (pcols, pvalid, ref)


# ---- 1. unit sizes ------------------------------------------------------------------------------------------------------------
UNIT_CASES = ([(u, 3, 1) for u in (512, 1024, 1536, 2560, 4096)] + [(2560, k, 1) for k in (1, 2, 6)] +
              [(1024, 3, 4), (2560, 3, 4), (2560, 2, 4), (1536, 6, 4)])


@pytest.mark.parametrize("unit,k,units_x", UNIT_CASES, ids=["u%d-k%d-x%d" % c for c in UNIT_CASES])
def test_unit_sizes(gpu_ctx, unit, k, units_x):
    """a streamable source (no validity, no selection) in units of 1 to 8 stage-0 steps, the last unit 300 rows short;
    hits, misses inside the tables' ranges, keys outside them, the key type's minimum, maximum, 0 and -1.  x1: one unit
    per probe wave; x4: four, so that a wave goes from unit to unit with the next unit's first step prefetched
    (SEVERAL_UNITS).  The smallest source also goes through the oracle"""
    rng = np.random.default_rng(1000 + unit + k + 7 * units_x)
    joins = _flat_bank(rng, k)
    try:
        gpu_ctx.set_pool_tuning(**(SMALL_POOL if units_x == 1 else SEVERAL_UNITS))
        n = _rows_for(gpu_ctx, unit, joins, [np.int32] * k, units_x=units_x)
        pcols = [_col(rng, n, *RANGES[c]) for c in range(k)]
        src = _fixed(pcols, None, joins)
        assert len(_want(src(None)[2])) > 1000
        run_orders(gpu_ctx, joins, _orders(k), unit, src)
        if unit == 512:
            oracle_check(pcols, None, joins, _orders(k)[:2], src(None)[2], _want(src(None)[2]))
    finally:
        gpu_ctx.set_pool_tuning()


# ---- 2. source forms ----------------------------------------------------------------------------------------------------------
SOURCE_FORMS = ["valid-stage0", "valid-deeper", "selection", "begin-1023", "begin-1022", "begin-1021", "begin-1024",
                "device-aligned", "device-4-bytes-off"]


SOURCE_CASES = [(f, 1) for f in SOURCE_FORMS] + [(f, 4) for f in ("selection", "begin-1023", "begin-1024", "device-4-bytes-off")]


@pytest.mark.parametrize("form,units_x", SOURCE_CASES, ids=["%s-x%d" % c for c in SOURCE_CASES])
def test_source_forms(gpu_ctx, form, units_x):
    """units of 2560 tuples, k = 3, where stage 0 is not streamable or only just: validity on the stage-0 column of path 0
    (the lane-per-tuple step) or only on a deeper one (streamed, NULLs dropped in the sweep); a selection; a round that
    begins at row 1023 / 1022 / 1021 (begin = 3, 2, 1 mod 4: no 16-byte loads) and at 1024 (the aligned control); a
    caller-owned stage-0 key column (POLR_COL_DEVICE over hipMalloc'ed memory) on a 16-byte boundary and 4 bytes past one.
    x4: four units per probe wave (SEVERAL_UNITS), where flat_prefetch_unit meets the same fallbacks and the control"""
    unit, k = 2560, 3
    rng = np.random.default_rng(2000 + SOURCE_FORMS.index(form) + 50 * units_x)
    joins = _flat_bank(rng, k)
    orders = _orders(k)
    try:
        gpu_ctx.set_pool_tuning(**(SMALL_POOL if units_x == 1 else SEVERAL_UNITS))
        rows = _rows_for(gpu_ctx, unit, joins, [np.int32] * k, units_x=units_x)
        kw = {}
        if form == "selection":
            n = int(rows / 0.6)
            sel = np.sort(rng.choice(n, rows, replace=False)).astype(np.uint32)
            kw["sel"] = sel
        elif form.startswith("begin"):
            cs = int(form.split("-")[1])
            n = rows + cs
            kw.update(chunk_size=cs, chunk_begin=1)
        else:
            n = rows
        pcols = [_col(rng, n, *RANGES[c]) for c in range(k)]
        if form.startswith("valid"):
            valids = [(rng.random(n) > 0.1).astype(np.uint8) for _ in range(k)]
            refs = {}

            def src(order):
                c = order[0] if form == "valid-stage0" else order[-1]
                pv = [valids[x] if x == c else None for x in range(k)]
                if c not in refs:
                    refs[c] = Ref(pcols, pv, joins)
                return pcols, pv, refs[c]
        elif form.startswith("device"):
            off = 0 if form == "device-aligned" else 1
            ref = Ref(pcols, None, joins)
            keep = []

            def src(order):
                c = order[0]  # stage 0 of path 0 reads the caller's memory in place
                while keep:
                    keep.pop().free()  # (the pipeline that read it is closed)
                buf = DevBuf(4 * (n + off))
                buf.upload(np.concatenate([np.zeros(off, np.int32), pcols[c]]))
                keep.append(buf)
                ptr = buf.ptr + 4 * off
                assert ptr % 16 == 4 * off
                return [capi.dev_col(ptr, 4, signed=True) if x == c else pcols[x] for x in range(k)], None, ref
        elif form == "selection":
            src = _fixed(pcols, None, joins, kw["sel"])
        elif form.startswith("begin"):
            src = _fixed(pcols, None, joins, np.arange(kw["chunk_size"], n))
        run_orders(gpu_ctx, joins, orders, unit, src, **kw)
        if form.startswith("device"):
            keep.pop().free()
    finally:
        gpu_ctx.set_pool_tuning()


# ---- 3. queue capacity --------------------------------------------------------------------------------------------------------
def _period_col(rng, n, j, first):
    """keys of join j with a period of 1024 rows: exactly `first` hits among the first 512 rows of a period (one stage-0
    step), at random places, then 512 hits"""
    lo, hi = j.perfect
    holes = np.setdiff1d(np.arange(lo, hi + 1), j.keys.astype(np.int64))
    assert len(holes) > 10
    miss = np.where(rng.random(n) < 0.5, rng.choice(holes, n), rng.integers(hi + 1, hi + 5000, n))
    periods = (n + 1023) // 1024
    step_a = np.argsort(rng.random((periods, 512)), axis=1) < first
    hit = np.concatenate([step_a, np.ones((periods, 512), bool)], axis=1).reshape(-1)[:n]
    assert hit[:512].sum() == first and hit[512:1024].all()
    return np.where(hit, rng.choice(j.keys.astype(np.int64), n), miss).astype(np.int32)


# (K = 2: 64 F + 1 = 513 survivors do not fit into a step of 512 tuples -- that one case does not exist)
QUEUE_CASES = [(k, d) for k in (2, 3) for d in (-1, 0, 1) if (k, d) != (2, 1)]


@pytest.mark.parametrize("k,delta", QUEUE_CASES, ids=["k%d-sweep%+d" % c for c in QUEUE_CASES])
def test_queue_at_capacity(gpu_ctx, k, delta):
    """units of 2048 tuples = two periods of the key pattern: a stage-0 step with 64 F - 1 survivors (one short of a sweep;
    F = 8 for K <= 2, else 4: flat_sweep_f) and then a step with 512 leave the queue behind stage 0 at exactly
    flat_qcap<K>() entries; with 64 F and 64 F + 1 the sweep fires in between.  In the K = 4 bank the second join lets
    every tuple through, so the queue behind it fills at the same rate"""
    unit = 2048
    rng = np.random.default_rng(3000 + 10 * k + delta)
    joins = _flat_bank(rng, k)
    if k == 3:
        joins[1] = Join(np.arange(0, 500, dtype=np.int32), 1, (0, 499))  # every key of its range
    try:
        gpu_ctx.set_pool_tuning(**SMALL_POOL)
        n = _rows_for(gpu_ctx, unit, joins, [np.int32] * k)
        ght = [j.device(gpu_ctx) for j in joins]
        tiny = capi.Pipeline(gpu_ctx, [np.zeros(64, np.int32)] * k, 64, [(h, [(-1, j.src)]) for h, j in zip(ght, joins)],
                             [list(range(k))])
        K = tiny.launch_info(False)["compiled_stages"]
        assert K == tiny.launch_info(True)["compiled_stages"] == (2 if k <= 2 else 4)
        tiny.close()
        for h in ght:
            h.close()
        F = 8 if K <= 2 else 4
        pcols = [_period_col(rng, n, joins[0], 64 * F + delta)]
        if k == 3:
            pcols.append(rng.integers(0, 500, n).astype(np.int32))
        pcols.append(_col(rng, n, *RANGES[k - 1], frac=0.08))  # few tuples leave
        ref = Ref(pcols, None, joins)
        first = list(range(k))
        assert ref.counts[0][:512].sum() == 64 * F + delta and ref.counts[0][512:1024].sum() == 512
        assert ref.counts[0][unit:unit + 512].sum() == 64 * F + delta  # (a unit begins with the sparse step)
        if k == 3:
            assert ref.stage_counts(first)[1] == ref.stage_counts(first)[0]
        run_orders(gpu_ctx, joins, _orders(k), unit, lambda order: (pcols, None, ref))
    finally:
        gpu_ctx.set_pool_tuning()


@pytest.mark.parametrize("survive", ["all", "none"])
def test_queues_of_the_widest_bank(gpu_ctx, survive):
    """k = 6 at units of 2048 tuples: every tuple survives every join (all five queues run full the whole time; the rows
    are checked for the first join order, the counts for every rotation), and none survives stage 0"""
    unit, k = 2048, 6
    rng = np.random.default_rng(3100 + len(survive))
    joins = _flat_bank(rng, k)
    try:
        gpu_ctx.set_pool_tuning(**SMALL_POOL)
        n = _rows_for(gpu_ctx, unit, joins, [np.int32] * k)
        pcols = [rng.choice(j.keys, n) for j in joins]
        if survive == "none":
            pcols[0] = np.where(rng.random(n) < 0.5, RANGES[0][1] + 1 + rng.integers(0, 100, n), RANGES[0][0] - 1).astype(np.int32)
        ref = Ref(pcols, None, joins)
        orders = _orders(k)
        assert ref.stage_counts(orders[0]) == ([n] * k if survive == "all" else [0] * k)
        run_orders(gpu_ctx, joins, orders, unit, lambda order: (pcols, None, ref), emit_orders=orders[:1])
    finally:
        gpu_ctx.set_pool_tuning()


# ---- 4. the cap ---------------------------------------------------------------------------------------------------------------
def test_units_of_65536_tuples(gpu_ctx):
    """the one large case: 65 536 x target + 70 000 rows (about 17 M; a unit of 65 536 tuples cannot be had from fewer than
    16 x 65 536 rows, and the tuning allows no fewer probe waves than a sixteenth of the device's), two 4-byte columns,
    k = 2.  Down path [0, 1] few tuples survive stage 0: those at unit positions 0, 1, 32 767, 32 768, 65 534 and 65 535
    of the first, a middle and the last whole unit and in the short last unit; down path [1, 0] half of all tuples wait
    in the queue as 16-bit positions.  Reference: boolean lookup tables (the same mathematics as searchsorted)"""
    rng = np.random.default_rng(4000)
    j0 = Join(np.arange(0, 1000, 2, dtype=np.int32), 0, (0, 999))
    j1 = Join(np.arange(-50, 51, dtype=np.int32)[rng.random(101) < 0.5], 1, (-50, 50))
    joins = [j0, j1]
    try:
        gpu_ctx.set_pool_tuning(**SMALL_POOL)
        ic, ie = _plan(gpu_ctx, joins, [np.int32] * 2)
        target = max(16, ic["pool_waves"])
        n = 65536 * target + 70000
        for info in (ic, ie):
            assert poolunits.unit_size(n, info["pool_waves"], 1, info["gran"], info["hi_tuples"], 1, info["hi_unit"]) == \
                (65536, target + 2)
        c0 = rng.integers(1000, I32_MAX, n, dtype=np.int64).astype(np.int32)  # outside join 0's range
        c0[rng.integers(0, n, n // 50)] = 501  # ... or a hole inside it
        c1 = rng.integers(-50, 51, n).astype(np.int32)
        at = np.array([u * 65536 + p for u in (0, target // 2, target - 1)
                       for p in (0, 1, 32767, 32768, 65534, 65535)] + [(target + 1) * 65536 + p for p in (0, 1, 4463)])
        assert at.max() == n - 1
        c0[at] = 2 * (np.arange(len(at)) % 500)
        c1[at[::2]] = j1.keys[0]
        pcols = [c0, c1]
        lut0 = np.zeros(1000, bool)
        lut0[j0.keys] = True
        lut1 = np.zeros(101, bool)
        lut1[j1.keys + 50] = True
        hit0 = (c0 >= 0) & (c0 <= 999) & lut0[np.clip(c0, 0, 999)]
        hit1 = lut1[c1 + 50]
        both = np.nonzero(hit0 & hit1)[0]
        assert set(at[::2].tolist()) <= set(both.tolist()) and len(both) < 5000
        want = sort_rows(np.column_stack([both, j0.id_to_row[c0[both]], j1.id_to_row[c1[both] + 50]]))
        n_chunks = (n + 1023) // 1024
        ght = [j.device(gpu_ctx) for j in joins]
        for order, stage in (([0, 1], [int(hit0.sum()), len(both)]), ([1, 0], [int(hit1.sum()), len(both)])):
            pipe = capi.Pipeline(gpu_ctx, pcols, n, [(h, [(-1, j.src)]) for h, j in zip(ght, joins)], [order])
            m = capi.DeviceMultiplexer(pipe, "default_path")
            out = capi.Output(pipe, 1024, chunks_for(len(want), 1024))
            for o in (None, out):
                info = capi.pool_info([m], o)
                assert info["flat"] == 1 and poolunits.unit_of(n, info) == 65536
                capi.run_resident([m], [(0, n_chunks)], out=o, reset=True, finish=True)
                assert m.finish()["stage_out"][0] == stage, (order, o is not None)
            assert np.array_equal(sort_rows(device_rows(out.fetch_ids(), joins)), want)
            out.close()
            m.close()
            pipe.close()
        for h in ght:
            h.close()
    finally:
        gpu_ctx.set_pool_tuning()


# ---- 5. table kinds and key types -----------------------------------------------------------------------------------------------
EDGE_KEYS = [(dt, kind) for dt in (np.int32, np.uint32) for kind in _perfect_ranges(dt)]


@pytest.mark.parametrize("dt,kind", EDGE_KEYS, ids=["%s-%s" % (np.dtype(d).name, k) for d, k in EDGE_KEYS])
def test_streamed_keys_at_the_type_edges(gpu_ctx, dt, kind):
    """units of 2560 tuples without probe validity (the 16-byte key stream): perfect ranges at the low end, the middle and
    the high end of int32 and uint32, probed with the range's edges, values just outside it and the type's own limits"""
    try:
        gpu_ctx.set_pool_tuning(**SMALL_POOL)
        j, _, _ = _key_case(dt, kind, seed=5000, n_probe=100)
        n = _rows_for(gpu_ctx, 2560, [j], [dt])
        j, pcols, _ = _key_case(dt, kind, seed=5000 + EDGE_KEYS.index((dt, kind)), n_probe=n)
        src = _fixed(pcols, None, [j])
        assert len(_want(src(None)[2])) > 1000
        run_orders(gpu_ctx, [j], [[0]], 2560, src)
    finally:
        gpu_ctx.set_pool_tuning()


def test_streamed_uint32_keys_across_the_sign_bit(gpu_ctx):
    """the middle of uint32 (joinref has no middle range for unsigned types): a perfect range of 3001 values around 2^31,
    where a 32-bit compare that took the key for signed would turn over; probed with both ends, the values next to them
    inside and outside, 2^31 - 1 and 2^31, 0 and 2^32 - 1"""
    rng = np.random.default_rng(5050)
    lo, hi = 2**31 - 1500, 2**31 + 1500
    inner = np.unique(np.concatenate([rng.integers(lo, hi + 1, 2000), [lo, lo + 1, 2**31 - 1, 2**31, hi - 1, hi]]))
    inner = inner[~np.isin(inner, [lo + 2, hi - 2])]  # holes next to both ends
    j = Join(rng.permutation(inner).astype(np.uint32), 0, (lo, hi), None, [(inner % 97).astype(np.int32)])
    try:
        gpu_ctx.set_pool_tuning(**SMALL_POOL)
        n = _rows_for(gpu_ctx, 2560, [j], [np.uint32])
        edges = np.array([lo - 1, lo, lo + 1, lo + 2, 2**31 - 1, 2**31, hi - 2, hi - 1, hi, hi + 1, 0, 2**32 - 1, 1,
                          lo - 2**31, hi - 2**31])  # (the last two: the ends with the top bit flipped)
        pk = np.concatenate([np.resize(edges, 3000), rng.integers(lo - 40, hi + 41, n // 2),
                             rng.integers(0, 2**32, n - n // 2 - 3000)])
        pcols = [rng.permutation(pk).astype(np.uint32)]
        src = _fixed(pcols, None, [j])
        assert len(_want(src(None)[2])) > 1000
        run_orders(gpu_ctx, [j], [[0]], 2560, src)
    finally:
        gpu_ctx.set_pool_tuning()


def _hbm_join(rng, src):
    return _perfect_join(rng, np.int32, 0, 8_000_000, 40_000, src)  # 1 MB of bits: never in LDS


def _hbm_col(rng, j, n):
    return np.where(rng.random(n) < 0.5, rng.choice(j.keys, n), rng.integers(-100, 8_000_101, n)).astype(np.int32)


def _s8_join(ctx, rng, src):
    keys, distinct, tail, cap = _wrap_keys(ctx, np.int32, 480, 120, 1, 3, 0)  # a cluster that wraps past the last slot group
    return Join(rng.permutation(keys), src, None, None, [np.arange(len(keys), dtype=np.int32)]), tail, distinct


def _s8_col(rng, tail, distinct, n):
    return rng.permutation(np.concatenate([rng.choice(tail, n // 2), rng.choice(distinct, n // 4),
                                           rng.integers(1, 2_000_000, n - n // 2 - n // 4)]).astype(np.int32))


@pytest.mark.parametrize("bank", ["hbm", "s8-wrap", "mixed"])
def test_table_kinds(gpu_ctx, bank):
    """units of 2560 tuples, streamed: a perfect table too large for LDS, an S8 unique-key hash table whose cluster wraps
    around the table's end (counting: flat; emitting: the generic kernel), and a bank of all three kinds"""
    rng = np.random.default_rng(5100 + len(bank))
    try:
        gpu_ctx.set_pool_tuning(**SMALL_POOL)
        if bank == "hbm":
            joins = [_hbm_join(rng, 0)]
        elif bank == "s8-wrap":
            j, tail, distinct = _s8_join(gpu_ctx, rng, 0)
            joins = [j]
        else:
            j, tail, distinct = _s8_join(gpu_ctx, rng, 2)
            joins = [_perfect_join(rng, np.int32, -300, 699, 1000, 0), _hbm_join(rng, 1), j]
        k = len(joins)
        flat_emit = bank == "hbm"
        n = _rows_for(gpu_ctx, 2560, joins, [np.int32] * k, flat_emit=flat_emit)
        if bank == "hbm":
            pcols = [_hbm_col(rng, joins[0], n)]
        elif bank == "s8-wrap":
            pcols = [_s8_col(rng, tail, distinct, n)]
        else:
            pcols = [_col(rng, n, -300, 699), _hbm_col(rng, joins[1], n), _s8_col(rng, tail, distinct, n)]
        if bank != "s8-wrap":
            ht = joins[-1 if bank == "hbm" else 1].device(gpu_ctx)
            pipe = capi.Pipeline(gpu_ctx, [pcols[0]], n, [(ht, [(-1, 0)])], [[0]])
            assert pipe.launch_info(False)["lds_tables"] == 0
            pipe.close()
            ht.close()
        src = _fixed(pcols, None, joins)
        assert len(_want(src(None)[2])) > 1000
        run_orders(gpu_ctx, joins, _orders(k), 2560, src, flat=(True, flat_emit))
    finally:
        gpu_ctx.set_pool_tuning()


# ---- 6. sinks -----------------------------------------------------------------------------------------------------------------
def test_output_chunk_capacities(gpu_ctx):
    """the emitting flat build at units of 2560 tuples into chunks of 64 and of 1024 rows"""
    rng = np.random.default_rng(6000)
    joins = _flat_bank(rng, 3)
    try:
        gpu_ctx.set_pool_tuning(**SMALL_POOL)
        n = _rows_for(gpu_ctx, 2560, joins, [np.int32] * 3)
        pcols = [_col(rng, n, *RANGES[c]) for c in range(3)]
        run_orders(gpu_ctx, joins, [[0, 1, 2], [2, 0, 1]], 2560, _fixed(pcols, None, joins), caps=(64, 1024))
    finally:
        gpu_ctx.set_pool_tuning()


def test_reset_on_the_context_stream_precedes_a_run_on_the_multiplexers(gpu_ctx):
    """Output.reset() only enqueues its memsets on the context's stream, and a run without a stream argument goes to the
    multiplexer's own: the library orders the run behind the reset (an event), or the reset could land behind the run
    and wipe the cursor -- counters right, no rows.  Pool launch and path kernel, 30 times each, every row every time.
    (This keeps the pair of calls exercised; it is no deterministic guard -- without the event the order of the two is a
    matter of timing, and the pair can come out right by chance.)"""
    rng = np.random.default_rng(6050)
    joins = _flat_bank(rng, 2)
    n = 20_000
    pcols = [_col(rng, n, *RANGES[c]) for c in range(2)]
    ref = Ref(pcols, None, joins)
    want = _want(ref)
    ght = [j.device(gpu_ctx) for j in joins]
    pipe = capi.Pipeline(gpu_ctx, pcols, n, [(h, [(-1, j.src)]) for h, j in zip(ght, joins)], [[0, 1]])
    out = capi.Output(pipe, 64, chunks_for(len(want), 64))  # (many chunk counters: a longer memset)
    pool, path = capi.DeviceMultiplexer(pipe, "default_path"), capi.DeviceMultiplexer(pipe, "default_path")
    for i in range(60):
        out.reset()
        if i % 2:
            m = pool
            capi.run_resident([m], [(0, (n + 1023) // 1024)], out=out, reset=True, finish=True)
        else:
            m = path
            m.reset()
            m.run(0, (n + 1023) // 1024, out=out)
        assert m.finish()["stage_out"][0] == ref.stage_counts([0, 1])
        assert out.stats()[0] == len(want), i
    assert np.array_equal(sort_rows(device_rows(out.fetch_ids(), joins)), want)
    pool.close()
    path.close()
    out.close()
    pipe.close()
    for h in ght:
        h.close()


@pytest.mark.parametrize("shape", ["slot0", "4096x8-global"])
def test_fused_group_by(gpu_ctx, shape):
    """the GROUP BY fused into the flat pool at units of 2560 tuples, cells in LDS and in global memory (the two shapes of
    test_gpu_engine_matrix.py::test_fused_sink_matrix), against exact Python sums over the reference row set"""
    raw_keys, in_lds = FUSED_SHAPES[shape]
    specs = FUSED_AGGS_8 if not in_lds else FUSED_AGGS_SMALL

    def build(n):
        joins, cols, valid = _fused_star(n=n, seed=6100)
        names = list(cols)
        keys = [(sj, names.index(sc) if sj < 0 else sc, mn, nv) for sj, sc, mn, nv in raw_keys]
        dspecs = [(fn, sj, 0 if sc is None else (names.index(sc) if sj < 0 else sc)) for fn, sj, sc in specs]
        pcols = list(cols.values())
        pvalid = [valid.get(c) for c in names]
        assert pvalid[0] is None and pvalid[1] is None  # the key columns carry no validity: streamed
        ght = [j.device(gpu_ctx) for j in joins]
        pipe = capi.Pipeline(gpu_ctx, pcols, n, [(h, [(-1, j.src)]) for h, j in zip(ght, joins)], [[0, 1], [1, 0]],
                             probe_valid=pvalid)
        out = capi.Output(pipe, 1024, 64)
        out.fuse_grouped(keys, dspecs)
        m = capi.DeviceMultiplexer(pipe, "default_path")
        return joins, cols, valid, names, keys, ght, pipe, out, m

    def close(ght, pipe, out, m):
        m.close()
        out.close()
        pipe.close()
        for h in ght:
            h.close()

    try:
        gpu_ctx.set_pool_tuning(**SMALL_POOL)
        *_, ght, pipe, out, m = build(2000)
        info = capi.pool_info([m], out)
        close(ght, pipe, out, m)
        n = poolunits.source_rows_for(2560, info, 1) - 300
        joins, cols, valid, names, keys, ght, pipe, out, m = build(n)
        li = pipe.launch_info(True)
        n_groups = int(np.prod([q[3] for q in keys]))
        assert li["flat"] == 1 and (li["lds_bytes_per_workgroup"] + 8 + 8 * n_groups * (1 + 2 * len(specs)) <= 160 * 1024) == in_lds
        info = capi.pool_info([m], out)
        assert info["flat"] == 1 and poolunits.unit_of(n, info) == 2560
        want, dropped, n_rows = _fused_want(joins, cols, valid, names, keys, specs, None)
        assert dropped > 0 and n_rows > 1000
        capi.run_resident([m], [(0, (n + 1023) // 1024)], out=out, reset=True, finish=True)
        assert m.finish()["stage_out"][0][1] == n_rows
        vals, _counts, got_dropped = out.fused_result()
        assert got_dropped == dropped
        assert vals == want
        close(ght, pipe, out, m)
    finally:
        gpu_ctx.set_pool_tuning()


# ---- 7. several executors and every tuning field ------------------------------------------------------------------------------------
def test_results_do_not_depend_on_executors_or_pool_size(gpu_ctx):
    """1, 3 and 8 executors over adjacent chunk ranges x units_x 1 and 4 x a whole, half and a sixteenth of the device: the
    per-position counts summed over the executors and the row set are the reference's (how many executors are still
    routing when a round is cut depends on timing, so the unit size is not asserted here)"""
    rng = np.random.default_rng(7000)
    joins = _flat_bank(rng, 3)
    n = 200_000 - 300
    pcols = [_col(rng, n, *RANGES[c]) for c in range(3)]
    ref = Ref(pcols, None, joins)
    want = _want(ref)
    order = [1, 2, 0]
    stage = ref.stage_counts(order)
    ght = [j.device(gpu_ctx) for j in joins]
    pipe = capi.Pipeline(gpu_ctx, pcols, n, [(h, [(-1, j.src)]) for h, j in zip(ght, joins)], [order, [0, 1, 2]])
    n_chunks = (n + 1023) // 1024
    out = capi.Output(pipe, 1024, chunks_for(len(want), 1024))
    ms = [capi.DeviceMultiplexer(pipe, "default_path") for _ in range(8)]
    try:
        for n_exec, units_x, share in itertools.product((1, 3, 8), (1, 4), (1, 2, 16)):
            gpu_ctx.set_pool_tuning(device_share=share, units_x=units_x)
            mm = ms[:n_exec]
            info = capi.pool_info(mm)
            assert info["share"] == share and info["units_x"] == units_x and info["flat"] == 1
            ranges = [((e * n_chunks) // n_exec, ((e + 1) * n_chunks) // n_exec) for e in range(n_exec)]
            for o in (None, out):
                out.reset()
                capi.run_resident(mm, ranges, out=o, reset=True, finish=True)
                sts = capi.finish_many(mm)
                got = [sum(st["stage_out"][0][x] for st in sts) for x in range(3)]
                assert got == stage, (n_exec, units_x, share, o is not None)
            assert np.array_equal(sort_rows(device_rows(out.fetch_ids(), joins)), want), (n_exec, units_x, share)
    finally:
        gpu_ctx.set_pool_tuning()
    for m in ms:
        m.close()
    out.close()
    pipe.close()
    for h in ght:
        h.close()


SMALL_ROUND_TUNINGS = [dict(hi_unit=u, hi_lottery=lot, **({} if p1 is None else {"hi_tuples_p1": p1}))
                       for u in (64, 320, 1024) for p1 in (1, 1025, None) for lot in (1, 8)] + [dict(idle_sleep=16)]


def _trace(ctx, pipe, routing, n_chunks):
    m = capi.DeviceMultiplexer(pipe, routing, max_log_rounds=1 << 14)
    capi.run_resident([m], [(0, n_chunks)], reset=True, finish=True)
    st = m.finish()
    path, tuples, inter = m.fetch_log()
    m.close()
    return (path.tolist(), tuples.tolist(), inter.tolist(), st["input_tuple_count_per_path"], st["num_intermediates"])


def _routing_does_not_depend_on_tuning(ctx, pipe, pcols, ojoins, paths, n, tunings):
    n_chunks = (n + 1023) // 1024
    for routing in ("adaptive_reinit", "dynamic"):
        o = orc.run_pipeline(pcols, ojoins, paths, routing=routing, caching=False, collect_output=False)
        base = _trace(ctx, pipe, routing, n_chunks)
        assert len(base[0]) > 3 and len(set(base[0])) > 1  # several rounds, more than one join order
        assert base[2] == o["intermediates_per_round"].tolist()
        assert base[3] == o["input_tuple_count_per_path"][:len(paths)] and base[4] == o["num_intermediates"]
        for tn in tunings:
            try:
                ctx.set_pool_tuning(**tn)
                got = _trace(ctx, pipe, routing, n_chunks)
            finally:
                ctx.set_pool_tuning()
            assert got == base, (routing, tn)


def test_routing_does_not_depend_on_small_round_tuning(gpu_ctx):
    """ADAPTIVE_REINIT and DYNAMIC over the flat kernel under hi_unit 64 / 320 / 1024 x hi_tuples 0 / 1024 / default x
    hi_lottery 1 / 8, and idle_sleep 16: the routing log, the tuples per join order and the intermediates are those of
    the run under default tuning, and the oracle's"""
    rng = np.random.default_rng(7100)
    joins = _flat_bank(rng, 3)
    n = 60_000
    pcols = [_col(rng, n, *RANGES[0], frac=0.3), _col(rng, n, *RANGES[1], frac=0.9), _col(rng, n, *RANGES[2], frac=0.6)]
    paths = [[0, 1, 2], [1, 2, 0], [2, 0, 1]]
    ght = [j.device(gpu_ctx) for j in joins]
    pipe = capi.Pipeline(gpu_ctx, pcols, n, [(h, [(-1, j.src)]) for h, j in zip(ght, joins)], paths)
    assert pipe.launch_info(False)["flat"] == 1
    _routing_does_not_depend_on_tuning(gpu_ctx, pipe, pcols, [j.oracle() for j in joins], paths, n, SMALL_ROUND_TUNINGS)
    pipe.close()
    for h in ght:
        h.close()


# ---- the generic kernel ---------------------------------------------------------------------------------------------------------
class ChainBank:
    """a repeated-key S16 join on probe column 0, a join keyed by payload column 0 of the join before it, and a join with
    a 2-byte key on probe column 1; the reference expands the row set join by join in path order (searchsorted runs)"""
    KEY_SRC = [[(-1, 0)], [(0, 0)], [(-1, 1)]]
    ORDERS = [[0, 1, 2], [2, 0, 1], [0, 2, 1]]  # (join 1 reads join 0's payload: it comes after it)

    def __init__(self, rng, n):
        k0 = rng.choice(np.arange(0, 40_000, 3, dtype=np.int32), 1500, replace=False)
        k0 = np.concatenate([k0, k0[:700], k0[:300]])  # 300 keys three times, 400 twice
        pay0 = rng.integers(0, 600, len(k0)).astype(np.int32)
        k1 = rng.choice(np.arange(0, 600, dtype=np.int32), 380, replace=False)
        k2 = rng.choice(np.arange(-2000, 2000, dtype=np.int16), 1500, replace=False)
        self.joins = [Join(rng.permutation(k0), 0, None, None, [pay0]), Join(k1, 0, None), Join(k2, 1, None)]
        self.pcols = [np.where(rng.random(n) < 0.25, rng.choice(k0, n), rng.integers(-5, 40_005, n)).astype(np.int32),
                      rng.integers(-2100, 2100, n).astype(np.int16)]
        self.n = n

    def key(self, x, t):
        sj, sc = self.KEY_SRC[x][0]
        return self.pcols[sc][t[:, 0]] if sj < 0 else self.joins[sj].payload[sc][t[:, 1 + sj]]

    def expand(self, order):
        """-> (rows after each join of `order`, the final rows (probe row, build row per join in the original order))"""
        t = np.full((self.n, 4), -1, np.int64)
        t[:, 0] = np.arange(self.n)
        counts = []
        for x in order:
            j = self.joins[x]
            key = self.key(x, t)
            left = np.searchsorted(j.sorted, key, "left")
            c = np.searchsorted(j.sorted, key, "right") - left
            rep = np.repeat(np.arange(len(t)), c)
            within = np.arange(len(rep)) - np.repeat(np.cumsum(c) - c, c)
            t = t[rep]
            t[:, 1 + x] = j.order[np.repeat(left, c) + within]
            counts.append(len(t))
        return counts, sort_rows(t)

    def device(self, ctx, paths):
        ght = [j.device(ctx) for j in self.joins]
        assert [h.info()["kind"] for h in ght] == [3, 2, 3]  # (S16: repeated keys; S8: unique 4-byte keys; S16: 2-byte keys)
        return ght, capi.Pipeline(ctx, self.pcols, self.n, list(zip(ght, self.KEY_SRC)), paths)

    def oracle_joins(self):
        return [orc.JoinSpec(orc.HashTable([j.keys], j.payload), ks) for j, ks in zip(self.joins, self.KEY_SRC)]


GENERIC_CASES = [(u, s) for u in (64, 1024, 8192) for s in ("share", "no-share")]


@pytest.mark.parametrize("unit,sharing", GENERIC_CASES, ids=["u%d-%s" % c for c in GENERIC_CASES])
def test_generic_kernel_unit_sizes(gpu_ctx, unit, sharing):
    """the generic kernel in units of 64, 1024 and 8192 tuples, work sharing at its default and switched off, counting and
    emitting"""
    tn = dict(SMALL_POOL, **({} if sharing == "share" else {"share_after": 0xFFFFFFFF}))
    rng = np.random.default_rng(8000 + unit)
    try:
        gpu_ctx.set_pool_tuning(**tn)
        small = ChainBank(rng, 64)
        ic, ie = _plan(gpu_ctx, small.joins, [np.int32, np.int16], key_src=ChainBank.KEY_SRC)
        assert ic["flat"] == 0 and ic["gran"] == 64 and ie["gran"] == 64
        # (a counting and an emitting run carry different tuple slots, so their pools may differ: each gets the source
        # size at which ITS round is cut into units of `unit`)
        sizes = [poolunits.source_rows_for(unit, i, 1) - 300 * (unit > 300) for i in (ic, ie)]
        for n in sorted(set(sizes)):
            bank = ChainBank(rng, n)
            for order in ChainBank.ORDERS:
                counts, want = bank.expand(order)
                assert len(want) > 100
                ght, pipe = bank.device(gpu_ctx, [order] + [o for o in ChainBank.ORDERS if o != order])
                m = capi.DeviceMultiplexer(pipe, "default_path")
                out = capi.Output(pipe, 1024, chunks_for(len(want), 1024))
                for emit in (0, 1):
                    if sizes[emit] != n:
                        continue
                    info = capi.pool_info([m], out if emit else None)
                    assert info["flat"] == 0 and poolunits.unit_of(n, info) == unit, info
                    capi.run_resident([m], [(0, (n + 1023) // 1024)], out=out if emit else None, reset=True, finish=True)
                    assert m.finish()["stage_out"][0] == counts, (order, emit)
                    if emit:
                        assert np.array_equal(sort_rows(out.fetch_ids()), want), order
                out.close()
                m.close()
                pipe.close()
                for h in ght:
                    h.close()
        if unit == 64:  # the oracle on the smallest source
            o = orc.run_pipeline(bank.pcols, bank.oracle_joins(), [ChainBank.ORDERS[0]], routing="default_path")
            counts, want = bank.expand(ChainBank.ORDERS[0])
            assert o["num_intermediates"] == sum(counts) and np.array_equal(sort_rows(o["out_rows"]), want)
    finally:
        gpu_ctx.set_pool_tuning()


def test_generic_routing_does_not_depend_on_tuning(gpu_ctx):
    """the same bank under ADAPTIVE_REINIT and DYNAMIC: hi_unit x hi_tuples as above, units_x 1 / 4 and a whole, half and
    a sixteenth of the device leave the routing log, the tuples per join order and the intermediates as they are"""
    rng = np.random.default_rng(8100)
    n = 60_000
    bank = ChainBank(rng, n)
    ght, pipe = bank.device(gpu_ctx, ChainBank.ORDERS)
    assert pipe.launch_info(False)["flat"] == 0
    tunings = [dict(hi_unit=u, **({} if p1 is None else {"hi_tuples_p1": p1})) for u in (64, 320, 1024) for p1 in (1, 1025, None)]
    tunings += [dict(units_x=x, device_share=s) for x in (1, 4) for s in (1, 2, 16)]
    _routing_does_not_depend_on_tuning(gpu_ctx, pipe, bank.pcols, bank.oracle_joins(), ChainBank.ORDERS, n, tunings)
    pipe.close()
    for h in ght:
        h.close()


# ---- tuning values outside the documented ranges --------------------------------------------------------------------------------------
def test_tuning_outside_its_ranges_is_refused(gpu_ctx, tuning_left_at_defaults):
    """polr_ctx_set_pool_tuning refuses a hi_unit that is not a multiple of 64, units_x = 5 (the rings are sized for 4) and
    device_share = 17 with POLR_E_INVALID, and what was set before stays in force"""
    ht, pipe, m = _tiny_pipe(gpu_ctx)
    try:
        gpu_ctx.set_pool_tuning(device_share=2, units_x=3, hi_unit=128)
        before = capi.pool_info([m])
        assert (before["share"], before["units_x"], before["hi_unit"]) == (2, 3, 128)
        for bad in (dict(hi_unit=100), dict(hi_unit=32), dict(hi_unit=1088), dict(units_x=5), dict(device_share=17),
                    dict(hi_lottery=3), dict(idle_sleep=32), dict(share_after=8)):
            with pytest.raises(capi.PolrError) as e:
                gpu_ctx.set_pool_tuning(**bad)
            assert e.value.code == capi.E_INVALID, bad
            assert capi.pool_info([m]) == before, bad
        for ok in (dict(hi_unit=64), dict(hi_unit=1024), dict(units_x=4), dict(device_share=16)):
            gpu_ctx.set_pool_tuning(**ok)
    finally:
        gpu_ctx.set_pool_tuning()
    assert capi.pool_info([m]) == tuning_left_at_defaults
    with pytest.raises(capi.PolrError) as e:  # a share beyond 16 in the run's flags is refused by the plan, not run
        capi.pool_info([m], share=17)
    assert e.value.code == capi.E_INVALID
    m.close()
    pipe.close()
    ht.close()
