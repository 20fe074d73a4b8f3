"""Cross-engine matrix: every probe engine against a plain numpy reference of the same equi-join, at the key types, table
edges, output shapes and GROUP BY sinks where a hand-written copy of a shared rule (polr_device.h) could drift.

The reference: the build keys sorted, np.searchsorted for each probe row's run of matching build rows, NULL never matching
on either side; the row set expanded join by join, per-position counts as the sum over probe rows of the product of the
match counts of the path's prefix; aggregates as exact Python ints over that row set.  Where the oracle accepts the shape
(`orc.run_pipeline`) its counts and rows are checked against the same reference.

Every pipeline asserts `launch_info(materialize)["flat"]`, so each case records which engine it reached:

  engine \\ table   perfect                               S8 (unique 4-byte key)              S16 (repeated, 1/2/8-byte keys)
  path kernel      test_key_types[*-perfect*],           test_key_types[int32/uint32-unique], test_key_types[*-repeated,
  (probe_rounds,   test_flat_*, test_output_chunks[path],test_wrap_around_clusters[s8],      1/2/8-byte unique],
   mpx.run)        test_fused_output_is_refused_...      test_flat_mixed_perfect_and_s8       test_wrap_around_clusters[s16-*]
  flat pool        test_key_types[(u)int32-perfect*]     test_key_types[int32/uint32-unique]  cannot be reached: plan_flat
                   (counting + emitting), test_flat_*,   (counting), test_wrap_around_        takes perfect and S8 tables only
                   test_output_chunks[flat],             clusters[s8] (counting),
                   test_fused_sink_matrix                test_flat_mixed_perfect_and_s8
  generic pool     test_key_types[1/2/8-byte perfect],   test_key_types[int32/uint32-unique]  test_key_types[*-repeated,
                   test_flat_k6_against_k7 (k = 7),      (emitting), test_wrap_around_        1/2/8-byte unique],
                   test_flat_mixed_perfect_and_s8 (emit) clusters[s8] (emitting),             test_wrap_around_clusters[s16-*],
                                                         test_output_chunks[generic]          test_key_types_under_a_selection
  unit sizes       every source here runs the flat pool in 512-tuple and the generic pool in 64-tuple units (a full
                   device's probe waves); units of 512 ... 65 536 / 64 ... 8192 tuples, source forms, queue capacity and
                   the pool tuning: tests/test_gpu_pool_units.py
The LIP scan's own probe loop: test_wrap_around_clusters (scan_filter with lip_joins=1); every key type and table kind of
test_key_types, the all-ones key and several joins in one scan: tests/test_gpu_scan_lip.py."""
import ctypes as C

import numpy as np
import pytest

from common import orc
from joinref import KEY_CASES, Join, Ref, _key_case, chunks_for, device_rows, sort_rows
from polr_amd import capi

pytestmark = pytest.mark.gpu


def oracle_check(pcols, pvalid, joins, paths, ref, want_rows):
    """the oracle, where it takes the shape, agrees with the numpy reference"""
    ojoins = [j.oracle() for j in joins]
    for path in paths:
        o = orc.run_pipeline(pcols, ojoins, [path], routing="default_path", probe_valid=pvalid)
        assert o["num_intermediates"] == sum(ref.stage_counts(path))
        assert np.array_equal(sort_rows(o["out_rows"]), want_rows)  # (the oracle reports build rows)
        for x, (j, oj) in enumerate(zip(joins, ojoins)):
            if oj.ht.pht:  # the device's build ids of a perfect table map back the way pht_orig_rows() says
                ok = j.id_to_row >= 0
                assert np.array_equal(oj.ht.pht_orig_rows()[ok].astype(np.int64), j.id_to_row[ok])


def check_engines(ctx, pcols, pvalid, joins, paths, flat, sel=None, emit_flat=None, resident=True):
    """Runs every join order through the path kernel (probe_rounds counting and emitting, DeviceMultiplexer.run emitting)
    and the pool launch (run_resident counting and emitting); per-position counts and the emitted row set against the
    reference.  flat / emit_flat: what launch_info says for counting / emitting runs."""
    ref = Ref(pcols, pvalid, joins, sel)
    want = sort_rows(ref.rows())
    n_src = len(sel) if sel is not None else len(pcols[0])
    n_chunks = (n_src + 1023) // 1024
    ght = [j.device(ctx) for j in joins]
    for p in range(len(paths)):
        order = [paths[p]] + [q for i, q in enumerate(paths) if i != p]  # DEFAULT_PATH takes path 0
        pipe = capi.Pipeline(ctx, pcols, len(pcols[0]), [(h, [(-1, j.src)]) for h, j in zip(ght, joins)], order,
                             probe_valid=pvalid)
        if sel is not None:
            pipe.set_selection(sel)
        assert pipe.launch_info(False)["flat"] == int(flat)
        assert pipe.launch_info(True)["flat"] == int(flat if emit_flat is None else emit_flat)
        stage = ref.stage_counts(paths[p])
        # path kernel
        counts = pipe.probe_rounds([(0, n_src, 0, 0)])
        assert counts[0].tolist() == stage, "probe_rounds counting, path %d" % p
        out = capi.Output(pipe, 1024, chunks_for(len(want), 1024))
        counts = pipe.probe_rounds([(0, n_src, 0, 1)], out=out)
        assert counts[0].tolist() == stage, "probe_rounds emitting, path %d" % p
        assert np.array_equal(sort_rows(device_rows(out.fetch_ids(), joins)), want), "probe_rounds rows, path %d" % p
        out.reset()
        mpx = capi.DeviceMultiplexer(pipe, "default_path")
        mpx.run(0, n_chunks, out=out)
        st = mpx.finish()
        assert st["stage_out"][0] == stage, "mpx.run, path %d" % p
        assert np.array_equal(sort_rows(device_rows(out.fetch_ids(), joins)), want), "mpx.run rows, path %d" % p
        if resident:
            # pool launch: flat or generic pipeline (launch_info above)
            m2 = capi.DeviceMultiplexer(pipe, "default_path")
            capi.run_resident([m2], [(0, n_chunks)], reset=True, finish=True)
            assert m2.finish()["stage_out"][0] == stage, "run_resident counting, path %d" % p
            out.reset()
            capi.run_resident([m2], [(0, n_chunks)], out=out, reset=True, finish=True)
            assert m2.finish()["stage_out"][0] == stage, "run_resident emitting, path %d" % p
            rows = device_rows(out.fetch_ids(), joins)
            assert np.array_equal(sort_rows(rows), want), "run_resident rows, path %d" % p
            m2.close()
        mpx.close()
        out.close()
        pipe.close()
    for h in ght:
        h.close()
    return ref, want


# ---- a. key types x table kinds x engines --------------------------------------------------------------------------------
def _engines_of(dt, kind):
    """(flat for counting, flat for emitting, the hash table kind) the library must choose"""
    four = np.dtype(dt).itemsize == 4
    if kind.startswith("perfect"):
        return four, four, 1
    if kind == "unique" and four:
        return True, False, 2  # S8: flat counting, generic emitting
    return False, False, 3


@pytest.mark.parametrize("dt,kind", KEY_CASES, ids=["%s-%s" % (np.dtype(d).name, k) for d, k in KEY_CASES])
def test_key_types(gpu_ctx, dt, kind):
    """every key dtype x perfect / unique-hash / repeated-hash table: min, max, 0, -1 and the perfect range's edges on both
    sides, values just outside it, NULLs on both sides -- through the path kernel and the pool launch"""
    j, pcols, pvalid = _key_case(dt, kind, seed=KEY_CASES.index((dt, kind)))
    flat, emit_flat, table_kind = _engines_of(dt, kind)
    ht = j.device(gpu_ctx)
    assert ht.info()["kind"] == table_kind
    ht.close()
    ref, want = check_engines(gpu_ctx, pcols, pvalid, [j], [[0]], flat, emit_flat=emit_flat)
    assert len(want) > 100
    oracle_check(pcols, pvalid, [j], [[0]], ref, want)


def test_uint64_perfect_range_as_int64_bit_patterns(gpu_ctx):
    """a uint64 perfect table above 2^63 takes min and max as their int64 bit patterns, compared unsigned: [2^63 + 5,
    2^63 + 100] is 96 slots; the same bits the other way round (max < min unsigned) and a range of 2^31 slots or more
    are refused"""
    keys = np.array([2**63 + 5, 2**63 + 6, 2**63 + 100], dtype=np.uint64)
    ht = capi.HashTable.from_columns(gpu_ctx, [keys], [])
    assert ht.finalize_perfect(-(2**63) + 5, -(2**63) + 100)
    assert ht.info()["capacity"] == 96 and ht.info()["n_rows"] == 3
    ht.close()
    for lo, hi in ((-(2**63) + 100, -(2**63) + 5), (-(2**63) + 5, -1)):
        bad = capi.HashTable.from_columns(gpu_ctx, [keys], [])
        with pytest.raises(capi.PolrError) as e:
            bad.finalize_perfect(lo, hi)
        assert e.value.code == capi.E_INVALID
        bad.close()


SEL_CASES = [(np.int32, "perfect_mid"), (np.uint32, "unique"), (np.int16, "repeated")]


@pytest.mark.parametrize("dt,kind", SEL_CASES, ids=["%s-%s" % (np.dtype(d).name, k) for d, k in SEL_CASES])
def test_key_types_under_a_selection(gpu_ctx, dt, kind):
    """the same through set_selection: flat pool (perfect, S8 counting), generic pool (S8 emitting, S16), path kernel"""
    j, pcols, pvalid = _key_case(dt, kind, seed=100 + SEL_CASES.index((dt, kind)))
    rng = np.random.default_rng(7)
    sel = np.sort(rng.choice(len(pcols[0]), len(pcols[0]) // 3, replace=False)).astype(np.uint32)
    flat, emit_flat, _ = _engines_of(dt, kind)
    check_engines(gpu_ctx, pcols, pvalid, [j], [[0]], flat, sel=sel, emit_flat=emit_flat)


# ---- b. linear probing that wraps past the last slot group ----------------------------------------------------------------
def _murmur(x):
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x ^ (x >> np.uint64(32))
        x = x * np.uint64(0xd6e8feb86659fd93)
        x = x ^ (x >> np.uint64(32))
        x = x * np.uint64(0xd6e8feb86659fd93)
        x = x ^ (x >> np.uint64(32))
    return x


def _wrap_keys(ctx, dt, n_rows, n_cluster, reps, tail_slots, base):
    """n_cluster distinct keys whose home slots are the last `tail_slots` slots of the table the library builds for
    n_rows rows (read from info()["capacity"]), plus filler keys elsewhere"""
    probe_ht = capi.HashTable.from_columns(ctx, [np.arange(n_rows).astype(dt)], []).finalize_hash()
    cap = probe_ht.info()["capacity"]
    probe_ht.close()
    cand = (np.arange(1, 2_000_000, dtype=np.uint64) + np.uint64(base)).astype(dt)
    home = _murmur(cand.astype(np.uint64)) & np.uint64(cap - 1)  # (positive keys: zero- and sign-extension agree)
    tail = cand[home >= np.uint64(cap - tail_slots)][:n_cluster]
    assert len(tail) == n_cluster
    L = orc.lib()
    for x in tail[:8]:  # the oracle's hash agrees on where they live
        assert L.orc_murmurhash64(int(x)) & (cap - 1) >= cap - tail_slots
    n_fill = n_rows // reps - n_cluster
    fill = cand[home < np.uint64(cap - 8)][:n_fill]
    distinct = np.concatenate([tail, fill])
    keys = np.repeat(distinct, reps)
    return keys, distinct, tail, cap


WRAP_CASES = ["s8", "s16-repeated", "s16-int64"]


@pytest.mark.parametrize("case", WRAP_CASES)
def test_wrap_around_clusters(gpu_ctx, case):
    """a cluster whose home slots are the table's last slots: every probe of it wraps through slot group 0 -- in the flat
    pool (counting, S8), the generic pool, the path kernel and the LIP scan's own probe loop"""
    dt, reps = {"s8": (np.int32, 1), "s16-repeated": (np.int32, 2), "s16-int64": (np.int64, 1)}[case]
    base = 0 if dt == np.int32 else 1 << 40
    keys, distinct, tail, cap = _wrap_keys(gpu_ctx, dt, 480, 120, reps, 3, base)
    rng = np.random.default_rng(WRAP_CASES.index(case))
    n = 60_000
    pk = np.concatenate([rng.choice(tail, n // 2), rng.choice(distinct, n // 4),
                         (rng.integers(1, 2_000_000, n - n // 2 - n // 4) + base)]).astype(dt)
    pk = rng.permutation(pk)
    flt = rng.integers(0, 100, n).astype(np.int32)
    pvalid = [(rng.random(n) > 0.02).astype(np.uint8), None]
    j = Join(rng.permutation(keys), 0, None, None, [np.arange(len(keys), dtype=np.int32)])
    ht = j.device(gpu_ctx)
    info = ht.info()
    assert info["capacity"] == cap and info["kind"] == (2 if case == "s8" else 3)
    ht.close()
    flat = case == "s8"
    ref, want = check_engines(gpu_ctx, [pk, flt], pvalid, [j], [[0]], flat, emit_flat=False)
    assert len(want) > n // 2
    oracle_check([pk, flt], pvalid, [j], [[0]], ref, want)
    # LIP: the scan thins the source by the join's own index
    ght = j.device(gpu_ctx)
    pipe = capi.Pipeline(gpu_ctx, [pk, flt], n, [(ght, [(-1, 0)])], [[0]], probe_valid=pvalid)
    pipe.scan_filter([(1, "<", 70)], lip_joins=1)
    sel, offs = pipe.fetch_scan()
    expect = np.nonzero((flt < 70) & np.isin(pk, keys) & pvalid[0].astype(bool))[0]
    assert np.array_equal(sel, expect)
    assert offs[-1] == len(sel)
    pipe.close()
    ght.close()


# ---- c. the flat engine's own edges ---------------------------------------------------------------------------------------
def _perfect_join(rng, dt, lo, hi, n_keys, src, holes=()):
    vals = np.unique(np.concatenate([rng.integers(lo, hi + 1, n_keys, dtype=np.int64), [lo, lo + 1, hi - 1, hi]]))
    vals = vals[~np.isin(vals, holes)]
    return Join(rng.permutation(vals).astype(dt), src, (lo, hi), None,
                [(vals % 7).astype(np.int16)])


EDGE_RANGES = [("int32-at-min", np.int32, -2**31, -2**31 + 5000), ("int32-at-max", np.int32, 2**31 - 1 - 5000, 2**31 - 1),
               ("int32-across-0", np.int32, -2500, 2500), ("uint32-at-max", np.uint32, 2**32 - 1 - 5000, 2**32 - 1)]


@pytest.mark.parametrize("name,dt,lo,hi", EDGE_RANGES, ids=[e[0] for e in EDGE_RANGES])
def test_flat_32bit_modular_range(gpu_ctx, name, dt, lo, hi):
    """a perfect table whose [min, max] touches INT32_MIN, INT32_MAX or UINT32_MAX (the flat lookup's range test is
    32-bit modular): probe keys at both ends, just outside on both sides, and at the other end of the domain -- one past
    max or before min modulo 2^32"""
    rng = np.random.default_rng(40 + [e[0] for e in EDGE_RANGES].index(name))
    info = np.iinfo(dt)
    j0 = _perfect_join(rng, dt, lo, hi, 2000, 0, holes=[lo + 2, hi - 2])
    j1 = _perfect_join(rng, np.int32, 0, 999, 900, 1)
    n = 50_000
    edge = [lo - 1, lo, lo + 1, lo + 2, hi - 2, hi - 1, hi, hi + 1, int(info.min), int(info.max), int(info.min) + 1,
            int(info.max) - 1, 0]  # (type max + 1 and type min - 1 modulo 2^32 are the other end of the domain)
    edge = [e for e in edge if info.min <= e <= info.max]
    k0 = np.concatenate([np.array(edge * 50, dtype=np.int64), rng.integers(lo - 100, hi + 101, n - 50 * len(edge))])
    k0 = np.clip(k0, int(info.min), int(info.max))
    k0 = rng.permutation(k0).astype(dt)
    k1 = rng.integers(-10, 1010, n).astype(np.int32)
    pv = [(rng.random(n) > 0.02).astype(np.uint8), None]
    pcols = [k0, k1]
    ref, want = check_engines(gpu_ctx, pcols, pv, [j0, j1], [[0, 1], [1, 0]], True, emit_flat=True)
    assert len(want) > 1000
    oracle_check(pcols, pv, [j0, j1], [[0, 1]], ref, want)


def test_flat_lds_and_hbm_bit_tables(gpu_ctx):
    """a bank of perfect tables some of which stay in LDS and one too big for the LDS budget (read from HBM)"""
    rng = np.random.default_rng(31)
    n = 80_000
    joins = [_perfect_join(rng, np.int32, 0, 999, 800, 0), _perfect_join(rng, np.int32, -3000, 3000, 5000, 1),
             _perfect_join(rng, np.int32, 0, 8_000_000, 40_000, 2)]  # 1 MB of bits: never in LDS
    pcols = [rng.integers(-5, 1005, n).astype(np.int32), rng.integers(-3005, 3005, n).astype(np.int32),
             np.where(rng.random(n) < 0.5, rng.choice(joins[2].keys, n), rng.integers(0, 8_000_001, n)).astype(np.int32)]
    pipe = capi.Pipeline(gpu_ctx, pcols, n, [(j.device(gpu_ctx), [(-1, j.src)]) for j in joins], [[0, 1, 2]])
    li = pipe.launch_info(False)
    assert li["flat"] == 1 and 1 <= li["lds_tables"] < 3
    pipe.close()
    check_engines(gpu_ctx, pcols, None, joins, [[0, 1, 2], [2, 1, 0], [1, 2, 0]], True, emit_flat=True)


def test_flat_one_build_side_joined_twice(gpu_ctx):
    """one HashTable behind two joins (two probe columns): the two share one LDS copy"""
    rng = np.random.default_rng(32)
    n = 60_000
    j = _perfect_join(rng, np.int32, -500, 1500, 1500, 0)
    j2 = Join(j.keys, 1, j.perfect, None, j.payload)
    pcols = [rng.integers(-520, 1520, n).astype(np.int32), rng.integers(-520, 1520, n).astype(np.int32)]
    ref = Ref(pcols, None, [j, j2])
    want = sort_rows(ref.rows())
    ht = j.device(gpu_ctx)
    n_chunks = (n + 1023) // 1024
    for paths in ([[0, 1], [1, 0]], [[1, 0], [0, 1]]):
        pipe = capi.Pipeline(gpu_ctx, pcols, n, [(ht, [(-1, 0)]), (ht, [(-1, 1)])], paths)
        li = pipe.launch_info(False)
        assert li["flat"] == 1 and pipe.launch_info(True)["flat"] == 1 and li["lds_tables"] == 1
        m = capi.DeviceMultiplexer(pipe, "default_path")
        capi.run_resident([m], [(0, n_chunks)], reset=True, finish=True)
        assert m.finish()["stage_out"][0] == ref.stage_counts(paths[0])
        out = capi.Output(pipe, 1024, chunks_for(len(want), 1024))
        capi.run_resident([m], [(0, n_chunks)], out=out, reset=True, finish=True)
        m.finish()
        assert np.array_equal(sort_rows(device_rows(out.fetch_ids(), [j, j2])), want)
        counts = pipe.probe_rounds([(0, n, 0, 0)])
        assert counts[0].tolist() == ref.stage_counts(paths[0])
        m.close()
        out.close()
        pipe.close()
    ht.close()


def test_flat_k6_against_k7(gpu_ctx):
    """k = 6, the largest flat bank, against the same six joins plus a seventh that matches every tuple (k = 7: generic
    pool): the same row count, per-position counts against the reference"""
    rng = np.random.default_rng(33)
    n = 60_000
    joins = [_perfect_join(rng, np.int32, 0, 199, 185, c) for c in range(6)]
    pcols = [rng.integers(0, 200, n).astype(np.int32) for _ in range(7)]
    every = Join(np.arange(0, 200, dtype=np.int32), 6, (0, 199))
    paths6 = [list(range(6)), [5, 4, 3, 2, 1, 0]]
    r6, w6 = check_engines(gpu_ctx, pcols, None, joins, paths6, True, emit_flat=True)
    paths7 = [list(range(7)), [6, 5, 4, 3, 2, 1, 0]]
    r7, w7 = check_engines(gpu_ctx, pcols, None, joins + [every], paths7, False, emit_flat=False)
    assert len(w6) == len(w7) > 100
    assert np.array_equal(w7[:, :7], w6)


def test_flat_mixed_perfect_and_s8(gpu_ctx):
    """a bank that mixes perfect and S8 tables: counting runs take the flat pool, emitting runs the generic one"""
    rng = np.random.default_rng(34)
    n = 60_000
    s8 = rng.choice(np.arange(-10**9, 10**9, 977, dtype=np.int64), 3000, replace=False).astype(np.int32)
    joins = [_perfect_join(rng, np.int32, -100, 899, 700, 0), Join(s8, 1, None), _perfect_join(rng, np.int32, 0, 99, 60, 2)]
    pcols = [rng.integers(-120, 920, n).astype(np.int32),
             np.where(rng.random(n) < 0.7, rng.choice(s8, n), rng.integers(-10**9, 10**9, n)).astype(np.int32),
             rng.integers(0, 110, n).astype(np.int32)]
    pv = [None, (rng.random(n) > 0.05).astype(np.uint8), None]
    ref, want = check_engines(gpu_ctx, pcols, pv, joins, [[0, 1, 2], [1, 2, 0], [2, 0, 1]], True, emit_flat=False)
    oracle_check(pcols, pv, joins, [[1, 2, 0]], ref, want)


# ---- d. output chunking ----------------------------------------------------------------------------------------------------
def _chunk_bank(rng, engine, n=40_000):
    j0 = _perfect_join(rng, np.int32, 0, 499, 450, 0)
    if engine == "generic":
        keys = rng.choice(np.arange(0, 10**6, 7, dtype=np.int64), 700, replace=False).astype(np.int32)
        j1 = Join(keys, 1, None)
        k1 = np.where(rng.random(n) < 0.8, rng.choice(keys, n), rng.integers(0, 10**6, n)).astype(np.int32)
    else:
        j1 = _perfect_join(rng, np.int32, 0, 99, 90, 1)
        k1 = rng.integers(0, 100, n).astype(np.int32)
    return [j0, j1], [rng.integers(0, 520, n).astype(np.int32), k1]


CHUNK_CASES = [(cap, eng) for cap in (65, 100, 127, 1000) for eng in ("path", "flat", "generic")]


@pytest.mark.parametrize("cap,engine", CHUNK_CASES, ids=["%d-%s" % c for c in CHUNK_CASES])
def test_output_chunks(gpu_ctx, cap, engine):
    """chunk capacities that are not multiples of 64: with room, the exact row set in no more than max_chunks and at least
    ceil(rows / capacity) chunks; with far too few chunks, overflow is reported, the counters stay exact and what was
    written is a duplicate-free subset of the row set"""
    rng = np.random.default_rng(cap)
    joins, pcols = _chunk_bank(rng, engine)
    n = len(pcols[0])
    ref = Ref(pcols, None, joins)
    want = sort_rows(ref.rows())
    stage = ref.stage_counts([0, 1])
    ght = [j.device(gpu_ctx) for j in joins]
    pipe = capi.Pipeline(gpu_ctx, pcols, n, [(h, [(-1, j.src)]) for h, j in zip(ght, joins)], [[0, 1]])
    assert pipe.launch_info(True)["flat"] == int(engine != "generic")  # (the path kernel runs the flat bank)
    n_chunks = (n + 1023) // 1024
    m = capi.DeviceMultiplexer(pipe, "default_path")

    def run(out):
        if engine == "path":
            counts = np.zeros((1, 2), dtype=np.uint64)
            rc = gpu_ctx.L.polr_probe_rounds(pipe.h, None, capi.make_rounds([(0, n, 0, 1)]), 1, out.h, counts.ctypes.data)
            return rc, counts[0].tolist()
        capi.run_resident([m], [(0, n_chunks)], out=out, reset=True, finish=True)
        return capi.OK, m.finish()["stage_out"][0]

    max_chunks = chunks_for(len(want), cap)
    out = capi.Output(pipe, cap, max_chunks)
    rc, counts = run(out)
    assert rc == capi.OK and counts == stage
    rows, chunks, over = out.stats()
    assert not over and rows == len(want)
    assert -(-rows // cap) <= chunks <= max_chunks
    assert np.array_equal(sort_rows(device_rows(out.fetch_ids(), joins)), want)
    out.close()
    # far too few chunks
    small = capi.Output(pipe, cap, 3)
    rc, counts = run(small)
    assert counts == stage  # the counters are exact
    rows, chunks, over = small.stats()
    assert over and chunks <= 3 and rows <= 3 * cap
    if engine == "path":
        assert rc == capi.E_OVERFLOW
    got = device_rows(small.fetch_ids(), joins)
    assert len({tuple(r) for r in got.tolist()}) == len(got)
    assert {tuple(r) for r in got.tolist()} <= {tuple(r) for r in want.tolist()}
    small.close()
    m.close()
    pipe.close()
    for h in ght:
        h.close()


# ---- e. the fused GROUP BY sink --------------------------------------------------------------------------------------------
def _fused_star(n=50_000, seed=51):
    """two perfect joins; NULL-able signed / unsigned aggregate columns with negatives on the probe side and a build side;
    group columns on the probe row (slot 0) and on both joins' payloads, with NULLs and values outside their domains"""
    rng = np.random.default_rng(seed)
    k0 = np.arange(0, 300, dtype=np.int32)
    k0 = k0[k0 % 11 != 3]
    p0 = rng.integers(-1, 64, len(k0)).astype(np.int16)  # group column: -1 is outside [0, 64)
    p0v = (rng.random(len(k0)) > 0.05).astype(np.uint8)
    k1 = np.arange(-40, 40, dtype=np.int32)
    p1 = rng.integers(0, 6, len(k1)).astype(np.uint8)  # group column: 5 is outside [0, 5)
    w1 = rng.integers(-128, 128, len(k1)).astype(np.int8)  # aggregated build column
    w1v = (rng.random(len(k1)) > 0.1).astype(np.uint8)
    j0 = Join(rng.permutation(k0), 0, (0, 299), None, [p0], [p0v])
    perm = rng.permutation(len(k1))
    j1 = Join(k1[perm], 1, (-40, 39), None, [p1[perm], w1[perm]], [None, w1v[perm]])
    cols = {
        "fk0": rng.integers(-5, 305, n).astype(np.int32),
        "fk1": rng.integers(-45, 45, n).astype(np.int32),
        "g": rng.integers(-1, 65, n).astype(np.int32),  # group column on the probe row
        "i8": rng.integers(-128, 128, n).astype(np.int8),
        "i16": rng.integers(-32768, 32768, n).astype(np.int16),
        "i32": rng.integers(-2**31, 2**31, n, dtype=np.int64).astype(np.int32),
        "u16": rng.integers(0, 65536, n).astype(np.uint16),
        "u32": rng.integers(0, 2**32, n, dtype=np.int64).astype(np.uint32),
        "f": rng.integers(0, 100, n).astype(np.int32),  # scan filter column
    }
    valid = {"g": (rng.random(n) > 0.03).astype(np.uint8), "i8": (rng.random(n) > 0.2).astype(np.uint8),
             "i16": (rng.random(n) > 0.1).astype(np.uint8), "u32": (rng.random(n) > 0.1).astype(np.uint8)}
    return [j0, j1], cols, valid


FUSED_SHAPES = {
    # name: (group keys [(src_join, column name or payload index, min, n_values)], in LDS)
    "slot0": ([(-1, "g", 0, 7)], True),
    "two-joins": ([(0, 0, 0, 8), (1, 0, 0, 5)], True),
    "three-keys": ([(-1, "g", 0, 4), (0, 0, 0, 8), (1, 0, 0, 5)], True),
    "4096x8-global": ([(-1, "g", 0, 64), (0, 0, 0, 64)], False),
}
FUSED_AGGS_SMALL = [("count_star", -1, None), ("count", -1, "i8"), ("sum", -1, "i8"), ("sum", 1, 1)]
FUSED_AGGS_8 = [("count_star", -1, None), ("count", -1, "i8"), ("sum", -1, "i8"), ("sum", -1, "i16"), ("sum", -1, "i32"),
                ("count", -1, "u32"), ("sum", -1, "u32"), ("sum", 1, 1)]
LAUNCHES = ["resident-1", "resident-4", "morsels", "ranges", "backpressure"]
FUSED_CASES = [(s, src, l) for s in FUSED_SHAPES for src in ("table", "scan") for l in LAUNCHES]


def _fused_want(joins, cols, valid, names, keys, specs, sel):
    pcols = list(cols.values())
    pvalid = [valid.get(c) for c in names]
    rows = Ref(pcols, pvalid, joins, sel).rows()

    def column(sj, sc):
        if sj < 0:
            c = names.index(sc) if isinstance(sc, str) else sc
            v = pvalid[c]
            r = rows[:, 0]
            return pcols[c][r].astype(np.int64), (np.ones(len(r), bool) if v is None else v[r].astype(bool))
        j = joins[sj]
        r = rows[:, 1 + sj]
        v = j.payload_valid[sc]
        return j.payload[sc][r].astype(np.int64), (np.ones(len(r), bool) if v is None else v[r].astype(bool))

    g = np.zeros(len(rows), np.int64)
    ok = np.ones(len(rows), bool)
    n_groups = 1
    for sj, sc, mn, nv in keys:
        val, v = column(sj, sc)
        off = val - mn
        ok &= v & (off >= 0) & (off < nv)
        g = g * nv + np.where(ok, off, 0)
        n_groups *= nv
    want = [[0 if fn != "sum" else None for fn, _, _ in specs] for _ in range(n_groups)]
    gs = g[ok]
    for a, (fn, sj, sc) in enumerate(specs):
        if fn == "count_star":
            cnt = np.bincount(gs, minlength=n_groups)
            for q in range(n_groups):
                want[q][a] = int(cnt[q])
            continue
        val, v = column(sj, sc)
        val, v = val[ok], v[ok]
        cnt = np.bincount(gs[v], minlength=n_groups)
        sums = {}
        for q, x in zip(gs[v].tolist(), val[v].tolist()):
            sums[q] = sums.get(q, 0) + x
        for q in range(n_groups):
            want[q][a] = int(cnt[q]) if fn == "count" else (sums[q] if cnt[q] else None)
    return want, int((~ok).sum()), len(rows)


@pytest.mark.parametrize("shape,source,launch", FUSED_CASES, ids=["-".join(c) for c in FUSED_CASES])
def test_fused_sink_matrix(gpu_ctx, shape, source, launch):
    """the GROUP BY fused into the flat pool against a numpy GROUP BY over the reference row set: group keys on slot 0 and
    on two joins' payloads, 1-3 keys, COUNT(*) / COUNT / SUM over NULL-able signed and unsigned narrow columns with
    negatives, NULL and out-of-domain keys counted in `dropped`; cells in LDS or (4096 groups x 8 aggregates) in global
    memory; whole table or scan-filtered source; every pool launch; two passes add up, reset() zeroes"""
    joins, cols, valid = _fused_star()
    names = list(cols)
    raw_keys, in_lds = FUSED_SHAPES[shape]
    keys = [(sj, names.index(sc) if sj < 0 else sc, mn, nv) for sj, sc, mn, nv in raw_keys]
    specs = FUSED_AGGS_8 if not in_lds else FUSED_AGGS_SMALL
    dspecs = [(fn, sj, 0 if sc is None else (names.index(sc) if sj < 0 else sc)) for fn, sj, sc in specs]
    pcols = list(cols.values())
    pvalid = [valid.get(c) for c in names]
    n = len(pcols[0])
    paths = [[0, 1], [1, 0]]
    ght = [j.device(gpu_ctx) for j in joins]
    pipe = capi.Pipeline(gpu_ctx, pcols, n, [(h, [(-1, j.src)]) for h, j in zip(ght, joins)], paths, probe_valid=pvalid)
    li = pipe.launch_info(True)
    assert li["flat"] == 1
    n_groups = int(np.prod([k[3] for k in keys]))
    words = n_groups * (1 + 2 * len(specs))
    assert (li["lds_bytes_per_workgroup"] + 8 + 8 * words <= 160 * 1024) == in_lds  # (polr_mpx.hip, fused_words)
    sel = None
    if source == "scan":
        _, n_chunks = pipe.scan_filter([(names.index("f"), "<", 60)])
        sel, _ = pipe.fetch_scan()
        assert np.array_equal(sel, np.nonzero(cols["f"] < 60)[0])
    else:
        n_chunks = (n + 1023) // 1024
    want, dropped, n_rows = _fused_want(joins, cols, valid, names, keys, specs, sel)
    assert dropped > 0 and n_rows > 1000
    out = capi.Output(pipe, 1024, 64)
    out.fuse_grouped(keys, dspecs)
    E = {"resident-1": 1, "resident-4": 4, "morsels": 4, "ranges": 2, "backpressure": 2}[launch]
    mpxs = [capi.DeviceMultiplexer(pipe, "backpressure" if launch == "backpressure" else "adaptive_reinit")
            for _ in range(E)]
    if source == "scan":
        for m in mpxs:
            m.use_scan_chunks()

    def one_pass():
        if launch.startswith("resident"):
            capi.run_resident(mpxs, [((e * n_chunks) // E, ((e + 1) * n_chunks) // E) for e in range(E)], out=out,
                              reset=True, finish=True)
        elif launch == "morsels":
            capi.run_resident_morsels(mpxs, 0, n_chunks, morsel_chunks=3, out=out, reset=True, finish=True)
        elif launch == "ranges":
            q = [(i * n_chunks) // 4 for i in range(5)]
            capi.run_resident_ranges(mpxs, [[(q[0], q[1]), (q[2], q[3])], [(q[1], q[2]), (q[3], q[4])]], out=out,
                                     reset=True, finish=True)
        else:
            capi.run_backpressure(mpxs, 0, n_chunks, morsel_chunks=3, out=out)
        stats = capi.finish_many(mpxs)
        k_out = sum(sum(st["stage_out"][p][1] for p in range(2)) for st in stats)
        assert k_out == n_rows  # every tuple went down exactly one join order

    for passes in (1, 2):  # the second pass adds to the cells (no reset in between)
        one_pass()
        vals, counts, got_dropped = out.fused_result()
        assert got_dropped == passes * dropped
        for q in range(n_groups):
            exp = [None if v is None else passes * v for v in want[q]]
            assert vals[q] == exp, "group %d" % q
    assert out.stats()[0] == 0  # nothing was emitted
    out.reset()
    vals, counts, got_dropped = out.fused_result()
    assert got_dropped == 0
    assert all(v == [0 if fn != "sum" else None for fn, _, _ in specs] for v in vals)
    for m in mpxs:
        m.close()
    out.close()
    pipe.close()
    for h in ght:
        h.close()


def test_fused_output_is_refused_by_the_path_kernel_entry_points(gpu_ctx):
    """probe_rounds, probe_rounds_async, mpx.run and run_many would launch the per-round path kernel, which never folds into
    a fused sink: each refuses such an output before enqueueing anything, and the output still works in a pool launch"""
    joins, cols, valid = _fused_star(n=20_000, seed=52)
    names = list(cols)
    pcols = list(cols.values())
    pvalid = [valid.get(c) for c in names]
    n = len(pcols[0])
    ght = [j.device(gpu_ctx) for j in joins]
    pipe = capi.Pipeline(gpu_ctx, pcols, n, [(h, [(-1, j.src)]) for h, j in zip(ght, joins)], [[0, 1]], probe_valid=pvalid)
    keys = [(0, 0, 0, 8)]
    specs = [("count_star", -1, 0), ("sum", -1, names.index("i16"))]
    out = capi.Output(pipe, 1024, 64)
    out.fuse_grouped(keys, specs)
    n_chunks = (n + 1023) // 1024

    def refused(e):
        assert e.value.code == capi.E_UNSUPPORTED and "pool launch" in str(e.value), str(e.value)

    with pytest.raises(capi.PolrError) as e:
        pipe.probe_rounds([(0, n, 0, 1)], out=out)
    refused(e)
    hip = C.CDLL("libamdhip64.so")  # (the HIP runtime the library runs on: a real device buffer for the counts)
    counts_dev = C.c_void_p()
    assert hip.hipMalloc(C.byref(counts_dev), C.c_size_t(64)) == 0
    with pytest.raises(capi.PolrError) as e:
        pipe.probe_rounds_async(capi.make_rounds([(0, n, 0, 1)]), 1, counts_dev, out=out)
    refused(e)
    m = [capi.DeviceMultiplexer(pipe, "adaptive_reinit") for _ in range(2)]
    with pytest.raises(capi.PolrError) as e:
        m[0].run(0, n_chunks, out=out)
    refused(e)
    with pytest.raises(capi.PolrError) as e:
        capi.run_many(m, [(0, n_chunks // 2), (n_chunks // 2, n_chunks)], out=out)
    refused(e)
    gpu_ctx.sync()
    assert hip.hipFree(counts_dev) == 0
    vals, _, dropped = out.fused_result()
    assert dropped == 0 and all(v == [0, None] for v in vals) and out.stats()[0] == 0  # nothing ran
    # the same output in a pool launch
    want, drop, _ = _fused_want(joins, cols, valid, names, keys, [("count_star", -1, None), ("sum", -1, "i16")], None)
    capi.run_resident(m, [(0, n_chunks // 2), (n_chunks // 2, n_chunks)], out=out, reset=True, finish=True)
    capi.finish_many(m)
    vals, _, dropped = out.fused_result()
    assert vals == want and dropped == drop
    for x in m:
        x.close()
    out.close()
    pipe.close()
    for h in ght:
        h.close()
