"""Source side of the pipeline: table scan with pushed-down filters.

CPU part: the oracle restatement of RowGroup::TemplatedScan / ColumnSegment::FilterSelection against
(1) the selection + chunk boundaries the JOB-light fixture is built from -- those reproduce the routing
traces the REFERENCE logged for the same filtered scan (tests/golden/job_light_01.json,
test_oracle_golden.test_job_light_bench_pipeline), which pins vector size, empty-vector skipping and row order --
and (2) a plain numpy statement of the predicate semantics (NULL passes no comparison).
GPU part (-m gpu): polr_pipeline_scan_filter == oracle, bit for bit, through the C ABI.

At the edges of the eight column types (edge_case / edge_constants) the reference is the same numpy statement over
columns of Python ints (astype(object)), so that a constant outside the column's type compares as the number it is; the
oracle is held to it on the CPU and the device to both.  The prefix sum over the vectors is held to numpy_scan at every
level it has (test_device_prefix_scan_levels), and the scan's limits and state transitions in
test_device_scan_limits_* / test_device_rescan_* / test_device_host_selection_*."""
import operator

import numpy as np
import pytest

import common
from common import chunk_bounds, orc, workloads

OPS = ["=", "!=", "<", ">", "<=", ">="]


def numpy_scan(cols, filters, V, valids=None):
    n = len(cols[0])
    keep = np.ones(n, dtype=bool)
    for col, op, const in filters:
        a = cols[col]
        valid = np.ones(n, dtype=bool) if valids is None or valids[col] is None else valids[col].astype(bool)
        if op == "is null":
            keep &= ~valid
            continue
        if op == "is not null":
            keep &= valid
            continue
        r = {"=": operator.eq, "!=": operator.ne, "<": operator.lt, ">": operator.gt, "<=": operator.le,
             ">=": operator.ge}[op](a, const)
        keep &= valid & np.asarray(r, dtype=bool)  # (a column given as Python ints compares to an object array)
    return chunk_bounds(np.nonzero(np.asarray(keep, dtype=bool))[0].astype(np.uint32), n, V)


def random_case(seed, n, dtype, with_nulls):
    rng = np.random.default_rng(seed)
    info = np.iinfo(dtype)
    lo, hi = max(info.min, -50), min(info.max, 50)
    a = rng.integers(lo, hi, size=n, endpoint=True).astype(dtype)
    b = rng.integers(0, 5, size=n).astype(np.uint8)
    va = (rng.random(n) > 0.2).astype(np.uint8) if with_nulls else None
    return [a, b], [va, None]


DTYPES = [np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.int64, np.uint64]
EDGE_SIZES = [(5000, 64), (1025, 1024), (300, 2)]


def edge_values(dtype):
    """what every edge column holds: type min, min + 1, -1 / 0 / 1, max - 1, max and, for an unsigned type, values with
    the top bit set"""
    info = np.iinfo(dtype)
    lo, hi = int(info.min), int(info.max)
    vals = [lo, lo + 1, 0, 1, hi - 1, hi]
    if lo < 0:
        vals += [-1, -2]
    else:
        top = 1 << (info.bits - 1)
        vals += [top, top + 1, top + (top >> 1), hi - 5]
    return sorted(set(vals))


def edge_case(seed, n, dtype, with_nulls):
    """three columns: two of `dtype` drawn over its whole domain with edge_values() planted in both, one small uint8
    column; a 20 % NULL mask on both `dtype` columns in the nullable variant (every planted value stays valid somewhere)"""
    rng = np.random.default_rng(1000 + seed)
    info = np.iinfo(dtype)
    sp = edge_values(dtype)
    cols, valids = [], []
    for _ in range(2):
        a = rng.integers(info.min, info.max, size=n, endpoint=True, dtype=dtype)
        where = rng.choice(n, 8 * len(sp), replace=False)
        a[where] = np.array(sp * 8, dtype=object).astype(dtype)
        v = (rng.random(n) > 0.2).astype(np.uint8) if with_nulls else None
        for x in sp:  # each planted value is seen as a valid row (and, when nullable, as a NULL row too)
            here = np.nonzero(a == dtype(x))[0]
            assert len(here) >= 8
            if v is not None:
                v[here[0]], v[here[1]] = 1, 0
        cols.append(a)
        valids.append(v)
    cols.append(rng.integers(0, 5, size=n).astype(np.uint8))
    valids.append(None)
    return cols, valids


def edge_constants(dtype):
    """type min and max, 0 and -1 (signed), one value just inside each bound, and -- for a type narrower than 64 bits --
    max + 1 and min - 1, which the column's own type cannot hold; uint64: 2^63 - 1 and its neighbours against the values
    above them.  (polr_scan_filter::constant is an int64: a uint64 constant of 2^63 or more has no spelling there.)"""
    info = np.iinfo(dtype)
    lo, hi = int(info.min), int(info.max)
    consts = [lo, hi, lo + 1, hi - 1]
    if lo < 0:
        consts += [0, -1]
    if info.bits < 64:
        consts += [hi + 1, lo - 1]
    if dtype == np.uint64:
        consts += [(1 << 63) - 1, (1 << 63) - 2, 1 << 63]
    return consts


def device_refuses(dtype, const):
    """an unsigned column takes no negative int64 constant -- which is also what a uint64 constant of 2^63 or more is:
    capi.Pipeline.scan_filter and orc.scan_filter store the constant in a ctypes c_int64 field, which keeps the low 64
    bits without a range check (2^64 - 1 arrives as -1).  The oracle turns those bits back into the uint64 for a uint64
    column, so it is still held to numpy there; the device refuses the negative number."""
    return np.iinfo(dtype).min == 0 and (const < 0 or const >= 1 << 63)


def as_ints(cols):
    return [c.astype(object) for c in cols]


def eight_filters(dtype):
    """8 filters over 3 columns, column 0 named three times"""
    info = np.iinfo(dtype)
    lo, hi = int(info.min), min(int(info.max), (1 << 63) - 1)  # (uint64: the largest constant an int64 spells)
    return [(0, ">=", lo + 1), (1, "is not null", 0), (0, "<=", hi - 1), (2, "!=", 3), (1, ">", lo), (0, "!=", 0),
            (1, "<", hi), (2, "<=", 4)]


def edge_filter_sets(dtype, device):
    """every comparison with every edge constant (AND-ed with a filter on the small column), the NULL tests with a
    negative constant, the 8-filter set -> (filters, refused on the device)"""
    sets = []
    for const in edge_constants(dtype):
        for op in OPS:
            sets.append(([(0, op, const), (2, "!=", 3)], device and device_refuses(dtype, const)))
    sets.append(([(0, "is null", -5)], False))
    sets.append(([(1, "is not null", -1), (0, ">", 1)], False))
    sets.append((eight_filters(dtype), False))
    return sets


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("with_nulls", [False, True])
def test_oracle_matches_exact_integers_at_type_edges(dtype, with_nulls):
    """orc_compare at the bounds of every column type, values with the top bit set and constants the column's type cannot
    hold, against comparisons of Python ints"""
    for seed, (n, V) in enumerate(EDGE_SIZES):
        cols, valids = edge_case(seed, n, dtype, with_nulls)
        ints = as_ints(cols)
        n_some = 0
        for flt, _ in edge_filter_sets(dtype, device=False):
            sel, offs = orc.scan_filter(cols, flt, vector_size=V, valids=valids)
            want_sel, want_offs = numpy_scan(ints, flt, V, valids)
            assert np.array_equal(sel, want_sel), (n, V, flt)
            assert np.array_equal(offs, want_offs), (n, V, flt)
            n_some += 0 < len(want_sel) < n
        assert n_some > 10  # (the cases are not all-or-nothing)


def test_oracle_matches_job_light_fixture_inputs():
    import bench
    wl = workloads.job_light_01(scale=0.1)
    cols = list(wl["probe"]["cols"].values())
    names = list(wl["probe"]["cols"].keys())
    sel, offs = orc.scan_filter(cols, [(names.index("company_type_id"), "=", 2)], vector_size=1024)
    want_sel = wl["probe"]["filter_sel"]
    assert np.array_equal(sel, want_sel)
    assert np.array_equal(offs, bench.chunk_offsets_for(want_sel, len(cols[0]), 1024))


@pytest.mark.parametrize("dtype", [np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.int64, np.uint64])
@pytest.mark.parametrize("with_nulls", [False, True])
def test_oracle_matches_numpy(dtype, with_nulls):
    for seed, (n, V) in enumerate([(0, 1024), (1, 1024), (1023, 1024), (1025, 1024), (5000, 64), (4097, 1000), (300, 2)]):
        cols, valids = random_case(seed, n, dtype, with_nulls)
        for op in OPS:
            const = 7 if np.iinfo(dtype).min == 0 else -3
            flt = [(0, op, const), (1, "!=", 3)]
            sel, offs = orc.scan_filter(cols, flt, vector_size=V, valids=valids)
            want_sel, want_offs = numpy_scan(cols, flt, V, valids)
            assert np.array_equal(sel, want_sel), (n, V, op)
            assert np.array_equal(offs, want_offs), (n, V, op)
        for op in ("is null", "is not null"):
            sel, offs = orc.scan_filter(cols, [(0, op, 0)], vector_size=V, valids=valids)
            want_sel, want_offs = numpy_scan(cols, [(0, op, 0)], V, valids)
            assert np.array_equal(sel, want_sel) and np.array_equal(offs, want_offs)


# ---- GPU -------------------------------------------------------------------------------------------
def _device_pipeline(ctx, cols, valids, key=None):
    from polr_amd import capi
    # a one-join pipeline over the columns (the scan does not care about the joins)
    keys = np.arange(16, dtype=np.int32)
    ht = capi.HashTable.from_columns(ctx, [keys], [])
    ht.finalize_hash()
    probe = [np.ascontiguousarray(c) for c in cols] + [np.zeros(len(cols[0]), dtype=np.int32) if key is None else key]
    pv = list(valids) + [None]
    pipe = capi.Pipeline(ctx, probe, len(cols[0]), [(ht, [(-1, len(cols))])], [[0]], probe_valid=pv)
    return pipe, ht


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.int64, np.uint64])
@pytest.mark.parametrize("with_nulls", [False, True])
def test_device_scan_matches_oracle(gpu_ctx, dtype, with_nulls):
    for seed, (n, V) in enumerate([(1, 1024), (1023, 1024), (1025, 1024), (70000, 1024), (5000, 64), (4097, 1000),
                                   (300, 2), (200000, 2048)]):
        cols, valids = random_case(seed, n, dtype, with_nulls)
        pipe, ht = _device_pipeline(gpu_ctx, cols, valids)
        const = 7 if np.iinfo(dtype).min == 0 else -3
        cases = [[(0, op, const), (1, "!=", 3)] for op in OPS] + [[(0, "is null", 0)], [(0, "is not null", 0)], [],
                                                                    [(0, "=", 49), (1, "=", 4), (0, ">", 0)]]
        for flt in cases:
            n_sel, n_chunks = pipe.scan_filter(flt, vector_size=V)
            sel, offs = pipe.fetch_scan()
            want_sel, want_offs = orc.scan_filter(cols, flt, vector_size=V, valids=valids)
            assert n_sel == len(want_sel) and n_chunks == len(want_offs) - 1, (n, V, flt)
            assert np.array_equal(sel, want_sel), (n, V, flt)
            assert np.array_equal(offs, want_offs), (n, V, flt)
        pipe.close()
        ht.close()


@pytest.mark.gpu
def test_device_scan_all_filtered_and_errors(gpu_ctx):
    from polr_amd import capi
    cols, valids = random_case(3, 5000, np.int32, False)
    pipe, ht = _device_pipeline(gpu_ctx, cols, valids)
    assert pipe.scan_filter([(0, ">", 1000)]) == (0, 0)  # nothing survives: no chunk at all
    sel, offs = pipe.fetch_scan()
    assert len(sel) == 0 and list(offs) == [0]
    with pytest.raises(capi.PolrError):
        pipe.scan_filter([(9, "=", 1)])  # no such column
    with pytest.raises(capi.PolrError):
        pipe.scan_filter([(1, "=", -1)])  # negative constant against an unsigned column
    pipe.close()
    ht.close()


@pytest.mark.gpu
@pytest.mark.parametrize("routing", ["adaptive_reinit", "dynamic"])
def test_pipeline_over_device_scan_matches_reference(gpu_ctx, routing):
    """bench.py's pipeline with the filter evaluated on the device: same routing trace and COUNT(*) as the
    reference's run of the SQL (golden), i.e. as with the host-computed selection"""
    from polr_amd import capi
    from test_oracle_golden import job_light_budget
    gold = common.load_golden("job_light_01")
    wl = workloads.job_light_01(scale=0.1)
    names = list(wl["probe"]["cols"].keys())
    cols = list(wl["probe"]["cols"].values())
    joins = capi.build_joins(gpu_ctx, wl)
    pipe = capi.Pipeline(gpu_ctx, cols, len(cols[0]), joins, [[0, 1], [1, 0]])
    n_sel, n_chunks = pipe.scan_filter([(names.index("company_type_id"), "=", 2)])
    assert n_sel == len(wl["probe"]["filter_sel"])
    for launch in ("rounds", "resident"):
        mpx = capi.DeviceMultiplexer(pipe, routing, regret_budget=job_light_budget(routing, len(cols[0])))
        mpx.use_scan_chunks()
        if launch == "resident":
            mpx.run_resident(0, n_chunks)
        else:
            mpx.run(0, n_chunks)
        st = mpx.finish()
        path, tuples, inter = mpx.fetch_log()
        g = gold["routing"][routing]
        assert list(inter) == g["rounds"]
        assert st["num_intermediates"] == g["intms"]
        assert st["input_tuple_count_per_path"] == g["tuple_counts"]
        assert sum(st["stage_out"][p][1] for p in range(2)) == gold["count_star"]
        mpx.close()
    pipe.close()


@pytest.mark.gpu
def test_device_scan_full_size_properties(gpu_ctx):
    """BASELINE configs[1] size: 2.6 M rows -- survivors ascending, exactly the rows that pass, chunk boundaries
    at the 1024-row vectors (size-independent properties; no oracle run needed)"""
    wl = workloads.job_light_01(scale=1.0)
    names = list(wl["probe"]["cols"].keys())
    cols = list(wl["probe"]["cols"].values())
    pipe, ht = _device_pipeline(gpu_ctx, cols, [None] * len(cols))
    ci = names.index("company_type_id")
    n_sel, n_chunks = pipe.scan_filter([(ci, "=", 2)])
    sel, offs = pipe.fetch_scan()
    assert n_sel == int((cols[ci] == 2).sum())
    assert np.all(np.diff(sel.astype(np.int64)) > 0)
    assert np.all(cols[ci][sel] == 2)
    assert offs[0] == 0 and offs[-1] == n_sel and np.all(np.diff(offs.astype(np.int64)) > 0)
    # every chunk lies inside one 1024-row vector, consecutive chunks in different vectors
    first = sel[offs[:-1].astype(np.int64)] // 1024
    last = sel[offs[1:].astype(np.int64) - 1] // 1024
    assert np.array_equal(first, last) and np.all(np.diff(first.astype(np.int64)) > 0)
    pipe.close()
    ht.close()


# ---- the column types' edges --------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("with_nulls", [False, True])
def test_device_scan_at_type_edges(gpu_ctx, dtype, with_nulls):
    """device == oracle == comparisons of Python ints: type bounds, values with the top bit set, constants outside the
    column's type (int8 < 300 holds for every valid row), 8 filters over 3 columns; a constant an unsigned column cannot
    take is refused and leaves the scan before it in place"""
    from polr_amd import capi
    for seed, (n, V) in enumerate(EDGE_SIZES):
        cols, valids = edge_case(seed, n, dtype, with_nulls)
        ints = as_ints(cols)
        pipe, ht = _device_pipeline(gpu_ctx, cols, valids)
        before = None
        for flt, refused in edge_filter_sets(dtype, device=True):
            if refused:
                assert before is not None
                with pytest.raises(capi.PolrError) as e:
                    pipe.scan_filter(flt, vector_size=V)
                assert e.value.code == capi.E_INVALID, (n, V, flt)
                sel, offs = pipe.fetch_scan()
                assert np.array_equal(sel, before[0]) and np.array_equal(offs, before[1]), (n, V, flt)
                continue
            n_sel, n_chunks = pipe.scan_filter(flt, vector_size=V)
            sel, offs = pipe.fetch_scan()
            want_sel, want_offs = numpy_scan(ints, flt, V, valids)
            o_sel, o_offs = orc.scan_filter(cols, flt, vector_size=V, valids=valids)
            assert np.array_equal(o_sel, want_sel) and np.array_equal(o_offs, want_offs), (n, V, flt)
            assert n_sel == len(want_sel) and n_chunks == len(want_offs) - 1, (n, V, flt)
            assert np.array_equal(sel, want_sel), (n, V, flt)
            assert np.array_equal(offs, want_offs), (n, V, flt)
            before = (want_sel, want_offs)
        pipe.close()
        ht.close()


# ---- the prefix sum over the vectors, at every level ---------------------------------------------------
PREFIX_CASES = [
    # name, rows, V, first vector, last vector
    ("two-blocks", 1024 * 64 + 1, 64, None, "full"),  # 1025 vectors, the last of one row
    ("three-blocks", 2048 * 64 + 17, 64, "empty", None),  # 2049 vectors
    ("second-pass-over-the-block-sums", 2 * 1024 * 1024 + 1, 2, None, "full"),  # 1024 * 1024 + 1 vectors: 1025 block sums
    ("longest-vector", 65536 + 3, 65536, "full", "empty"),  # two vectors, 1024 steps of the wave's inner loop
    ("last-vector-of-one-row", 64 * 6 + 1, 64, "full", "full"),
    ("first-vector-empty", 64 * 7, 64, "empty", "full"),
    ("last-vector-empty", 64 * 6 + 5, 64, "full", "empty"),
]


def prefix_case(seed, n, V, first, last):
    """one int8 column for the filter `>= 0`: about 40 % of the vectors hold negative values only (with few vectors: every
    third one), first and last as told"""
    rng = np.random.default_rng(2000 + seed)
    n_vec = (n + V - 1) // V
    a = rng.integers(-128, 128, n).astype(np.int8)
    empty = rng.random(n_vec) < 0.4 if n_vec > 16 else np.arange(n_vec) % 3 == 1
    for v, what in ((0, first), (n_vec - 1, last)):
        if what is not None:
            empty[v] = what == "empty"
            a[v * V] = 1  # (a vector told to be full has a survivor)
    a[empty[np.arange(n) // V]] |= np.int8(-128)
    return a


@pytest.mark.gpu
@pytest.mark.parametrize("name,n,V,first,last", PREFIX_CASES, ids=[c[0] for c in PREFIX_CASES])
def test_device_prefix_scan_levels(gpu_ctx, name, n, V, first, last):
    """selection and chunk boundaries with 2 and 3 blocks of the apply kernel, with 1025 block sums (the carry between two
    passes of the sums kernel), with the longest vector, and with empty / one-row vectors at both ends -- in full against
    numpy_scan; between 10 % and 90 % of the vectors are empty, so chunk c is not vector c"""
    a = prefix_case(PREFIX_CASES.index((name, n, V, first, last)), n, V, first, last)
    flt = [(0, ">=", 0)]
    want_sel, want_offs = numpy_scan([a.astype(np.int64)], flt, V)
    n_vec = (n + V - 1) // V
    assert 0.1 <= (n_vec - (len(want_offs) - 1)) / n_vec <= 0.9
    if first is not None:
        assert (want_sel[0] >= V) == (first == "empty")
    if last is not None:
        assert (want_sel[-1] < (n_vec - 1) * V) == (last == "empty")
    pipe, ht = _device_pipeline(gpu_ctx, [a], [None])
    n_sel, n_chunks = pipe.scan_filter(flt, vector_size=V)
    sel, offs = pipe.fetch_scan()
    assert n_sel == len(want_sel) and n_chunks == len(want_offs) - 1
    assert np.array_equal(sel, want_sel)
    assert np.array_equal(offs, want_offs)
    pipe.close()
    ht.close()


# ---- limits and state transitions -----------------------------------------------------------------------
def _keyed_pipeline(ctx, seed, n, dtype, with_nulls):
    """random_case's columns + a key column two thirds of which find a build row -> pipe, table, columns, validity and
    what a DEFAULT_PATH run over a selection must count"""
    from joinref import Join, Ref
    cols, valids = random_case(seed, n, dtype, with_nulls)
    key = np.random.default_rng(3000 + seed).integers(0, 24, n).astype(np.int32)
    pipe, ht = _device_pipeline(ctx, cols, valids, key=key)
    join = Join(np.arange(16, dtype=np.int32), len(cols))

    def count(sel):
        return Ref(cols + [key], None, [join], sel).stage_counts([0])

    return pipe, ht, cols, valids, count


def _run(m, n_chunks, launch):
    from polr_amd import capi
    if launch == "run":
        m.reset()
        m.run(0, n_chunks)
    elif launch == "run_resident":
        capi.run_resident([m], [(0, n_chunks)], reset=True, finish=True)
    else:
        capi.run_backpressure([m], 0, n_chunks, morsel_chunks=3)
    return m.finish()["stage_out"][0]


LAUNCHES = ["run", "run_resident", "run_backpressure"]


def _refused_as_scanned_again(m, n_chunks):
    from polr_amd import capi
    for launch in LAUNCHES:
        with pytest.raises(capi.PolrError) as e:
            _run(m, n_chunks, launch)
        assert e.value.code == capi.E_INVALID and "scanned again" in str(e.value), launch


@pytest.mark.gpu
def test_device_scan_limits_leave_the_previous_scan(gpu_ctx):
    """vector sizes 1 and 65537, a 9th filter, comparison codes 8 and 9 are refused; after each, fetch_scan returns the
    scan before it and a multiplexer attached to that scan runs and counts as before; 2, 65536 and 8 filters are taken"""
    from polr_amd import capi
    n = 5000
    pipe, ht, cols, valids, count = _keyed_pipeline(gpu_ctx, 11, n, np.int16, True)
    ints = as_ints(cols)
    flt0 = [(0, "<", 20), (1, "!=", 3)]
    n_sel, n_chunks = pipe.scan_filter(flt0, vector_size=64)
    sel0, offs0 = pipe.fetch_scan()
    want_sel, want_offs = numpy_scan(ints, flt0, 64, valids)
    assert np.array_equal(sel0, want_sel) and np.array_equal(offs0, want_offs) and 0 < n_sel < n
    m = capi.DeviceMultiplexer(pipe, "default_path")
    m.use_scan_chunks()
    count0 = count(sel0)
    assert _run(m, n_chunks, "run_resident") == count0 and 0 < count0[0] < n_sel
    nine = [(0, "!=", c) for c in range(9)]
    for flt, V, code in [(flt0, 1, capi.E_INVALID), (flt0, 65537, capi.E_INVALID), (nine, 64, capi.E_UNSUPPORTED),
                         ([(0, 8, 1)], 64, capi.E_INVALID),  # (8: POLR_CMP_STR_EQ, a join condition only)
                         ([(1, "!=", 3), (0, 9, 1)], 64, capi.E_INVALID)]:
        with pytest.raises(capi.PolrError) as e:
            pipe.scan_filter(flt, vector_size=V)
        assert e.value.code == code, (flt, V)
        sel, offs = pipe.fetch_scan()
        assert np.array_equal(sel, sel0) and np.array_equal(offs, offs0), (flt, V)
        for launch in LAUNCHES:
            assert _run(m, n_chunks, launch) == count0, (flt, V, launch)
    for flt, V in [(flt0, 2), (flt0, 65536), (nine[:8], 64)]:
        n_sel, n_chunks = pipe.scan_filter(flt, vector_size=V)
        sel, offs = pipe.fetch_scan()
        want_sel, want_offs = numpy_scan(ints, flt, V, valids)
        assert n_sel == len(want_sel) and n_chunks == len(want_offs) - 1
        assert np.array_equal(sel, want_sel) and np.array_equal(offs, want_offs), (flt, V)
    m.close()
    pipe.close()
    ht.close()


@pytest.mark.gpu
def test_device_scan_refuses_2_to_the_23_vectors(gpu_ctx):
    """2^24 rows of a 1-byte column in vectors of 2: refused before anything is allocated or freed -- the scan before it
    (vectors of 1024) is still there, in full, and its multiplexer still runs"""
    from polr_amd import capi
    n = 1 << 24
    a = np.random.default_rng(12).integers(0, 5, n).astype(np.uint8)
    pipe, ht = _device_pipeline(gpu_ctx, [a], [None])
    flt = [(0, "=", 3)]
    n_sel, n_chunks = pipe.scan_filter(flt, vector_size=1024)
    want_sel, want_offs = numpy_scan([a.astype(np.int64)], flt, 1024)
    sel0, offs0 = pipe.fetch_scan()
    assert np.array_equal(sel0, want_sel) and np.array_equal(offs0, want_offs)
    m = capi.DeviceMultiplexer(pipe, "default_path")
    m.use_scan_chunks()
    assert _run(m, n_chunks, "run_resident") == [n_sel]  # (the key column is 0 throughout: every tuple finds one row)
    with pytest.raises(capi.PolrError) as e:
        pipe.scan_filter(flt, vector_size=2)
    assert e.value.code == capi.E_UNSUPPORTED and "2^23 scan vectors" in str(e.value)
    sel, offs = pipe.fetch_scan()
    assert np.array_equal(sel, sel0) and np.array_equal(offs, offs0)
    assert _run(m, n_chunks, "run_resident") == [n_sel]
    m.close()
    pipe.close()
    ht.close()


@pytest.mark.gpu
def test_device_fetch_scan_without_a_scan(gpu_ctx):
    from polr_amd import capi
    pipe, ht, cols, valids, count = _keyed_pipeline(gpu_ctx, 13, 3000, np.int32, False)
    with pytest.raises(capi.PolrError) as e:
        pipe.fetch_scan()  # a fresh pipeline
    assert e.value.code == capi.E_INVALID
    pipe.scan_filter([(0, ">", 0)])
    sel, _ = pipe.fetch_scan()
    assert np.array_equal(sel, np.nonzero(cols[0] > 0)[0])
    pipe.set_selection(None)  # the whole table again: the scan result is gone
    with pytest.raises(capi.PolrError) as e:
        pipe.fetch_scan()
    assert e.value.code == capi.E_INVALID
    m = capi.DeviceMultiplexer(pipe, "default_path")
    with pytest.raises(capi.PolrError) as e:
        m.use_scan_chunks()
    assert e.value.code == capi.E_INVALID
    assert _run(m, (3000 + 1023) // 1024, "run_resident") == count(None)
    m.close()
    pipe.close()
    ht.close()


@pytest.mark.gpu
def test_device_rescan_grows_and_reuses_the_buffers(gpu_ctx):
    """one pipeline scanned with vectors of 1024, 64, 2 and 1024 rows and different filters (the buffers grow twice while
    the installed selection is the scan's own buffer, then are reused): each result is the reference's; the multiplexer of
    the scan before is refused by every launch until it is attached again, then counts what the reference counts"""
    from polr_amd import capi
    n = 70_000
    pipe, ht, cols, valids, count = _keyed_pipeline(gpu_ctx, 14, n, np.int8, True)
    ref_cols = [c.astype(np.int64) for c in cols]
    m = capi.DeviceMultiplexer(pipe, "default_path")
    steps = [(1024, [(0, "<", -3), (1, "!=", 3)]), (64, [(0, ">=", 10)]), (2, [(0, "is null", 0), (1, "<", 2)]),
             (1024, [(1, "=", 4), (0, "is not null", 0), (0, "!=", 7)])]
    before = None
    for V, flt in steps:
        n_sel, n_chunks = pipe.scan_filter(flt, vector_size=V)
        sel, offs = pipe.fetch_scan()
        want_sel, want_offs = numpy_scan(ref_cols, flt, V, valids)
        o_sel, o_offs = orc.scan_filter(cols, flt, vector_size=V, valids=valids)
        assert np.array_equal(o_sel, want_sel) and np.array_equal(o_offs, want_offs), (V, flt)
        assert n_sel == len(want_sel) and n_chunks == len(want_offs) - 1 and 0 < n_sel < n, (V, flt)
        assert np.array_equal(sel, want_sel) and np.array_equal(offs, want_offs), (V, flt)
        if before is not None:
            assert not np.array_equal(before, want_sel)
            _refused_as_scanned_again(m, min(n_chunks, 1))
        m.use_scan_chunks()
        want_count = count(want_sel)
        for launch in LAUNCHES:
            assert _run(m, n_chunks, launch) == want_count, (V, launch)
        before = want_sel
    m.close()
    pipe.close()
    ht.close()


@pytest.mark.gpu
def test_device_host_selection_after_a_scan(gpu_ctx):
    """set_selection with a host selection after a scan: the scan's multiplexer is refused, a plain one over the host
    selection counts what the reference counts; the next scan_filter (which frees the copy of the host selection the
    pipeline owns) is the reference's again, and so is the run over it"""
    from polr_amd import capi
    n = 40_000
    pipe, ht, cols, valids, count = _keyed_pipeline(gpu_ctx, 15, n, np.int32, True)
    ints = as_ints(cols)
    flt = [(0, ">", -20), (1, "!=", 0)]
    n_sel, n_chunks = pipe.scan_filter(flt, vector_size=64)
    m = capi.DeviceMultiplexer(pipe, "default_path")
    m.use_scan_chunks()
    want_sel, want_offs = numpy_scan(ints, flt, 64, valids)
    assert _run(m, n_chunks, "run_resident") == count(want_sel)
    host_sel = np.sort(np.random.default_rng(16).choice(n, n // 3, replace=False)).astype(np.uint32)
    pipe.set_selection(host_sel)
    _refused_as_scanned_again(m, 1)
    plain = capi.DeviceMultiplexer(pipe, "default_path")
    for launch in LAUNCHES:
        assert _run(plain, (len(host_sel) + 1023) // 1024, launch) == count(host_sel), launch
    plain.close()
    for V, f in [(64, flt), (1024, [(0, "<=", 5)])]:
        n_sel, n_chunks = pipe.scan_filter(f, vector_size=V)
        sel, offs = pipe.fetch_scan()
        want_sel, want_offs = numpy_scan(ints, f, V, valids)
        assert n_sel == len(want_sel) and n_chunks == len(want_offs) - 1
        assert np.array_equal(sel, want_sel) and np.array_equal(offs, want_offs)
        _refused_as_scanned_again(m, 1)
        m.use_scan_chunks()
        for launch in LAUNCHES:
            assert _run(m, n_chunks, launch) == count(want_sel), launch
    m.close()
    pipe.close()
    ht.close()
