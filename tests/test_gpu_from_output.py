"""polr_ht_from_output (HashTable.from_output): the output of pipeline A as the build side of pipeline B, built on the device.

The reference of a chained build side has two parts, neither computed by the code under test: fetch_ids() of output A
indexes A's source columns on the host (numpy), and a TWIN table is built from those host columns with
HashTable.from_columns (VARCHAR: cells and heap blocks from string_blocks, handed over with set_payload_heaps).  Pipeline B
is run over the new table and over the twin: row sets and materialised payloads must be equal, and equal to joinref.Ref over
the host-materialised build side.  Build row r of the new table is output row r of A, so B's build ids index A's fetch_ids.

polr_out_create takes chunk capacities of 64 .. 65536 only: the capacities 1 and 63 of the chunk-edge cases do not exist (the
test asserts the refusal) and chunks that HOLD 1 and 63 rows stand in for them, next to the capacities 64, 65 and 1000.
The refusal of an output of 2^32 - 16 rows or more is checked where it is decided, in tests/test_fromout_plan.py: such an
output would take minutes to produce."""
import ctypes as C

import numpy as np
import pytest

import buildside
from joinref import MAX_WAVE_CHUNKS, Join, Ref, device_rows, sort_rows
from polr_amd import capi
from test_gpu_group_varchar import dirty_padding
from test_gpu_sink_matrix import string_blocks

pytestmark = pytest.mark.gpu


# ---- pipeline A and what the host knows of it -------------------------------------------------------------------------------
class Source:
    """pipeline A: probe columns x joins (joinref.Join), run into an Output; cols[(src_join, src_col)] = (array or [bytes],
    validity or None) of every column a reference may name"""

    def __init__(self, ctx, pcols, pvalid, joins, cap=64, engine="path", strings=None, heaps=True, run=True, rounds=None,
                 max_chunks=None):
        self.ctx, self.joins, self.n = ctx, joins, len(pcols[0])
        self.cols = {(-1, i): (c, None if pvalid is None else pvalid[i]) for i, c in enumerate(pcols)}
        for x, j in enumerate(joins):
            for i, p in enumerate(j.payload):
                self.cols[(x, i)] = (p, j.payload_valid[i])
        # strings: {(src_join, src_col): ([bytes], validity, n_blocks)} -- the numpy column at that place holds the cells
        self.keep = []
        dev_p, dev_j = list(pcols), [list(j.payload) for j in joins]
        for (sj, sc), (vals, valid, n_blocks) in (strings or {}).items():
            cells, blocks = string_blocks(vals, valid, n_blocks, seed=17 * sc + sj + 40)
            dirty_padding(cells, vals, valid, np.random.default_rng(sc))
            self.keep.append((cells, blocks))
            self.cols[(sj, sc)] = (vals, valid)
            if sj < 0:
                dev_p[sc] = cells
            else:
                dev_j[sj][sc] = cells
        self.hts = []
        for x, j in enumerate(joins):
            ht = capi.HashTable.from_columns(ctx, [j.keys], dev_j[x], key_valid=[j.valid], payload_valid=j.payload_valid)
            for (sj, sc), (_v, _ok, _nb) in (strings or {}).items():
                if sj == x and heaps:
                    ht.set_payload_heaps(sc, [b for c, b in self.keep if c is dev_j[x][sc]][0])
            if j.perfect is not None:
                assert ht.finalize_perfect(*j.perfect)
            else:
                ht.finalize_hash()
            self.hts.append(ht)
        k = len(joins)
        paths = [list(range(k)), list(range(k))[::-1]] if k > 1 else [[0]]
        self.pipe = capi.Pipeline(ctx, dev_p, self.n, [(h, [(-1, j.src)]) for h, j in zip(self.hts, joins)], paths,
                                  probe_valid=[self.cols[(-1, i)][1] for i in range(len(pcols))])
        for (sj, sc), _ in (strings or {}).items():
            if sj < 0 and heaps:
                self.pipe.set_probe_heaps(sc, [b for c, b in self.keep if c is dev_p[sc]][0])
        self.flat = self.pipe.launch_info(True)["flat"]
        self.want = sort_rows(Ref(pcols, pvalid, joins).rows())
        self.out = capi.Output(self.pipe, cap, max_chunks or len(self.want) // cap + 1 + MAX_WAVE_CHUNKS)
        if run:
            self.run(engine, rounds)

    def run(self, engine, rounds=None):
        if engine == "path":
            for r in rounds or [(0, self.n)]:
                self.pipe.probe_rounds([(r[0], r[1], 0, 1)], out=self.out)
        else:
            mx = capi.DeviceMultiplexer(self.pipe, "default_path")
            capi.run_resident([mx], [(0, (self.n + 1023) // 1024)], out=self.out, reset=True, finish=True)
            mx.finish()
            mx.close()
        self.rows = device_rows(self.out.fetch_ids(), self.joins)  # output row -> (probe row, build row per join)
        assert np.array_equal(sort_rows(self.rows), self.want)

    def host(self, ref):
        """column `ref` over the output rows, in the order of fetch_ids -> (numpy array or [bytes], validity uint8)"""
        vals, valid = self.cols[ref]
        r = self.rows[:, 1 + ref[0]] if ref[0] >= 0 else self.rows[:, 0]
        ok = np.ones(len(r), np.uint8) if valid is None else np.asarray(valid)[r].astype(np.uint8)
        return ([vals[i] for i in r.tolist()] if isinstance(vals, list) else vals[r]), ok

    def close(self):
        self.out.close()
        self.pipe.close()
        for h in self.hts:
            h.close()


def twin_table(ctx, src, keys, payload):
    """the same build side from the host: from_columns over A's columns indexed by A's fetch_ids"""
    kc = [src.host(r) for r in keys]
    pc, pv, heaps, keep = [], [], {}, []
    for i, r in enumerate(payload):
        vals, ok = src.host(r)
        if isinstance(vals, list):
            cells, blocks = string_blocks(vals, ok, 2, seed=i)
            keep.append((cells, blocks))
            heaps[i] = blocks
            vals = cells
        pc.append(vals)
        pv.append(ok)
    ht = capi.HashTable.from_columns(ctx, [c for c, _ in kc], pc, key_valid=[v for _, v in kc], payload_valid=pv)
    for i, blocks in heaps.items():
        ht.set_payload_heaps(i, blocks)
    ht._keep = keep
    return ht


def probe_b(ctx, ht, pk_cols, pk_valid, payload_dtypes, cap=64):
    """pipeline B over `ht` -> (ids sorted by (probe row, build id), [(data, valid) per payload column] in that order);
    payload_dtypes[i] None: a VARCHAR column, decoded to [bytes or None]"""
    n = len(pk_cols[0])
    pipe = capi.Pipeline(ctx, pk_cols, n, [(ht, [(-1, i) for i in range(len(pk_cols))])], [[0]], probe_valid=pk_valid)
    out = capi.Output(pipe, cap, 40 * n // cap + 1 + MAX_WAVE_CHUNKS)
    pipe.probe_rounds([(0, n, 0, 1)], out=out)
    ids = out.fetch_ids().astype(np.int64)
    order = np.lexsort(ids.T[::-1])
    mats = []
    for i, dt in enumerate(payload_dtypes):
        if dt is None:
            s = out.materialize_strings(0, i)
            mats.append([s[j] for j in order.tolist()])
        else:
            d, v = out.materialize(0, i, dt)
            mats.append((d[order], v[order]))
    out.close()
    pipe.close()
    return ids[order], mats


def same(a, b):
    if isinstance(a, list):
        return a == b
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def dtypes_of(src, payload):
    return [None if isinstance(src.cols[r][0], list) else src.cols[r][0].dtype for r in payload]


def finalize(ht, how, key_flags=()):
    """how: "hash", ("perfect", min, max) or ("auto", min, max) -> the table's kind"""
    for c, f in enumerate(key_flags):
        if f:
            ht.set_key_flags(c, f)
    if how == "hash":
        ht.finalize_hash()
    elif how[0] == "auto":
        assert ht.finalize_auto(*how[1:]) == ht.info()["kind"]
    else:
        assert ht.finalize_perfect(*how[1:])
    return ht.info()["kind"]


def chain(ctx, src, keys, payload, pk_cols, pk_valid=None, how="hash", key_flags=(), against_ref=True):
    """from_output vs the twin through pipeline B, and vs joinref.Ref for a single plain key -> (ids, mats, n_rows kept)"""
    new = capi.HashTable.from_output(src.out, keys, payload)
    twin = twin_table(ctx, src, keys, payload)
    n_out = len(src.rows)
    assert new.info()["kind"] == 0 and new.info()["n_keys"] == len(keys)
    kinds = [finalize(t, how, key_flags) for t in (new, twin)]
    assert kinds[0] == kinds[1]
    assert new.info()["n_rows"] == twin.info()["n_rows"]
    dts = dtypes_of(src, payload)
    ids, mats = probe_b(ctx, new, pk_cols, pk_valid, dts)
    ids_t, mats_t = probe_b(ctx, twin, pk_cols, pk_valid, dts)
    assert np.array_equal(ids, ids_t) and len(ids) > 0
    for a, b in zip(mats, mats_t):
        assert same(a, b)
    if against_ref:
        kv, kok = src.host(keys[0])
        jb = Join(kv, 0, how[1:] if kinds[0] == 1 else None, kok)
        rows = sort_rows(Ref([pk_cols[0]], pk_valid, [jb]).rows())
        got = sort_rows(device_rows(ids, [jb]))
        assert np.array_equal(got, rows)
        build_rows = device_rows(ids, [jb])[:, 1]
        assert build_rows.max() < n_out
        for (vals, ok), r, m in zip([src.host(r) for r in payload], payload, mats):
            if isinstance(vals, list):
                assert m == [vals[b] if ok[b] else None for b in build_rows.tolist()]
            else:
                assert np.array_equal(m[1], ok[build_rows]) and np.array_equal(m[0], np.where(ok[build_rows], vals[build_rows], 0))
        # B's build ids index A's fetch_ids: the source row behind the key cell is the one that holds the probed value
        key_src_rows = src.rows[build_rows, 1 + keys[0][0]] if keys[0][0] >= 0 else src.rows[build_rows, 0]
        assert np.array_equal(src.cols[keys[0]][0][key_src_rows], pk_cols[0][ids[:, 0]])
    kept = new.info()["n_rows"]
    new.close()
    twin.close()
    return ids, mats, kept


# ---- 1. chain, generic pipeline ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ["path", "generic"], ids=["probe_rounds", "run_resident"])
def test_chain_generic_pipeline(gpu_ctx, engine):
    rng = np.random.default_rng(1)
    n, nb0, nk1 = 3000, 500, 300
    reps = rng.integers(1, 6, nk1)  # 1-5 build rows per key
    k1 = rng.permutation(np.repeat(np.arange(nk1, dtype=np.int32), reps))
    j0 = Join(rng.permutation(nb0).astype(np.int32), 0, payload=[rng.integers(-3000, 3000, nb0).astype(np.int16)],
              payload_valid=[(rng.random(nb0) > 0.2).astype(np.uint8)])
    j1 = Join(k1, 1, payload=[rng.permutation(len(k1)).astype(np.int32), k1.copy()], payload_valid=[None, None])
    pcols = [rng.integers(-20, nb0 + 20, n).astype(np.int32), rng.integers(-10, nk1 + 30, n).astype(np.int32),
             rng.integers(-(1 << 62), 1 << 62, n).astype(np.int64)]
    pvalid = [None, None, (rng.random(n) > 0.1).astype(np.uint8)]
    src = Source(gpu_ctx, pcols, pvalid, [j0, j1], cap=64, engine=engine)
    assert src.flat == 0 and len(src.rows) > 3000
    n_rows, n_chunks, _ = src.out.stats()
    assert n_chunks * 64 > n_rows  # (partly filled chunks)
    pk2 = rng.integers(-30, len(k1) + 30, 2000).astype(np.int32)
    ids, mats, kept = chain(gpu_ctx, src, [(1, 0)], [(-1, 2), (0, 0), (1, 1)], [pk2])
    assert kept == n_rows and len(ids) > 2000 and not mats[1][1].all() and not mats[0][1].all()
    src.close()


# ---- 2. chain, flat pipeline ------------------------------------------------------------------------------------------------
def test_chain_flat_pipeline(gpu_ctx):
    rng = np.random.default_rng(2)
    n, nb = 3000, 400
    j0 = Join(rng.permutation(nb).astype(np.int32), 0, (0, nb - 1), payload=[rng.integers(0, 50, nb).astype(np.int32)],
              payload_valid=[None])
    j1 = Join(rng.permutation(nb).astype(np.int32), 1, (0, nb - 1), payload=[rng.integers(-9, 9, nb).astype(np.int64)],
              payload_valid=[(rng.random(nb) > 0.2).astype(np.uint8)])
    pcols = [rng.integers(-20, nb + 20, n).astype(np.int32), rng.integers(-20, nb + 20, n).astype(np.int32),
             rng.permutation(n).astype(np.int32)]
    src = Source(gpu_ctx, pcols, None, [j0, j1], cap=64, engine="pool")
    assert src.flat == 1 and len(src.rows) > 2000  # two perfect tables, run by the pool launch: build ids are key offsets
    pk2 = rng.integers(-30, n + 30, 2000).astype(np.int32)
    payload = [(0, 0), (1, 0), (-1, 0)]
    # a unique key (the probe table's row number column): a perfect table, and whatever finalize_auto picks
    chain(gpu_ctx, src, [(-1, 2)], payload, [pk2], how=("perfect", 0, n - 1))
    chain(gpu_ctx, src, [(-1, 2)], payload, [pk2], how=("auto", 0, n - 1))
    # a duplicate key: POLR_E_DUPLICATE, the handle stays un-finalized, finalize_hash works
    new = capi.HashTable.from_output(src.out, [(0, 0)], payload)
    assert new.finalize_perfect(0, 49) is False and new.info()["kind"] == 0
    new.close()
    pk3 = rng.integers(-5, 55, 300).astype(np.int32)
    chain(gpu_ctx, src, [(0, 0)], payload, [pk3])
    src.close()


# ---- 3. cell matrix ---------------------------------------------------------------------------------------------------------
DTS = [np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.int64, np.uint64]
_MATRIX = {}


def matrix_source(ctx):
    """probe columns: pk, then every width signed and unsigned without (1..8) and with (9..16) a validity array, values from
    a small domain (they serve as keys); a repeated-key join with a payload of its own"""
    if "m" not in _MATRIX:
        rng = np.random.default_rng(3)
        n, nk = 1500, 200
        bk = rng.permutation(np.repeat(np.arange(nk, dtype=np.int32), 2))
        j = Join(bk, 0, payload=[rng.integers(0, 40, len(bk)).astype(np.uint16), rng.integers(-40, 40, len(bk)).astype(np.int64)],
                 payload_valid=[(rng.random(len(bk)) > 0.15).astype(np.uint8), None])
        pcols = [rng.integers(-10, nk + 10, n).astype(np.int32)]
        pvalid = [None]
        for with_valid in (False, True):
            for dt in DTS:
                lo = -20 if np.dtype(dt).kind == "i" else 0
                pcols.append(rng.integers(lo, lo + 40, n).astype(dt))
                pvalid.append((rng.random(n) > 0.15).astype(np.uint8) if with_valid else None)
        _MATRIX["m"] = Source(ctx, pcols, pvalid, [j], cap=64)
    return _MATRIX["m"]


@pytest.fixture(scope="module", autouse=True)
def _close_matrix():
    yield
    for s in _MATRIX.values():
        s.close()
    _MATRIX.clear()


ALL_PAYLOAD = [(-1, i) for i in range(1, 17)] + [(0, 0), (0, 1)]


@pytest.mark.parametrize("key_col", [9, 12, 13, 16, 2, 7], ids=["i8-valid", "u16-valid", "i32-valid", "u64-valid", "u8", "i64"])
def test_cell_matrix_every_width_as_payload_and_key(gpu_ctx, key_col):
    src = matrix_source(gpu_ctx)
    rng = np.random.default_rng(key_col)
    dt = src.cols[(-1, key_col)][0].dtype
    lo = -25 if dt.kind == "i" else 0
    pk = rng.integers(lo, lo + 50, 400).astype(dt)
    pv = (rng.random(400) > 0.1).astype(np.uint8)
    ids, mats, kept = chain(gpu_ctx, src, [(-1, key_col)], ALL_PAYLOAD, [pk], [pv])
    ok = src.host((-1, key_col))[1]
    assert kept == int(ok.sum()) and (kept < len(ok)) == (key_col >= 9)  # NULL key rows are dropped
    # NULL cells come through in every column that has them (the key's own column aside: its NULL rows are gone)
    assert len(mats) == 18 and all(m[1].all() for m in mats[:8])
    assert all(not m[1].all() for i, m in enumerate(mats[8:17], 8) if i != key_col - 1)


@pytest.mark.parametrize("key_cols", [(3, 10), (12, 1, 6, 15)], ids=["2-keys", "4-keys"])
@pytest.mark.parametrize("null_equal", [False, True], ids=["null-drops", "null-equal"])
def test_cell_matrix_composite_keys_and_null_keys(gpu_ctx, key_cols, null_equal):
    """composite keys of 2 and 4 columns of mixed widths; a row with a NULL key is dropped, and kept under KEY_NULL_EQUAL
    where a NULL probe key finds it; the key columns are named again as payload, one of them twice"""
    src = matrix_source(gpu_ctx)
    rng = np.random.default_rng(sum(key_cols))
    keys = [(-1, c) for c in key_cols]
    # probe B with rows of A's own output (so composite keys do match), shuffled, NULLs where A had them
    take = rng.integers(0, len(src.rows), 500)
    host = [src.host(k) for k in keys]
    pk = [np.ascontiguousarray(v[take]) for v, _ in host]
    pv = [np.ascontiguousarray(ok[take]) for _, ok in host]
    flags = [capi.KEY_NULL_EQUAL if null_equal else 0] * len(keys)
    payload = keys + [keys[1], (0, 1), keys[1]]
    ids, mats, kept = chain(gpu_ctx, src, keys, payload, pk, pv, key_flags=flags, against_ref=False)
    all_ok = np.ones(len(src.rows), bool)
    for _, ok in host:
        all_ok &= ok.astype(bool)
    assert not all_ok.all()
    assert kept == (len(src.rows) if null_equal else int(all_ok.sum()))
    # exact reference of the row set: composite keys reduced to codes (buildside.key_codes)
    bc, bok, pc, pok = buildside.key_codes([v for v, _ in host], [ok for _, ok in host], pk, pv, [null_equal] * len(keys))
    jb = Join(bc, 0, None, bok.astype(np.uint8))
    want = sort_rows(Ref([pc], [pok.astype(np.uint8)], [jb]).rows())
    assert np.array_equal(sort_rows(ids), want)
    null_probe = ~np.logical_and.reduce([v.astype(bool) for v in pv])
    assert null_probe.any() and bool(np.isin(ids[:, 0], np.nonzero(null_probe)[0]).any()) == null_equal
    assert same(mats[1], mats[len(keys)]) and same(mats[1], mats[len(keys) + 2])  # the same column three times


# ---- 4. chunk edges ---------------------------------------------------------------------------------------------------------
def edge_source(ctx, n, cap, hit=True, run=True, rounds=None):
    rng = np.random.default_rng(n + cap)
    nb = 64
    j = Join(np.arange(nb, dtype=np.int32), 0, payload=[rng.integers(-99, 99, nb).astype(np.int32)], payload_valid=[None])
    pcols = [(rng.integers(0, nb, n) if hit else rng.integers(nb, 2 * nb, n)).astype(np.int32), rng.permutation(n).astype(np.int32)]
    return Source(ctx, pcols, None, [j], cap=cap, run=run, rounds=rounds, max_chunks=n // cap + 64)


EDGES = {"cap64-multiple": (4 * 64, 64), "cap65": (1000, 65), "cap65-multiple": (3 * 65, 65), "cap1000": (2500, 1000),
         "cap1000-multiple": (2000, 1000), "cap64": (1000, 64), "one-row": (1, 64)}


@pytest.mark.parametrize("case", list(EDGES))
def test_chunk_edges_rows_equal_the_twin(gpu_ctx, case):
    n, cap = EDGES[case]
    src = edge_source(gpu_ctx, n, cap)
    assert len(src.rows) == n  # (every probe row meets its one build row)
    pk = np.arange(-2, n + 2, dtype=np.int32)
    ids, mats, kept = chain(gpu_ctx, src, [(-1, 1)], [(0, 0), (-1, 0)], [pk])
    assert kept == n and len(ids) == n
    src.close()


def test_chunk_edges_chunks_of_1_and_63_rows(gpu_ctx):
    """chunk capacities below 64 do not exist (polr_out_create refuses them); chunks that hold 1, 63, 64 and 65 - 64 rows do:
    every probe_rounds call starts chunks of its own"""
    src = edge_source(gpu_ctx, 1 + 63 + 64 + 65, 64, rounds=[(0, 1), (1, 63), (64, 64), (128, 65)])
    for cap in (1, 63):
        with pytest.raises(capi.PolrError) as e:
            capi.Output(src.pipe, cap, 16)
        assert e.value.code == capi.E_INVALID
    n_rows, n_chunks, _ = src.out.stats()
    assert n_rows == 193 and n_chunks >= 5
    chain(gpu_ctx, src, [(-1, 1)], [(0, 0), (-1, 0)], [np.arange(-2, 200, dtype=np.int32)])
    src.close()


@pytest.mark.parametrize("filled", [True, False], ids=["zero-rows", "never-filled"])
def test_empty_output_gives_a_table_of_no_rows(gpu_ctx, filled):
    src = edge_source(gpu_ctx, 500, 64, hit=False, run=filled)
    if filled:
        assert len(src.rows) == 0
    new = capi.HashTable.from_output(src.out, [(-1, 1)], [(0, 0), (-1, 0)])
    assert new.info()["n_rows"] == 0 and new.info()["kind"] == 0
    new.finalize_hash()
    src.close()
    pk = np.arange(0, 500, dtype=np.int32)
    pipe = capi.Pipeline(gpu_ctx, [pk], len(pk), [(new, [(-1, 0)])], [[0]])
    out = capi.Output(pipe, 64, 64)
    counts = pipe.probe_rounds([(0, len(pk), 0, 1)], out=out)
    assert counts.sum() == 0 and out.stats()[0] == 0
    out.close()
    pipe.close()
    new.close()


# ---- 5. VARCHAR -------------------------------------------------------------------------------------------------------------
POOL = [b"", b"a", b"abcd", b"hello world", b"x" * 12, b"y" * 13, b"UNITED STATES", b"Q" * 100, bytes(range(256)) * 19 + b"z" * 136,
        b"abcdefghijkl", b"abcdefghijklm", b"\x00" * 12, b"\xff" * 13]
assert len(POOL[8]) == 5000 and {12, 13} <= {len(v) for v in POOL}


def string_source(ctx, seed, heaps=True, pool=POOL):
    """probe (pk, p_g key domain, p_s VARCHAR in two heap blocks) x a repeated-key join with payload (b_s VARCHAR, b_i)"""
    rng = np.random.default_rng(seed)
    n, nk = 2000, 150
    bk = rng.permutation(np.repeat(np.arange(nk, dtype=np.int32), 2))
    b_s = [pool[i] for i in rng.integers(0, len(pool), len(bk))]
    b_ok = (rng.random(len(bk)) > 0.15).astype(np.uint8)
    p_s = [pool[i] for i in rng.integers(0, len(pool), n)]
    p_ok = (rng.random(n) > 0.15).astype(np.uint8)
    j = Join(bk, 0, payload=[np.zeros(len(bk), "V16"), rng.integers(-5, 5, len(bk)).astype(np.int32)], payload_valid=[b_ok, None])
    pcols = [rng.integers(0, nk, n).astype(np.int32), rng.integers(0, 300, n).astype(np.int32), np.zeros(n, "V16")]
    return Source(ctx, pcols, [None, None, p_ok], [j], cap=64, strings={(-1, 2): (p_s, p_ok, 2), (0, 0): (b_s, b_ok, 3)}, heaps=heaps)


def test_varchar_columns_outlive_their_sources(gpu_ctx):
    rng = np.random.default_rng(5)
    src = string_source(gpu_ctx, 50)
    assert np.bincount(src.rows[:, 1]).max() >= 2  # one build row behind many output rows: each gets its own heap copy
    keys, payload = [(-1, 1)], [(-1, 2), (0, 0), (0, 1)]
    new = capi.HashTable.from_output(src.out, keys, payload)
    twin = twin_table(gpu_ctx, src, keys, payload)
    # (a table from an output counts as rebased: a heap of the caller's is refused)
    with pytest.raises(capi.PolrError) as e:
        new.set_payload_heap(0, np.zeros(64, np.uint8))
    assert e.value.code == capi.E_INVALID
    host = [src.host(r) for r in payload]
    kv, kok = src.host(keys[0])
    for long_needed in host[:2]:
        assert any(ok and len(v) == 5000 for v, ok in zip(*long_needed)) and not all(long_needed[1])
    # sorted dictionary codes of the build-side VARCHAR column: the twin's
    codes = [t.encode_dictionary(1, sorted=True) for t in (new, twin)]
    assert codes[0] == codes[1] and codes[0][1] == len({v for v, ok in zip(*host[1]) if ok})
    assert new.dictionary(codes[0][0], str_cap=1 << 16) == twin.dictionary(codes[1][0], str_cap=1 << 16) == sorted({v for v, ok in zip(*host[1]) if ok})
    new.finalize_hash()
    twin.finalize_hash()
    src.close()  # output A, its pipeline, its source tables
    src.keep.clear()
    pk = rng.integers(-10, 310, 400).astype(np.int32)
    jb = Join(kv, 0, None, kok)
    want_rows = sort_rows(Ref([pk], None, [jb]).rows())
    dts = [None, None, np.int32, np.uint32]
    ids, mats = probe_b(gpu_ctx, new, [pk], None, dts)
    ids_t, mats_t = probe_b(gpu_ctx, twin, [pk], None, dts)
    assert np.array_equal(ids, want_rows) and np.array_equal(ids_t, want_rows) and len(ids) > 1000
    b = ids[:, 1].tolist()
    for c in (0, 1):
        vals, ok = host[c]
        want = [vals[r] if ok[r] else None for r in b]
        assert mats[c] == want and mats_t[c] == want
    assert same(mats[2], mats_t[2]) and same(mats[3], mats_t[3])
    # the string MIN / MAX sink over B reads the new table's own heap
    pipe = capi.Pipeline(gpu_ctx, [pk], len(pk), [(new, [(-1, 0)])], [[0]])
    out = capi.Output(pipe, 64, 40 * len(pk) // 64 + 1 + MAX_WAVE_CHUNKS)
    pipe.probe_rounds([(0, len(pk), 0, 1)], out=out)
    for c in (0, 1):
        live = [v for v in mats[c] if v is not None]
        assert out.aggregate_string("min", 0, c, cap=8192) == min(live) and out.aggregate_string("max", 0, c, cap=8192) == max(live)
    out.close()
    pipe.close()
    new.close()
    twin.close()


def test_varchar_heap_never_came(gpu_ctx):
    live0 = capi.device_bytes_live()
    src = string_source(gpu_ctx, 51, heaps=False)
    live1 = capi.device_bytes_live()
    for ref in [(-1, 2), (0, 0)]:
        h = C.c_void_p(0xDEAD)
        rc = gpu_ctx.L.polr_ht_from_output(src.out.h, None, capi._out_col_refs([(-1, 1)]), 1, capi._out_col_refs([(0, 1), ref]), 2, C.byref(h))
        assert rc == capi.E_INVALID and not h.value
        assert "heap was never put on the device" in gpu_ctx.L.polr_last_error(gpu_ctx.h).decode()
        assert capi.device_bytes_live() == live1
    src.close()
    # the same columns holding inline strings only need no heap
    inline = [v for v in POOL if len(v) <= 12]
    src = string_source(gpu_ctx, 52, heaps=False, pool=inline)
    pk = np.arange(-5, 305, dtype=np.int32)
    chain(gpu_ctx, src, [(-1, 1)], [(-1, 2), (0, 0)], [pk])
    src.close()
    assert capi.device_bytes_live() == live0


# ---- 6. ownership -----------------------------------------------------------------------------------------------------------
def test_ownership_and_accounting(gpu_ctx):
    live0 = capi.device_bytes_live()
    src = string_source(gpu_ctx, 60)
    n = len(src.rows)
    live1 = capi.device_bytes_live()
    new = capi.HashTable.from_output(src.out, [(-1, 1)], [(-1, 2), (0, 1), (0, 0)])
    heap = [sum(len(v) for v, ok in zip(*src.host(r)) if ok and len(v) > 12) for r in [(-1, 2), (0, 0)]]
    def up(x):
        return (x + 255) // 256 * 256

    # every byte the table holds: the cells and validity arrays (one allocation, each array at a multiple of 256 bytes) and
    # the two packed heaps as counted here, plus the descriptors of its columns (a few dozen bytes each)
    own = sum(up(n * w) + up(n) for w in (4, 16, 4, 16)) + sum(heap)
    assert own < new.info()["device_bytes"] <= own + 256
    assert capi.device_bytes_live() - live1 == new.info()["device_bytes"]
    new.close()
    assert capi.device_bytes_live() == live1
    # a table without VARCHAR columns clones like any other (export -> alloc_like -> device copies)
    new = capi.HashTable.from_output(src.out, [(-1, 1)], [(0, 1), (-1, 0)])
    new.finalize_hash()
    kv, kok = src.host((-1, 1))
    src.close()
    twin = buildside.clone(gpu_ctx, new)
    pk = np.arange(-5, 305, dtype=np.int32)
    dts = [np.int32, np.int32]
    ids, mats = probe_b(gpu_ctx, new, [pk], None, dts)
    new.close()
    ids_c, mats_c = probe_b(gpu_ctx, twin, [pk], None, dts)
    assert np.array_equal(ids, ids_c) and all(same(a, b) for a, b in zip(mats, mats_c))
    assert np.array_equal(ids, sort_rows(Ref([pk], None, [Join(kv, 0, None, kok)]).rows())) and len(ids) > 1000
    twin.close()
    assert capi.device_bytes_live() == live0


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------
def raw_call(ctx, out_h, keys, n_keys, payload, n_payload, want_out=True):
    h = C.c_void_p(0xDEAD)
    rc = ctx.L.polr_ht_from_output(out_h, None, None if keys is None else capi._out_col_refs(keys), n_keys,
                                   None if payload is None else capi._out_col_refs(payload), n_payload, C.byref(h) if want_out else None)
    return rc, h.value


def test_refusals(gpu_ctx):
    src = matrix_source(gpu_ctx)
    k = [(-1, 5)]
    live0 = capi.device_bytes_live()
    many = [(-1, 1 + i % 16) for i in range(63)]
    cases = {
        "NULL output": ((None, k, 1, [], 0), capi.E_INVALID),
        "NULL keys": ((src.out.h, None, 1, [], 0), capi.E_INVALID),
        "NULL payload with a count": ((src.out.h, k, 1, None, 2), capi.E_INVALID),
        "key reference out of range": ((src.out.h, [(-1, 17)], 1, [], 0), capi.E_INVALID),
        "key join out of range": ((src.out.h, [(1, 0)], 1, [], 0), capi.E_INVALID),
        "payload reference out of range": ((src.out.h, k, 1, [(0, 2)], 1), capi.E_INVALID),
        "no keys": ((src.out.h, k, 0, [], 0), capi.E_UNSUPPORTED),
        "five keys": ((src.out.h, k * 5, 5, [], 0), capi.E_UNSUPPORTED),
        "63 payload columns": ((src.out.h, k, 1, many, 63), capi.E_UNSUPPORTED),
    }
    for what, (args, code) in cases.items():
        rc, h = raw_call(gpu_ctx, *args)
        assert rc == code and not h, what
        assert capi.device_bytes_live() == live0, what
    rc, _ = raw_call(gpu_ctx, src.out.h, k, 1, [], 0, want_out=False)
    assert rc == capi.E_INVALID and capi.device_bytes_live() == live0
    # the limits themselves are fine: 4 keys, 62 payload columns
    new = capi.HashTable.from_output(src.out, [(-1, 5), (-1, 1), (-1, 3), (-1, 7)], many[:62])
    assert new.info()["n_keys"] == 4
    new.close()
    # a key wider than 8 bytes
    s = string_source(gpu_ctx, 70)
    live1 = capi.device_bytes_live()
    rc, h = raw_call(gpu_ctx, s.out.h, [(-1, 2)], 1, [], 0)
    assert rc == capi.E_UNSUPPORTED and not h and capi.device_bytes_live() == live1
    assert "VARCHAR join keys" in gpu_ctx.L.polr_last_error(gpu_ctx.h).decode()
    s.close()


def test_refuses_an_output_with_a_fused_sink(gpu_ctx):
    rng = np.random.default_rng(8)
    n, nb = 2000, 100
    j0 = Join(rng.permutation(nb).astype(np.int32), 0, (0, nb - 1), payload=[rng.integers(0, 8, nb).astype(np.int32)], payload_valid=[None])
    j1 = Join(rng.permutation(nb).astype(np.int32), 1, (0, nb - 1), payload=[rng.integers(0, 8, nb).astype(np.int32)], payload_valid=[None])
    pcols = [rng.integers(0, nb, n).astype(np.int32), rng.integers(0, nb, n).astype(np.int32)]
    src = Source(gpu_ctx, pcols, None, [j0, j1], run=False)
    assert src.flat == 1
    fused = capi.Output(src.pipe, 1024, 64)
    fused.fuse_grouped([(0, 0, 0, 8)], [("count_star", -1, 0)])
    live0 = capi.device_bytes_live()
    rc, h = raw_call(gpu_ctx, fused.h, [(0, 0)], 1, [(-1, 0)], 1)
    assert rc == capi.E_INVALID and not h and capi.device_bytes_live() == live0
    assert "fused GROUP BY sink" in gpu_ctx.L.polr_last_error(gpu_ctx.h).decode()
    fused.close()
    src.close()
