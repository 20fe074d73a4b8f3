"""Every route by which a build side reaches the device, besides HashTable.from_columns + finalize: row blobs
(polr_ht_upload_rows + polr_deserialize_col_kernel), perfect tables the host built (polr_pht_upload +
polr_pack_bitmap_kernel), and clones (polr_ht_export -> polr_ht_alloc_like -> buffer copies, what polr_bcast_build does on a
receiving rank); and the carry of polr_scan_blocksums_kernel (hash tables of more than 2^20 slots).

Each case builds one logical table by the route under test and by from_columns (its twin); both go through check_table
against joinref.Ref over the INPUT rows (composite keys reduced to codes by buildside.key_codes): per-position counts of
probe_rounds and run_resident, the emitted row set, every payload column's cells and validity, SUM / MIN / MAX of a signed
narrow payload column as exact Python ints, info(), and the engine launch_info reports.  Device build ids go back to input
rows through kept_rows (blob ordinals) or id_to_row (perfect tables).  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

from buildside import clone, col_shape, key_codes, perfect_arrays, row_blob
from joinref import DTYPES, U64, Join, Ref, _key_case, _perfect_ranges, chunks_for, sort_rows
from polr_amd import capi
from test_buildside_helpers import ten_columns

pytestmark = pytest.mark.gpu

INFO_FIELDS = ("kind", "n_keys", "n_rows", "capacity", "max_run", "has_null", "is_dense")
N_BUILD, N_PROBE = 3000, 8000


class Table:
    """one logical build side over its input rows"""

    def __init__(self, keys, key_valid=None, payload=(), payload_valid=None, null_equal=(), key_flags=()):
        self.keys = [np.ascontiguousarray(k) for k in keys]
        self.n = len(self.keys[0])
        self.key_valid = list(key_valid) if key_valid else [None] * len(self.keys)
        self.payload = [np.ascontiguousarray(p) for p in payload]
        self.payload_valid = list(payload_valid) if payload_valid else [None] * len(self.payload)
        self.key_flags = list(key_flags) or [capi.KEY_NULL_EQUAL if f else 0 for f in null_equal] or [0] * len(self.keys)
        self.null_equal = [bool(f & capi.KEY_NULL_EQUAL) for f in self.key_flags]

    def take(self, rows):
        """the table of these input rows only (what a route that drops rows on the host uploads)"""
        def pick(a):
            return None if a is None else np.ascontiguousarray(np.asarray(a)[rows])
        return Table([pick(k) for k in self.keys], [pick(v) for v in self.key_valid], [pick(p) for p in self.payload],
                     [pick(v) for v in self.payload_valid], key_flags=self.key_flags)

    def columns(self, ctx):
        """the twin's upload: from_columns with the key flags set, not finalized"""
        ht = capi.HashTable.from_columns(ctx, self.keys, self.payload, key_valid=self.key_valid,
                                         payload_valid=self.payload_valid)
        for c, f in enumerate(self.key_flags):
            if f:
                ht.set_key_flags(c, f)
        return ht

    def rows(self, ctx, blob=None):
        """the route: polr_ht_upload_rows of the reference's row image (blob: one made by hand) -> (table, kept_rows)"""
        blob, row_width, offs, kept = blob or row_blob(self.keys, self.key_valid, self.payload, self.payload_valid,
                                                       self.null_equal)
        wid, sgn = col_shape(self.keys + self.payload)
        ht = capi.HashTable.from_rows(ctx, blob, len(kept), row_width, offs, wid, sgn, len(self.keys), len(self.payload))
        for c, f in enumerate(self.key_flags):
            if f:
                ht.set_key_flags(c, f)
        return ht, kept

    def info(self, kind, perfect=None):
        """info() of the finalized table as the inputs give it: kind 1 with perfect = (lo, hi), or "hash" (S8 for a unique
        4-byte key without flags, else S16)"""
        codes, ok, _, _ = key_codes(self.keys, self.key_valid, [k[:0] for k in self.keys], None, self.null_equal)
        n_rows = int(ok.sum())
        if kind == 1:
            size = ((perfect[1] - perfect[0]) & U64) + 1
            return {"kind": 1, "n_keys": 1, "n_rows": n_rows, "capacity": size, "max_run": int(n_rows > 0),
                    "has_null": int(n_rows < self.n), "is_dense": int(n_rows == size and n_rows == self.n)}
        max_run = int(np.bincount(codes[ok]).max()) if n_rows else 0
        cap = 1024
        while cap < 2 * self.n:
            cap *= 2
        s8 = max_run <= 1 and len(self.keys) == 1 and self.keys[0].dtype.itemsize == 4 and not any(self.key_flags)
        return {"kind": 2 if s8 else 3, "n_keys": len(self.keys), "n_rows": n_rows, "capacity": cap, "max_run": max_run,
                "has_null": int(n_rows < self.n), "is_dense": 0}


class Probe:
    """probe key columns (+ validity) and one filter column behind them; the reference of a Table over them"""

    def __init__(self, keys, valid, seed=0):
        self.keys = [np.ascontiguousarray(k) for k in keys]
        self.n = len(self.keys[0])
        self.flt = np.random.default_rng(seed).integers(0, 100, self.n).astype(np.int32)
        self.cols = self.keys + [self.flt]
        self.valid = list(valid) + [None]

    def ref(self, t):
        bc, bok, pc, pok = key_codes(t.keys, t.key_valid, self.keys, self.valid[:-1], t.null_equal)
        r = Ref([pc], [pok.astype(np.uint8)], [Join(bc, 0, None, bok.astype(np.uint8))])
        r.want = sort_rows(r.rows())
        return r


def py_agg(fn, vals, ok):
    v = [int(x) for x in vals[ok].tolist()]
    if fn == "count":
        return len(v)
    return None if not v else {"sum": sum, "min": min, "max": max}[fn](v)


def check_sinks(out, t, rows, agg_col, what):
    """every payload column of the emitted build rows, cell by cell; SUM / MIN / MAX of the signed narrow one"""
    b = rows[:, 1]
    for c, (p, v) in enumerate(zip(t.payload, t.payload_valid)):
        data, valid = out.materialize(0, c, p.dtype)
        ok = np.ones(len(b), bool) if v is None else np.asarray(v)[b].astype(bool)
        assert np.array_equal(valid.astype(bool), ok), "%s: validity of payload column %d" % (what, c)
        assert data[ok].tobytes() == p[b][ok].tobytes(), "%s: cells of payload column %d" % (what, c)
    if agg_col is not None:
        p, v = t.payload[agg_col], t.payload_valid[agg_col]
        assert p.dtype.kind == "i" and p.dtype.itemsize <= 2
        ok = np.ones(len(b), bool) if v is None else np.asarray(v)[b].astype(bool)
        fns = ("count", "sum", "min", "max")
        got = out.aggregate([("count_star", -1, 0)] + [(fn, 0, agg_col) for fn in fns])
        assert got == [len(b)] + [py_agg(fn, p[b], ok) for fn in fns], "%s: aggregates" % what


def check_table(ctx, ht, t, probe, ref, id_map=None, agg_col=None, lip=True, what=""):
    """one finalized table against the reference `ref` of Table t (see the module docstring) -> (info, flat of counting
    and emitting runs).  id_map: device build id -> input row (None: the same).  lip: the table also runs as the LIP join
    of a source scan (single plain keys; the packed forms are refused there)."""
    n, nk = probe.n, len(t.keys)
    pipe = capi.Pipeline(ctx, probe.cols, n, [(ht, [(-1, c) for c in range(nk)])], [[0]], probe_valid=probe.valid)
    flat = (pipe.launch_info(False)["flat"], pipe.launch_info(True)["flat"])
    stage, want = ref.stage_counts([0]), ref.want
    n_chunks = (n + 1023) // 1024
    assert pipe.probe_rounds([(0, n, 0, 0)])[0].tolist() == stage, what + ": probe_rounds counting"
    m = capi.DeviceMultiplexer(pipe, "default_path")
    capi.run_resident([m], [(0, n_chunks)], reset=True, finish=True)
    assert m.finish()["stage_out"][0] == stage, what + ": run_resident counting"
    out = capi.Output(pipe, 1024, chunks_for(len(want), 1024))
    for engine in ("probe_rounds", "run_resident"):
        out.reset()
        if engine == "probe_rounds":
            counts = pipe.probe_rounds([(0, n, 0, 1)], out=out)[0].tolist()
        else:
            capi.run_resident([m], [(0, n_chunks)], out=out, reset=True, finish=True)
            counts = m.finish()["stage_out"][0]
        assert counts == stage, "%s: %s emitting" % (what, engine)
        rows = out.fetch_ids().astype(np.int64)
        if id_map is not None:
            rows[:, 1] = np.asarray(id_map, dtype=np.int64)[rows[:, 1]]
        assert np.array_equal(sort_rows(rows), want), "%s: %s rows" % (what, engine)
        check_sinks(out, t, rows, agg_col, "%s: %s" % (what, engine))
    if lip:
        expect = np.nonzero((probe.flt < 70) & (ref.counts[0] > 0))[0]
        n_sel, n_lip_chunks = pipe.scan_filter([(nk, "<", 70)], lip_joins=1)
        sel, offs = pipe.fetch_scan()
        assert n_sel == len(expect) and np.array_equal(sel, expect), what + ": LIP selection"
        assert offs[-1] == len(sel)
        if n_lip_chunks:  # LIP thins the source, never the output
            m.use_scan_chunks()
            capi.run_resident([m], [(0, n_lip_chunks)], reset=True, finish=True)
            assert m.finish()["stage_out"][0] == [int(ref.counts[0][expect].sum())], what + ": run over the LIP scan"
    else:
        with pytest.raises(capi.PolrError) as e:
            pipe.scan_filter([(nk, "<", 70)], lip_joins=1)
        assert "LIP" in str(e.value)
    m.close()
    out.close()
    pipe.close()
    info = ht.info()
    return {f: info[f] for f in INFO_FIELDS}, flat


def check_pair(ctx, route, twin, t, probe, id_map, want_info, agg_col=None, lip=True, flat=None):
    """the table the route made and its from_columns twin: both against the reference, the same info() (want_info: as
    the inputs give it) and the same engine (flat: what it must be, where the case says)"""
    ref = probe.ref(t)
    got = [check_table(ctx, h, t, probe, ref, id_map, agg_col, lip, what) for h, what in ((route, "route"), (twin, "twin"))]
    assert got[0][0] == want_info, "route info()"
    assert got[1][0] == want_info, "twin info()"
    assert got[0][1] == got[1][1], "the route changed the engine"
    if flat is not None:
        assert got[0][1] == flat
    route.close()
    twin.close()
    return ref


def payload_mix(rng, n):
    """payload columns of 1 to 16 bytes, three of them with validity; column 0 is the signed narrow one (negative values)"""
    pay = [rng.integers(-128, 128, n).astype(np.int8), rng.integers(0, 2**16, n).astype(np.uint16),
           rng.integers(-2**31, 2**31, n).astype(np.int32), rng.integers(0, 2**64, n, dtype=np.uint64),
           np.frombuffer(rng.bytes(16 * n), dtype="V16").copy()]
    pv = [(rng.random(n) > 0.2).astype(np.uint8), None, (rng.random(n) > 0.1).astype(np.uint8), None,
          (rng.random(n) > 0.3).astype(np.uint8)]
    return pay, pv


def two_payloads(rng, n):
    """an int16 column with negative values and NULLs, and a V16 column without validity"""
    return ([rng.integers(-30000, 30000, n).astype(np.int16), np.frombuffer(rng.bytes(16 * n), dtype="V16").copy()],
            [(rng.random(n) > 0.15).astype(np.uint8), None])


def no_leak(ctx, code, call):
    live = capi.device_bytes_live()
    with pytest.raises(capi.PolrError) as e:
        call()
    assert e.value.code == code
    assert capi.device_bytes_live() == live


# ---- a. row blobs ------------------------------------------------------------------------------------------------------------
def test_rows_ten_unaligned_columns(gpu_ctx):
    """10 columns, 43-byte rows, two validity bytes, a packed two-key S16 table whose second key is NULL = NULL: every
    payload column (widths 1, 2, 4, 8, signed and unsigned; NULLs in columns 7, 8, 9) read back through the sinks"""
    keys, kv, pay, pv, ne = ten_columns(11, N_BUILD)
    t = Table(keys, kv, pay, pv, null_equal=ne)
    rng = np.random.default_rng(12)
    pk = [rng.integers(-45, 45, N_PROBE).astype(np.int16), rng.integers(0, 14, N_PROBE).astype(np.uint8)]
    pvalid = [(rng.random(N_PROBE) > 0.03).astype(np.uint8), (rng.random(N_PROBE) > 0.1).astype(np.uint8)]
    route, kept = t.rows(gpu_ctx)
    assert 0 < len(kept) < N_BUILD
    up = t.take(kept)
    twin = up.columns(gpu_ctx)
    route.finalize_hash()
    twin.finalize_hash()
    want = up.info("hash")
    assert want["kind"] == 3 and want["has_null"] == 0 and want["max_run"] > 1
    ref = check_pair(gpu_ctx, route, twin, t, Probe(pk, pvalid), kept, want, agg_col=0, lip=False)
    null_rows = np.nonzero(kv[1][ref.want[:, 1]] == 0)[0]
    assert len(null_rows) > 10 and len(ref.want) > 1000  # NULL keys joined NULL keys


FINALIZE = ["perfect", "hash-unique", "hash-repeated", "auto-unique", "auto-repeated"]


@pytest.mark.parametrize("dt", DTYPES, ids=[np.dtype(d).name for d in DTYPES])
def test_rows_single_key(gpu_ctx, dt):
    """one key of every type, an int16 payload with NULLs and a V16 payload, through finalize_perfect, finalize_hash (S8
    for the unique 4-byte keys, else S16) and finalize_auto"""
    for x, how in enumerate(FINALIZE):
        perfect_kind = list(_perfect_ranges(dt))[-1]
        kind = perfect_kind if how in ("perfect", "auto-unique") else how.split("-")[1]
        j, pcols, pvalid = _key_case(dt, kind, seed=300 + 10 * DTYPES.index(dt) + x, n_probe=N_PROBE)
        rng = np.random.default_rng(x)
        pay, pv = two_payloads(rng, len(j.keys))
        t = Table([j.keys], [j.valid], pay, pv)
        route, kept = t.rows(gpu_ctx)
        up = t.take(kept)
        twin = up.columns(gpu_ctx)
        id_map = kept
        if how == "perfect":
            assert route.finalize_perfect(*j.perfect) and twin.finalize_perfect(*j.perfect)
            want = up.info(1, j.perfect)
        elif how.startswith("hash"):
            route.finalize_hash()
            twin.finalize_hash()
            want = up.info("hash")
            assert want["kind"] == (2 if kind == "unique" and np.dtype(dt).itemsize == 4 else 3)
        else:
            ok = j.keys[j.valid.astype(bool)]
            lo, hi = int(ok.min()), int(ok.max())
            if dt == np.uint64:  # (as int64 bit patterns)
                lo, hi = lo - (1 << 64) if lo >> 63 else lo, hi - (1 << 64) if hi >> 63 else hi
            kinds = [route.finalize_auto(lo, hi), twin.finalize_auto(lo, hi)]
            want = up.info(1, (lo, hi)) if how == "auto-unique" else up.info("hash")
            assert kinds == [want["kind"]] * 2
        if want["kind"] == 1:  # ids of a perfect table are key offsets
            id_map = perfect_arrays(j.keys, j.valid, [], None, *(j.perfect if how == "perfect" else (lo, hi)))[3]
        ref = check_pair(gpu_ctx, route, twin, t, Probe(pcols, pvalid), id_map, want, agg_col=0)
        assert len(ref.want) > 50, how


def test_rows_null_equal_key(gpu_ctx):
    """POLR_KEY_NULL_EQUAL by the row route: NULL-key rows stay in the blob with the key bit cleared and join NULL probe
    keys (IS NOT DISTINCT FROM), nothing else"""
    rng = np.random.default_rng(21)
    bk = rng.integers(-300, 300, N_BUILD).astype(np.int32)
    bv = (rng.random(N_BUILD) > 0.02).astype(np.uint8)
    pay, pv = two_payloads(rng, N_BUILD)
    t = Table([bk], [bv], pay, pv, null_equal=[True])
    pk = rng.integers(-330, 330, N_PROBE).astype(np.int32)
    pvalid = (rng.random(N_PROBE) > 0.02).astype(np.uint8)
    route, kept = t.rows(gpu_ctx)
    assert len(kept) == N_BUILD  # nothing left out
    twin = t.columns(gpu_ctx)
    route.finalize_hash()
    twin.finalize_hash()
    want = t.info("hash")
    assert want["kind"] == 3 and want["n_rows"] == N_BUILD and want["has_null"] == 0
    ref = check_pair(gpu_ctx, route, twin, t, Probe([pk], [pvalid]), None, want, agg_col=0, lip=False)
    nulls = ref.want[pvalid[ref.want[:, 0]] == 0]
    assert len(nulls) == int((pvalid == 0).sum()) * int((bv == 0).sum()) > 1000
    assert (bv[nulls[:, 1]] == 0).all()


def test_rows_with_cleared_key_bits_and_no_null_equal(gpu_ctx):
    """a blob made by hand that still holds its NULL-key rows, uploaded without NULL_EQUAL: they never match, has_null is
    set, n_rows leaves them out and row ids stay blob ordinals"""
    rng = np.random.default_rng(22)
    bk = rng.integers(-300, 300, N_BUILD).astype(np.int32)
    bv = (rng.random(N_BUILD) > 0.1).astype(np.uint8)
    pay, pv = two_payloads(rng, N_BUILD)
    t = Table([bk], [bv], pay, pv)
    blob = row_blob([bk], [bv], pay, pv, null_equal=[True])  # (keeps every row; the key bit of the NULL ones cleared)
    assert len(blob[3]) == N_BUILD
    route, _ = t.rows(gpu_ctx, blob)
    twin = t.columns(gpu_ctx)
    route.finalize_hash()
    twin.finalize_hash()
    want = t.info("hash")
    assert want["has_null"] == 1 and want["n_rows"] == int(bv.sum()) < N_BUILD
    pk = rng.integers(-330, 330, N_PROBE).astype(np.int32)
    pk[::7] = 0  # the zeroed cells of the NULL rows are not keys
    pvalid = (rng.random(N_PROBE) > 0.02).astype(np.uint8)
    ref = check_pair(gpu_ctx, route, twin, t, Probe([pk], [pvalid]), None, want, agg_col=0)
    assert bv[ref.want[:, 1]].all() and len(ref.want) > 1000


@pytest.mark.parametrize("n_rows", [0, 1, 256, 257])
def test_rows_around_one_launch_block(gpu_ctx, n_rows):
    rng = np.random.default_rng(23 + n_rows)
    bk = rng.permutation(np.arange(-128, 129, dtype=np.int64))[:n_rows]
    bv = (rng.random(n_rows) > 0.05).astype(np.uint8)
    pay, pv = two_payloads(rng, n_rows)
    t = Table([bk], [bv], pay, pv)
    route, kept = t.rows(gpu_ctx)
    up = t.take(kept)
    twin = up.columns(gpu_ctx)
    route.finalize_hash()
    twin.finalize_hash()
    pk = rng.integers(-140, 140, 2000).astype(np.int64)
    ref = check_pair(gpu_ctx, route, twin, t, Probe([pk], [(rng.random(2000) > 0.05).astype(np.uint8)]), kept,
                     up.info("hash"), agg_col=0)
    assert (len(ref.want) > 0) == (len(kept) > 0)


def test_rows_refusals(gpu_ctx):
    rows = np.zeros(64 * 16, np.uint8)

    def upload(row_width, offs, wid, n_keys, n_payload):
        return lambda: capi.HashTable.from_rows(gpu_ctx, rows, 16, row_width, offs, wid, [0] * len(offs), n_keys, n_payload)

    no_leak(gpu_ctx, capi.E_INVALID, upload(16, [1, 9], [4, 8], 1, 1))       # a column running past row_width
    no_leak(gpu_ctx, capi.E_INVALID, upload(1, [0] * 8, [1] * 8, 1, 7))      # two validity bytes in a one-byte row
    no_leak(gpu_ctx, capi.E_INVALID, upload(16, [1, 5], [4, 3], 1, 1))       # a column of 3 bytes
    ok = upload(16, [1, 5], [4, 2], 1, 1)()  # (the shape next to them is taken)
    ok.close()


# ---- b. perfect tables the host built ---------------------------------------------------------------------------------------
# (name, key type, min, slots, fill): the word edges of polr_pack_bitmap_kernel (one thread per 32 slots, 256 threads per
# block: 8193 slots need a second block), every key width and sign, a negative min, whole 8- and 16-bit domains, a uint64
# range above 2^63
PERFECT = [("int32-1", np.int32, -7, 1, "some"), ("uint8-31", np.uint8, 100, 31, "some"),
           ("int16-32", np.int16, -16, 32, "some"), ("uint32-33-at-max", np.uint32, 2**32 - 33, 33, "some"),
           ("int64-64-at-min", np.int64, -2**63, 64, "some"), ("uint64-8192-above-2^63", np.uint64, 2**64 - 8192, 8192, "some"),
           ("int32-8193", np.int32, 10, 8193, "some"), ("uint32-8224", np.uint32, 0, 8193 + 31, "some"),
           ("int8-domain", np.int8, -128, 256, "some"), ("uint16-domain", np.uint16, 0, 65536, "some"),
           ("int32-none-set", np.int32, -50, 100, "none"), ("int32-all-set", np.int32, -4000, 8193, "all")]


def perfect_case(rng, dt, lo, size, fill):
    """-> (Table over the input rows, (min, max) as polr_pht_upload takes them, Probe): about three quarters of the slots
    set, both ends set and their neighbours unset; rows with a NULL key among the input; probe keys on every slot, just
    outside the range on both sides, and NULL"""
    info = np.iinfo(dt)
    wide = np.uint64 if dt == np.uint64 else np.int64
    offs = np.arange(size)
    if fill == "some":
        setm = rng.random(size) < 0.75
        setm[[0, -1]] = True
        if size >= 5:
            setm[[1, -2]] = False
    else:
        setm = np.full(size, fill == "all")
    keys = rng.permutation((offs[setm] + lo).astype(wide)).astype(dt) if dt != np.uint64 else \
        rng.permutation(np.array([lo + int(o) for o in offs[setm]], dtype=np.uint64))
    n_null = 0 if fill == "all" else 40
    keys = np.concatenate([keys, np.full(n_null, lo, wide).astype(dt)])
    kv = np.concatenate([np.ones(int(setm.sum()), np.uint8), np.zeros(n_null, np.uint8)])
    perm = rng.permutation(len(keys))
    keys, kv = keys[perm], kv[perm]
    pay, pv = payload_mix(rng, len(keys))
    hi = lo + size - 1
    span = [v for v in range(lo - 40, hi + 41) if info.min <= v <= info.max] if size <= 1024 else \
        [v for v in list(range(lo - 40, lo + 80)) + list(range(hi - 80, hi + 41)) if info.min <= v <= info.max]
    pk = [lo + int(o) for o in rng.integers(0, size, N_PROBE // 2)] + [span[i] for i in rng.integers(0, len(span), N_PROBE // 2)]
    pk = rng.permutation(np.array(pk, dtype=wide)).astype(dt)
    pvalid = (rng.random(N_PROBE) > 0.03).astype(np.uint8)
    mm = (lo, hi) if dt != np.uint64 else tuple(v - (1 << 64) if v >> 63 else v for v in (lo, hi))
    return Table([keys], [kv], pay, pv), mm, Probe([pk], [pvalid])


@pytest.mark.parametrize("name,dt,lo,size,fill", PERFECT, ids=[p[0] for p in PERFECT])
def test_uploaded_perfect_table(gpu_ctx, name, dt, lo, size, fill):
    rng = np.random.default_rng(400 + [p[0] for p in PERFECT].index(name))
    t, (mn, mx), probe = perfect_case(rng, dt, lo, size, fill)
    bitmap, cells, cell_valid, id_to_row = perfect_arrays(t.keys[0], t.key_valid[0], t.payload, t.payload_valid, mn, mx)
    assert len(bitmap) == size
    route = capi.HashTable.from_perfect(gpu_ctx, np.dtype(dt).itemsize, np.dtype(dt).kind == "i", mn, mx, bitmap, cells,
                                        cell_valid)
    up = t.take(np.nonzero(t.key_valid[0])[0])  # (the arrays carry no NULL-key row: neither does the twin)
    twin = up.columns(gpu_ctx)
    assert twin.finalize_perfect(mn, mx)
    want = up.info(1, (mn, mx))
    assert want["n_rows"] == int(bitmap.sum()) and want["has_null"] == 0
    if fill == "none":
        assert (want["n_rows"], want["max_run"], want["is_dense"]) == (0, 0, 0)
    if fill == "all":
        assert want["is_dense"] == 1 and want["n_rows"] == size
    four = np.dtype(dt).itemsize == 4
    ref = check_pair(gpu_ctx, route, twin, t, probe, id_to_row, want, agg_col=0, flat=(int(four), int(four)))
    assert (len(ref.want) == 0) if fill == "none" else (len(ref.want) > N_PROBE // 4)


def test_uploaded_perfect_table_refusals(gpu_ctx):
    bitmap = np.ones(64, np.uint8)

    def upload(width, mn, mx):
        return lambda: capi.HashTable.from_perfect(gpu_ctx, width, True, mn, mx, bitmap)

    no_leak(gpu_ctx, capi.E_INVALID, upload(4, 0, 2**31))         # a range of 2^31
    no_leak(gpu_ctx, capi.E_INVALID, upload(8, -2**62, 2**62))    # ... and far beyond
    no_leak(gpu_ctx, capi.E_INVALID, upload(8, 2**63 - 1, -2**63))  # max < min in the key's own order (a wrapped range of 1)
    no_leak(gpu_ctx, capi.E_INVALID, upload(3, 0, 63))
    no_leak(gpu_ctx, capi.E_INVALID, upload(16, 0, 63))
    live = capi.device_bytes_live()
    h = C.c_void_p()
    assert gpu_ctx.L.polr_pht_upload(gpu_ctx.h, 4, capi.COL_SIGNED, 0, 63, None, None, 0, C.byref(h)) == capi.E_INVALID
    assert not h.value and capi.device_bytes_live() == live
    upload(4, 0, 63)().close()


# ---- c. clones ---------------------------------------------------------------------------------------------------------------
def clone_case(ctx, name):
    """-> (Table, the source table finalized, the twin finalized, id_map, info as the inputs give it, Probe, lip, flat)"""
    rng = np.random.default_rng(500 + CLONES.index(name))
    lip, flat, id_map = True, None, None
    if name in ("finalize_perfect", "from_perfect"):
        t, (mn, mx), probe = perfect_case(rng, np.int32, -1000, 3000, "some")
        id_map = perfect_arrays(t.keys[0], t.key_valid[0], [], None, mn, mx)[3]
        flat = (1, 1)
        if name == "finalize_perfect":
            src, twin, want = t.columns(ctx), t.columns(ctx), t.info(1, (mn, mx))
            assert src.finalize_perfect(mn, mx)
        else:
            bitmap, cells, cell_valid, _ = perfect_arrays(t.keys[0], t.key_valid[0], t.payload, t.payload_valid, mn, mx)
            src = capi.HashTable.from_perfect(ctx, 4, True, mn, mx, bitmap, cells, cell_valid)
            up = t.take(np.nonzero(t.key_valid[0])[0])
            twin, want = up.columns(ctx), up.info(1, (mn, mx))
        assert twin.finalize_perfect(mn, mx)
        return t, src, twin, id_map, want, probe, lip, flat
    if name == "s8":
        bk = rng.choice(np.arange(-10**9, 10**9, 977, dtype=np.int64), N_BUILD, replace=False).astype(np.int32)
        bv = [(rng.random(N_BUILD) > 0.03).astype(np.uint8)]
        pay, pv = payload_mix(rng, N_BUILD)
        t = Table([bk], bv, pay, pv)
        pk = np.where(rng.random(N_PROBE) < 0.7, rng.choice(bk, N_PROBE), rng.integers(-10**9, 10**9, N_PROBE)).astype(np.int32)
        probe, flat = Probe([pk], [(rng.random(N_PROBE) > 0.03).astype(np.uint8)]), (1, 0)
    elif name == "s16-runs-and-sentinel":
        distinct = rng.integers(0, 2**64, 200, dtype=np.uint64)
        bk = np.concatenate([np.repeat(distinct, 1 + np.arange(200) % 30), np.full(3, U64, np.uint64)])
        bk = rng.permutation(bk)
        bv = [(rng.random(len(bk)) > 0.02).astype(np.uint8)]
        bv[0][bk == np.uint64(U64)] = 1
        pay, pv = payload_mix(rng, len(bk))
        pv = [pv[0], None, None, None, None]
        t = Table([bk], bv, pay, pv)
        pk = np.concatenate([rng.choice(distinct, N_PROBE // 2), np.full(200, U64, np.uint64),
                             rng.integers(0, 2**64, N_PROBE - N_PROBE // 2 - 200, dtype=np.uint64)])
        probe = Probe([rng.permutation(pk)], [(rng.random(N_PROBE) > 0.03).astype(np.uint8)])
    elif name == "packed-three-keys":
        bk = [rng.integers(-40, 40, N_BUILD).astype(np.int32), rng.integers(0, 9, N_BUILD).astype(np.uint8),
              rng.integers(100, 130, N_BUILD).astype(np.int64)]
        bv = [(rng.random(N_BUILD) > 0.02).astype(np.uint8), (rng.random(N_BUILD) > 0.1).astype(np.uint8), None]
        pay, pv = payload_mix(rng, N_BUILD)
        t = Table(bk, bv, pay, pv, key_flags=[0, capi.KEY_NULL_EQUAL, capi.KEY_BY_VALUE])
        pk = [rng.integers(-42, 42, N_PROBE).astype(np.int32), rng.integers(0, 10, N_PROBE).astype(np.uint8),
              rng.integers(98, 132, N_PROBE).astype(np.int32)]  # (the third by value: INTEGER against BIGINT)
        probe = Probe(pk, [(rng.random(N_PROBE) > 0.03).astype(np.uint8), (rng.random(N_PROBE) > 0.1).astype(np.uint8), None])
        lip = False
    else:
        n = {"no-rows": 0, "one-row": 1}[name]
        pay, pv = payload_mix(rng, n)
        t = Table([np.full(n, 5, np.int64)], [None], pay, pv)
        probe = Probe([rng.integers(0, 10, 2000).astype(np.int64)], [(rng.random(2000) > 0.03).astype(np.uint8)])
    src, twin = t.columns(ctx).finalize_hash(), t.columns(ctx).finalize_hash()
    return t, src, twin, id_map, t.info("hash"), probe, lip, flat


CLONES = ["finalize_perfect", "from_perfect", "s8", "s16-runs-and-sentinel", "packed-three-keys", "no-rows", "one-row"]


@pytest.mark.parametrize("name", CLONES)
def test_clone(gpu_ctx, name):
    """export -> alloc_like -> buffer copies, the source closed before the clone is probed: the clone alone against the
    reference and a twin built anew.  (one-row: polr_ht_export used to list every buffer with at least 16 bytes, more
    than a table of fewer than 16 rows holds in its row ids, narrow payload columns and validity bytes -- a copy or a
    broadcast of that many bytes read past the source's allocation.)"""
    t, src, twin, id_map, want, probe, lip, flat = clone_case(gpu_ctx, name)
    sizes = [n for _, n in src.export()[1]]
    # the slots or bits, the row ids of an S16 table, then data (+ validity) per payload column; a perfect table's re-ordered
    # columns all have validity (an unset slot is invalid)
    n_valid = len(t.payload) if want["kind"] == 1 else sum(v is not None for v in t.payload_valid)
    n_buffers = (2 if want["kind"] == 3 else 1) + len(t.payload) + n_valid
    assert len(sizes) == n_buffers and min(sizes) > 0
    if name == "no-rows":  # an empty table still has every buffer: 16 bytes each behind the slots
        assert sizes[1:] == [16] * (n_buffers - 1)
    if name == "one-row":  # ... and a buffer is listed with the bytes the table holds, no more: one row, 1 to 16 bytes
        assert sizes[1:] == [4, 1, 1, 2, 4, 1, 8, 16, 1]
    route = clone(gpu_ctx, src)
    assert route.info()["device_bytes"] == sum(sizes)  # the clone owns exactly what was copied into it
    src.close()
    if name == "s16-runs-and-sentinel":
        assert want["kind"] == 3 and want["max_run"] == 30
    if name == "s8":
        assert want["kind"] == 2
    ref = check_pair(gpu_ctx, route, twin, t, probe, id_map, want, agg_col=0, lip=lip, flat=flat)
    if name == "s16-runs-and-sentinel":
        ones = ref.want[probe.keys[0][ref.want[:, 0]] == np.uint64(U64)]
        assert len(ones) == 3 * int(((probe.keys[0] == np.uint64(U64)) & (probe.valid[0] == 1)).sum()) > 300
    assert (len(ref.want) > 0) == (name != "no-rows")


def test_clone_metadata_refusals(gpu_ctx):
    """a metadata blob cut short, with another magic, a table kind that does not exist, too many payload columns, a payload
    column of 3 bytes or a hash table of 1000 slots"""
    ht = capi.HashTable.from_columns(gpu_ctx, [np.arange(100, dtype=np.int32)], [np.arange(100, dtype=np.int16)]).finalize_hash()
    meta, _ = ht.export()
    ht.close()
    words = np.frombuffer(meta, dtype=np.uint32)
    assert words[0] == 0x504F4C52 and words[1] == 2 and words[2] == 1 and words[3] == 1  # magic, kind, n_keys, n_payload
    assert words[14] == 1024 and words[15] == 0 and words[64] == 2  # capacity (64-bit), the payload column's width

    def patched(word, value):
        w = words.copy()
        w[word] = value
        return w.tobytes()

    for bad in (meta[:-1], patched(0, 0x504F4C53), patched(1, 0), patched(1, 7), patched(3, 63), patched(64, 3), patched(14, 1000)):
        no_leak(gpu_ctx, capi.E_INVALID, lambda: capi.HashTable.alloc_like(gpu_ctx, bad))
    capi.HashTable.alloc_like(gpu_ctx, meta).close()


# ---- d. the carry of the block-sum scan -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows", [2**19, 2**19 + 1], ids=["2^19", "2^19+1"])
def test_hash_table_beyond_1024_block_sums(gpu_ctx, n_rows):
    """finalize_hash scans one block sum per 1024 slots, 1024 sums per iteration of polr_scan_blocksums_kernel: 2^19 + 1
    rows (2^21 slots) is the smallest table whose scan carries a running total into a second iteration, 2^19 rows
    (2^20 slots) the largest without"""
    rng = np.random.default_rng(600)
    bk = rng.permutation(np.arange(n_rows, dtype=np.int64) // 2 * 7)
    bv = (rng.random(n_rows) > 0.02).astype(np.uint8)
    pay, pv = two_payloads(rng, n_rows)
    t = Table([bk], [bv], pay, pv)
    pk = rng.integers(-100, int(bk.max()) + 100, 20_000).astype(np.int64)
    pk[::2] = pk[::2] // 7 * 7  # (every other one a multiple of 7: a key, if inside the range)
    probe = Probe([pk], [(rng.random(20_000) > 0.02).astype(np.uint8)])
    ht = t.columns(gpu_ctx).finalize_hash()
    want = t.info("hash")
    assert want["capacity"] == (2**20 if n_rows == 2**19 else 2**21) and want["max_run"] == 2
    ref = probe.ref(t)
    assert len(ref.want) > 15_000
    info, _ = check_table(gpu_ctx, ht, t, probe, ref, agg_col=0)
    assert info == want
    ht.close()
