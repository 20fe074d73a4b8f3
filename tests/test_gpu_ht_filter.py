"""polr_ht_filter (HashTable.filter): the rows of an un-finalized build side filtered and compacted on the device.

The reference is never the code under test.  scanexpr.passing(expr, cols, n) over the host columns gives the kept rows (it
is pinned to the reference engine by tests/golden/scan_expr.json); a TWIN table is built with HashTable.from_columns from the
numpy-filtered host columns (VARCHAR: cells and heap blocks from scanstr.cells, handed over with set_payload_heaps).  Then
filter_rows() must equal the expected rows, every payload column materialised through a one-join probe pipeline must equal
the twin's, and the pipeline's row set -- build id -> filter_rows -> uploaded row -- must equal the twin's and joinref.Ref
over the filtered build side.  The raw cells and validity arrays of a hash-finalized table are read back through
polr_ht_export where a property cannot be seen through a pipeline (the cell of a kept NULL row is zero; a column has a
validity array iff it had one).

Tiles are 1024 rows, a pass-bit word 64, the prefix over the tile counts takes 1024 tiles a step: the row counts are the
edges of all three."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import buildside
import common
import scanexpr
import scanstr
from joinref import MAX_WAVE_CHUNKS, Join, Ref, sort_rows
from polr_amd import capi
from test_gpu_from_output import probe_b, same

pytestmark = pytest.mark.gpu

DTS = [np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.int64, np.uint64]


# ---- a build side on the host ---------------------------------------------------------------------------------------------
class Side:
    """keys: integer arrays; payload: integer arrays or [bytes or None] (VARCHAR); kvalid / pvalid: uint8 arrays or None (a
    VARCHAR column's validity is its Nones)"""

    def __init__(self, keys, payload=(), kvalid=None, pvalid=None):
        self.keys, self.payload = list(keys), list(payload)
        self.kvalid = list(kvalid) if kvalid else [None] * len(self.keys)
        self.pvalid = list(pvalid) if pvalid else [None] * len(self.payload)
        self.n = len(self.keys[0])

    def cols(self):
        """the table's columns in the filter's numbering (keys first, then payload), as scanexpr takes them"""
        return [(k, v) for k, v in zip(self.keys, self.kvalid)] + \
               [p if isinstance(p, list) else (p, v) for p, v in zip(self.payload, self.pvalid)]

    def take(self, rows):
        rows = np.asarray(rows, dtype=np.int64)
        t = lambda a: None if a is None else [a[i] for i in rows.tolist()] if isinstance(a, list) else a[rows]
        return Side([t(k) for k in self.keys], [t(p) for p in self.payload], [t(v) for v in self.kvalid], [t(v) for v in self.pvalid])

    def device_payload(self, null_cell=b"ab", dirty_seed=None, n_blocks=2):
        """-> (payload arrays with V16 cells for the VARCHAR columns, validity arrays, {payload column: heap blocks})"""
        cols, valid, heaps = [], [], {}
        for i, (p, v) in enumerate(zip(self.payload, self.pvalid)):
            if isinstance(p, list):
                cells, ok, blocks = scanstr.cells(p, n_blocks=n_blocks, null_cell=null_cell, dirty_seed=dirty_seed)
                cols.append(cells)
                valid.append(ok)
                heaps[i] = blocks
            else:
                cols.append(p)
                valid.append(v)
        return cols, valid, heaps

    def upload(self, ctx, heaps=True, **kw):
        cols, valid, blocks = self.device_payload(**kw)
        ht = capi.HashTable.from_columns(ctx, self.keys, cols, key_valid=self.kvalid, payload_valid=valid)
        ht._keep = (cols, valid, blocks)
        if heaps is True:
            heaps = list(blocks)
        for i in heaps or []:
            ht.set_payload_heaps(i, blocks[i])
        return ht

    def dtypes(self):
        return [None if isinstance(p, list) else p.dtype for p in self.payload]


def finalize(ht, how):
    if how == "hash":
        ht.finalize_hash()
    elif how[0] == "auto":
        ht.finalize_auto(*how[1:])
    else:
        assert ht.finalize_perfect(*how[1:])
    return ht.info()["kind"]


def probe_keys(side, rng, extra=40):
    """one probe column per key column: every uploaded key tuple once (so the rows dropped by the filter are probed for and
    must miss) and a few tuples no row holds"""
    cols = []
    for k in side.keys:
        info = np.iinfo(k.dtype)
        miss = rng.integers(int(info.min), int(info.max), extra, dtype=k.dtype, endpoint=True)
        cols.append(np.concatenate([k, miss]))
    valid = [None if v is None else np.concatenate([v, np.ones(extra, np.uint8)]) for v in side.kvalid]
    return cols, valid


def check_downstream(ctx, side, want, ht, how="hash", rng=None):
    """the filtered table against the twin and joinref.Ref, through a one-join probe pipeline"""
    rng = rng or np.random.default_rng(len(want))
    rows = ht.filter_rows()
    assert rows.dtype == np.uint32 and np.array_equal(rows, want)
    kept = side.take(want)
    twin = kept.upload(ctx)
    kinds = [finalize(t, how) for t in (ht, twin)]
    assert kinds[0] == kinds[1] and ht.info()["n_rows"] == twin.info()["n_rows"]
    pk, pv = probe_keys(side, rng)
    ids, mats = probe_b(ctx, ht, pk, pv, side.dtypes())
    ids_t, mats_t = probe_b(ctx, twin, pk, pv, side.dtypes())
    assert np.array_equal(ids, ids_t)
    for a, b in zip(mats, mats_t):
        assert same(a, b)
    if len(side.keys) == 1:
        jb = Join(kept.keys[0], 0, how[1:] if kinds[0] == 1 else None, kept.kvalid[0])
        ref = Ref([pk[0]], pv, [jb]).rows()
        ref[:, 1] = want[ref[:, 1]] if len(ref) else ref[:, 1]
        got = ids.copy()
        if kinds[0] == 1:
            got[:, 1] = jb.id_to_row[got[:, 1]]
        got[:, 1] = rows[got[:, 1]] if len(got) else got[:, 1]
        assert np.array_equal(sort_rows(got), sort_rows(ref))  # (build id -> filter_rows: the rows as uploaded)
        for p, v, m in zip(side.payload, side.pvalid, mats):
            up = got[:, 1]
            if isinstance(p, list):
                assert m == [p[r] for r in up.tolist()]
            else:
                ok = np.ones(len(up), np.uint8) if v is None else v[up]
                assert np.array_equal(m[1], ok) and np.array_equal(m[0], np.where(ok, p[up], 0))
    twin.close()
    return ids


def filtered(ctx, side, expr, ht=None, how="hash", downstream=True, **upload):
    """upload, filter, check -> the kept rows"""
    want = scanexpr.passing(expr, side.cols(), side.n)
    own = ht is None
    ht = ht or side.upload(ctx, **upload)
    assert ht.filter(expr) == len(want)
    if downstream:
        check_downstream(ctx, side, want, ht, how)
    else:
        assert np.array_equal(ht.filter_rows(), want)
    if own:
        ht.close()
    return want


def raw_columns(ht, widths):
    """the payload columns of a hash-finalized table as the device holds them -> [(cells uint8[n, w], validity or None)]"""
    meta, bufs = ht.export()
    n = ht._n_kept
    bufs = bufs[1 + (1 if ht.info()["kind"] == 3 else 0):]
    has_valid = np.frombuffer(meta, np.uint8)[256 + 62 * 8:256 + 62 * 8 + len(widths)]  # PolrHtMeta::payload_has_valid
    hip = C.CDLL("libamdhip64.so")  # (the HIP runtime the library runs on)
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = []
    for w, hv in zip(widths, has_valid):
        def get(nbytes):
            ptr, size = bufs.pop(0)
            a = np.zeros(max(nbytes, 1), np.uint8)
            assert size >= nbytes and (nbytes == 0 or hip.hipMemcpy(a.ctypes.data, ptr, nbytes, 2) == 0)
            return a[:nbytes]
        cells = get(n * w).reshape(n, w)
        out.append((cells, get(n) if hv else None))
    assert not bufs
    return out


# ---- 1. shapes: row counts x kept-row patterns ------------------------------------------------------------------------------
def patterns(n):
    i = np.arange(n)
    return {"none": np.zeros(n, bool), "all": np.ones(n, bool), "first": i == 0, "last": i == n - 1, "alternate": i % 2 == 1,
            "word": (i // 64) % 2 == 1,   # a full 64-row word kept next to an empty one
            "tile": (i // 1024) % 2 == 1}  # a tile kept whole next to an empty tile


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1023, 1024, 1025, 4097])
def test_row_counts_and_patterns(gpu_ctx, n):
    rng = np.random.default_rng(n)
    key = rng.permutation(n).astype(np.int32)
    pay = rng.integers(-(1 << 40), 1 << 40, n).astype(np.int64)
    for name, keep in patterns(n).items():
        side = Side([key], [keep.astype(np.uint8), pay], pvalid=[None, (rng.random(n) > 0.3).astype(np.uint8)])
        want = filtered(gpu_ctx, side, ("cmp", 1, "=", 1))
        assert np.array_equal(want, np.nonzero(keep)[0]), name
    side = Side([key], [pay])
    assert len(filtered(gpu_ctx, side, None)) == n  # n_nodes == 0 keeps every row


def test_more_tiles_than_one_prefix_step(gpu_ctx):
    """1026 tiles: the prefix over the tile counts carries from its first step of 1024 tiles into the second"""
    n = 1024 * 1024 + 1025
    i = np.arange(n)
    key = i.astype(np.int32)
    flag = ((i % 3 == 0) | (i >= n - 1500) | ((i // 1024) == 1023)).astype(np.uint8)
    flag[1024 * 1024 - 700:1024 * 1024] = 0
    side = Side([key], [flag])
    want = np.nonzero(flag)[0].astype(np.uint32)
    ht = side.upload(gpu_ctx)
    assert ht.filter(("cmp", 1, "=", 1)) == len(want)
    rows = ht.filter_rows()
    assert np.array_equal(rows, want)
    ht.finalize_hash()
    rng = np.random.default_rng(5)
    pk = np.concatenate([rng.integers(0, n, 4000), np.arange(n - 2100, n), np.arange(1024 * 1024 - 1100, 1024 * 1024 + 100)]).astype(np.int32)
    ids, mats = probe_b(gpu_ctx, ht, [pk], None, [np.uint8])
    hit = flag[pk].astype(bool)
    assert np.array_equal(ids[:, 0], np.nonzero(hit)[0]) and np.array_equal(rows[ids[:, 1]], pk[hit]) and mats[0][0].all()
    ht.close()


# ---- 2. columns: widths, keys and payload, validity --------------------------------------------------------------------------
@pytest.mark.parametrize("kdt", DTS, ids=[np.dtype(d).name for d in DTS])
def test_every_width_as_key_and_payload(gpu_ctx, kdt):
    rng = np.random.default_rng(np.dtype(kdt).itemsize * 3 + (np.dtype(kdt).kind == "i"))
    n = 1500
    info = np.iinfo(kdt)
    key = rng.integers(max(int(info.min), -120), min(int(info.max), 120), n, dtype=kdt, endpoint=True)
    kvalid = (rng.random(n) > 0.1).astype(np.uint8)
    payload, pvalid = [], []
    for x, dt in enumerate(DTS):
        ii = np.iinfo(dt)
        p = rng.integers(int(ii.min), int(ii.max), n, dtype=dt, endpoint=True)
        p[::7] = rng.integers(0, 5, len(p[::7]))  # (a small domain among them: the filters below select on it)
        payload.append(p)
        pvalid.append((rng.random(n) > 0.25).astype(np.uint8) if x % 2 else None)
    strs = [None if rng.random() < 0.2 else bytes(rng.integers(97, 100, int(rng.integers(0, 20)), dtype=np.uint8)) for _ in range(n)]
    payload.append(strs)
    pvalid.append(None)
    side = Side([key], payload, [kvalid], pvalid)
    over_key = ("cmp", 0, ">=", 0)
    over_payload = ("or", ("cmp", 1 + 5, "<", 5), ("cmp", 1 + 1, "is null"), ("like", 1 + 8, "%ab%"))
    for expr in (over_key, over_payload, ("and", over_key, ("not", over_payload))):
        want = filtered(gpu_ctx, side, expr, null_cell=b"xxabxx", dirty_seed=3)
        assert 0 < len(want) < n
    # the cells themselves: kept NULL rows whose source cells hold garbage come out zero, kept valid cells bit for bit,
    # and a column has a validity array afterwards iff it had one before
    ht = side.upload(gpu_ctx, heaps=False, null_cell=b"xxabxx", dirty_seed=3)
    cols, valid, _ = ht._keep
    want = scanexpr.passing(over_key, side.cols(), n)
    assert ht.filter(over_key) == len(want)
    ht.finalize_hash()
    for (cells, ok), src, sv in zip(raw_columns(ht, [c.dtype.itemsize for c in cols]), cols, valid):
        assert (ok is None) == (sv is None)
        w = src.dtype.itemsize
        src = np.ascontiguousarray(src).view(np.uint8).reshape(n, w)[want]
        alive = np.ones(len(want), bool) if sv is None else sv[want].astype(bool)
        assert np.array_equal(cells, np.where(alive[:, None], src, 0))
        assert ok is None or np.array_equal(ok, sv[want])
    assert not all(v is None or v[want].all() for v in valid)
    ht.close()


def test_four_keys_and_62_payload_columns(gpu_ctx):
    rng = np.random.default_rng(66)
    n = 1300
    keys = [(np.arange(n) % 13).astype(np.int8), (np.arange(n) // 13).astype(np.int32), rng.integers(0, 3, n).astype(np.uint16),
            rng.integers(-5, 5, n).astype(np.int64)]
    payload = [rng.integers(0, 1 << 15, n).astype(DTS[i % 8]) for i in range(62)]
    pvalid = [(rng.random(n) > 0.2).astype(np.uint8) if i % 3 == 0 else None for i in range(62)]
    side = Side(keys, payload, None, pvalid)
    expr = ("or", ("cmp", 4 + 61, "<", 9000), ("and", ("cmp", 3, ">", 0), ("cmp", 4, "is not null")))
    want = scanexpr.passing(expr, side.cols(), n)
    ht = side.upload(gpu_ctx)
    assert ht.filter(expr) == len(want) and 0 < len(want) < n
    ids = check_downstream(gpu_ctx, side, want, ht)
    # the key tuples are unique: probe row p (the tuple of uploaded row p) finds uploaded row p iff the filter kept it
    assert np.array_equal(ids[:, 0], want) and np.array_equal(ht.filter_rows()[ids[:, 1]], want)
    ht.close()


# ---- 3. the other routes to a table -------------------------------------------------------------------------------------------
def test_table_from_rows(gpu_ctx):
    rng = np.random.default_rng(8)
    n = 2500
    key = rng.permutation(n).astype(np.int32)
    payload = [rng.integers(-100, 100, n).astype(np.int16), rng.integers(0, 1 << 60, n).astype(np.uint64)]
    pvalid = [(rng.random(n) > 0.2).astype(np.uint8), None]
    blob, row_width, offs, kept_rows = buildside.row_blob([key], [None], payload, pvalid)
    assert len(kept_rows) == n
    widths, signed = buildside.col_shape([key] + payload)
    ht = capi.HashTable.from_rows(gpu_ctx, blob, n, row_width, offs, widths, signed, 1, 2)
    # (upload_rows gives every column a validity array: all ones where the host has none)
    side = Side([key], payload, [np.ones(n, np.uint8)], [pvalid[0], np.ones(n, np.uint8)])
    filtered(gpu_ctx, side, ("and", ("cmp", 1, ">", -40), ("cmp", 0, "<", 2000)), ht=ht)
    ht.close()


def test_table_from_output(gpu_ctx):
    """pipeline A's output as a build side, filtered before it is finalized: fetch_ids of A, then filter_rows, name A's rows"""
    rng = np.random.default_rng(9)
    n, nb = 3000, 400
    j = Join(rng.permutation(nb).astype(np.int32), 0, payload=[rng.integers(0, 50, nb).astype(np.int32)], payload_valid=[None])
    pk = rng.integers(-20, nb + 20, n).astype(np.int32)
    tag = rng.permutation(n).astype(np.int64)
    hj = j.device(gpu_ctx)
    pipe = capi.Pipeline(gpu_ctx, [pk, tag], n, [(hj, [(-1, 0)])], [[0]])
    out = capi.Output(pipe, 64, n // 64 + 1 + MAX_WAVE_CHUNKS)
    pipe.probe_rounds([(0, n, 0, 1)], out=out)
    a = out.fetch_ids().astype(np.int64)
    live0 = capi.device_bytes_live()
    ht = capi.HashTable.from_output(out, [(-1, 1)], [(0, 0), (-1, 0)])
    side = Side([tag[a[:, 0]]], [j.payload[0][a[:, 1]], pk[a[:, 0]]], [np.ones(len(a), np.uint8)], [np.ones(len(a), np.uint8)] * 2)
    before, live1 = ht.info()["device_bytes"], capi.device_bytes_live()
    assert live1 - live0 == before  # (a table from_output made accounts for every byte of it)
    expr = ("in", 1, [3, 4, 5, 6, 7, 40])
    want = scanexpr.passing(expr, side.cols(), side.n)
    assert ht.filter(expr) == len(want) and 0 < len(want) < len(a) // 2
    # the allocation from_output made is gone: the table is smaller than it was, and the count says so
    assert capi.device_bytes_live() - live0 == ht.info()["device_bytes"] < before
    check_downstream(gpu_ctx, side, want, ht)
    ht.close()
    assert capi.device_bytes_live() == live0
    out.close()
    pipe.close()
    hj.close()


def test_device_columns_are_left_alone(gpu_ctx):
    """POLR_COL_DEVICE columns (torch tensors): never written, and no longer referenced once the call has returned"""
    import torch
    rng = np.random.default_rng(10)
    n = 5000
    key = rng.permutation(n).astype(np.int32)
    pay = rng.integers(-(1 << 50), 1 << 50, n).astype(np.int64)
    pval = (rng.random(n) > 0.3).astype(np.uint8)
    t_key, t_pay, t_val = (torch.from_numpy(a).to("cuda:0") for a in (key, pay, pval))
    live0 = capi.device_bytes_live()
    ht = capi.HashTable.from_cols(gpu_ctx, [capi.dev_col(t_key.data_ptr(), 4, True)],
                                  [capi.dev_col(t_pay.data_ptr(), 8, True, t_val.data_ptr())], n)
    assert ht.info()["device_bytes"] == 0
    side = Side([key], [pay], None, [pval])
    expr = ("or", ("cmp", 1, ">", 0), ("cmp", 1, "is null"))
    want = scanexpr.passing(expr, side.cols(), n)
    assert ht.filter(expr) == len(want)
    torch.cuda.synchronize()
    assert np.array_equal(t_key.cpu().numpy(), key) and np.array_equal(t_pay.cpu().numpy(), pay) and np.array_equal(t_val.cpu().numpy(), pval)
    assert ht.info()["device_bytes"] > 0 and capi.device_bytes_live() - live0 >= ht.info()["device_bytes"]
    # the tensors go, and their memory is overwritten: the table has no VARCHAR column, so it holds nothing of theirs
    t_key.fill_(-1)
    t_pay.fill_(-1)
    t_val.fill_(0)
    del t_key, t_pay, t_val
    torch.cuda.empty_cache()
    check_downstream(gpu_ctx, side, want, ht)
    ht.close()
    assert capi.device_bytes_live() == live0


# ---- 4. strings ---------------------------------------------------------------------------------------------------------------
def string_side(n, seed):
    rng = np.random.default_rng(seed)
    return Side([rng.permutation(n).astype(np.int32)],
                [scanstr.fixture_column(seed, n), rng.integers(0, 100, n).astype(np.int32), scanstr.fixture_column(seed + 1, n)],
                None, [None, (rng.random(n) > 0.1).astype(np.uint8), None])


@pytest.mark.parametrize("which", ["like", "in", "cmp", "mixed"])
def test_varchar_filters(gpu_ctx, which):
    """inline cells with dirty padding, heaps in two blocks, NULL rows whose cells would match"""
    side = string_side(3000, 21)
    strs = [s for s in side.payload[0] if s is not None]
    long = [s for s in strs if len(s) > 12]
    expr = {
        "like": ("like", 1, "%a%"),
        "in": ("in", 1, [b"", b"no row holds this", strs[5], strs[17], long[3], long[40], long[3][:12], long[3] + b"!"]),
        "cmp": ("cmp", 1, ">=", long[7]),
        "mixed": ("or", ("and", ("like", 1, "Jap%"), ("cmp", 2, "<", 50)), ("not", ("like", 3, "%_%")), ("cmp", 1, "is null")),
    }[which]
    want = filtered(gpu_ctx, side, expr, null_cell=b"Japan", dirty_seed=7, n_blocks=2)
    assert 0 < len(want) < side.n


def test_heap_set_after_the_filter(gpu_ctx):
    """for a column no leaf reads, polr_ht_set_payload_heaps may come afterwards: it rebases the kept cells only"""
    side = string_side(2000, 33)
    expr = ("and", ("like", 1, "%b%"), ("cmp", 2, ">=", 10))
    want = scanexpr.passing(expr, side.cols(), side.n)
    ht = side.upload(gpu_ctx, heaps=[0])  # the heap of payload column 2 has not come yet
    assert ht.filter(expr) == len(want)
    ht.set_payload_heaps(2, ht._keep[2][2])
    assert any(s is not None and len(s) > 12 for s in side.take(want).payload[2])
    check_downstream(gpu_ctx, side, want, ht)
    ht.close()


def test_heap_that_never_came(gpu_ctx):
    side = string_side(2000, 34)
    n_long = sum(1 for s in side.payload[0] if s is not None and len(s) > 12)
    live0 = capi.device_bytes_live()
    ht = side.upload(gpu_ctx, heaps=[2])
    live1, info1 = capi.device_bytes_live(), ht.info()
    with pytest.raises(capi.PolrError) as e:
        ht.filter(("like", 1, "%a%"))
    assert e.value.code == capi.E_INVALID and "filter column 1: %d rows hold strings longer than 12 bytes" % n_long in str(e.value)
    assert "polr_ht_set_payload_heaps" in str(e.value)
    assert capi.device_bytes_live() == live1 and ht.info() == info1
    # IS NULL reads no cell, and a filter over the other columns does not look at this one: both are accepted
    expr = ("and", ("cmp", 1, "is not null"), ("like", 3, "%a%"))
    want = scanexpr.passing(expr, side.cols(), side.n)
    assert ht.filter(expr) == len(want) and np.array_equal(ht.filter_rows(), want)
    # ... and the column is still the library's own: the heap comes now, for the kept cells
    ht.set_payload_heaps(0, ht._keep[2][0])
    check_downstream(gpu_ctx, side, want, ht)
    ht.close()
    assert capi.device_bytes_live() == live0


# ---- 5. the fixture of the reference engine -----------------------------------------------------------------------------------
GOLD = json.load(open(os.path.join(common.ROOT, "tests", "golden", "scan_expr.json"), encoding="utf-8"))


def test_fixture_of_the_reference_engine(gpu_ctx):
    """every WHERE clause of tests/golden/scan_expr.json over a table whose payload columns are the fixture's columns: the
    kept rows are the recorded row sets"""
    n = GOLD["n_rows"]
    values = scanstr.fixture_column(GOLD["seed"], n)
    assert scanstr.column_digest(values) == GOLD["column_sha1"]
    ints, ivalid = scanexpr.fixture_int(GOLD["int_seed"], n)
    side = Side([np.arange(n, dtype=np.int32)], [values, ints], None, [None, ivalid])
    cols, valid, blocks = side.device_payload(n_blocks=2)
    for q in GOLD["queries"]:
        ht = capi.HashTable.from_columns(gpu_ctx, side.keys, cols, payload_valid=valid)
        ht.set_payload_heaps(0, blocks[0])
        kept = ht.filter(scanexpr.bind(q["expr"], {"s": 1, "i": 2}))
        assert kept == q["count"] and scanstr.rows_digest(ht.filter_rows()) == {"count": q["count"], "sha1": q["sha1"]}, q["where"]
        ht.close()


# ---- 6. downstream ---------------------------------------------------------------------------------------------------------------
def test_finalize_on_filtered_tables(gpu_ctx):
    """a range that only the filtered rows keep duplicate-free finalizes perfect where the unfiltered table is a duplicate"""
    rng = np.random.default_rng(12)
    n = 4000
    key = np.concatenate([rng.permutation(3000), rng.integers(0, 3000, 1000)]).astype(np.int32)
    first = np.concatenate([np.ones(3000, np.uint8), np.zeros(1000, np.uint8)])
    order = rng.permutation(n)
    side = Side([key[order]], [first[order], rng.integers(0, 9, n).astype(np.int16)])
    plain = side.upload(gpu_ctx)
    assert plain.finalize_perfect(0, 2999) is False  # POLR_E_DUPLICATE
    plain.close()
    expr = ("cmp", 1, "=", 1)
    for how in ("hash", ("perfect", 0, 2999), ("auto", 0, 2999)):
        ht = side.upload(gpu_ctx)
        want = filtered(gpu_ctx, side, expr, ht=ht, how=how)
        assert len(want) == 3000 and ht.info()["kind"] == (2 if how == "hash" else 1) and ht.info()["n_rows"] == 3000
        ht.close()


def test_dictionary_after_the_filter(gpu_ctx):
    """SSB Q4.1: c_region = 'AMERICA' leaves the five nations of one region -- five codes, not 25"""
    rng = np.random.default_rng(13)
    n = 3000
    nation = rng.integers(0, 25, n)
    regions = [b"AFRICA", b"AMERICA", b"ASIA", b"EUROPE", b"MIDDLE EAST"]
    side = Side([np.arange(n, dtype=np.int32)], [[regions[x // 5] for x in nation], [b"NATION %02d of twenty-five" % x for x in nation]])
    ht = side.upload(gpu_ctx)
    want = scanexpr.passing(("cmp", 1, "=", "AMERICA"), side.cols(), n)
    assert ht.filter(("cmp", 1, "=", "AMERICA")) == len(want)
    code_col, n_codes, has_null = ht.encode_dictionary(1)
    kept = [side.payload[1][r] for r in want.tolist()]
    assert (code_col, n_codes, has_null) == (2, 5, 0) and sorted(ht.dictionary(code_col)) == sorted(set(kept))
    with pytest.raises(capi.PolrError) as e:  # filter first, then encode
        ht.filter(None)
    assert e.value.code == capi.E_INVALID and "payload column 1 is dictionary-encoded: filter first, then encode" in str(e.value)
    ht.finalize_hash()
    pk = np.arange(n, dtype=np.int32)
    ids, mats = probe_b(gpu_ctx, ht, [pk], None, [None, None, np.uint32])
    assert np.array_equal(ids[:, 0], want) and mats[1] == kept
    names = ht.dictionary(code_col)
    assert [names[c] for c in mats[2][0].tolist()] == kept
    ht.close()


def test_resident_run_over_a_filtered_table(gpu_ctx):
    """a two-join pipeline with one filtered table, run by the pool launch: COUNT(*) and the row set of the twin's"""
    rng = np.random.default_rng(14)
    n, nb = 20000, 1500
    j0 = Join(rng.permutation(nb).astype(np.int32), 0, payload=[rng.integers(0, 5, nb).astype(np.int32)], payload_valid=[None])
    j1 = Join(np.repeat(np.arange(300, dtype=np.int32), 2), 1)
    side = Side([j0.keys], [j0.payload[0]])
    want = scanexpr.passing(("in", 1, [1, 3]), side.cols(), nb)
    pcols = [rng.integers(-10, nb + 10, n).astype(np.int32), rng.integers(-5, 320, n).astype(np.int32)]
    results = []
    for filtered_here in (True, False):
        ht0 = side.upload(gpu_ctx) if filtered_here else side.take(want).upload(gpu_ctx)
        if filtered_here:
            assert ht0.filter(("in", 1, [1, 3])) == len(want)
        ht0.finalize_hash()
        ht1 = j1.device(gpu_ctx)
        pipe = capi.Pipeline(gpu_ctx, pcols, n, [(ht0, [(-1, 0)]), (ht1, [(-1, 1)])], [[0, 1], [1, 0]])
        out = capi.Output(pipe, 1024, 64 + MAX_WAVE_CHUNKS)
        mx = capi.DeviceMultiplexer(pipe, "adaptive_reinit")
        capi.run_resident([mx], [(0, (n + 1023) // 1024)], out=out, reset=True, finish=True)
        st = mx.finish()
        ids = out.fetch_ids().astype(np.int64)
        ids[:, 1] = want[ids[:, 1]]  # (both tables hold the kept rows in the same order)
        results.append((len(ids), sort_rows(ids)))
        assert sum(st["stage_out"][p][1] for p in range(2)) == len(ids)
        for h in (mx, out, pipe, ht0, ht1):
            h.close()
    ref = Ref(pcols, None, [Join(j0.keys[want], 0), j1]).rows()
    ref[:, 1] = want[ref[:, 1]]
    assert results[0][0] == results[1][0] == len(ref) > 0
    assert np.array_equal(results[0][1], results[1][1]) and np.array_equal(results[0][1], sort_rows(ref))


# ---- 7. refusals and atomicity ------------------------------------------------------------------------------------------------
def test_refusals_leave_the_table_as_it_was(gpu_ctx):
    rng = np.random.default_rng(15)
    n = 1200
    side = Side([rng.permutation(n).astype(np.int32)], [rng.integers(0, 10, n).astype(np.int32)] + [np.zeros(n, np.int8)] * 8)
    L = gpu_ctx.L
    live0 = capi.device_bytes_live()
    assert L.polr_ht_filter(None, None, None, 0, None, 0, None) == capi.E_INVALID  # NULL ht
    assert L.polr_ht_fetch_filter_rows(None, None, None, 0) == capi.E_INVALID
    ht = side.upload(gpu_ctx)
    live1, info1 = capi.device_bytes_live(), ht.info()

    def refused(code, text, *call):
        with pytest.raises(capi.PolrError) as e:
            call[0](*call[1:])
        assert e.value.code == code and text in str(e.value), str(e.value)
        assert capi.device_bytes_live() == live1 and ht.info() == info1

    refused(capi.E_INVALID, "never filtered", ht.filter_rows)
    refused(capi.E_INVALID, "node 0: column 10 out of range", ht.filter, ("cmp", 10, "=", 1))
    refused(capi.E_INVALID, "node 1: AND / OR needs two operands", ht.filter_raw, [("cmp", 1, 0, 0, 1), ("and", 0, 0, 0, 0)], [(1, None, 0)])
    refused(capi.E_UNSUPPORTED, "more than 8 distinct columns", ht.filter, ("or",) + tuple(("cmp", 1 + i, "=", 0) for i in range(9)))
    refused(capi.E_INVALID, "a count without its array", ht.filter_raw, [], [], None, 1, 0)
    # ... after which a filter behaves as if the refused calls had never been made
    expr = ("cmp", 1, "<", 4)
    want = scanexpr.passing(expr, side.cols(), n)
    assert ht.filter(expr) == len(want)
    info2 = ht.info()
    assert capi.device_bytes_live() - live1 == info2["device_bytes"] - info1["device_bytes"] < 0  # (the table shrank)
    live2 = capi.device_bytes_live()
    info1, live1 = info2, live2
    refused(capi.E_INVALID, "filtered already (once per table)", ht.filter, expr)
    rows = np.zeros(len(want), np.uint32)
    assert L.polr_ht_fetch_filter_rows(ht.h, None, rows.ctypes.data, len(want) - 1) == capi.E_OVERFLOW
    assert L.polr_ht_fetch_filter_rows(ht.h, None, rows.ctypes.data, len(want)) == 0 and np.array_equal(rows, want)
    check_downstream(gpu_ctx, side, want, ht)
    refused_info = ht.info()
    with pytest.raises(capi.PolrError) as e:  # a finalized table
        ht.filter(expr)
    assert e.value.code == capi.E_INVALID and "the table is finalized" in str(e.value) and ht.info() == refused_info
    ht.close()
    # tables that are finalized from the start: polr_pht_upload, polr_ht_alloc_like
    pht = capi.HashTable.from_perfect(gpu_ctx, 4, True, 0, 99, np.ones(100, np.uint8), [np.arange(100, dtype=np.int32)])
    meta, _ = pht.export()
    like = capi.HashTable.alloc_like(gpu_ctx, meta)
    for t in (pht, like):
        with pytest.raises(capi.PolrError) as e:
            t.filter(None)
        assert e.value.code == capi.E_INVALID and "the table is finalized" in str(e.value)
        t.close()
    assert capi.device_bytes_live() == live0


def test_live_bytes_are_at_their_baseline(gpu_ctx):
    """every table of this file was closed: nothing a filter allocated is left (a fresh table, filtered and closed)"""
    import gc
    gc.collect()
    live0 = capi.device_bytes_live()
    side = Side([np.arange(5000, dtype=np.int32)], [np.arange(5000, dtype=np.int64)], None, [np.ones(5000, np.uint8)])
    ht = side.upload(gpu_ctx)
    before, live1 = ht.info()["device_bytes"], capi.device_bytes_live()
    na, va, _keep = capi._filter_arrays(*capi.flatten_filter_expr(("cmp", 0, "<", 100)))
    assert gpu_ctx.L.polr_ht_filter(ht.h, None, na, 1, va, 1, None) == 0  # (n_kept may be NULL)
    assert capi.device_bytes_live() - live1 == ht.info()["device_bytes"] - before < 0
    rows = np.zeros(100, np.uint32)
    assert gpu_ctx.L.polr_ht_fetch_filter_rows(ht.h, None, rows.ctypes.data, 100) == 0 and np.array_equal(rows, np.arange(100))
    ht.close()
    assert capi.device_bytes_live() == live0
