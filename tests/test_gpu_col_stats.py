"""polr_ht_column_stats / polr_pipeline_column_stats / polr_ht_finalize_auto_stats (HashTable.column_stats,
Pipeline.column_stats, HashTable.finalize_auto_stats): min / max / counts of columns that live on the device, and a finalize
call that takes them.

The reference is never the code under test: every device result is compared with tests/colstats.py, a few lines of numpy per
kind (checked against hand-written cases by tests/test_colstats_abi.py), over the host copy of the same column.  The results
are exact integers: nothing here has a tolerance.  polr_ht_finalize_auto_stats is compared with a TWIN table, built with
HashTable.from_columns and finalized with finalize_auto(numpy min, numpy max).

The row counts come from polr_col_stats_plan_info -- cells per load, rows per tile, the rows the grid covers before a
workgroup takes its second tile -- never from a restated kernel shape."""
import gc

import numpy as np
import pytest

import buildside
import colstats
import scanexpr
import scanstr
from joinref import MAX_WAVE_CHUNKS, Join, Ref, sort_rows
from polr_amd import capi
from test_gpu_ht_filter import DTS, Side
from test_gpu_ht_semi_filter import By, want_rows

pytestmark = pytest.mark.gpu

PERFECT, S8, S16 = 1, 2, 3
GARBAGE = np.frombuffer(b"\xff" * 16, "V16")[0]  # the cell of a NULL VARCHAR row: a length of 2^32 - 1 and a wild pointer


def ref_of(cols, valids, names, rows=None):
    return [colstats.reference(cols[c], valids[c], rows) for c in names]


def check_table(ctx, keys, payload, kvalid=None, pvalid=None, names=None):
    """upload with from_columns, take the statistics of `names` (default: every column) in one call, compare"""
    kvalid, pvalid = kvalid or [None] * len(keys), pvalid or [None] * len(payload)
    live0 = capi.device_bytes_live()
    ht = capi.HashTable.from_columns(ctx, keys, payload, key_valid=kvalid, payload_valid=pvalid)
    live1 = capi.device_bytes_live()
    names = list(range(len(keys) + len(payload))) if names is None else names
    got = ht.column_stats(names)
    assert got == ref_of(list(keys) + list(payload), list(kvalid) + list(pvalid), names)
    assert capi.device_bytes_live() == live1  # the scratch is gone
    ht.close()
    assert capi.device_bytes_live() == live0
    return got


# ---- 1. row counts: the edges of a load, a tile and the first stride ------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.int8, np.uint64], ids=["1_byte", "8_bytes"])
def test_row_counts_from_the_plan(gpu_ctx, dt):
    w = np.dtype(dt).itemsize
    info = capi.col_stats_plan_info(1 << 40, w)
    v, tile, stride = info["cells_per_load"], info["tile_rows"], info["stride_rows"]
    assert v == 16 // w and tile == v * info["loads_in_flight"] * 256 and stride == tile * info["n_workgroups"]
    assert capi.col_stats_plan_info(stride + 1, w)["n_workgroups"] * tile == stride  # some workgroup loops twice
    rng = np.random.default_rng(w)
    ii = np.iinfo(dt)
    big = rng.integers(int(ii.min) // 2, int(ii.max) // 2, stride + 1, dtype=dt)
    ok = (rng.random(stride + 1) > 0.1).astype(np.uint8)
    for n in (0, 1, 63, 64, 65, v - 1, v, v + 1, tile - 1, tile, tile + 1, tile + v, stride - 1, stride, stride + 1):
        col, valid = big[:n].copy(), ok[:n].copy()
        if n:  # the extremes in the last row, valid: a pass that stops short of it misses both... and in the first
            col[-1], valid[-1] = ii.max, 1
            col[0], valid[0] = (ii.min, 1) if n > 1 else (col[0], 1)
        payload = [col[::-1].copy()] if n <= tile + v else []  # (as payload too, without a validity array)
        got = check_table(gpu_ctx, [col], payload, [valid], [None] * len(payload))
        assert got[0]["n_rows"] == n and (n == 0 or got[0]["max_value"] == colstats.as_i64(ii.max))


# ---- 2. every width and signedness, as key and as payload -----------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS, ids=[np.dtype(d).name for d in DTS])
def test_every_width_and_signedness(gpu_ctx, dt):
    dt = np.dtype(dt)
    tile = capi.col_stats_plan_info(1, dt.itemsize)["tile_rows"]
    n = 2 * tile + 37
    rng = np.random.default_rng(dt.itemsize * 2 + (dt.kind == "i"))
    ii = np.iinfo(dt)
    lo, hi = int(ii.min) // 4, int(ii.max) // 4
    mid = lambda: rng.integers(lo, hi, n, dtype=dt)
    # the type's extremes -- INT64_MIN / INT64_MAX for int64 -- in the first row, the last row, the last row of a tile and the
    # first row of the next
    spots = [(0, n - 1), (tile - 1, tile), (n - 1, 0), (tile, tile - 1), (2 * tile - 1, 2 * tile)]
    cols, valids = [], []
    for at_min, at_max in spots:
        c = mid()
        c[at_min], c[at_max] = ii.min, ii.max
        cols.append(c)
        valids.append((rng.random(n) > 0.2).astype(np.uint8))
        valids[-1][[at_min, at_max]] = 1
    # a value whose top bit decides: -1 in every signed width is the maximum of negative numbers; 0x80 / 0x8000 / 0x80000000 /
    # 2^63 + 5 in an unsigned width is the maximum of small numbers and the minimum of large ones
    top = -1 if dt.kind == "i" else (2 ** 63 + 5 if dt.itemsize == 8 else 1 << (8 * dt.itemsize - 1))
    if dt.kind == "i":
        below = rng.integers(int(ii.min), -2, n, dtype=dt, endpoint=True)
        above = rng.integers(0, int(ii.max), n, dtype=dt, endpoint=True)
    else:
        below = rng.integers(0, (1 << (8 * dt.itemsize - 1)) - 1, n, dtype=dt, endpoint=True)
        above = rng.integers(top + 1, int(ii.max), n, dtype=dt, endpoint=True)
    for c, at in ((below, 5), (above, tile + 1)):
        c[at] = top
        cols.append(c)
        valids.append(None)
    # all equal; all NULL over garbage; NULL rows whose cells hold the extremes; no validity array over the full range
    cols.append(np.full(n, top, dtype=dt))
    valids.append(None)
    cols.append(rng.integers(int(ii.min), int(ii.max), n, dtype=dt, endpoint=True))
    valids.append(np.zeros(n, np.uint8))
    c, ok = mid(), (rng.random(n) > 0.3).astype(np.uint8)
    ends = np.array([ii.min, ii.max], dtype=dt)
    c[ok == 0] = ends[rng.integers(0, 2, int((ok == 0).sum()))]
    c[[0, tile - 1, tile, n - 1]], ok[[0, tile - 1, tile, n - 1]] = ends[[0, 1, 0, 1]], 0
    cols.append(c)
    valids.append(ok)
    cols.append(rng.integers(int(ii.min), int(ii.max), n, dtype=dt, endpoint=True))
    valids.append(None)
    assert len(cols) == 11
    # column 0 is the table's key, the others its payload; then the other way round: the last one the key
    got = check_table(gpu_ctx, cols[:1], cols[1:], valids[:1], valids[1:])
    assert [(g["min_value"], g["max_value"]) for g in got[:5]] == [(colstats.as_i64(ii.min), colstats.as_i64(ii.max))] * 5
    assert got[5]["max_value"] == colstats.as_i64(top) and got[6]["min_value"] == colstats.as_i64(top)
    assert got[7]["min_value"] == got[7]["max_value"] == colstats.as_i64(top) and got[7]["n_valid"] == n
    assert (got[8]["n_valid"], got[8]["min_value"], got[8]["max_value"]) == (0, 0, 0)
    assert lo <= (got[9]["min_value"] if dt.kind == "i" else got[9]["min_value"] & (2 ** 64 - 1)) and got[9]["n_valid"] == int(ok.sum())
    assert all(g["width"] == dt.itemsize and g["flags"] == (1 if dt.kind == "i" else 0) for g in got)
    check_table(gpu_ctx, cols[-1:], cols[:-1], valids[-1:], valids[:-1], names=[0, 10, 9, 1])


# ---- 3. bases that are only as aligned as their cells ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 40, 70001])
def test_misaligned_device_columns(gpu_ctx, n):
    """POLR_COL_DEVICE tensors that start 1, 3 and 7 elements into an allocation, their validity arrays at odd bytes"""
    import torch
    rng = np.random.default_rng(n)
    host, valid, tensors, dev = [], [], [], []
    key = rng.permutation(n).astype(np.int32)
    t_key = torch.from_numpy(key).to("cuda:0")
    for dt in (np.int8, np.uint8, np.int16, np.int32):
        for off, voff in ((1, 1), (3, 5), (7, 3)):
            ii = np.iinfo(dt)
            col = rng.integers(int(ii.min), int(ii.max), n, dtype=dt, endpoint=True)
            ok = (rng.random(n) > 0.25).astype(np.uint8)
            col[ok == 0] = ii.max
            ok[[0, n - 1]] = 1
            whole = torch.zeros(n + 16, dtype=getattr(torch, np.dtype(dt).name), device="cuda:0")
            vwhole = torch.ones(n + 16, dtype=torch.uint8, device="cuda:0")
            whole[:] = int(ii.max) if np.dtype(dt).kind == "u" else int(ii.min)  # (what a pass that strays outside would see)
            t, tv = whole[off:off + n], vwhole[voff:voff + n]
            t.copy_(torch.from_numpy(col))
            tv.copy_(torch.from_numpy(ok))
            assert t.data_ptr() % 16 == (off * np.dtype(dt).itemsize) % 16 and tv.data_ptr() % 2 == 1
            host.append(col)
            valid.append(ok)
            tensors += [whole, vwhole]
            dev.append(capi.dev_col(t.data_ptr(), np.dtype(dt).itemsize, np.dtype(dt).kind == "i", tv.data_ptr()))
    torch.cuda.synchronize()
    before = [t.clone() for t in tensors]
    live0 = capi.device_bytes_live()
    ht = capi.HashTable.from_cols(gpu_ctx, [capi.dev_col(t_key.data_ptr(), 4, True)], dev, n)
    live1 = capi.device_bytes_live()
    want = ref_of(host, valid, range(len(host)))
    assert ht.column_stats(range(1, 1 + len(host))) == want
    assert ht.column_stats([0]) == [colstats.reference(key)]
    # the same memory as a pipeline's probe columns
    j = Join(np.arange(8, dtype=np.int32), 0).device(gpu_ctx)
    pipe = capi.Pipeline(gpu_ctx, [capi.dev_col(t_key.data_ptr(), 4, True)] + dev, n, [(j, [(-1, 0)])], [[0]])
    live2 = capi.device_bytes_live()
    assert pipe.column_stats(range(1, 1 + len(host))) == want
    sel = np.sort(rng.permutation(n)[:max(1, n // 3)]).astype(np.uint32)
    pipe.set_selection(sel)
    live2 = capi.device_bytes_live()
    assert pipe.column_stats(range(1, 1 + len(host)), selected=True) == ref_of(host, valid, range(len(host)), rows=sel)
    assert capi.device_bytes_live() == live2
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(tensors, before))  # a caller's memory is only read
    for h in (pipe, j):
        h.close()
    assert capi.device_bytes_live() == live1
    ht.close()
    assert capi.device_bytes_live() == live0


# ---- 4. VARCHAR: lengths only ---------------------------------------------------------------------------------------------------
def test_varchar_lengths_without_a_heap(gpu_ctx):
    rng = np.random.default_rng(4)
    n = 2600
    lens = rng.choice([0, 1, 11, 12, 13, 14, 100], n)
    lens[[3, 1024, n - 1]] = 4096
    lens[[0, 1023]] = 0
    vals = [None if rng.random() < 0.2 else bytes([97 + i % 26]) * int(l) for i, l in enumerate(lens)]
    vals[3], vals[n - 1], vals[0] = b"q" * 4096, b"r" * 4096, b""
    cells, ok, _blocks = scanstr.cells(vals, null_cell=GARBAGE, dirty_seed=1)
    assert ok is not None and (colstats.lengths(cells)[ok == 0] == 2 ** 32 - 1).all()
    key = np.arange(n, dtype=np.int32)
    # the library uploads the cells; the heap never comes: the call reads lengths only and succeeds
    got = check_table(gpu_ctx, [key], [cells, cells.copy()], None, [ok, None])
    live = [len(v) for v in vals if v is not None]
    assert got[1] == {"min_value": 0, "max_value": 4096, "n_rows": n, "n_valid": len(live), "n_long": sum(l > 12 for l in live),
                      "long_bytes": sum(l for l in live if l > 12), "width": 16, "flags": 0}
    assert got[2]["max_value"] == 2 ** 32 - 1 and got[2]["n_valid"] == n  # (without the validity array the garbage counts)
    # only 12 and 13: the boundary of a long string
    edge = [b"x" * 12, b"y" * 13] * 40
    cells, ok, _ = scanstr.cells(edge)
    got = check_table(gpu_ctx, [np.arange(80, dtype=np.int64)], [cells])
    assert (got[1]["min_value"], got[1]["max_value"], got[1]["n_long"], got[1]["long_bytes"]) == (12, 13, 40, 520)


# ---- 5. every route to a table ---------------------------------------------------------------------------------------------------
def test_table_from_rows(gpu_ctx):
    rng = np.random.default_rng(50)
    n = 2500
    key = rng.permutation(n).astype(np.int32) - 700
    payload = [rng.integers(-100, 100, n).astype(np.int16), rng.integers(0, 1 << 63, n).astype(np.uint64) * np.uint64(2)]
    pvalid = [(rng.random(n) > 0.2).astype(np.uint8), None]
    blob, row_width, offs, _kept = buildside.row_blob([key], [None], payload, pvalid)
    widths, signed = buildside.col_shape([key] + payload)
    ht = capi.HashTable.from_rows(gpu_ctx, blob, n, row_width, offs, widths, signed, 1, 2)
    assert ht.column_stats([2, 0, 1]) == ref_of([key] + payload, [None] + pvalid, [2, 0, 1])
    ht.close()


def output_fixture(ctx, seed=51, n=3000, nb=400):
    """a one-join pipeline run into an output: (out, the handles to close, host arrays of its rows: tag, val, pk, name)"""
    rng = np.random.default_rng(seed)
    names = [None if i % 9 == 0 else b"name %03d %s" % (i % 37, b"z" * (i % 5 * 4)) for i in range(nb)]
    cells, ok, blocks = scanstr.cells(names)
    val = rng.integers(-20, 50, nb).astype(np.int32)
    vok = (rng.random(nb) > 0.1).astype(np.uint8)
    dim_key = rng.permutation(nb).astype(np.int32)
    hj = capi.HashTable.from_columns(ctx, [dim_key], [val, cells], payload_valid=[vok, ok])
    hj.set_payload_heaps(1, blocks)
    hj.finalize_hash()
    pk = rng.integers(-20, nb + 20, n).astype(np.int32)
    tag = (rng.permutation(n).astype(np.int64) - 1000) * 3
    pipe = capi.Pipeline(ctx, [pk, tag], n, [(hj, [(-1, 0)])], [[0]])
    out = capi.Output(pipe, 64, n // 64 + 1 + MAX_WAVE_CHUNKS)
    pipe.probe_rounds([(0, n, 0, 1)], out=out)
    a = out.fetch_ids().astype(np.int64)
    host = {"tag": tag[a[:, 0]], "val": val[a[:, 1]], "val_ok": vok[a[:, 1]], "pk": pk[a[:, 0]],
            "name": [names[r] for r in a[:, 1].tolist()]}
    return out, [out, pipe, hj], host, blocks


def test_table_and_pipeline_from_output(gpu_ctx):
    out, handles, h, _blocks = output_fixture(gpu_ctx)
    n = len(h["tag"])
    live0 = capi.device_bytes_live()
    ht = capi.HashTable.from_output(out, [(-1, 1)], [(0, 0), (-1, 0), (0, 1)])
    live1 = capi.device_bytes_live()
    name_cells, name_ok, _ = scanstr.cells(h["name"])
    want = [colstats.reference(h["tag"], np.ones(n, np.uint8)), colstats.reference(h["val"], h["val_ok"]),
            colstats.reference(h["pk"], np.ones(n, np.uint8)), colstats.reference(name_cells, name_ok)]
    assert ht.column_stats([0, 1, 2, 3]) == want and want[3]["n_long"] > 0 and capi.device_bytes_live() == live1
    # ... and as the source of a next pipeline
    j = Join(np.arange(8, dtype=np.int32), 0).device(gpu_ctx)
    live1 = capi.device_bytes_live()
    pipe = capi.Pipeline.from_output(out, [(-1, 0), (0, 0), (0, 1)], [(j, [(-1, 0)])], [[0]])
    live2 = capi.device_bytes_live()
    assert pipe.column_stats([1, 0, 2, 1]) == [want[1], want[2], want[3], want[1]] and capi.device_bytes_live() == live2
    n_sel, _ = pipe.scan_filter_expr(("cmp", 1, ">", 10))
    sel, _ = pipe.fetch_scan()
    assert 0 < n_sel < n
    assert pipe.column_stats([0, 1], selected=True) == [colstats.reference(h["pk"], np.ones(n, np.uint8), sel),
                                                        colstats.reference(h["val"], h["val_ok"], sel)]
    pipe.close()
    j.close()
    ht.close()
    assert capi.device_bytes_live() == live0
    for x in handles:
        x.close()


def test_after_filter_semi_filter_and_dictionary(gpu_ctx):
    """the statistics describe the rows the table holds now"""
    rng = np.random.default_rng(52)
    n = 5000
    nation = rng.integers(0, 25, n)
    names = [None if i % 11 == 0 else b"NATION %02d of twenty-five" % x for i, x in enumerate(nation)]
    side = Side([rng.permutation(n).astype(np.int32) + 10_000],
                [rng.integers(-3000, 3000, n).astype(np.int16), rng.integers(0, 1 << 40, n).astype(np.int64), names],
                None, [(rng.random(n) > 0.1).astype(np.uint8), None, None])
    ht = side.upload(gpu_ctx)
    cells, valid, _ = ht._keep
    cols, valids = side.keys + cells, [None] + valid
    assert ht.column_stats([0, 1, 2, 3]) == ref_of(cols, valids, [0, 1, 2, 3])
    expr = ("cmp", 1, "<", 700)
    kept = scanexpr.passing(expr, side.cols(), n)
    assert ht.filter(expr) == len(kept) and 0 < len(kept) < n
    got = ht.column_stats([0, 1, 2, 3])
    assert got == ref_of(cols, valids, [0, 1, 2, 3], rows=kept) and got[1]["max_value"] <= 699 and got[1]["n_rows"] == len(kept)
    # the kept rows only: the survivors of a SEMI join on the 8-byte column
    by = By([cols[2][kept][::3].copy()], kind=None)
    thin = side.take(kept)
    rows2 = kept[want_rows(thin, [(by, [2], False)])]
    d = by.device(gpu_ctx)
    assert ht.semi_filter([(d, [2], False)]) == len(rows2) and 0 < len(rows2) < len(kept)
    d.close()
    assert ht.column_stats([2, 0, 1, 3]) == ref_of(cols, valids, [2, 0, 1, 3], rows=rows2)
    # sorted codes with a validity array: max = n_codes - 1, n_valid = the non-NULL strings
    code_col, n_codes, has_null = ht.encode_dictionary(2, sorted=True, null_invalid=True)
    live = [names[r] for r in rows2.tolist() if names[r] is not None]
    st = ht.column_stats([1 + code_col])[0]
    assert (st["min_value"], st["max_value"], st["n_valid"], st["n_rows"], st["width"]) == (0, n_codes - 1, len(live), len(rows2), 4)
    assert n_codes == len(set(live)) and len(live) < len(rows2)
    ht.close()


def test_sixteen_columns_one_of_them_twice(gpu_ctx):
    rng = np.random.default_rng(53)
    n = 20011
    cols, valids = [], []
    for i in range(15):
        dt = DTS[i % 8]
        ii = np.iinfo(dt)
        cols.append(rng.integers(int(ii.min), int(ii.max), n, dtype=dt, endpoint=True))
        valids.append((rng.random(n) > 0.5).astype(np.uint8) if i % 3 else None)
    names = [14, 0, 7, 3, 9, 1, 2, 4, 5, 3, 6, 8, 10, 11, 12, 13]  # column 3 twice, keys and payload in any order
    got = check_table(gpu_ctx, cols[:2], cols[2:], valids[:2], valids[2:], names=names)
    assert len(got) == 16 and got[3] == got[9]


# ---- 6. pipelines ------------------------------------------------------------------------------------------------------------------
def test_probe_columns_and_selections(gpu_ctx):
    rng = np.random.default_rng(60)
    n = 30000
    cols = [rng.integers(-500, 500, n).astype(np.int32), rng.integers(0, 1 << 63, n).astype(np.uint64) * np.uint64(2) + np.uint64(1),
            rng.integers(-128, 127, n).astype(np.int8)]
    valids = [(rng.random(n) > 0.2).astype(np.uint8), None, (rng.random(n) > 0.5).astype(np.uint8)]
    j = Join(np.arange(100, dtype=np.int32), 0).device(gpu_ctx)
    pipe = capi.Pipeline(gpu_ctx, cols, n, [(j, [(-1, 0)])], [[0]], probe_valid=valids)
    live = capi.device_bytes_live()
    whole = ref_of(cols, valids, [0, 1, 2])
    assert pipe.column_stats([0, 1, 2]) == whole and capi.device_bytes_live() == live
    assert pipe.column_stats([0, 1, 2], selected=True) == whole  # no selection in force: all rows
    sel = rng.permutation(n)[:7001].astype(np.uint32)  # any order
    pipe.set_selection(sel)
    assert pipe.column_stats([2, 1, 0], selected=True) == ref_of(cols, valids, [2, 1, 0], rows=sel)
    assert pipe.column_stats([0, 1, 2]) == whole  # without the flag: all n_probe_rows
    n_sel, _ = pipe.scan_filter_expr(("and", ("cmp", 0, ">=", 100), ("cmp", 2, "is not null")))
    scan, _ = pipe.fetch_scan()
    assert 0 < n_sel == len(scan) < n
    live = capi.device_bytes_live()  # (the scan's buffers stay with the pipeline)
    got = pipe.column_stats([0, 1, 2], selected=True)
    assert capi.device_bytes_live() == live
    assert got == ref_of(cols, valids, [0, 1, 2], rows=scan) and got[0]["min_value"] == 100 and got[2]["n_valid"] == n_sel
    pipe.set_selection(np.zeros(0, np.uint32))  # an empty selection: zero rows, nothing launched
    empty = pipe.column_stats([0, 1], selected=True)
    assert empty == ref_of(cols, valids, [0, 1], rows=[]) and empty[0]["n_rows"] == 0 and empty[1]["width"] == 8
    pipe.set_selection(None)
    assert pipe.column_stats([1], selected=True) == whole[1:2]
    pipe.close()
    j.close()


# ---- 7. polr_ht_finalize_auto_stats against its twin ----------------------------------------------------------------------------------
def auto_cases():
    rng = np.random.default_rng(70)
    n = 3000
    c = {}
    c["dense_unique"] = ([rng.permutation(n).astype(np.int32) - 1200], [None], (), PERFECT)
    c["small_range_few_rows"] = ([(rng.permutation(900_000)[:50] + 5).astype(np.int64)], [None], (), PERFECT)
    c["sparse"] = ([rng.integers(0, 1 << 40, n).astype(np.int64)], [None], (), None)
    dup = rng.permutation(n).astype(np.int32)
    dup[17] = dup[2100]
    c["duplicate_in_a_dense_range"] = ([dup], [None], (), None)
    c["dense_with_null_keys_holding_extremes"] = ([np.where(np.arange(n) % 7 == 0, 2 ** 31 - 1, np.arange(n)).astype(np.int32)],
                                                  [(np.arange(n) % 7 != 0).astype(np.uint8)], (), PERFECT)
    c["unsigned_8_bytes_across_2_63"] = ([(np.arange(n, dtype=np.uint64) + np.uint64(2 ** 63 - 1500))[rng.permutation(n)]], [None], (), PERFECT)
    c["all_null"] = ([rng.permutation(n).astype(np.int32)], [np.zeros(n, np.uint8)], (), None)
    c["two_keys"] = ([rng.integers(0, 50, n).astype(np.int32), rng.integers(0, 50, n).astype(np.int32)], [None, None], (), None)
    c["by_value_key"] = ([rng.permutation(n).astype(np.int32)], [None], (capi.KEY_BY_VALUE,), None)
    return c


@pytest.mark.parametrize("name", list(auto_cases()))
def test_finalize_auto_stats_equals_finalize_auto_with_numpy_statistics(gpu_ctx, name):
    keys, kvalid, flags, kind = auto_cases()[name]
    n = len(keys[0])
    rng = np.random.default_rng(71)
    pay = rng.integers(0, 1000, n).astype(np.int32)
    live0 = capi.device_bytes_live()
    tables = []
    for twin in (True, False):
        ht = capi.HashTable.from_columns(gpu_ctx, keys, [pay], key_valid=kvalid)
        for c, f in enumerate(flags):
            ht.set_key_flags(c, f)
        st = colstats.reference(keys[0], kvalid[0])
        if not twin:
            got_kind, key_stats = ht.finalize_auto_stats()
            assert key_stats == st  # filled for key column 0 in every case
        elif st["n_valid"]:
            got_kind = ht.finalize_auto(st["min_value"], st["max_value"])
        else:
            got_kind = ht.finalize_hash().info()["kind"]  # no non-NULL key: there is no minimum to hand to finalize_auto
        assert got_kind == ht.info()["kind"] and (kind is None or got_kind == kind), (got_kind, kind)
        tables.append(ht)
    assert tables[0].info() == tables[1].info()
    # a two-join pipeline over each: the same row ids and the same counts
    j1 = Join(np.repeat(np.arange(40, dtype=np.int32), 2), len(keys))
    pcols = [np.concatenate([k[:2000], k[:500]]) for k in keys] + [rng.integers(-5, 45, 2500).astype(np.int32)]
    pvalid = [None if v is None else np.concatenate([v[:2000], v[:500]]) for v in kvalid] + [None]
    results = []
    for ht in tables:
        h1 = j1.device(gpu_ctx)
        pipe = capi.Pipeline(gpu_ctx, pcols, 2500, [(ht, [(-1, c) for c in range(len(keys))]), (h1, [(-1, len(keys))])],
                             [[0, 1], [1, 0]], probe_valid=pvalid)
        out = capi.Output(pipe, 64, 40 * 2500 // 64 + 1 + MAX_WAVE_CHUNKS)
        counts = pipe.probe_rounds([(0, 1300, 0, 1), (1300, 1200, 1, 1)], out=out)
        results.append((sort_rows(out.fetch_ids()), counts.copy()))
        for h in (out, pipe, h1):
            h.close()
    assert np.array_equal(results[0][0], results[1][0]) and np.array_equal(results[0][1], results[1][1])
    assert name == "all_null" or len(results[0][0]) > 0
    for ht in tables:
        ht.close()
    assert capi.device_bytes_live() == live0


def test_finalize_auto_stats_without_key_stats_and_on_a_finalized_table(gpu_ctx):
    L, C = gpu_ctx.L, capi.C
    ht = capi.HashTable.from_columns(gpu_ctx, [np.arange(500, dtype=np.int32)[::-1].copy()])
    kind = C.c_uint32()
    assert L.polr_ht_finalize_auto_stats(ht.h, None, C.byref(kind), None) == 0 and kind.value == PERFECT  # key_stats may be NULL
    info = ht.info()
    with pytest.raises(capi.PolrError) as e:  # as polr_ht_finalize_auto: a table is finalized once
        ht.finalize_auto_stats()
    assert e.value.code == capi.E_INVALID and "table already finalized" in str(e.value) and ht.info() == info
    ht.close()
    ht = capi.HashTable.from_columns(gpu_ctx, [np.arange(500, dtype=np.int32)])
    assert L.polr_ht_finalize_auto_stats(ht.h, None, None, None) == 0 and ht.info()["kind"] == PERFECT  # kind_out too
    ht.close()


# ---- 8. the chain without the host ---------------------------------------------------------------------------------------------------
def test_the_chain_needs_no_column_on_the_host(gpu_ctx):
    """from_output -> filter -> semi_filter -> encode_dictionary -> finalize_auto_stats, then a resident run into a grouped sink
    whose domains come from column_stats alone; the result against numpy over the same data"""
    out, handles, h, _blocks = output_fixture(gpu_ctx, seed=80, n=4000, nb=500)
    rng = np.random.default_rng(81)
    ht = capi.HashTable.from_output(out, [(-1, 1)], [(0, 0), (-1, 0), (0, 1)])  # key tag; payload val, pk, name
    for x in handles:
        x.close()
    expr = ("and", ("cmp", 1, ">=", -10), ("cmp", 2, "<", 450))
    by_keys = np.arange(0, 500, 3, dtype=np.int32)
    d = capi.HashTable.from_columns(gpu_ctx, [by_keys]).finalize_hash()
    n_kept = ht.filter(expr)
    n_kept = ht.semi_filter([(d, [2], False)])
    d.close()
    code_col, n_codes, _ = ht.encode_dictionary(2, sorted=True, null_invalid=True)
    val_st, code_st = ht.column_stats([1, 1 + code_col])
    kind, key_st = ht.finalize_auto_stats()
    # the same on the host
    ok = h["val_ok"].astype(bool) & (h["val"] >= -10) & (h["pk"] < 450) & np.isin(h["pk"], by_keys)
    rows = np.nonzero(ok)[0]
    assert n_kept == len(rows) and 50 < n_kept < len(ok)
    tag, val = h["tag"][rows], h["val"][rows]
    names = [h["name"][r] for r in rows.tolist()]
    codes_of = {s: i for i, s in enumerate(sorted(set(s for s in names if s is not None)))}
    assert n_codes == len(codes_of) and key_st == colstats.reference(tag) and kind == ht.info()["kind"] == PERFECT
    assert (val_st["min_value"], val_st["max_value"]) == (int(val.min()), int(val.max()))
    assert (code_st["min_value"], code_st["max_value"], code_st["n_valid"]) == (0, n_codes - 1, sum(s is not None for s in names))
    # the next pipeline: fact rows keyed by tag, grouped by (val, name code), domains from the statistics
    n = 20000
    fk = np.concatenate([rng.choice(h["tag"], n - 500), rng.integers(-5000, 12000, 500)]).astype(np.int64)
    x = rng.integers(-1000, 1000, n).astype(np.int32)
    other = rng.integers(-5, 320, n).astype(np.int32)
    j1 = Join(np.repeat(np.arange(300, dtype=np.int32), 2), 2)
    h1 = j1.device(gpu_ctx)
    pipe = capi.Pipeline(gpu_ctx, [fk, x, other], n, [(ht, [(-1, 0)]), (h1, [(-1, 2)])], [[0, 1], [1, 0]])
    sink = capi.Output(pipe, 1024, 64 + MAX_WAVE_CHUNKS)
    mx = capi.DeviceMultiplexer(pipe, "adaptive_reinit")
    capi.run_resident([mx], [(0, (n + 1023) // 1024)], out=sink, reset=True, finish=True)
    mx.finish()
    nv, nc = val_st["max_value"] - val_st["min_value"] + 1, code_st["max_value"] - code_st["min_value"] + 1
    values, counts, dropped = sink.aggregate_grouped([(0, 0, val_st["min_value"], nv), (0, code_col, code_st["min_value"], nc)],
                                                     [("count_star", -1, 0), ("sum", -1, 1)])
    ref = Ref([fk, x, other], None, [Join(tag, 0), j1]).rows()
    want_cnt, want_sum, want_dropped = np.zeros(nv * nc, np.int64), np.zeros(nv * nc, np.int64), 0
    for p, b in zip(ref[:, 0].tolist(), ref[:, 1].tolist()):
        if names[b] is None:
            want_dropped += 1  # a NULL group key is not aggregated
            continue
        g = (int(val[b]) - val_st["min_value"]) * nc + codes_of[names[b]]
        want_cnt[g] += 1
        want_sum[g] += int(x[p])
    assert len(ref) > 1000 and dropped == want_dropped
    assert [v[0] for v in values] == want_cnt.tolist()
    assert [v[1] if c else 0 for v, c in zip(values, want_cnt.tolist())] == want_sum.tolist()
    for hnd in (mx, sink, pipe, h1, ht):
        hnd.close()


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_touch_nothing(gpu_ctx):
    gc.collect()
    C = capi.C
    live0 = capi.device_bytes_live()
    ht = capi.HashTable.from_columns(gpu_ctx, [np.arange(900, dtype=np.int32)], [np.arange(900, dtype=np.int64), np.arange(900, dtype=np.int8)])
    done = capi.HashTable.from_columns(gpu_ctx, [np.arange(900, dtype=np.int32)], [np.arange(900, dtype=np.int64)]).finalize_hash()
    pht = capi.HashTable.from_perfect(gpu_ctx, 2, False, 100, 199, (np.arange(100) % 3 == 0).astype(np.uint8))
    like = capi.HashTable.alloc_like(gpu_ctx, done.export()[0])
    j = Join(np.arange(8, dtype=np.int32), 0).device(gpu_ctx)
    pipe = capi.Pipeline(gpu_ctx, [np.arange(700, dtype=np.int32), np.arange(700, dtype=np.int16)], 700, [(j, [(-1, 0)])], [[0]])
    live1 = capi.device_bytes_live()
    st = (capi.ColStats * 17)()

    def mark():
        for s in st:
            s.min_value, s.n_rows, s.width = -77, 99, 123

    def refused(code, text, call, *args, **kw):
        mark()
        with pytest.raises(capi.PolrError) as e:
            call(*args, stats=st, **kw)
        assert e.value.code == code and text in str(e.value), str(e.value)
        assert all((s.min_value, s.n_rows, s.width, s.n_valid) == (-77, 99, 123, 0) for s in st)  # stats is untouched
        assert capi.device_bytes_live() == live1

    T, P = "polr_ht_column_stats: ", "polr_pipeline_column_stats: "
    L = gpu_ctx.L
    cols1 = (C.c_uint32 * 1)(0)
    assert L.polr_ht_column_stats(None, None, cols1, 1, st) == capi.E_INVALID
    assert L.polr_pipeline_column_stats(None, None, cols1, 1, 0, st) == capi.E_INVALID
    refused(capi.E_INVALID, T + "cols is NULL", ht.column_stats_raw, None, 1)
    mark()
    assert L.polr_ht_column_stats(ht.h, None, cols1, 1, None) == capi.E_INVALID and capi.device_bytes_live() == live1
    assert "stats is NULL" in L.polr_last_error(gpu_ctx.h).decode()
    refused(capi.E_INVALID, T + "no columns (n_cols is 0)", ht.column_stats_raw, [0], 0)
    refused(capi.E_UNSUPPORTED, T + "17 columns (at most 16 in one call)", ht.column_stats_raw, [0] * 17, 17)
    for t in (done, pht, like):
        refused(capi.E_INVALID, T + "the table is finalized", t.column_stats_raw, [0], 1)
    refused(capi.E_INVALID, T + "cols[1]: column 3 out of range (3 columns)", ht.column_stats_raw, [2, 3, 4], 3)
    # ... in their order: the earlier one answers
    refused(capi.E_UNSUPPORTED, T + "17 columns", done.column_stats_raw, [9] * 17, 17)
    refused(capi.E_INVALID, T + "the table is finalized", done.column_stats_raw, [9], 1)
    refused(capi.E_INVALID, P + "cols is NULL", pipe.column_stats_raw, None, 1, 0)
    refused(capi.E_INVALID, P + "no columns (n_cols is 0)", pipe.column_stats_raw, [0], 0, 0)
    refused(capi.E_UNSUPPORTED, P + "17 columns (at most 16 in one call)", pipe.column_stats_raw, [0] * 17, 17, 2)
    refused(capi.E_INVALID, P + "flags 0x2 (0 or POLR_STATS_SELECTED)", pipe.column_stats_raw, [5], 1, 2)
    refused(capi.E_INVALID, P + "flags 0x3", pipe.column_stats_raw, [0], 1, 3)
    refused(capi.E_INVALID, P + "cols[0]: column 2 out of range (2 columns)", pipe.column_stats_raw, [2, 0], 2, 1)
    # after which the calls work as if nothing had been refused
    assert ht.column_stats([2, 0]) == [colstats.reference(np.arange(900, dtype=np.int8)), colstats.reference(np.arange(900, dtype=np.int32))]
    assert pipe.column_stats([1]) == [colstats.reference(np.arange(700, dtype=np.int16))]
    assert capi.device_bytes_live() == live1
    for hnd in (pipe, j, like, pht, done, ht):
        hnd.close()
    assert capi.device_bytes_live() == live0
