"""polr_out_materialize_strings (Output.materialize_strings_raw / materialize_strings): a VARCHAR column of a join result as
complete string_t cells plus a packed heap, against exact Python -- joinref's row set (the Bank asserts it), the Python
bytes lists this file built, the row order of fetch_ids.  Nothing the code under test computed is used as a reference.

Every case asserts which engine emitted the row ids (Bank: `launch_info(True)["flat"]`):
  path     the path kernel (probe_rounds) over a repeated-key hash table: a build row reaches several output rows
  generic  the generic pool (run_resident) over the same table
  flat     the emitting flat pool over a perfect table (string heap set before finalize_perfect)
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import common
from joinref import device_rows
from polr_amd import capi
from polr_amd import job_family as jf
from test_gpu_group_varchar import Bank
from test_gpu_sink_matrix import MAX_WAVE_CHUNKS, DevBuf, random_strings, string_blocks

pytestmark = pytest.mark.gpu

ENGINES = ["path", "generic", "flat"]
FILL = 0xA5


def cut_over():
    text = open(os.path.join(common.ROOT, "duckdb-polr_amd", "csrc", "polr_strcopy.h")).read()
    return int(re.search(r"#define POLR_STRCOPY_LANE_MAX (\d+)u", text).group(1))


# ---- banks, built once and shared: the tests only read them ---------------------------------------------------------------
_BANKS = {}


def bank(ctx, key, **kw):
    if key not in _BANKS:
        _BANKS[key] = Bank(ctx, **kw)
    return _BANKS[key]


@pytest.fixture(scope="module", autouse=True)
def _close_banks():
    yield
    for b in _BANKS.values():
        b.close()
    _BANKS.clear()


def main_bank(ctx, engine, cap):
    return bank(ctx, ("main", engine, cap), engine=engine, seed=300 + 10 * ENGINES.index(engine) + (cap > 64), cap=cap,
                probe_blocks=1, build_blocks=3, dirty=True)


# ---- the exact expectation ------------------------------------------------------------------------------------------------
def wanted(b, name):
    """the column's values over the output rows in the order of fetch_ids: ([bytes or None], table rows)"""
    ids = device_rows(b.out.fetch_ids(), [b.join])
    rows = (ids[:, 0] if name in Bank.PROBE else ids[:, 1]).tolist()
    vals, valid = b.cols[name], b.valid[name]
    return [vals[r] if valid[r] else None for r in rows], rows


def packed(want):
    """(offsets of the long rows by output row, heap bytes)"""
    offs, at, parts = {}, 0, []
    for i, v in enumerate(want):
        if v is not None and len(v) > 12:
            offs[i] = at
            at += len(v)
            parts.append(v)
    return offs, b"".join(parts)


def wanted_cells(want, base):
    """the destination cells, byte for byte: NULL rows all-zero, inline strings zero-padded, long ones with the pointer
    base + packed offset"""
    offs, _ = packed(want)
    out = []
    for i, v in enumerate(want):
        if v is None:
            out.append(bytes(16))
        elif len(v) <= 12:
            out.append(len(v).to_bytes(4, "little") + v + bytes(12 - len(v)))
        else:
            out.append(len(v).to_bytes(4, "little") + v[:4] + (base + offs[i]).to_bytes(8, "little"))
    return out


def check(want, cells, valid, heap, used, base):
    """cells [n*16] uint8, valid [n] uint8, heap uint8: everything the contract states, row by row"""
    n = len(want)
    assert len(valid) == n and len(cells) == 16 * n
    assert valid.tolist() == [int(v is not None) for v in want]
    _, blob = packed(want)
    assert used == len(blob)
    assert heap[:used].tobytes() == blob
    got = cells.tobytes()
    exp = wanted_cells(want, base)
    if got != b"".join(exp):
        bad = [i for i in range(n) if got[16 * i:16 * i + 16] != exp[i]]
        assert not bad, (bad[:5], want[bad[0]], got[16 * bad[0]:16 * bad[0] + 16], exp[bad[0]])


def host_call(b, name, stream=None):
    cells, valid, heap, used = b.out.materialize_strings_raw(*b.col(name), stream=stream)
    return cells.view(np.uint8), valid, heap, used, heap.ctypes.data


# ---- main case ------------------------------------------------------------------------------------------------------------
MAIN = [(e, cap) for e in ENGINES for cap in (64, 1024)]


@pytest.mark.parametrize("engine,cap", MAIN, ids=["%s-%d" % c for c in MAIN])
def test_cells_and_heap_row_by_row(gpu_ctx, engine, cap):
    """probe-side column (heap in 1 block) and build-side column (heap in 3 blocks; a perfect table's re-ordered copy for
    `flat`), NULL rows whose source cells hold garbage lengths and pointers, dirty padding in the inline cells, chunk
    capacities 64 and 1024"""
    b = main_bank(gpu_ctx, engine, cap)
    for name in ("p_s", "b_s"):
        want, rows = wanted(b, name)
        assert len(want) > 5000 and None in want
        assert sum(v is not None and len(v) > 12 for v in want) > 1000 and sum(v is not None and len(v) < 12 for v in want) > 1000
        if name == "b_s" and engine != "flat":
            # the repeated-key table hands one build row to several output rows: each gets its own copy
            assert np.bincount(np.asarray(rows)).max() >= 2
        check(want, *host_call(b, name))
        # the decoded form
        assert b.out.materialize_strings(*b.col(name)) == want


def test_alignments_and_long_strings(gpu_ctx):
    """lengths around the cut-over between "a lane alone" and "the whole wave", 4097 and 100 000 bytes among short strings;
    all 64 pairs of (source offset mod 8, destination offset mod 8) occur among the long strings -- from the layout this
    test built: the source heap is one block packed in table order, the destination heap is packed in output order"""
    cut = cut_over()
    rng = np.random.default_rng(77)
    n = 20_000
    special = [cut - 1, cut, cut + 1, 4097, 100_000]
    lens = rng.integers(0, 45, n)
    for k, ln in enumerate(special):
        lens[100 + 16 * k:100 + 16 * k + 16] = ln  # (16 rows each: which of them find a join partner is the seed's business)
    strs = [rng.integers(0, 256, int(ln), dtype=np.uint8).tobytes() for ln in lens]
    p_valid = (rng.random(n) > 0.08).astype(np.uint8)
    p_valid[100:100 + 16 * len(special)] = 1
    b = bank(gpu_ctx, "align", engine="generic", seed=411, p_strs=strs, p_valid=p_valid, cap=64, dirty=True)
    want, rows = wanted(b, "p_s")
    assert {len(v) for v in want if v is not None} >= set(special)
    # where the test put the strings: source offsets in table order, destination offsets in output order
    src_off, at = {}, 0
    for r, v in enumerate(strs):
        if p_valid[r] and len(v) > 12:
            src_off[r] = at
            at += len(v)
    dst_off, _ = packed(want)
    pairs = {(src_off[rows[i]] % 8, off % 8) for i, off in dst_off.items()}
    assert len(pairs) == 64, sorted(set((s, d) for s in range(8) for d in range(8)) - pairs)
    wave = {(src_off[rows[i]] % 8, off % 8) for i, off in dst_off.items() if len(want[i]) > cut}
    assert len(wave) >= 8  # (the whole-wave form meets several alignments, too)
    check(want, *host_call(b, "p_s"))


# ---- protocol -------------------------------------------------------------------------------------------------------------
def raw(ctx, out, col, cells, valid, n, heap, cap, flags=0):
    used = C.c_uint64(0xDEAD)
    rc = ctx.L.polr_out_materialize_strings(out.h, None, col[0], col[1], cells, valid, n, heap, cap, C.byref(used), flags)
    return rc, used.value


def filled(n):
    return np.full(n, FILL, np.uint8)


def test_sizing_overflow_and_retry(gpu_ctx):
    b = main_bank(gpu_ctx, "generic", 64)
    want, _ = wanted(b, "b_s")
    n, (_, blob) = len(want), packed(want)
    live0 = capi.device_bytes_live()
    cells, valid, heap = filled(16 * n), filled(n), filled(len(blob))
    # the sizing call: no heap at all
    rc, used = raw(gpu_ctx, b.out, b.col("b_s"), cells.ctypes.data, valid.ctypes.data, n, None, 0)
    assert rc == capi.E_OVERFLOW and used == len(blob)
    # one byte short
    rc, used = raw(gpu_ctx, b.out, b.col("b_s"), cells.ctypes.data, valid.ctypes.data, n, heap.ctypes.data, len(blob) - 1)
    assert rc == capi.E_OVERFLOW and used == len(blob)
    assert (cells == FILL).all() and (valid == FILL).all() and (heap == FILL).all()
    assert capi.device_bytes_live() == live0
    # the retry
    rc, used = raw(gpu_ctx, b.out, b.col("b_s"), cells.ctypes.data, valid.ctypes.data, n, heap.ctypes.data, len(blob))
    assert rc == capi.OK
    check(want, cells, valid, heap, used, heap.ctypes.data)
    assert capi.device_bytes_live() == live0
    # more room than needed, and no validity array
    heap2, cells2 = filled(len(blob) + 64), filled(16 * n)
    rc, used = raw(gpu_ctx, b.out, b.col("b_s"), cells2.ctypes.data, None, n, heap2.ctypes.data, len(heap2))
    assert rc == capi.OK and used == len(blob) and (heap2[used:] == FILL).all()
    check(want, cells2, valid, heap2, used, heap2.ctypes.data)
    with pytest.raises(capi.PolrError) as e:
        b.out.materialize_strings_raw(*b.col("b_s"), heap_cap=len(blob) - 1)
    assert e.value.code == capi.E_OVERFLOW


def inline_strings(rng, n):
    return [v for v in random_strings(rng, 4 * n) if len(v) <= 12][:n]


def test_no_heap_needed(gpu_ctx):
    """all-inline, all-NULL and empty outputs succeed with dst_heap = NULL and heap_used = 0; the all-inline bank never
    handed a heap over (heaps=False), which such a column does not need"""
    rng = np.random.default_rng(5)
    n, nb = 20_000, 3000
    b = bank(gpu_ctx, "inline", engine="path", seed=421, p_strs=inline_strings(rng, n), b_strs=inline_strings(rng, nb),
             heaps=False, dirty=True)
    for name in ("p_s", "b_s"):
        want, _ = wanted(b, name)
        m = len(want)
        assert m > 5000 and all(v is None or len(v) <= 12 for v in want) and any(v is not None and len(v) == 12 for v in want)
        cells, valid = filled(16 * m), filled(m)
        rc, used = raw(gpu_ctx, b.out, b.col(name), cells.ctypes.data, valid.ctypes.data, m, None, 0)
        assert rc == capi.OK and used == 0
        check(want, cells, valid, np.zeros(0, np.uint8), used, 0)
        assert b.out.materialize_strings(*b.col(name)) == want
    # all NULL: the source cells hold garbage, none is read
    bn = bank(gpu_ctx, "all-null", engine="generic", seed=422, p_valid=np.zeros(n, np.uint8))
    want, _ = wanted(bn, "p_s")
    m = len(want)
    assert m > 5000 and set(want) == {None}
    cells, valid = filled(16 * m), filled(m)
    rc, used = raw(gpu_ctx, bn.out, bn.col("p_s"), cells.ctypes.data, valid.ctypes.data, m, None, 0)
    assert rc == capi.OK and used == 0 and not cells.any() and not valid.any()
    # no rows: an output nothing has been emitted into
    empty = capi.Output(bn.pipe, 64, 16)
    rc, used = raw(gpu_ctx, empty, bn.col("p_s"), None, None, 0, None, 0)
    assert rc == capi.OK and used == 0
    assert empty.materialize_strings(*bn.col("p_s")) == []
    empty.close()


def test_refusals_write_nothing(gpu_ctx):
    b = main_bank(gpu_ctx, "generic", 64)
    want, _ = wanted(b, "p_s")
    n, (_, blob) = len(want), packed(want)
    cells, valid, heap = filled(16 * n), filled(n), filled(len(blob))
    live0 = capi.device_bytes_live()
    p = (cells.ctypes.data, valid.ctypes.data)
    calls = {
        "an integer column": (b.col("p_i"), *p, n, heap.ctypes.data, len(blob)),
        "a column out of range": ((0, 17), *p, n, heap.ctypes.data, len(blob)),
        "too few rows": (b.col("p_s"), *p, n - 1, heap.ctypes.data, len(blob)),
        "no cells": (b.col("p_s"), None, valid.ctypes.data, n, heap.ctypes.data, len(blob)),
        "heap NULL with a capacity": (b.col("p_s"), *p, n, None, len(blob)),
    }
    for what, args in calls.items():
        rc, used = raw(gpu_ctx, b.out, *args)
        assert rc == capi.E_INVALID and used == 0, what
        assert (cells == FILL).all() and (valid == FILL).all() and (heap == FILL).all(), what
        assert capi.device_bytes_live() == live0, what
    msg = gpu_ctx.L.polr_last_error(gpu_ctx.h).decode()
    assert "NULL" in msg
    rc, _ = raw(gpu_ctx, b.out, b.col("p_s"), *p, n - 1, heap.ctypes.data, len(blob))
    assert "destination holds %d rows, output has %d" % (n - 1, n) in gpu_ctx.L.polr_last_error(gpu_ctx.h).decode()
    # a column the library uploaded whose heap never came, with long strings among the output rows
    bh = bank(gpu_ctx, "no-heaps", engine="path", seed=423, heaps=False)
    for name in ("p_s", "b_s"):
        want, _ = wanted(bh, name)
        m, (_, blob) = len(want), packed(want)
        assert len(blob) > 0
        cells, valid, heap = filled(16 * m), filled(m), filled(len(blob))
        live0 = capi.device_bytes_live()  # (this bank's memory included)
        rc, used = raw(gpu_ctx, bh.out, bh.col(name), cells.ctypes.data, valid.ctypes.data, m, heap.ctypes.data, len(blob))
        assert rc == capi.E_INVALID and used == 0
        assert "heap was never put on the device" in gpu_ctx.L.polr_last_error(gpu_ctx.h).decode()
        assert (cells == FILL).all() and (valid == FILL).all() and (heap == FILL).all()
        assert capi.device_bytes_live() == live0


# ---- device destination -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ENGINES)
def test_device_destination(gpu_ctx, engine):
    b = main_bank(gpu_ctx, engine, 1024)
    for name in ("p_s", "b_s"):
        want, _ = wanted(b, name)
        n, (_, blob) = len(want), packed(want)
        dc, dv, dh = DevBuf(16 * n), DevBuf(n), DevBuf(len(blob))
        dc.upload(filled(16 * n))
        dv.upload(filled(n))
        dh.upload(filled(len(blob)))
        live0 = capi.device_bytes_live()
        rc, used = raw(gpu_ctx, b.out, b.col(name), dc.ptr, dv.ptr, n, dh.ptr, len(blob) - 1, capi.COL_DEVICE)
        assert rc == capi.E_OVERFLOW and used == len(blob)
        assert (dc.download() == FILL).all() and (dv.download() == FILL).all() and (dh.download() == FILL).all()
        rc, used = raw(gpu_ctx, b.out, b.col(name), dc.ptr, dv.ptr, n, dh.ptr, len(blob), capi.COL_DEVICE)
        assert rc == capi.OK
        gpu_ctx.sync()
        assert capi.device_bytes_live() == live0
        check(want, dc.download(), dv.download(), dh.download(), used, dh.ptr)
        for d in (dc, dv, dh):
            d.free()


def test_binding_returns_device_tensors(gpu_ctx):
    """Output.materialize_strings_raw(device=True): torch tensors, the cells' pointers inside the heap tensor (the time of
    this test is torch's own start when nothing has imported it before)"""
    b = main_bank(gpu_ctx, "generic", 1024)
    want, _ = wanted(b, "b_s")
    cells, valid, heap, used = b.out.materialize_strings_raw(*b.col("b_s"), device=True)
    assert cells.is_cuda and heap.is_cuda
    check(want, cells.cpu().numpy().reshape(-1), valid.cpu().numpy(), heap.cpu().numpy(), used, heap.data_ptr())


# ---- agreement with the existing sinks ----------------------------------------------------------------------------------------
def test_job_pipeline_agrees_with_the_string_min_max_sink(gpu_ctx):
    """a JOB-shaped pipeline built as tests/test_job_family.py builds them, with a MIN(varchar) select list that is
    non-NULL at the fixture's scale: MIN / MAX of the materialised strings = polr_out_aggregate_string"""
    from test_job_family import _each_last_once, _tables
    gold = common.load_golden("job_family")
    shapes = jf.shapes()
    name = next(q for q in sorted(shapes) if gold["queries"][q]["select_min"]
                and all(m is not None for m in gold["queries"][q]["select_min"]) and gold["queries"][q]["count_star"] >= 50)
    g = gold["queries"][name]
    wl = jf.workload(name, _tables(gold["scale"]), shapes[name])
    pn = list(wl["probe"]["cols"].keys())
    paths = _each_last_once(wl)
    joins = capi.build_joins(gpu_ctx, wl, auto=True)
    cols = list(wl["probe"]["cols"].values())
    pstr = [capi.string_cells(v) for v in wl["probe"].get("strings", {}).values()]
    pipe = capi.Pipeline(gpu_ctx, cols + [c for c, _h in pstr], len(cols[0]), joins, paths)
    for i, (_c, heap) in enumerate(pstr):
        pipe.set_probe_heap(len(cols) + i, heap)
    flt = wl["probe"].get("filter")
    if flt:
        _n, n_chunks = pipe.scan_filter([(pn.index(c), op, const) for c, op, const in flt])
    else:
        n_chunks = (len(cols[0]) + 1023) // 1024
    out = capi.Output(pipe, 1024, 16384)
    mpx = capi.DeviceMultiplexer(pipe, "adaptive_reinit")
    if flt:
        mpx.use_scan_chunks()
    capi.run_resident([mpx], [(0, n_chunks)], out=out, reset=True, finish=True)
    mpx.finish()
    assert out.stats()[0] == g["count_star"]
    for (sj, col), ref_min in zip(wl["select"], g["select_min"]):
        src = (-1, len(cols) + list(wl["probe"]["strings"].keys()).index(col)) if sj < 0 else \
            (sj, capi.string_payload_index(wl["joins"][sj], col))
        live = [v for v in out.materialize_strings(*src) if v is not None]
        assert len(live) > 0
        assert min(live) == out.aggregate_string("min", *src) == ref_min.encode()
        assert max(live) == out.aggregate_string("max", *src)
    mpx.close()
    out.close()
    pipe.close()
    for ht, _ in joins:
        ht.close()


def test_dictionary_column_agrees(gpu_ctx):
    """a dictionary-encoded build column: the materialised strings are fetch_dictionary()[code] row by row, NULL rows carry
    the code n_codes"""
    rng = np.random.default_rng(9)
    nb, n = 3000, 20_000
    bk = rng.permutation(np.repeat(np.arange(0, nb, 2, dtype=np.int32), 2))
    pool = random_strings(rng, 60)
    strs = [pool[i] for i in rng.integers(0, len(pool), nb)]
    valid = (rng.random(nb) > 0.1).astype(np.uint8)
    cells, blocks = string_blocks(strs, valid, 2, seed=9)
    ht = capi.HashTable.from_columns(gpu_ctx, [bk], [cells], payload_valid=[valid])
    ht.set_payload_heaps(0, blocks)
    code_col, n_codes, has_null = ht.encode_dictionary(0)
    ht.finalize_hash()
    pk = rng.integers(-100, nb + 100, n).astype(np.int32)
    pipe = capi.Pipeline(gpu_ctx, [pk], n, [(ht, [(-1, 0)])], [[0]])
    out = capi.Output(pipe, 64, 2 * n // 64 + 1 + MAX_WAVE_CHUNKS)
    pipe.probe_rounds([(0, n, 0, 1)], out=out)
    words = ht.dictionary(code_col)
    assert len(words) == n_codes and has_null == 1 and set(words) == {s for s, ok in zip(strs, valid) if ok}
    codes, _ = out.materialize(0, code_col, np.uint32)
    got = out.materialize_strings(0, 0)
    assert len(got) == len(codes) > 5000
    assert got == [None if c == n_codes else words[c] for c in codes.tolist()]
    ids = out.fetch_ids()
    assert got == [strs[r] if valid[r] else None for r in ids[:, 1].tolist()]
    out.close()
    pipe.close()
    ht.close()
