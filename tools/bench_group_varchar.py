"""Times polr_out_aggregate_hashed_str against polr_out_aggregate_hashed (integer codes) over the same materialised output.
usage: python tools/bench_group_varchar.py <library.so> <tag>   -> one JSON line per shape (host clock around the C call, which
ends in a synchronise: 3 warm-up calls, then 9 timed ones; median, min, max).  Both entry points run polr_hash_agg_kernel:
the string sink its <true>, the integer sink its <false> instance.  To compare two builds of the library, run it on each,
alternating, one process each; kernel times: the same command under `rocprofv3 --kernel-trace --stats -- python ...` in a
run of its own per library.  Results: profiles/README.md"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "duckdb-polr_amd", "python"))
from polr_amd import capi, ssb_skew  # noqa: E402

capi.LIB_PATH = os.path.abspath(sys.argv[1])
TAG = sys.argv[2]
REPS, WARM = 9, 3


def cells_fixed(strs_u8):
    """(n, L) uint8 -> string_t cells + heap (every row its own heap copy when L > 12)"""
    n, L = strs_u8.shape
    cells = np.zeros((n, 16), np.uint8)
    cells[:, 0:4] = np.frombuffer(np.uint32(L).tobytes(), np.uint8)
    heap = np.ascontiguousarray(strs_u8).reshape(-1).copy()
    if L <= 12:
        cells[:, 4:4 + L] = strs_u8
    else:
        cells[:, 4:8] = strs_u8[:, :4]
        ptr = (heap.ctypes.data + np.arange(n, dtype=np.uint64) * np.uint64(L))
        cells[:, 8:16] = ptr.view(np.uint8).reshape(n, 8)
    return cells.reshape(-1).view("V16"), heap


def timed(fn):
    for _ in range(WARM):
        fn()
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return {"median_ms": round(ts[len(ts) // 2], 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4)}


def caller(ctx, out, cols, specs, max_groups, str_cap, string):
    ka = (capi.GroupKey * len(cols))()
    for i, (sj, sc) in enumerate(cols):
        ka[i].src_join, ka[i].src_col = sj, sc
    sa = (capi.AggSpec * len(specs))(*[capi.AggSpec(capi.AGG[fn], sj, sc) for fn, sj, sc in specs])
    keys = np.zeros((max_groups, len(cols)), np.int64)
    nulls = np.zeros(max_groups, np.uint32)
    res = (capi.AggValue * (max_groups * len(specs)))()
    arena = np.zeros(max(str_cap, 1), np.uint8)
    n_groups, used = C.c_uint64(), C.c_uint64()
    L = ctx.L

    def call():
        if string:
            rc = L.polr_out_aggregate_hashed_str(out.h, None, ka, len(cols), sa, len(specs), max_groups, keys.ctypes.data,
                                                 nulls.ctypes.data, res, C.byref(n_groups), arena.ctypes.data, str_cap, C.byref(used))
        else:
            rc = L.polr_out_aggregate_hashed(out.h, None, ka, len(cols), sa, len(specs), max_groups, keys.ctypes.data,
                                             nulls.ctypes.data, res, C.byref(n_groups))
        assert rc == 0, (rc, ctx.L.polr_last_error(ctx.h))
        return n_groups.value
    return call


def q41(ctx, sf, long_names):
    wl = ssb_skew.workload("q4.1", sf=sf)
    inst = wl["instance"]
    m = inst.lineorder(0, inst.n_lo, cols=["lo_revenue", "lo_supplycost"])
    names = list(wl["probe"]["cols"].keys()) + ["lo_revenue", "lo_supplycost"]
    cols = list(wl["probe"]["cols"].values()) + [m["lo_revenue"], m["lo_supplycost"]]
    n = len(cols[0])
    cust = wl["joins"][0]
    table = {c: (b"NATION NAME NUMBER %02d OF 25" % c if long_names else b"NATION %02d" % c) for c in range(64)}
    cust["strings"] = {"name": [table[int(c)] for c in cust["payload"]["c_nation"].tolist()]}
    joins = capi.build_joins(ctx, wl, auto=True)
    pipe = capi.Pipeline(ctx, cols, n, joins, [[0, 1, 2, 3]])
    out = capi.Output(pipe, 1024, n // 1024 + 1 + 8192)
    mpx = capi.DeviceMultiplexer(pipe, "default_path")
    capi.run_resident([mpx], [(0, (n + 1023) // 1024)], out=out, reset=True, finish=True)
    mpx.finish()
    rows = out.stats()[0]
    specs = [("sum", -1, names.index("lo_revenue")), ("sum", -1, names.index("lo_supplycost"))]
    s = caller(ctx, out, [(3, 0), (0, capi.string_payload_index(cust, "name"))], specs, 1024, 1 << 16, True)
    i = caller(ctx, out, [(3, 0), (0, 0)], specs, 1024, 0, False)
    assert s() == i()
    r = {"tag": TAG, "shape": "q41 sf=%g %s names" % (sf, "28-byte" if long_names else "9-byte"), "rows": rows, "groups": s(),
         "str": timed(s), "int": timed(i)}
    print(json.dumps(r), flush=True)


def distinct(ctx, n, L):
    rng = np.random.default_rng(1)
    strs = np.full((n, L), ord("k"), np.uint8)
    hexd = np.frombuffer(b"0123456789abcdef", np.uint8)
    ids = rng.permutation(n).astype(np.uint32)
    for d in range(8):
        strs[:, L - 1 - d] = hexd[(ids >> (4 * d)) & 15]
    cells, heap = cells_fixed(strs)
    codes = ids.astype(np.int64) * 0x9E3779B1
    val = rng.integers(-1 << 40, 1 << 40, n)
    ht = capi.HashTable.from_columns(ctx, [np.arange(n, dtype=np.int32)], [])
    assert ht.finalize_perfect(0, n - 1)
    pk = rng.permutation(n).astype(np.int32)
    pipe = capi.Pipeline(ctx, [pk, cells, codes, val], n, [(ht, [(-1, 0)])], [[0]])
    if L > 12:
        pipe.set_probe_heaps(1, [heap])
    out = capi.Output(pipe, 1024, n // 1024 + 1 + 8192)
    pipe.probe_rounds([(0, n, 0, 1)], out=out)
    assert out.stats()[0] == n
    specs = [("sum", -1, 3)]
    s = caller(ctx, out, [(-1, 1)], specs, n, n * (4 + L), True)
    i = caller(ctx, out, [(-1, 2)], specs, n, 0, False)
    assert s() == i() == n
    r = {"tag": TAG, "shape": "2^20 distinct %d-byte" % L, "rows": n, "groups": n, "str": timed(s), "int": timed(i)}
    print(json.dumps(r), flush=True)


ctx = capi.Context(0)
q41(ctx, 0.2, True)
q41(ctx, 0.2, False)
q41(ctx, 1.0, True)
distinct(ctx, 1 << 20, 20)
distinct(ctx, 1 << 20, 12)
