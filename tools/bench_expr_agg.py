"""Times the three aggregate sinks over the SSB-skew Q4.1 join output (sf 1: 6 M lineorder rows): the plain calls with their
current specs -- SUM(lo_revenue), SUM(lo_supplycost), the two sums flight 4 is assembled from -- and, where the library has
them, the expression calls with the one aggregate SUM(lo_revenue - lo_supplycost).

usage: python tools/bench_expr_agg.py <library.so> <tag>   -> one JSON line per sink and form.

Per call form: 3 warm-up calls, then 7 windows of 20 calls each between two HIP events on the context's stream (a window is
several milliseconds; every call ends in a synchronise, so the window holds the calls' kernels, copies and host steps), and the
host clock around the same windows (profiler off: the end-to-end number).  Reported per call: median, min, max of the windows.
To compare two builds, run it on each, alternating, one process each (A B A B); a library from before the expression form
reports the plain calls only.  Results: profiles/README.md"""
import ctypes as C
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "duckdb-polr_amd", "python"))
from polr_amd import capi, ssb_skew  # noqa: E402

capi.LIB_PATH = os.path.abspath(sys.argv[1])
TAG = sys.argv[2]
WARM, WINDOWS, CALLS = 3, 7, 20
EXPR_NAMES = ["polr_out_aggregate_expr", "polr_out_aggregate_grouped_expr", "polr_out_aggregate_hashed_expr"]

# a library from before the expression form (the parent of a comparison) lacks three symbols the binding declares prototypes
# for when it loads: give it placeholders that are never called
_cdll = C.CDLL
_probe = _cdll(capi.LIB_PATH)
HAS_EXPR = all(hasattr(_probe, n) for n in EXPR_NAMES)


def _open(path, *a, **kw):
    lib = _cdll(path, *a, **kw)
    if os.path.abspath(str(path)) == capi.LIB_PATH and not HAS_EXPR:
        for n in EXPR_NAMES:
            setattr(lib, n, types.SimpleNamespace())
    return lib


C.CDLL = _open
capi.load()
C.CDLL = _cdll

hip = C.CDLL("libamdhip64.so")
hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
hip.hipEventSynchronize.argtypes = [C.c_void_p]
hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]


def timed(stream, fn):
    for _ in range(WARM):
        fn()
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    dev, host = [], []
    for _ in range(WINDOWS):
        t0 = time.perf_counter()
        assert hip.hipEventRecord(e0, stream) == 0
        for _ in range(CALLS):
            fn()
        assert hip.hipEventRecord(e1, stream) == 0 and hip.hipEventSynchronize(e1) == 0
        host.append((time.perf_counter() - t0) * 1e6 / CALLS)
        ms = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
        dev.append(ms.value * 1e3 / CALLS)
    hip.hipEventDestroy(e0)
    hip.hipEventDestroy(e1)

    def stats(v):
        v = sorted(v)
        return {"median_us": round(v[len(v) // 2], 1), "min_us": round(v[0], 1), "max_us": round(v[-1], 1)}
    return {"events": stats(dev), "host": stats(host), "window_ms": round(sorted(dev)[len(dev) // 2] * CALLS / 1e3, 2)}


def main():
    ctx = capi.Context(0)
    L = ctx.L
    wl = ssb_skew.workload("q4.1", sf=1.0)
    inst = wl["instance"]
    m = inst.lineorder(0, inst.n_lo, cols=["lo_revenue", "lo_supplycost"])
    names = list(wl["probe"]["cols"].keys()) + ["lo_revenue", "lo_supplycost"]
    # (INTEGER measures: the type under which the reference answers the difference)
    cols = list(wl["probe"]["cols"].values()) + [m["lo_revenue"].astype(np.int32), m["lo_supplycost"].astype(np.int32)]
    n = len(cols[0])
    joins = capi.build_joins(ctx, wl, auto=True)
    pipe = capi.Pipeline(ctx, cols, n, joins, [[0, 1, 2, 3]])
    out = capi.Output(pipe, 1024, n // 1024 + 1 + 8192)
    mpx = capi.DeviceMultiplexer(pipe, "default_path")
    capi.run_resident([mpx], [(0, (n + 1023) // 1024)], out=out, reset=True, finish=True)
    mpx.finish()
    rows = out.stats()[0]
    stream = ctx.stream()
    rev, sup = (-1, names.index("lo_revenue")), (-1, names.index("lo_supplycost"))
    plain = (capi.AggSpec * 2)(capi.AggSpec(capi.AGG["sum"], *rev), capi.AggSpec(capi.AGG["sum"], *sup))
    expr = capi.make_agg_exprs([("sum", "-", rev, sup, np.int32)])
    years = wl["joins"][3]["payload"]["d_year"]
    y0, ny = int(years.min()), int(years.max()) - int(years.min()) + 1
    gk = (capi.GroupKey * 2)()
    gk[0].src_join, gk[0].src_col, gk[0].min_value, gk[0].n_values = 3, 0, y0, ny
    gk[1].src_join, gk[1].src_col, gk[1].min_value, gk[1].n_values = 0, 0, 0, 25
    n_groups, max_groups = ny * 25, 1024
    res = (capi.AggValue * (max_groups * 2))()
    hkeys = np.zeros((max_groups, 2), np.int64)
    hnulls = np.zeros(max_groups, np.uint32)
    arena = np.zeros(64, np.uint8)
    dropped, oor, found, used = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()

    def ok(rc):
        assert rc == 0, (rc, L.polr_last_error(ctx.h))

    forms = {
        "ungrouped": (lambda: ok(L.polr_out_aggregate(out.h, None, plain, 2, res)),
                      lambda: ok(L.polr_out_aggregate_expr(out.h, None, expr, 1, res, C.byref(oor)))),
        "grouped": (lambda: ok(L.polr_out_aggregate_grouped(out.h, None, gk, 2, plain, 2, res, n_groups, C.byref(dropped))),
                    lambda: ok(L.polr_out_aggregate_grouped_expr(out.h, None, gk, 2, expr, 1, res, n_groups, C.byref(dropped),
                                                                 C.byref(oor)))),
        "hashed": (lambda: ok(L.polr_out_aggregate_hashed(out.h, None, gk, 2, plain, 2, max_groups, hkeys.ctypes.data,
                                                          hnulls.ctypes.data, res, C.byref(found))),
                   lambda: ok(L.polr_out_aggregate_hashed_expr(out.h, None, gk, 2, expr, 1, max_groups, hkeys.ctypes.data,
                                                               hnulls.ctypes.data, res, C.byref(found), arena.ctypes.data, 64,
                                                               C.byref(used), C.byref(oor)))),
    }
    # the two forms agree before anything is timed: SUM(a - b) = SUM(a) - SUM(b)
    if HAS_EXPR:
        a = out.aggregate([("sum", *rev), ("sum", *sup)])
        assert out.aggregate_expr([("sum", "-", rev, sup, np.int32)]) == [a[0] - a[1]]
    for sink, (plain_call, expr_call) in forms.items():
        r = {"tag": TAG, "sink": sink, "rows": rows, "plain_two_sums": timed(stream, plain_call)}
        if HAS_EXPR:
            r["expr_one_sum_of_difference"] = timed(stream, expr_call)
        print(json.dumps(r), flush=True)


main()
