#!/usr/bin/env python3
"""polr_ht_column_stats and polr_ht_finalize_auto_stats on the MI355X: the statistics of a build side that lives in HBM, and
the finalize call that takes them, against the route a caller has without them -- copy the key column to the host, numpy
min / max, polr_ht_finalize_auto.

The table is customer-shaped: --rows (30 M) rows of a 4-byte key (a permutation: dense and unique), two 4-byte columns, one
8-byte column and one VARCHAR column of 20-byte strings.  The columns are in HBM already (torch tensors, POLR_COL_DEVICE), so
a fresh table costs nothing and the call's own work is what the clock sees.

Every figure is the median of --reps (5) WHOLE CALLS after one warm-up call, [min, max]: a host clock around a call that
returns when the numbers are on the host (two launches, one 40-byte-per-column copy, one synchronise).  The shapes given with
--ab are timed in the same repetitions, one after the other, so that they share whatever else the machine is doing.

  key alone / five columns in one call / five calls of one column each
      algorithmic bytes: the cell widths -- a VARCHAR cell counts with its 16 bytes, although only its length word is used:
      the lines that hold it are moved whole -- and their share of 8 TB/s
  finalize_auto_stats on a fresh table  against  D2H copy of the key + numpy min / max + finalize_auto on a fresh table

--ab 'LABEL=LIB' names a build of the calls with another kernel shape (make colstats-ab: libpolr_colstats_shape1.so -- one row
per lane, a wave reduction, one atomic pair per wave on one record --, libpolr_colstats_shape2.so -- the launches once per
column): the same cases through it.

    python tools/bench_col_stats.py --rows 30000000 --json col_stats.json

Needs the GPU; there is no fallback.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "duckdb-polr_amd")
sys.path.insert(0, os.path.join(PKG, "python"))

HBM_BYTES_PER_S = 8e12
WIDTHS = [4, 4, 4, 8, 16]  # (no column has a validity array)
STRING_BYTES = 20


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=30_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ab", action="append", default=[], metavar="LABEL=LIB",
                    help="a library whose statistics calls have another kernel shape ('one row per lane=libpolr_colstats_shape1.so')")
    ap.add_argument("--json")
    a = ap.parse_args()
    import torch
    from polr_amd import capi
    if not torch.cuda.is_available():
        sys.exit("bench_col_stats.py needs the MI355X")
    torch.cuda.set_device(0)
    n = a.rows
    rng = np.random.default_rng(1)
    ctx = capi.Context(0)
    key = rng.permutation(n).astype(np.int32)
    c1 = rng.integers(-1 << 30, 1 << 30, n).astype(np.int32)
    c2 = rng.integers(0, 4_000_000, n).astype(np.int32)
    pay = rng.integers(-1 << 60, 1 << 60, n).astype(np.int64)
    cells = np.zeros((n, 4), np.uint32)  # string_t: length, 4 bytes of prefix, a pointer nobody follows here
    cells[:, 0] = STRING_BYTES
    cells[:, 1] = 0x61616161
    host = [key, c1, c2, pay, cells]
    tensors = [torch.from_numpy(x.view(np.int32) if x is cells else x).to("cuda:0") for x in host]
    torch.cuda.synchronize()

    def fresh():
        cols = [capi.dev_col(t.data_ptr(), w, w < 16) for t, w in zip(tensors, WIDTHS)]
        return capi.HashTable.from_cols(ctx, cols[:1], cols[1:], n)

    libs = {"polr_ht_column_stats": ctx.L}
    for ab in a.ab:
        label, path = ab.split("=", 1)
        other = C.CDLL(os.path.abspath(path))
        other.polr_ht_column_stats.argtypes = ctx.L.polr_ht_column_stats.argtypes
        other.polr_ht_finalize_auto_stats.argtypes = ctx.L.polr_ht_finalize_auto_stats.argtypes
        libs[label] = other
    result = {"rows": n, "reps": a.reps, "cases": {}}

    def report(case, route, times, alg=None):
        med = statistics.median(times)
        row = {"ms": med, "min_ms": min(times), "max_ms": max(times)}
        text = "%-34s %-30s %9.3f ms [%.3f, %.3f]" % (case, route, med, min(times), max(times))
        if alg is not None:
            row.update(algorithmic_bytes=alg, fraction_of_8TBps=alg / (med * 1e-3) / HBM_BYTES_PER_S)
            text += "  %.3f GB algorithmic = %.1f %% of 8 TB/s" % (alg / 1e9, 100 * row["fraction_of_8TBps"])
        print(text, flush=True)
        result["cases"].setdefault(case, {})[route] = row

    # the statistics calls: every case through every shape, alternating inside a repetition
    ht = fresh()
    want = None
    cases = {"key alone": [[0]], "five columns, one call": [[0, 1, 2, 3, 4]], "five calls of one column": [[c] for c in range(5)]}
    for case, calls in cases.items():
        times = {route: [] for route in libs}
        for rep in range(a.reps + 1):
            for route, lib in libs.items():
                got = []
                ctx.sync()
                t0 = time.perf_counter()
                for cols in calls:
                    st = (capi.ColStats * len(cols))()
                    ctx.check(lib.polr_ht_column_stats(ht.h, None, (C.c_uint32 * len(cols))(*cols), len(cols), st))
                    got += [(s.min_value, s.max_value, s.n_rows, s.n_valid, s.n_long, s.long_bytes) for s in st]
                t1 = time.perf_counter()
                if rep:  # (the first call warms up)
                    times[route].append((t1 - t0) * 1e3)
                if case != "key alone":  # every shape returns the same numbers
                    want = want or got
                    assert got == want, (route, got, want)
        alg = n * sum(WIDTHS[c] for cols in calls for c in cols)
        for route in libs:
            report(case, route, times[route], alg)
    assert want[0][:2] == (0, n - 1) and want[3][:2] == (int(pay.min()), int(pay.max()))
    assert want[4] == (STRING_BYTES, STRING_BYTES, n, n, n, n * STRING_BYTES)
    ht.close()

    # finalize: the statistics on the device against the route of unchanged calls
    times = {"finalize_auto_stats": [], "D2H + numpy min / max + finalize_auto": []}
    for rep in range(a.reps + 1):
        ht = fresh()
        ctx.sync()
        t0 = time.perf_counter()
        kind, ks = ht.finalize_auto_stats()
        t1 = time.perf_counter()
        info = ht.info()
        ht.close()
        ht = fresh()
        ctx.sync()
        t2 = time.perf_counter()
        k = tensors[0].cpu().numpy()
        kind2 = ht.finalize_auto(int(k.min()), int(k.max()))
        t3 = time.perf_counter()
        assert kind == kind2 == 1 and (ks["min_value"], ks["max_value"]) == (0, n - 1)
        assert {f: v for f, v in ht.info().items()} == info
        ht.close()
        if rep:
            times["finalize_auto_stats"].append((t1 - t0) * 1e3)
            times["D2H + numpy min / max + finalize_auto"].append((t3 - t2) * 1e3)
    for route, t in times.items():
        report("finalize a dense unique key", route, t)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
