#!/usr/bin/env python3
"""polr_ht_filter on the MI355X: a customer-shaped dimension at SF1000 size filtered and compacted on the device, against
what callers did before it existed -- a numpy mask on the host and polr_ht_upload_columns of the survivors.

The dimension: 30 M rows of a 4-byte key, two 4-byte payload columns (region 0..4, nation 0..24) and one VARCHAR column of
20-byte strings (city) with its heap.  The columns live in HBM already (torch tensors, POLR_COL_DEVICE; the string cells
point into a heap tensor), so a fresh table costs nothing and the filter's own work is what the clock sees.

  region = c        keeps about 1/5                      (an integer comparison)
  city LIKE '%x%'   keeps about 1 - (253/254)^20 = 7.6 %  (the matcher follows every row's heap pointer)

Per filter, the median of --reps (5) calls on fresh tables after one warm-up call, [min, max], the algorithmic bytes

    per table row:  the widths of the distinct filter columns plus their validity, once; 2 x 1/8 for the pass bit
    per kept row:   over all columns 2 x (width + validity), + 4 for the row list

(the LIKE filter's heap reads -- 20 bytes a row -- are counted on top and reported separately), their fraction of 8 TB/s,
and for context the host route: numpy mask + survivors' columns + from_columns, host to device (--host-reps, 3).

    python tools/bench_ht_filter.py --rows 30000000 --json ht_filter.json

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

STR_LEN = 20
HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=30_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--json")
    a = ap.parse_args()
    import torch
    from polr_amd import capi
    if not torch.cuda.is_available():
        sys.exit("bench_ht_filter.py needs the MI355X")
    torch.cuda.set_device(0)
    n = a.rows
    rng = np.random.default_rng(1)
    ctx = capi.Context(0)
    key = rng.permutation(n).astype(np.int32)
    nation = rng.integers(0, 25, n).astype(np.int32)
    region = (nation // 5).astype(np.int32)
    heap = rng.integers(1, 255, n * STR_LEN, dtype=np.uint8)
    t_key, t_region, t_nation, t_heap = (torch.from_numpy(x).to("cuda:0") for x in (key, region, nation, heap))

    def cells_for(heap_rows, base):
        m = len(heap_rows)
        cells = np.zeros((m, 16), np.uint8)
        cells[:, 0:4] = np.full(m, STR_LEN, np.uint32).view(np.uint8).reshape(m, 4)
        cells[:, 4:8] = heap_rows[:, :4]
        cells[:, 8:16] = (np.arange(m, dtype=np.uint64) * np.uint64(STR_LEN) + np.uint64(base)).view(np.uint8).reshape(m, 8)
        return cells

    t_cells = torch.from_numpy(cells_for(heap.reshape(n, STR_LEN), t_heap.data_ptr())).to("cuda:0")
    torch.cuda.synchronize()

    def fresh():
        return capi.HashTable.from_cols(ctx, [capi.dev_col(t_key.data_ptr(), 4, True)],
                                        [capi.dev_col(t_region.data_ptr(), 4, True), capi.dev_col(t_nation.data_ptr(), 4, True),
                                         capi.dev_col(t_cells.data_ptr(), 16)], n)

    filters = {"region = 2": (("cmp", 1, "=", 2), 4, 0), "city LIKE '%x%'": (("like", 3, "%x%"), 16, STR_LEN)}
    widths = [4, 4, 4, 16]  # (no column has a validity array)
    result = {"rows": n, "filters": {}}
    for name, (expr, filter_bytes, heap_bytes) in filters.items():
        nodes, values = capi.flatten_filter_expr(expr)
        na, va, keep = capi._filter_arrays(nodes, values)
        row = result["filters"][name] = {}
        times, kept = [], C.c_uint64()
        for rep in range(a.reps + 1):
            ht = fresh()
            ctx.sync()
            t0 = time.perf_counter()
            ctx.check(ctx.L.polr_ht_filter(ht.h, None, na, len(nodes), va, len(values), C.byref(kept)))
            t1 = time.perf_counter()
            ht.close()
            if rep:  # (the first call warms up)
                times.append((t1 - t0) * 1e3)
        alg = n * (filter_bytes + 0.25) + kept.value * (sum(2 * w for w in widths) + 4)
        med = statistics.median(times)
        row["polr_ht_filter"] = {"kept": kept.value, "ms": med, "min_ms": min(times), "max_ms": max(times), "algorithmic_bytes": alg,
                                 "heap_bytes_read": n * heap_bytes, "fraction_of_8TBps": alg / (med * 1e-3) / HBM_BYTES_PER_S}
        print("%-16s %-18s kept %9d  %8.3f ms [%.3f, %.3f]  %.3f GB algorithmic = %.1f %% of 8 TB/s%s" %
              (name, "polr_ht_filter", kept.value, med, min(times), max(times), alg / 1e9, 100 * row["polr_ht_filter"]["fraction_of_8TBps"],
               "  (+ %.2f GB of heap reads)" % (n * heap_bytes / 1e9) if heap_bytes else ""), flush=True)
        # what callers do today: mask on the host, the survivors' columns, host to device
        times = []
        if not a.host_reps:
            continue
        for rep in range(a.host_reps):
            t0 = time.perf_counter()
            if expr[0] == "cmp":
                mask = region == 2
            else:
                mask = (heap.reshape(n, STR_LEN) == ord("x")).any(axis=1)
            h_rows = np.ascontiguousarray(heap.reshape(n, STR_LEN)[mask])
            cells = cells_for(h_rows, h_rows.ctypes.data).reshape(-1).view("V16")
            ht = capi.HashTable.from_columns(ctx, [key[mask]], [region[mask], nation[mask], cells])
            ht.set_payload_heap(2, h_rows.reshape(-1))
            ctx.sync()
            t1 = time.perf_counter()
            assert int(mask.sum()) == kept.value
            ht.close()
            times.append((t1 - t0) * 1e3)
        row["host mask + from_columns"] = {"ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times)}
        print("%-16s %-18s kept %9d  %8.1f ms [%.1f, %.1f]" % (name, "host + upload", kept.value, statistics.median(times), min(times),
                                                             max(times)), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
