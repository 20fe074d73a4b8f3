#!/usr/bin/env python3
"""polr_ht_semi_filter on the MI355X: a large build side thinned by the keys of a 1 M-key table and compacted on the device,
against the two routes that existed before it -- a one-join pipeline whose output becomes the build side
(polr_ht_from_output; correct only for a unique-key `by` and only for SEMI), and np.isin on the host with
polr_ht_upload_columns of the survivors.

The dimension: --rows (30 M) rows of a 4-byte key, two 4-byte columns fk, fk2 uniform over [0, 4 M) and an 8-byte column.
The columns live in HBM already (torch tensors, POLR_COL_DEVICE), so a fresh table costs nothing and the call's own work is
what the clock sees.  `by`, 1 M keys each:

  perfect       the even values of [0, 2 M): a bit table of 250 KB                  fk matches 25 %
  unique hash   1 M distinct values of [0, 4 M): {key32, row} slots, 16 MB           fk matches 25 %
  run hash      500 k distinct values of [0, 4 M), each twice: 16-byte slots, 32 MB  fk matches 12.5 %

Per case SEMI and ANTI, the median of --reps (5) calls on fresh tables after one warm-up call, [min, max], the algorithmic
bytes

    per table row:  the key column's 4 bytes; one probe -- a 4-byte bit-table word or a 32-byte slot group --; 2 x 1/8 for
                    the pass bit
    per kept row:   over all columns 2 x width, + 4 for the row list

and their fraction of 8 TB/s.  Then two filters (fk by the unique hash table, fk2 by the perfect table) in one call against
two calls.  --ab 'LABEL=LIB' names a build of the call with another lane shape in its counting kernel (make htsemi-r4: FOUR
rows per lane): the same cases through it, for the A/B of the lane shape.

    python tools/bench_ht_semi.py --rows 30000000 --json ht_semi.json

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
DOMAIN, BY_KEYS = 4_000_000, 1_000_000
WIDTHS = [4, 4, 4, 8]  # (no column has a validity array)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=30_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--ab", action="append", default=[], metavar="LABEL=LIB",
                    help="a library whose polr_ht_semi_filter has another lane shape ('four rows per lane=libpolr_htsemi_r4.so')")
    ap.add_argument("--json")
    a = ap.parse_args()
    import torch
    from polr_amd import capi
    if not torch.cuda.is_available():
        sys.exit("bench_ht_semi.py needs the MI355X")
    torch.cuda.set_device(0)
    n = a.rows
    rng = np.random.default_rng(1)
    ctx = capi.Context(0)
    key = rng.permutation(n).astype(np.int32)
    fk = rng.integers(0, DOMAIN, n).astype(np.int32)
    fk2 = rng.integers(0, DOMAIN, n).astype(np.int32)
    pay = rng.integers(-1 << 60, 1 << 60, n).astype(np.int64)
    tensors = [torch.from_numpy(x).to("cuda:0") for x in (key, fk, fk2, pay)]
    torch.cuda.synchronize()

    def dev_cols():
        return [capi.dev_col(t.data_ptr(), w, True) for t, w in zip(tensors, WIDTHS)]

    def fresh():
        cols = dev_cols()
        return capi.HashTable.from_cols(ctx, cols[:1], cols[1:], n)

    by_keys = {"perfect": np.arange(0, 2 * BY_KEYS, 2, dtype=np.int32),
               "unique hash": rng.permutation(DOMAIN)[:BY_KEYS].astype(np.int32),
               "run hash": np.repeat(rng.permutation(DOMAIN)[:BY_KEYS // 2].astype(np.int32), 2)}
    bys = {}
    for name, k in by_keys.items():
        t = capi.HashTable.from_columns(ctx, [k])
        if name == "perfect":
            assert t.finalize_perfect(0, 2 * BY_KEYS - 1)
        else:
            t.finalize_hash()
        assert t.info()["kind"] == {"perfect": 1, "unique hash": 2, "run hash": 3}[name]
        bys[name] = t
    probe_bytes = {"perfect": 4, "unique hash": 32, "run hash": 32}
    libs = {"polr_ht_semi_filter": ctx.L}
    for ab in a.ab:
        label, path = ab.split("=", 1)
        other = C.CDLL(os.path.abspath(path))
        other.polr_ht_semi_filter.argtypes = ctx.L.polr_ht_semi_filter.argtypes
        libs[label] = other

    def timed(lib, calls):
        """calls: the filter lists of successive calls on one fresh table -> (ms of each repetition, kept)"""
        times, kept = [], C.c_uint64()
        for rep in range(a.reps + 1):
            ht = fresh()
            ctx.sync()
            t0 = time.perf_counter()
            for fl in calls:
                arr = (capi.SemiFilter * len(fl))(*[capi.SemiFilter(b.h, 1, (C.c_uint32 * 4)(col, 0, 0, 0), int(anti)) for b, col, anti in fl])
                ctx.check(lib.polr_ht_semi_filter(ht.h, None, arr, len(fl), C.byref(kept)))
            t1 = time.perf_counter()
            ht.close()
            if rep:  # (the first call warms up)
                times.append((t1 - t0) * 1e3)
        return times, kept.value

    def report(case, route, times, kept, alg=None):
        med = statistics.median(times)
        row = {"kept": kept, "ms": med, "min_ms": min(times), "max_ms": max(times)}
        text = "%-28s %-22s kept %9d  %9.3f ms [%.3f, %.3f]" % (case, route, kept, med, min(times), max(times))
        if alg is not None:
            row.update(algorithmic_bytes=alg, fraction_of_8TBps=alg / (med * 1e-3) / HBM_BYTES_PER_S)
            text += "  %.3f GB algorithmic = %.1f %% of 8 TB/s" % (alg / 1e9, 100 * row["fraction_of_8TBps"])
        print(text, flush=True)
        result["cases"].setdefault(case, {})[route] = row

    result = {"rows": n, "by_keys": BY_KEYS, "cases": {}}
    per_kept = sum(2 * w for w in WIDTHS) + 4
    for name, by in bys.items():
        for anti in (False, True):
            case = "%s %s" % (name, "ANTI" if anti else "SEMI")
            for route, lib in libs.items():
                times, kept = timed(lib, [[(by, 1, anti)]])
                report(case, route, times, kept, n * (4 + probe_bytes[name] + 0.25) + kept * per_kept)
            want = np.isin(fk, by_keys[name])
            assert kept == int((~want if anti else want).sum()), case
    # two filters: one call against two
    two = [(bys["unique hash"], 1, False), (bys["perfect"], 2, False)]
    for route, lib in libs.items():
        times, kept = timed(lib, [two])
        report("two filters", route + ", one call", times, kept)
        times, kept2 = timed(lib, [two[:1], two[1:]])
        report("two filters", route + ", two calls", times, kept2)
        assert kept == kept2 == int((np.isin(fk, by_keys["unique hash"]) & np.isin(fk2, by_keys["perfect"])).sum())
    # what callers without a device route do: np.isin on the host, the survivors' columns, host to device
    for name in by_keys if a.host_reps else ():
        times = []
        for rep in range(a.host_reps):
            t0 = time.perf_counter()
            mask = np.isin(fk, by_keys[name])
            ht = capi.HashTable.from_columns(ctx, [key[mask]], [fk[mask], fk2[mask], pay[mask]])
            ctx.sync()
            t1 = time.perf_counter()
            ht.close()
            times.append((t1 - t0) * 1e3)
        report("%s SEMI" % name, "host np.isin + upload", times, int(mask.sum()))
    # the device route that existed: a one-join pipeline over the dimension's columns, its output as the build side
    # (one build row per MATCH: a SEMI join only because the keys of `by` are unique)
    by = bys["unique hash"]
    times = []
    for rep in range(min(a.reps, 3) + 1):
        ctx.sync()
        t0 = time.perf_counter()
        pipe = capi.Pipeline(ctx, dev_cols(), n, [(by, [(-1, 1)])], [[0]])
        out = capi.Output(pipe, 1024, n // 1024 + 1 + 8192)
        mx = capi.DeviceMultiplexer(pipe, "default_path", log_rounds=False)
        capi.run_resident([mx], [(0, (n + 1023) // 1024)], out=out, reset=True, finish=True)
        mx.finish()
        ht = capi.HashTable.from_output(out, [(-1, 0)], [(-1, 1), (-1, 2), (-1, 3)])
        ctx.sync()
        t1 = time.perf_counter()
        kept = out.stats()[0]
        for h in (ht, mx, out, pipe):
            h.close()
        if rep:
            times.append((t1 - t0) * 1e3)
    report("unique hash SEMI", "pipeline + from_output", times, int(kept))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")
    for t in bys.values():
        t.close()
    ctx.close()


if __name__ == "__main__":
    main()
