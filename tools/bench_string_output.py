#!/usr/bin/env python3
"""polr_out_materialize_strings on the MI355X: what a string column of a join result costs, and where the cut-over
between "a lane copies the string" and "the whole wave copies it" (POLR_STRCOPY_LANE_MAX, csrc/polr_strcopy.h) belongs.

One emitted output of a few million rows (a fact table joined to one dimension of --build rows through a perfect table;
the pool launch emits the row ids), three VARCHAR columns of the dimension gathered by it:

  inline   every string at most 12 bytes: no heap at all
  20-40    every string 20 to 40 bytes
  1%-4K    1 % of the strings 4096 bytes, the others 8 bytes

each written to a DEVICE destination, timed at every candidate cut-over (the measurement builds `make -C duckdb-polr_amd
strout-cuts`: libpolr_strout_cut<N>.so holds the entry point compiled with that constant and takes everything else from
libpolr_hip.so, so all candidates run in this one process on the same output, alternating), beside two yardsticks taken
in the same run:

  gather   polr_out_materialize of the same column to a device destination: the cell gather alone
  memcpy   a device-to-device hipMemcpy of heap_used bytes: the heap written once, read once, by the copy engine's kernel

Times are host clock around calls that return after the stream is idle (the call includes its scratch allocations: that is
what a caller pays); --warmup calls, then --reps timed rounds, a round = every candidate and both yardsticks once, in turn.
Reported: median and [min, max] in ms, and GB/s over the algorithmic bytes of DESIGN.md (per row 4 + 1 + 4 read in the
measuring pass, 4 + 1 + 16 + 8 read and 16 + 1 + 8 written around it, plus twice the heap bytes).

    python tools/bench_string_output.py --rows 4000000 --json string_output.json

Needs the GPU; there is no fallback.
"""
import argparse
import ctypes as C
import glob
import json
import os
import re
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "duckdb-polr_amd")
sys.path.insert(0, os.path.join(PKG, "python"))

from polr_amd import capi  # noqa: E402


def cells_for(lens, rng):
    """string_t cells + heap for strings of the given lengths with random bytes (numpy throughout: millions of rows)"""
    n = len(lens)
    lens = lens.astype(np.uint32)
    long_ = lens > 12
    off = np.cumsum(np.where(long_, lens, 0).astype(np.uint64)) - np.where(long_, lens, 0).astype(np.uint64)
    total = int(np.where(long_, lens, 0).astype(np.uint64).sum())
    heap = rng.integers(1, 255, max(total, 1), dtype=np.uint8)
    cells = np.zeros((n, 16), np.uint8)
    cells[:, 0:4] = lens.view(np.uint8).reshape(n, 4)
    inline = rng.integers(1, 255, (n, 12), dtype=np.uint8)
    inline[np.arange(12)[None, :] >= lens[:, None]] = 0
    cells[~long_, 4:16] = inline[~long_]
    idx = np.nonzero(long_)[0]
    first = off[idx].astype(np.int64)
    for b in range(4):
        cells[idx, 4 + b] = heap[first + b]
    cells[idx, 8:16] = (off[idx] + np.uint64(heap.ctypes.data)).view(np.uint8).reshape(-1, 8)
    return cells.reshape(-1).view("V16"), heap


def columns(nb, rng):
    lens = {"inline": rng.integers(0, 13, nb), "20-40": rng.integers(20, 41, nb),
            "1%-4K": np.where(rng.random(nb) < 0.01, 4096, 8)}
    return {k: cells_for(v, rng) for k, v in lens.items()}, lens


def timed(fn, sync):
    t0 = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=4_000_000, help="fact rows = output rows")
    ap.add_argument("--build", type=int, default=1_000_000, help="dimension rows")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--json")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_string_output.py needs the MI355X")
    torch.cuda.set_device(0)
    libs = {}
    for path in glob.glob(os.path.join(PKG, "libpolr_strout_cut*.so")):
        lib = C.CDLL(path)
        lib.polr_out_materialize_strings.argtypes = capi.load().polr_out_materialize_strings.argtypes
        libs[int(re.search(r"cut(\d+)\.so$", path).group(1))] = lib
    if len(libs) < 3:
        sys.exit("build the candidates first: make -C duckdb-polr_amd strout-cuts")
    rng = np.random.default_rng(1)
    ctx = capi.Context(0)
    nb, n = a.build, a.rows
    cols, lens = columns(nb, rng)
    names = list(cols)
    bk = rng.permutation(nb).astype(np.int32)
    ht = capi.HashTable.from_columns(ctx, [bk], [cols[c][0] for c in names])
    for i, c in enumerate(names):
        ht.set_payload_heap(i, cols[c][1])
    assert ht.finalize_perfect(0, nb - 1)
    pk = rng.integers(0, nb, n).astype(np.int32)
    pipe = capi.Pipeline(ctx, [pk], n, [(ht, [(-1, 0)])], [[0]])
    out = capi.Output(pipe, 1024, n // 1024 + 1 + 8192)
    mx = capi.DeviceMultiplexer(pipe, "default_path")
    capi.run_resident([mx], [(0, (n + 1023) // 1024)], out=out, reset=True, finish=True)
    mx.finish()
    n_out, n_chunks, _ = out.stats()
    assert n_out == n
    dev =torch.device("cuda", 0)
    cells = torch.empty((n_out, 16), dtype=torch.uint8, device=dev)
    valid = torch.empty((n_out,), dtype=torch.uint8, device=dev)
    sync = torch.cuda.synchronize
    result = {"rows": n_out, "chunks": n_chunks, "build_rows": nb, "warmup": a.warmup, "reps": a.reps, "columns": {}}
    for ci, name in enumerate(names):
        used = C.c_uint64()  # (the sizing call: the heap's size comes from the library itself)
        rc = capi.load().polr_out_materialize_strings(out.h, None, 0, ci, cells.data_ptr(), valid.data_ptr(), n_out, None, 0,
                                                      C.byref(used), capi.COL_DEVICE)
        assert rc in (capi.OK, capi.E_OVERFLOW), rc
        heap_used = used.value
        heap = torch.empty((max(heap_used, 1),), dtype=torch.uint8, device=dev)
        heap2 = torch.empty_like(heap)
        sync()

        def strings(lib):
            u = C.c_uint64()
            rc = lib.polr_out_materialize_strings(out.h, None, 0, ci, cells.data_ptr(), valid.data_ptr(), n_out,
                                                  heap.data_ptr() if heap_used else None, heap_used, C.byref(u), capi.COL_DEVICE)
            assert rc == capi.OK and u.value == heap_used, (rc, u.value)

        def gather():
            ctx.check(ctx.L.polr_out_materialize(out.h, None, 0, ci, cells.data_ptr(), valid.data_ptr(), n_out, capi.COL_DEVICE))
            ctx.sync()

        def memcpy():
            heap2.copy_(heap)

        runs = {"cut %d" % c: (lambda lib=libs[c]: strings(lib)) for c in sorted(libs)}
        runs["gather"] = gather
        if heap_used:
            runs["memcpy"] = memcpy
        times = {k: [] for k in runs}
        for r in range(a.warmup + a.reps):
            for k, fn in runs.items():
                t = timed(fn, sync)
                if r >= a.warmup:
                    times[k].append(t)
        bytes_strings = n_out * (9 + 29 + 25) + 2 * heap_used
        row = {"heap_used": heap_used, "algorithmic_bytes": bytes_strings, "ms": {}}
        for k, ts in times.items():
            b = bytes_strings if k.startswith("cut") else (n_out * (4 + 1 + 16 + 16 + 1) if k == "gather" else 2 * heap_used)
            row["ms"][k] = {"median": statistics.median(ts), "min": min(ts), "max": max(ts),
                            "GB/s at median": b / statistics.median(ts) / 1e6}
        result["columns"][name] = row
    keys = list(result["columns"][names[-1]]["ms"].keys())
    print("| column | heap MB | " + " | ".join(keys) + " |")
    for name, row in result["columns"].items():
        shown = ["%.2f [%.2f, %.2f] (%.0f GB/s)" % (v["median"], v["min"], v["max"], v["GB/s at median"]) if v else "-"
                 for v in (row["ms"].get(k) for k in keys)]
        print("| %s | %.1f | %s |" % (name, row["heap_used"] / 1e6, " | ".join(shown)))
    print(json.dumps(result))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    mx.close()
    out.close()
    pipe.close()
    ht.close()


if __name__ == "__main__":
    main()
