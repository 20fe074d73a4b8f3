#!/usr/bin/env python3
"""polr_pipeline_from_output on the MI355X against the route a caller had to compose before it existed, on the same output:
the workload of tools/bench_from_output.py, its output handed on as the SOURCE of a next pipeline instead of a build side.

One emitted output of about 16 M rows (a fact table joined to two dimensions through perfect tables; the pool launch emits
the row ids) becomes the probe side of a one-join pipeline: 1 + 4 fixed-width columns of 4 and 8 bytes (a payload column of
the second dimension, which the new join is keyed by, two columns of the fact table, two of the first dimension); the second
step adds one VARCHAR column of 20-byte strings (a payload column of the second dimension).

  from_output   polr_pipeline_from_output: one call
  composed      polr_out_stats, one device buffer pair per column (torch.empty: the caching allocator, so after the
                warm-up call this costs next to nothing), polr_out_materialize to device memory per column,
                polr_out_materialize_strings for the VARCHAR column (its sizing call first), polr_pipeline_create over
                POLR_COL_DEVICE columns -- a pipeline that only borrows the caller's buffers
  composed-fresh  the same with every buffer from hipMalloc, as polr_pipeline_from_output has to take its own: what the
                composed route costs a caller without a caching allocator (the buffers are freed outside the clock, like the
                pipelines)

Times are host clock around calls that return after the stream is idle; destroying the pipeline is outside the clock.  One
warm-up call of each route, then --reps (5) timed calls in turn; reported: the median and [min, max] in ms.

Each step builds its own output in a process of its own, under its own time limit; a step that fails ends the run.

    python tools/bench_pipeline_from_output.py --rows 16000000 --json pipeline_from_output.json

Needs the GPU; there is no fallback.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "duckdb-polr_amd")
sys.path.insert(0, os.path.join(PKG, "python"))

STEPS = ["fixed", "varchar"]
STR_LEN = 20


def string_column(nb, rng):
    """nb strings of STR_LEN random bytes -> (cells, heap), numpy throughout"""
    heap = rng.integers(1, 255, nb * STR_LEN, dtype=np.uint8)
    cells = np.zeros((nb, 16), np.uint8)
    cells[:, 0:4] = np.full(nb, STR_LEN, np.uint32).view(np.uint8).reshape(nb, 4)
    cells[:, 4:8] = heap.reshape(nb, STR_LEN)[:, :4]
    cells[:, 8:16] = (np.arange(nb, dtype=np.uint64) * np.uint64(STR_LEN) + np.uint64(heap.ctypes.data)).view(np.uint8).reshape(nb, 8)
    return cells.reshape(-1).view("V16"), heap


def step(a):
    import torch
    from polr_amd import capi
    if not torch.cuda.is_available():
        sys.exit("bench_pipeline_from_output.py needs the MI355X")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1)
    ctx = capi.Context(0)
    n, nb = a.rows, a.build
    with_str = a.step == "varchar"
    d0 = [rng.integers(-1 << 30, 1 << 30, nb).astype(np.int32), rng.integers(-1 << 60, 1 << 60, nb).astype(np.int64)]
    d1 = [rng.permutation(nb).astype(np.int32)]
    cells, heap = string_column(nb, rng)
    ht0 = capi.HashTable.from_columns(ctx, [rng.permutation(nb).astype(np.int32)], d0)
    ht1 = capi.HashTable.from_columns(ctx, [rng.permutation(nb).astype(np.int32)], d1 + [cells])
    ht1.set_payload_heap(1, heap)
    assert ht0.finalize_perfect(0, nb - 1) and ht1.finalize_perfect(0, nb - 1)
    probe = [rng.integers(0, nb, n).astype(np.int32), rng.integers(0, nb, n).astype(np.int32),
             rng.integers(-1 << 30, 1 << 30, n).astype(np.int32), rng.integers(-1 << 60, 1 << 60, n).astype(np.int64)]
    pipe = capi.Pipeline(ctx, probe, n, [(ht0, [(-1, 0)]), (ht1, [(-1, 1)])], [[0, 1], [1, 0]])
    out = capi.Output(pipe, 1024, n // 1024 + 1 + 8192)
    mx = capi.DeviceMultiplexer(pipe, "default_path")
    capi.run_resident([mx], [(0, (n + 1023) // 1024)], out=out, reset=True, finish=True)
    mx.finish()
    n_out, n_chunks, _ = out.stats()
    assert n_out == n
    # the next pipeline: one join, keyed by the first carried column (the second dimension's permutation column)
    ht2 = capi.HashTable.from_columns(ctx, [np.arange(nb, dtype=np.int32)], [])
    assert ht2.finalize_perfect(0, nb - 1)
    joins2, paths2 = [(ht2, [(-1, 0)])], [[0]]
    cols = [(1, 0), (-1, 2), (-1, 3), (0, 0), (0, 1)] + ([(1, 1)] if with_str else [])
    widths = {(1, 0): 4, (-1, 2): 4, (-1, 3): 8, (0, 0): 4, (0, 1): 8, (1, 1): 16}
    L = ctx.L

    def from_output():
        return capi.Pipeline.from_output(out, cols, joins2, paths2)

    hip = C.CDLL("libamdhip64.so")

    class Fresh:
        """device memory straight from hipMalloc, freed when the pipeline that borrows it is closed"""

        def __init__(self, nbytes):
            p = C.c_void_p()
            assert hip.hipMalloc(C.byref(p), C.c_size_t(max(nbytes, 16))) == 0
            self.p = p

        def data_ptr(self):
            return self.p.value

        def __del__(self):
            hip.hipFree(self.p)

    def composed(fresh=False):
        rows, _, _ = out.stats()
        dcols, keep = [], []

        def buf(nbytes):
            return Fresh(nbytes) if fresh else torch.empty((nbytes,), dtype=torch.uint8, device=dev)

        for sj, sc in cols:
            w = widths[(sj, sc)]
            data, valid = buf(rows * w), buf(rows)
            keep += [data, valid]
            if w == 16:
                used = C.c_uint64()
                rc = L.polr_out_materialize_strings(out.h, None, sj, sc, data.data_ptr(), valid.data_ptr(), rows, None, 0,
                                                    C.byref(used), capi.COL_DEVICE)
                assert rc == capi.E_OVERFLOW, rc
                sheap = buf(used.value)
                keep.append(sheap)
                ctx.check(L.polr_out_materialize_strings(out.h, None, sj, sc, data.data_ptr(), valid.data_ptr(), rows,
                                                         sheap.data_ptr(), used.value, C.byref(used), capi.COL_DEVICE))
            else:
                ctx.check(L.polr_out_materialize(out.h, None, sj, sc, data.data_ptr(), valid.data_ptr(), rows, capi.COL_DEVICE))
            dcols.append(capi.dev_col(data.data_ptr(), w, signed=w < 16, valid_ptr=valid.data_ptr()))
        p = capi.Pipeline(ctx, dcols, rows, joins2, paths2)  # (POLR_COL_DEVICE cells point into HBM already: no heap call)
        ctx.sync()
        p._keep = keep  # (the pipeline borrows them)
        return p

    routes = {"from_output": from_output, "composed": composed, "composed-fresh": lambda: composed(fresh=True)}
    times = {k: [] for k in routes}
    for r in range(1 + a.reps):
        for k, fn in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            p = fn()
            torch.cuda.synchronize()
            t = (time.perf_counter() - t0) * 1e3
            if r:
                times[k].append(t)
            p.close()
            p._keep = None
            del p
    fixed_bytes = sum(2 * (widths[c] + 1) for c in cols if widths[c] < 16)
    result = {"step": a.step, "rows": n_out, "chunks": n_chunks, "build_rows": nb, "reps": a.reps,
              "fixed_width_bytes_per_row": 4 * 3 + fixed_bytes,
              "ms": {k: {"median": statistics.median(ts), "min": min(ts), "max": max(ts)} for k, ts in times.items()}}
    print("RESULT " + json.dumps(result))
    mx.close()
    out.close()
    pipe.close()
    ht0.close()
    ht1.close()
    ht2.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=16_000_000, help="fact rows = output rows")
    ap.add_argument("--build", type=int, default=1_000_000, help="rows of each dimension")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds a step may take")
    ap.add_argument("--step", choices=STEPS, help="run this one step in this process (what the driver starts)")
    ap.add_argument("--json")
    a = ap.parse_args()
    if a.step:
        step(a)
        return
    results = []
    for s in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", s, "--rows", str(a.rows), "--build", str(a.build),
               "--reps", str(a.reps)]
        try:
            run = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
        except subprocess.TimeoutExpired:
            sys.exit("step %s: no result within %d s; nothing further is started" % (s, a.step_timeout))
        if run.returncode != 0:
            sys.stderr.write(run.stdout[-2000:] + run.stderr[-4000:])
            sys.exit("step %s ended with status %d; nothing further is started" % (s, run.returncode))
        results.append(json.loads([ln for ln in run.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
    print("| step | rows | from_output ms | composed ms | composed-fresh ms |")
    for r in results:
        shown = ["%.2f [%.2f, %.2f]" % (r["ms"][k]["median"], r["ms"][k]["min"], r["ms"][k]["max"])
                 for k in ("from_output", "composed", "composed-fresh")]
        print("| %s | %d | %s |" % (r["step"], r["rows"], " | ".join(shown)))
    print(json.dumps(results))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
