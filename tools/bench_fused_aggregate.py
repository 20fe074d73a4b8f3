#!/usr/bin/env python3
"""The fused ungrouped aggregate sink (polr_out_fuse_aggregate) on the MI355X against the routes a caller has without it.

Two pipelines:

  star   the 2-join, 16 M-output-row pipeline of tools/bench_from_output.py (a fact table joined to two dimensions through
         perfect tables; every fact row survives).  Its emitting runs take the FLAT kernel; the fused sink runs it on the
         generic one.
  job    one fan-out shape of the JOB family (--job-shape, --job-scale): joins keyed by earlier build columns, repeated build
         keys, a filtered source; every route runs on the generic kernel.

Four aggregates: COUNT(*), SUM of a 4-byte probe column, MIN and MAX of build columns.  Three routes, one ADAPTIVE_REINIT
executor over the whole source each:

  count+emit   a counting run, an output sized by its COUNT(*), an emitting run, polr_out_aggregate: today's route when
               the size of the result is not known (allocating the output is inside the clock)
  emit         one emitting run into an output sized beforehand by an oracle, then polr_out_aggregate
  fused        one run with the sink attached, then polr_out_fused_aggregate_result
  fused-atomics  (--ab, after `make -C duckdb-polr_amd fuseagg-ab`) the same through libpolr_hip_fuseagg1.so, the measurement
               build with the OTHER shape of the fold: one wave reduction and one atomic per cell word for every batch of final
               tuples, instead of the shipped wave-private cell table (a vector register, lane w = word w) flushed where the
               wave leaves its loop.  The second library is loaded beside the product one in the same process, with a context,
               tables and a pipeline of its own over the same arrays, so that all four routes alternate inside each repetition.

Times are host clock around calls that return after the stream is idle.  One warm-up round, then --reps (5) rounds with the
routes alternating inside each round; reported: the median and [min, max] in ms.  All routes must agree on all
four aggregates.  Each pipeline runs in a process of its own, under its own time limit; a step that fails ends the run.

    python tools/bench_fused_aggregate.py --json fused_aggregate.json

Needs the GPU; there is no fallback.
"""
import argparse
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

STEPS = ["star", "job"]
ROUTES = ["count+emit", "emit", "fused"]
AB_ROUTE = "fused-atomics"
AB_LIB = os.path.join(PKG, "libpolr_hip_fuseagg1.so")


def second_binding(lib_path):
    """the python binding once more, bound to another build of the library"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("polr_amd_capi_ab", os.path.join(PKG, "python", "polr_amd", "capi.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.LIB_PATH = lib_path
    return mod


def star(ctx, capi, a):
    rng = np.random.default_rng(1)
    n, nb = a.rows, a.build
    d0 = [rng.integers(-1 << 30, 1 << 30, nb).astype(np.int32), rng.integers(-1 << 60, 1 << 60, nb).astype(np.int64)]
    d1 = [rng.permutation(nb).astype(np.int32)]
    ht0 = capi.HashTable.from_columns(ctx, [rng.permutation(nb).astype(np.int32)], d0)
    ht1 = capi.HashTable.from_columns(ctx, [rng.permutation(nb).astype(np.int32)], d1)
    assert ht0.finalize_perfect(0, nb - 1) and ht1.finalize_perfect(0, nb - 1)
    probe = [rng.integers(0, nb, n).astype(np.int32), rng.integers(0, nb, n).astype(np.int32),
             rng.integers(-1 << 30, 1 << 30, n).astype(np.int32), rng.integers(-1 << 60, 1 << 60, n).astype(np.int64)]
    pipe = capi.Pipeline(ctx, probe, n, [(ht0, [(-1, 0)]), (ht1, [(-1, 1)])], [[0, 1], [1, 0]])
    specs = [("count_star", -1, 0), ("sum", -1, 2), ("min", 0, 1), ("max", 1, 0)]
    return pipe, [ht0, ht1], (n + 1023) // 1024, False, specs, "2 perfect joins, %d fact rows" % n


def job(ctx, capi, a):
    from polr_amd import host as phost
    from polr_amd import job_family as jf
    wl = jf.workload(a.job_shape, jf.Tables(scale=a.job_scale), jf.shapes()[a.job_shape])
    names = list(wl["probe"]["cols"].keys())
    paths = phost.generate_join_orders("each_last_once", len(names), [len(j["payload"]) for j in wl["joins"]],
                                       wl["cond_left_index"], [len(j["keys"][0]) for j in wl["joins"]], max_join_orders=8)[0]
    for j in wl["joins"]:
        j.pop("strings", None)  # (integer columns only: the routes compared here share polr_agg_spec)
    joins = capi.build_joins(ctx, wl, auto=True)
    cols = list(wl["probe"]["cols"].values())
    pipe = capi.Pipeline(ctx, cols, len(cols[0]), joins, paths)
    flt = wl["probe"].get("filter")
    if flt:
        _n, n_chunks = pipe.scan_filter([(names.index(c), op, const) for c, op, const in flt])
    else:
        n_chunks = (len(cols[0]) + 1023) // 1024
    with_payload = [x for x, j in enumerate(wl["joins"]) if len(j["payload"])]
    p32 = [i for i, c in enumerate(cols) if c.dtype.itemsize == 4][0]
    specs = [("count_star", -1, 0), ("sum", -1, p32), ("min", with_payload[0], 0), ("max", with_payload[-1], 0)]
    what = "JOB %s at scale %g: %d joins, %d join orders, %d source rows" % (a.job_shape, a.job_scale, len(joins), len(paths), len(cols[0]))
    return pipe, [h for h, _ in joins], n_chunks, bool(flt), specs, what


def step(a):
    import torch
    from polr_amd import capi
    if not torch.cuda.is_available():
        sys.exit("bench_fused_aggregate.py needs the MI355X")
    torch.cuda.set_device(0)
    ctx = capi.Context(0)
    pipe, hts, n_chunks, scanned, specs, what = (star if a.step == "star" else job)(ctx, capi, a)
    mpx = capi.DeviceMultiplexer(pipe, "adaptive_reinit", log_rounds=False)
    if scanned:
        mpx.use_scan_chunks()
    k = pipe.k

    def run(out):
        capi.run_resident([mpx], [(0, n_chunks)], out=out, reset=True, finish=True)
        st = mpx.finish()
        return sum(st["stage_out"][p][k - 1] for p in range(pipe.n_paths))

    n_out = run(None)  # the oracle of the `emit` route
    sized = capi.Output(pipe, 1024, n_out // 1024 + 1 + 8192)
    fused = capi.Output(pipe, 64, 1)
    fused.fuse_aggregate(specs)

    def count_emit():
        rows = run(None)
        out = capi.Output(pipe, 1024, rows // 1024 + 1 + 8192)
        run(out)
        res = out.aggregate(specs)
        out.close()
        return res

    def emit():
        sized.reset()
        run(sized)
        return sized.aggregate(specs)

    def fuse():
        fused.reset()
        run(fused)
        return fused.fused_aggregate_result()

    routes = dict(zip(ROUTES, (count_emit, emit, fuse)))
    names = list(ROUTES)
    ab = None
    if a.ab:
        if not os.path.exists(AB_LIB):
            sys.exit("--ab needs %s (make -C duckdb-polr_amd fuseagg-ab)" % AB_LIB)
        capi2 = second_binding(AB_LIB)
        ctx2 = capi2.Context(0)
        pipe2, hts2, n_chunks2, scanned2, specs2, _what = (star if a.step == "star" else job)(ctx2, capi2, a)
        assert (n_chunks2, specs2) == (n_chunks, specs)
        mpx2 = capi2.DeviceMultiplexer(pipe2, "adaptive_reinit", log_rounds=False)
        if scanned2:
            mpx2.use_scan_chunks()
        fused2 = capi2.Output(pipe2, 64, 1)
        fused2.fuse_aggregate(specs)
        ab = (mpx2, fused2, pipe2, hts2)

        def fuse_acc():
            fused2.reset()
            capi2.run_resident([mpx2], [(0, n_chunks)], out=fused2, reset=True, finish=True)
            mpx2.finish()
            return fused2.fused_aggregate_result()

        routes[AB_ROUTE] = fuse_acc
        names.append(AB_ROUTE)
    times = {r: [] for r in names}
    answers = {}
    for rep in range(1 + a.reps):
        for r in names:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            answers[r] = routes[r]()
            torch.cuda.synchronize()
            if rep:
                times[r].append((time.perf_counter() - t0) * 1e3)
    assert all(answers[r] == answers["emit"] for r in names), answers
    assert fused.stats()[0] == 0 and answers["fused"][0] == n_out
    flat = [pipe.launch_info(False)["flat"], pipe.launch_info(True)["flat"], capi.pool_info([mpx], fused)["flat"]]
    result = {"step": a.step, "what": what, "output_rows": n_out, "reps": a.reps,
              "flat_kernel": dict(zip(("counting", "emitting", "fused"), flat)),
              "ms": {r: {"median": statistics.median(ts), "min": min(ts), "max": max(ts)} for r, ts in times.items()}}
    print("RESULT " + json.dumps(result))
    mpx.close()
    sized.close()
    fused.close()
    pipe.close()
    for h in hts:
        h.close()
    if ab:
        ab[0].close()
        ab[1].close()
        ab[2].close()
        for h in ab[3]:
            h.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=16_000_000, help="star: fact rows = output rows")
    ap.add_argument("--build", type=int, default=1_000_000, help="star: rows of each dimension")
    ap.add_argument("--job-shape", default="17e")
    ap.add_argument("--job-scale", type=float, default=0.2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ab", action="store_true", help="also the fold's other shape, through libpolr_hip_fuseagg1.so (make fuseagg-ab)")
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
               "--job-shape", a.job_shape, "--job-scale", str(a.job_scale), "--reps", str(a.reps)] + (["--ab"] if a.ab else [])
        try:
            run = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
        except subprocess.TimeoutExpired:
            sys.exit("step %s: no result within %d s; nothing further is started" % (s, a.step_timeout))
        if run.returncode != 0:
            sys.stderr.write(run.stdout[-2000:] + run.stderr[-4000:])
            sys.exit("step %s ended with status %d; nothing further is started" % (s, run.returncode))
        results.append(json.loads([ln for ln in run.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
    shown_routes = ROUTES + ([AB_ROUTE] if a.ab else [])
    print("| pipeline | output rows | " + " | ".join(k + " ms" for k in shown_routes) + " |")
    for r in results:
        shown = ["%.2f [%.2f, %.2f]" % (r["ms"][k]["median"], r["ms"][k]["min"], r["ms"][k]["max"]) for k in shown_routes]
        print("| %s | %d | %s |" % (r["what"], r["output_rows"], " | ".join(shown)))
    print(json.dumps(results))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
