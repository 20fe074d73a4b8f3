#!/usr/bin/env python3
"""Range stealing against the other launch modes on the headline workload (runs ON THE GPU BOX, one process).

The tables, the bank of join orders, the strategy (adaptive_reinit) and the executors (384) are those of bench.py's
default line (SSB-skew Q4.1 at SF100), then the same for Q4.2.  Variants, per workload:

    fixed           polr_mpx_run_resident over E even ranges: the baseline (bench.py's default launch)
    morsels-512     polr_mpx_run_resident_morsels, 512 chunks per pull
    ranges-2        polr_mpx_run_resident_ranges, bench.py's --ranges-per-executor 2 layout
    steal-G         polr_mpx_run_resident_stealing over the SAME even ranges, grants of G = 64 .. 1024 chunks

Per variant 3 warm-up passes, then 20 passes enqueued back to back; the time is the pool kernel's own (HIP events around
every launch: polr_mpx_enable_timing / polr_mpx_kernel_time), mean per pass.  The whole list is run twice, the second time
in reverse order; both figures are kept.  Per stealing variant also: steals, chunks stolen, and COUNT(*) against the
fixed-range run's.

    python tools/sweep_stealing.py --out profiles/r04_stealing_sweep.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "duckdb-polr_amd", "python"))

GRANTS = (64, 128, 256, 512, 1024)


def setup(torch, dev, ctx, query, scale, routing, max_join_orders, V=1024):
    """bench.py's run_case for an SSB-skew query on one GPU: lineorder columns in HBM, dimension tables, the sampled bank"""
    from polr_amd import capi, ssb_skew
    from polr_amd import host as phost
    z = ssb_skew.sizes(scale)
    n_rows = z["n_lo"]
    wl0 = ssb_skew.workload(query, sf=scale, n_lo=n_rows, host_probe=False)
    inst = wl0["instance"]
    names = list(ssb_skew.PROBE_COLS)
    cols_t = inst.lineorder_torch(0, n_rows, dev, cols=names, row_salt=0)
    tens = [cols_t[c] for c in names]
    dim_rows = {"customer": len(inst.c_custkey), "supplier": inst.n_s, "part": inst.n_p, "date": 2556}
    node_info = [(n_rows, False, False)] + [(dim_rows[j["name"]], j["name"] in ssb_skew.QUERY_WHERE[query], True)
                                            for j in wl0["joins"]]
    cond_left = [[j["key_src"][0][1]] for j in wl0["joins"]]
    gen = phost.generate_join_orders("sample", len(names), [0] * len(wl0["joins"]), cond_left,
                                     [len(j["keys"][0]) for j in wl0["joins"]], max_join_orders=max_join_orders,
                                     routing=routing, node_info=node_info, return_routing=True)
    paths, routing = gen[0], gen[3]
    joins = capi.build_joins(ctx, wl0, auto=True)
    cols = [capi.dev_col(t.data_ptr(), t.element_size(), signed=False) for t in tens]
    pipe = capi.Pipeline(ctx, cols, n_rows, joins, paths)
    torch.cuda.synchronize()
    return {"pipe": pipe, "tens": tens, "joins": joins, "n_rows": n_rows, "n_chunks": (n_rows + V - 1) // V,
            "routing": routing, "k": len(wl0["joins"]), "n_paths": len(paths)}


def variants(n_chunks, E):
    from polr_amd import capi
    ranges = [((e * n_chunks) // E, ((e + 1) * n_chunks) // E) for e in range(E)]
    lists = []
    for e in range(E):  # (bench.py --ranges-per-executor 2)
        lst = []
        for r in range(2):
            lo, hi = (r * n_chunks) // 2, ((r + 1) * n_chunks) // 2
            lst.append((lo + (e * (hi - lo)) // E, lo + ((e + 1) * (hi - lo)) // E))
        lists.append(lst)
    out = [("fixed", lambda ms: capi.run_resident(ms, ranges, reset=True, finish=True)),
           ("morsels-512", lambda ms: capi.run_resident_morsels(ms, 0, n_chunks, 512, reset=True, finish=True)),
           ("ranges-2", lambda ms: capi.run_resident_ranges(ms, lists, reset=True, finish=True))]
    for g in GRANTS:
        out.append(("steal-%d" % g, lambda ms, g=g: capi.run_resident_stealing(ms, ranges, g, reset=True, finish=True)))
    return out


def measure(case, mpxs, launch, warmup, passes):
    from polr_amd import capi
    k, P = case["k"], case["n_paths"]
    lead = mpxs[0]  # (the multiplexer that leads a run owns its launch events)
    for _ in range(warmup):
        launch(mpxs)
    capi.finish_many_raw(mpxs)
    lead.kernel_time()
    lead.enable_timing(True)
    for _ in range(passes):
        launch(mpxs)
    raw = capi.finish_many_raw(mpxs)
    ms, n = lead.kernel_time()
    lead.enable_timing(False)
    if n != passes:
        raise SystemExit("%d timed launches for %d passes" % (n, passes))
    stats = capi.stats_dicts(raw, mpxs)
    steal = [m.steal_stats() for m in mpxs]
    return {"kernel_ms_per_pass": round(ms / n, 4),
            "count_star": sum(sum(st["stage_out"][p][k - 1] for p in range(P)) for st in stats),
            "routed_tuples": sum(sum(st["input_tuple_count_per_path"]) for st in stats),
            "total_intermediates": sum(st["num_intermediates"] for st in stats),
            "n_steals": sum(s["n_steals"] for s in steal), "chunks_stolen": sum(s["chunks_stolen"] for s in steal),
            "chunks_routed": sum(s["chunks_routed"] for s in steal)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", default="ssb_skew_q41,ssb_skew_q42")
    ap.add_argument("--scale", type=float, default=100.0)
    ap.add_argument("--executors", type=int, default=384)
    ap.add_argument("--routing", default="adaptive_reinit")
    ap.add_argument("--max-join-orders", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--passes", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r04_stealing_sweep.json"))
    a = ap.parse_args()
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")  # (as bench.py)
    import torch
    from polr_amd import capi
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    ctx = capi.Context(0)
    queries = {"ssb_skew_q41": "q4.1", "ssb_skew_q42": "q4.2", "ssb_skew_q43": "q4.3"}
    result = {"scale": a.scale, "executors": a.executors, "routing": a.routing, "warmup": a.warmup, "passes": a.passes,
              "time": "pool kernel, HIP events around every launch, mean per pass of one block of back-to-back passes; "
                      "two blocks per variant (the list forwards, then backwards)",
              "device": torch.cuda.get_device_name(0), "workloads": {}}
    for wname in a.workloads.split(","):
        case = setup(torch, dev, ctx, queries[wname], a.scale, a.routing, a.max_join_orders)
        E = max(1, min(a.executors, case["n_chunks"]))
        mpxs = [capi.DeviceMultiplexer(case["pipe"], case["routing"], chunk_size=1024, log_rounds=False) for _ in range(E)]
        vs = variants(case["n_chunks"], E)
        rows = {name: [] for name, _ in vs}
        for order in (vs, vs[::-1]):
            for name, launch in order:
                rows[name].append(measure(case, mpxs, launch, a.warmup, a.passes))
        want = rows["fixed"][0]
        rec = {"n_rows": case["n_rows"], "n_chunks": case["n_chunks"], "executors": E, "variants": {}}
        for name, _ in vs:
            r = rows[name]
            rec["variants"][name] = {
                "kernel_ms_per_pass": [x["kernel_ms_per_pass"] for x in r],
                "count_star": r[-1]["count_star"],
                "count_star_equals_fixed": all(x["count_star"] == want["count_star"] for x in r),
                "routed_tuples_equal_fixed": all(x["routed_tuples"] == want["routed_tuples"] for x in r),
                "total_intermediates": [x["total_intermediates"] for x in r],
                "n_steals": [x["n_steals"] for x in r], "chunks_stolen": [x["chunks_stolen"] for x in r]}
            print("%-14s %-12s %s ms  steals %s  chunks stolen %s  COUNT(*) %s" % (
                wname, name, rec["variants"][name]["kernel_ms_per_pass"], rec["variants"][name]["n_steals"],
                rec["variants"][name]["chunks_stolen"],
                "= fixed" if rec["variants"][name]["count_star_equals_fixed"] else "DIFFERS"), flush=True)
        result["workloads"][wname] = rec
        for m in mpxs:
            m.close()
        case["pipe"].close()
        for j in case["joins"]:
            j[0].close()
        del case
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
