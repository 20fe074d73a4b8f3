"""SSB-skew Q4.1 with c_nation as a VARCHAR column (names of tests/strref.py): three routes to GROUP BY d_year, c_nation
over the same tables, alternating A B C A B C in one process:

  parent     emitting pool run + polr_out_aggregate_hashed_str (a string hashed and compared per output row): what a caller
             with a VARCHAR c_nation could do before polr_ht_encode_dictionary existed; pass time = run + sink
  new        polr_out_fuse_grouped on the dictionary code column of the customer build side
  yardstick  polr_out_fuse_grouped on caller-made integer codes with the 50-value domain (the shipped-Q4.1 sub-record path)

usage: python tools/bench_dict_fused.py [scale factor, default 1]   -> one JSON line per route (host clock around reset +
run + the C call that returns the result into buffers made once, which ends in a synchronise; the results are decoded
outside the clock: 3 warm-up passes, then 9 timed ones; min, median, max), then one line for the
one-off cost of polr_ht_encode_dictionary on the customer build side next to the table's finalize.  Kernel times: the same
command under `rocprofv3 --kernel-trace --stats -- python ...` in a run of its own.  Results: profiles/README.md"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "duckdb-polr_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import strref  # noqa: E402
from polr_amd import capi, ssb_skew  # noqa: E402
from polr_amd import host as phost  # noqa: E402

SF = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
REPS, WARM = 9, 3


def spread(ts):
    ts = sorted(ts)
    return {"min_ms": round(ts[0], 4), "median_ms": round(ts[len(ts) // 2], 4), "max_ms": round(ts[-1], 4)}


ctx = capi.Context(0)
wl = ssb_skew.workload("q4.1", sf=SF)
inst = wl["instance"]
m = inst.lineorder(0, inst.n_lo, cols=["lo_revenue", "lo_supplycost"])
names = list(wl["probe"]["cols"].keys()) + ["lo_revenue", "lo_supplycost"]
cols = list(wl["probe"]["cols"].values()) + [m["lo_revenue"], m["lo_supplycost"]]
n = len(cols[0])
k = len(wl["joins"])
cust = wl["joins"][0]
assert cust["name"] == "customer" and wl["joins"][3]["name"] == "date"
cust["strings"] = {"c_nation_name": strref.nation_names(cust["payload"]["c_nation"])}
cust["dictionary"] = ["c_nation_name"]
joins = capi.build_joins(ctx, wl, auto=True)
code_col, (n_codes, has_null) = capi.dictionary_payload_index(cust, "c_nation_name")
words = joins[0][0].dictionary(code_col)
dim_rows = {"customer": len(inst.c_custkey), "supplier": inst.n_s, "part": inst.n_p, "date": 2556}
node_info = [(n, False, False)] + [(dim_rows[j["name"]], j["name"] in ssb_skew.QUERY_WHERE["q4.1"], True) for j in wl["joins"]]
gen = phost.generate_join_orders("sample", 4, [0] * k, [[j["key_src"][0][1]] for j in wl["joins"]],
                                 [len(j["keys"][0]) for j in wl["joins"]], max_join_orders=3, routing="adaptive_reinit",
                                 node_info=node_info, return_routing=True)
paths, routing = gen[0], gen[3]
pipe = capi.Pipeline(ctx, cols, n, joins, paths)
assert pipe.launch_info(True)["flat"] == 1
n_chunks = (n + 1023) // 1024
E = 384 if n_chunks > 65536 else 32
mpxs = [capi.DeviceMultiplexer(pipe, routing, log_rounds=False) for _ in range(E)]
ranges = [((e * n_chunks) // E, ((e + 1) * n_chunks) // E) for e in range(E)]
dy = wl["joins"][3]["payload"]["d_year"]
y0, ny = int(dy.min()), int(dy.max()) - int(dy.min()) + 1
specs = [("count_star", -1, 0), ("sum", -1, names.index("lo_revenue")), ("sum", -1, names.index("lo_supplycost"))]
stream = ctx.stream()

out_parent = capi.Output(pipe, 1024, n // 1024 + 1 + 8192)
out_new = capi.Output(pipe, 1024, 64)
out_new.fuse_grouped([(3, 0, y0, ny), (0, code_col, 0, n_codes + has_null)], specs)
out_yard = capi.Output(pipe, 1024, 64)
out_yard.fuse_grouped([(3, 0, y0, ny), (0, 0, 0, 50)], specs)
str_col = capi.string_payload_index(cust, "c_nation_name")


def agg_specs():
    return (capi.AggSpec * len(specs))(*[capi.AggSpec(capi.AGG[fn], sj, sc) for fn, sj, sc in specs])


def value(r):
    return None if r.is_null else (r.hi << 64) + (r.lo & 0xFFFFFFFFFFFFFFFF)


def parent_route():
    """-> (step, decode): step = reset + run + the C call into buffers made here, once; decode reads them, outside the clock"""
    max_groups, cap = 1024, 1 << 16
    ka = (capi.GroupKey * 2)()
    ka[0].src_join, ka[0].src_col, ka[1].src_join, ka[1].src_col = 3, 0, 0, str_col
    sa = agg_specs()
    keys = np.zeros((max_groups, 2), np.int64)
    nulls = np.zeros(max_groups, np.uint32)
    res = (capi.AggValue * (max_groups * len(specs)))()
    arena = np.zeros(cap, np.uint8)
    n_groups, used = C.c_uint64(), C.c_uint64()

    def step():
        out_parent.reset()
        capi.run_resident(mpxs, ranges, out=out_parent, reset=True, finish=True, stream=stream)
        rc = ctx.L.polr_out_aggregate_hashed_str(out_parent.h, stream, ka, 2, sa, len(specs), max_groups, keys.ctypes.data,
                                                 nulls.ctypes.data, res, C.byref(n_groups), arena.ctypes.data, cap, C.byref(used))
        assert rc == 0, rc

    def decode():
        raw, got = arena.tobytes(), {}
        for g in range(n_groups.value):
            at = int(keys[g, 1])
            name = None if (nulls[g] >> 1) & 1 else raw[at + 4:at + 4 + int.from_bytes(raw[at:at + 4], "little")]
            got[(int(keys[g, 0]), name)] = value(res[g * 3 + 1]) - value(res[g * 3 + 2])
        return got
    return step, decode


def fused_route(out, nv, name_of):
    res = (capi.AggValue * (ny * nv * len(specs)))()
    dropped = C.c_uint64()

    def step():
        out.reset()
        capi.run_resident(mpxs, ranges, out=out, reset=True, finish=True, stream=stream)
        rc = ctx.L.polr_out_fused_result(out.h, stream, res, ny * nv, C.byref(dropped))
        assert rc == 0, rc

    def decode():
        assert dropped.value == 0
        return {(y0 + g // nv, name_of(g % nv)): value(res[g * 3 + 1]) - value(res[g * 3 + 2]) for g in range(ny * nv)
                if res[g * 3].lo}
    return step, decode


routes = [("parent", parent_route()), ("new", fused_route(out_new, n_codes + has_null, lambda c: words[c] if c < n_codes else None)),
          ("yardstick", fused_route(out_yard, 50, lambda c: strref.NATION_NAMES[c]))]
results = []
for _name, (step, decode) in routes:
    step()
    results.append(decode())
assert results[0] == results[1] == results[2] and results[0]  # (the three routes agree before anything is timed)
times = {name: [] for name, _r in routes}
for rep in range(WARM + REPS):
    for name, (step, _decode) in routes:
        t0 = time.perf_counter()
        step()
        if rep >= WARM:
            times[name].append((time.perf_counter() - t0) * 1e3)
rows = int(sum(sum(st["stage_out"][p][k - 1] for p in range(len(paths))) for st in capi.finish_many(mpxs)))
for name, _r in routes:
    print(json.dumps({"route": name, "sf": SF, "tuples": n, "output_rows": rows, "groups": len(results[0]), "executors": E,
                      "group_cells": {"parent": None, "new": ny * (n_codes + has_null), "yardstick": ny * 50}[name],
                      **spread(times[name])}), flush=True)

# the one-off cost: encode the customer build side (whole call, host clock) next to the same table's finalize
cells, heap = capi.string_cells(cust["strings"]["c_nation_name"])
enc, fin = [], []
for rep in range(WARM + REPS):
    ht = capi.HashTable.from_columns(ctx, cust["keys"], list(cust["payload"].values()) + [cells])
    ht.set_payload_heap(len(cust["payload"]), heap)
    ctx.sync()
    t0 = time.perf_counter()
    got = ht.encode_dictionary(len(cust["payload"]))
    t1 = time.perf_counter()
    ht.finalize_auto(int(cust["keys"][0].min()), int(cust["keys"][0].max()))
    t2 = time.perf_counter()
    assert got == (code_col, n_codes, has_null)
    if rep >= WARM:
        enc.append((t1 - t0) * 1e3)
        fin.append((t2 - t1) * 1e3)
    ht.close()
print(json.dumps({"one_off": "customer build side", "sf": SF, "rows": len(cust["keys"][0]), "distinct": n_codes,
                  "encode_dictionary": spread(enc), "finalize_auto": spread(fin)}), flush=True)
