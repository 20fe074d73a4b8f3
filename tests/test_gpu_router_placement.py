"""Routers inside the probe workgroups of the flat pool kernel (the mixed layout) and the separate layout it falls back
to: E executors over disjoint chunk ranges in ONE launch = E single-executor launches over the same ranges -- same
round logs, same statistics -- whichever workgroup and wave an executor's router lands in.  SSB-skew Q4.1 sample (the
flat pipeline, bit tables in LDS), small inputs."""
import json
import os

import numpy as np
import pytest

import common
from polr_amd import capi, ssb_skew
from test_gpu_engine_matrix import FUSED_AGGS_SMALL, FUSED_SHAPES, _fused_star, _fused_want

pytestmark = pytest.mark.gpu

STAT_KEYS = ("num_intermediates", "num_rounds", "input_tuple_count_per_path", "path_resistances", "stage_out")
_state = {}


def _ssb(ctx):
    if "pipe" not in _state:
        gold = json.load(open(os.path.join(common.GOLDEN, "ssb_skew_sample.json")))
        case = gold["cases"]["q4.1/3"]
        wl = ssb_skew.workload("q4.1", **gold["shape"])
        paths = np.asarray(case["paths"], dtype=np.int32)
        joins = capi.build_joins(ctx, wl, auto=True)
        cols = list(wl["probe"]["cols"].values())
        pipe = capi.Pipeline(ctx, cols, len(cols[0]), joins, paths)
        assert pipe.launch_info()["flat"] == 1
        _state.update(pipe=pipe, joins=joins, paths=paths, cols=cols, n=len(cols[0]), n_paths=len(paths), k=len(wl["joins"]),
                      count_star=case["count_star"])
    return _state


def _ranges(n_chunks, n_exec):
    return [((e * n_chunks) // n_exec, ((e + 1) * n_chunks) // n_exec) for e in range(n_exec)]


def _single_runs(pipe, routing, ranges, scan):
    """every range as a launch of its own, one executor: (statistics, round log) per range"""
    want = []
    m = capi.DeviceMultiplexer(pipe, routing)
    if scan:
        m.use_scan_chunks()
    for a, b in ranges:
        capi.run_resident([m], [(a, b)], reset=True, finish=True)
        want.append((m.finish(), m.fetch_log()))
    m.close()
    return want


def _check(pipe, routing, n_chunks, n_exec, share, scan):
    ranges = _ranges(n_chunks, n_exec)
    want = _single_runs(pipe, routing, ranges, scan)
    mpxs = [capi.DeviceMultiplexer(pipe, routing) for _ in range(n_exec)]
    if scan:
        for m in mpxs:
            m.use_scan_chunks()
    for rep in range(2):  # (the second pass starts from what the first left in the arrival counters and rings)
        capi.run_resident(mpxs, ranges, reset=True, finish=True, share=share)
        stats = capi.finish_many(mpxs)
        for e in range(n_exec):
            for key in STAT_KEYS:
                assert stats[e][key] == want[e][0][key], (rep, e, key)
            for got, exp in zip(mpxs[e].fetch_log(), want[e][1]):
                assert np.array_equal(got, exp), (rep, e)
    for m in mpxs:
        m.close()
    return stats


# 100 does not divide a grid of 256 (or any power of two): some workgroups host a router, some none.
# 520 on the whole device, 40 on a sixteenth of it: more executors than the workgroups' router areas (2 each) can host
# -> router workgroups in front of the grid.
@pytest.mark.parametrize("n_exec,share", [(1, 1), (7, 1), (100, 1), (520, 1), (7, 4), (20, 4), (7, 16), (40, 16)])
def test_executors_match_single_executor_runs(gpu_ctx, n_exec, share):
    s = _ssb(gpu_ctx)
    n_chunks = (s["n"] + 1023) // 1024
    stats = _check(s["pipe"], "adaptive_reinit", n_chunks, n_exec, share, scan=False)
    k = s["k"]
    assert sum(sum(st["stage_out"][p][k - 1] for p in range(s["n_paths"])) for st in stats) == s["count_star"]
    assert sum(sum(st["input_tuple_count_per_path"]) for st in stats) == s["n"]


@pytest.mark.parametrize("routing", ["adaptive_reinit", "opportunistic"])
@pytest.mark.parametrize("n_exec", [7, 100])
def test_filtered_source_with_chunk_offsets(gpu_ctx, routing, n_exec):
    """a scan-filtered source: chunks of unequal size, their boundaries read through the router's LDS window"""
    s = _ssb(gpu_ctx)
    # (a pipeline of its own: the scan leaves its selection behind)
    pipe = capi.Pipeline(gpu_ctx, s["cols"], s["n"], s["joins"], s["paths"])
    assert pipe.launch_info()["flat"] == 1
    cut = int(np.median(s["cols"][1]))
    n_sel, n_chunks = pipe.scan_filter([(1, "<=", cut)])
    assert 0 < n_sel < s["n"] and n_chunks > 100
    stats = _check(pipe, routing, n_chunks, n_exec, 1, scan=True)
    assert sum(sum(st["input_tuple_count_per_path"]) for st in stats) == n_sel
    pipe.close()


def test_backpressure_totals(gpu_ctx):
    """BACKPRESSURE: one executor per join order racing for morsels -- which executor gets a morsel is not fixed, the
    totals are"""
    s = _ssb(gpu_ctx)
    pipe = s["pipe"]
    n_chunks = (s["n"] + 1023) // 1024
    mpxs = [capi.DeviceMultiplexer(pipe, "backpressure") for _ in range(s["n_paths"])]
    for _ in range(2):
        capi.run_backpressure(mpxs, 0, n_chunks, morsel_chunks=5)
        stats = capi.finish_many(mpxs)
        k = s["k"]
        assert sum(sum(st["stage_out"][p][k - 1] for p in range(s["n_paths"])) for st in stats) == s["count_star"]
        assert sum(sum(st["input_tuple_count_per_path"]) for st in stats) == s["n"]
    for m in mpxs:
        m.close()


@pytest.mark.parametrize("n_exec,share", [(7, 1), (100, 1), (7, 16), (40, 16)])
def test_fused_sink_in_lds(gpu_ctx, n_exec, share):
    """a fused GROUP BY sink whose cells live in the workgroup's LDS, behind the router areas: the routers of a workgroup
    take part in its closing flush"""
    joins, cols, valid = _fused_star()
    names = list(cols)
    raw_keys, in_lds = FUSED_SHAPES["two-joins"]
    assert in_lds
    keys = [(sj, names.index(sc) if sj < 0 else sc, mn, nv) for sj, sc, mn, nv in raw_keys]
    specs = FUSED_AGGS_SMALL
    dspecs = [(fn, sj, 0 if sc is None else (names.index(sc) if sj < 0 else sc)) for fn, sj, sc in specs]
    pcols = list(cols.values())
    pvalid = [valid.get(c) for c in names]
    n = len(pcols[0])
    ght = [j.device(gpu_ctx) for j in joins]
    pipe = capi.Pipeline(gpu_ctx, pcols, n, [(h, [(-1, j.src)]) for h, j in zip(ght, joins)], [[0, 1], [1, 0]],
                         probe_valid=pvalid)
    li = pipe.launch_info(True)
    n_groups = int(np.prod([key[3] for key in keys]))
    assert li["flat"] == 1 and li["lds_bytes_per_workgroup"] + 8 + 8 * n_groups * (1 + 2 * len(specs)) <= 160 * 1024
    want, dropped, n_rows = _fused_want(joins, cols, valid, names, keys, specs, None)
    out = capi.Output(pipe, 1024, 64)
    out.fuse_grouped(keys, dspecs)
    n_chunks = (n + 1023) // 1024
    mpxs = [capi.DeviceMultiplexer(pipe, "adaptive_reinit") for _ in range(n_exec)]
    for passes in (1, 2):
        capi.run_resident(mpxs, _ranges(n_chunks, n_exec), out=out, reset=True, finish=True, share=share)
        stats = capi.finish_many(mpxs)
        assert sum(sum(st["stage_out"][p][1] for p in range(2)) for st in stats) == n_rows
        vals, counts, got_dropped = out.fused_result()
        assert got_dropped == passes * dropped
        for q in range(n_groups):
            assert vals[q] == [None if v is None else passes * v for v in want[q]], "group %d" % q
    for m in mpxs:
        m.close()
    out.close()
    pipe.close()
    for h in ght:
        h.close()
