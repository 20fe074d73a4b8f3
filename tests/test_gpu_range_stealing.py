"""polr_mpx_run_resident_stealing: executors that work through their own contiguous chunk range grant by grant and, once
dry, take the far half of whoever has most left (protocol: duckdb-polr_amd/csrc/polr_steal.h; on the host:
tests/test_steal_protocol.py).  Whatever the thieves do, every chunk of the ranges is routed exactly once: routed
tuples, COUNT(*) and the emitted row set equal single-executor runs over the same chunks.  While nobody has two grants
to give the run is the fixed-range run, bit for bit; one executor alone is the morsel run with morsel = grant."""
import numpy as np
import pytest

import common
from common import workloads
from polr_amd import capi

pytestmark = pytest.mark.gpu

GOLD = common.load_golden("ssb_skew_q41")
STAT_KEYS = ("num_intermediates", "num_rounds", "input_tuple_count_per_path", "path_resistances", "stage_out")
_cache = {}


def _sorted_rows(ids):
    return ids[np.lexsort(ids.T[::-1])]


def q41(ctx):
    """SSB-skew Q4.1 at sf 0.2 (tests/test_ssb_config.py): the flat pipeline, ~1.2 M rows in 1 172 chunks"""
    if "q41" not in _cache:
        wl = workloads.ssb_skew_q41(sf=GOLD["sf"])
        paths = np.asarray(GOLD["paths"], dtype=np.int32)
        joins = capi.build_joins(ctx, wl, auto=True)
        cols = list(wl["probe"]["cols"].values())
        n = len(cols[0])
        pipe = capi.Pipeline(ctx, cols, n, joins, paths)
        assert pipe.launch_info(True)["flat"] == 1
        _cache["q41"] = (wl, pipe, joins, n, (n + 1023) // 1024, len(wl["joins"]))
    return _cache["q41"]


def star(ctx):
    """star_skew (chained + perfect + duplicate-key join, each_last_once): the generic pipeline"""
    from test_gpu_mpx import pipeline_for
    wl, paths, pipe, joins, n = pipeline_for(ctx, "star_skew", "each_last_once")
    return wl, paths, pipe, n, (n + 1023) // 1024, len(wl["joins"])


def chunk_tuples(ranges, n):
    return sum(min(b * 1024, n) - min(a * 1024, n) for a, b in ranges)


def reference_rows(ctx, routing, ranges_key, ranges):
    """COUNT(*) and sorted row ids of single-executor run_resident calls over `ranges` (computed once per routing)"""
    key = ("ref", routing, ranges_key)
    if key not in _cache:
        wl, pipe, joins, n, n_chunks, k = q41(ctx)
        out = capi.Output(pipe, 1024, 16384)
        count = 0
        for a, b in ranges:
            one = capi.DeviceMultiplexer(pipe, routing)
            capi.run_resident([one], [(a, b)], out=out, reset=True, finish=True)
            st = one.finish()
            count += sum(st["stage_out"][p][k - 1] for p in range(pipe.n_paths))
            one.close()
        _cache[key] = (count, _sorted_rows(out.fetch_ids()))
        out.close()
    return _cache[key]


N_CHUNKS_Q41 = 1172
LAYOUTS = {
    # name: (grant, ranges, the single-executor runs to compare against)
    "even-4": (16, [((e * N_CHUNKS_Q41) // 4, ((e + 1) * N_CHUNKS_Q41) // 4) for e in range(4)], "whole"),
    "one-owner-7": (5, [(0, 0)] * 3 + [(0, N_CHUNKS_Q41)] + [(0, 0)] * 3, "whole"),
    "gaps-5": (1, [(10, 300), (300, 301), (0, 0), (700, N_CHUNKS_Q41), (44, 44)], "gaps"),
}


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("routing", ["adaptive_reinit", "default_path", "opportunistic"])
def test_flat_pipeline_routes_every_chunk_once(gpu_ctx, routing, layout):
    wl, pipe, joins, n, n_chunks, k = q41(gpu_ctx)
    assert n_chunks == N_CHUNKS_Q41
    grant, ranges, ref = LAYOUTS[layout]
    ref_ranges = [(0, n_chunks)] if ref == "whole" else [r for r in ranges if r[0] < r[1]]
    want_count, want_rows = reference_rows(gpu_ctx, routing, ref, ref_ranges)
    if ref == "whole":
        assert want_count == GOLD["count_star"]
    mpxs = [capi.DeviceMultiplexer(pipe, routing) for _ in ranges]
    out = capi.Output(pipe, 1024, 16384)
    capi.run_resident_stealing(mpxs, ranges, grant, out=out, reset=True, finish=True)
    stats = capi.finish_many(mpxs)
    steal = [m.steal_stats() for m in mpxs]
    print(layout, routing, steal)
    assert sum(sum(st["input_tuple_count_per_path"]) for st in stats) == chunk_tuples(ranges, n)
    assert sum(sum(st["stage_out"][p][k - 1] for p in range(pipe.n_paths)) for st in stats) == want_count
    assert np.array_equal(_sorted_rows(out.fetch_ids()), want_rows)
    assert sum(s["chunks_routed"] for s in steal) == sum(b - a for a, b in ranges)
    for s in steal:
        assert s["chunks_stolen"] % grant == 0
        assert (s["n_steals"] == 0) == (s["chunks_stolen"] == 0)
    if layout == "one-owner-7":
        # all seven routers start together; the owner takes 5 of its 1 172 chunks per grant and needs at least one
        # routing step (a round trip through the probe pool) per grant, the thieves need one scan of seven words and one
        # compare-and-swap: for nothing to be stolen the owner would have to get through several hundred dependent
        # routing steps before the first thief's compare-and-swap
        assert sum(s["chunks_stolen"] for s in steal) > 0
    for m in mpxs:
        m.close()
    out.close()


def test_without_a_steal_it_is_the_fixed_range_run(gpu_ctx):
    """3 executors, even ranges, grant 5 000 >= every range: nobody has two grants, nobody can steal -- statistics and
    round logs of every executor equal those of run_resident over the same ranges"""
    wl, pipe, joins, n, n_chunks, k = q41(gpu_ctx)
    E = 3
    ranges = [((e * n_chunks) // E, ((e + 1) * n_chunks) // E) for e in range(E)]
    fixed = [capi.DeviceMultiplexer(pipe, "adaptive_reinit", max_log_rounds=1 << 16) for _ in range(E)]
    capi.run_resident(fixed, ranges, reset=True, finish=True)
    want_stats = capi.finish_many(fixed)
    want_logs = [m.fetch_log() for m in fixed]
    assert all(len(l[0]) > 0 for l in want_logs)
    mpxs = [capi.DeviceMultiplexer(pipe, "adaptive_reinit", max_log_rounds=1 << 16) for _ in range(E)]
    capi.run_resident_stealing(mpxs, ranges, 5000, reset=True, finish=True)
    stats = capi.finish_many(mpxs)
    for e in range(E):
        for key in STAT_KEYS:
            assert stats[e][key] == want_stats[e][key], (e, key)
        for a_, b_ in zip(mpxs[e].fetch_log(), want_logs[e]):
            assert np.array_equal(a_, b_)
        s = mpxs[e].steal_stats()
        assert s["n_steals"] == 0 and s["chunks_stolen"] == 0 and s["chunks_routed"] == ranges[e][1] - ranges[e][0]
    for m in fixed + mpxs:
        m.close()


@pytest.mark.parametrize("grant", [3, 120])
@pytest.mark.parametrize("pipeline", ["flat", "generic"])
def test_one_executor_is_the_morsel_run(gpu_ctx, pipeline, grant):
    """one executor has nobody to steal from: its grants are morsels of `grant` chunks pulled in order"""
    if pipeline == "flat":
        wl, pipe, joins, n, n_chunks, k = q41(gpu_ctx)
    else:
        wl, paths, pipe, n, n_chunks, k = star(gpu_ctx)
    a = capi.DeviceMultiplexer(pipe, "adaptive_reinit", max_log_rounds=1 << 16)
    capi.run_resident_morsels([a], 0, n_chunks, grant, reset=True, finish=True)
    want = a.finish()
    want_log = a.fetch_log()
    b = capi.DeviceMultiplexer(pipe, "adaptive_reinit", max_log_rounds=1 << 16)
    capi.run_resident_stealing([b], [(0, n_chunks)], grant, reset=True, finish=True)
    got = b.finish()
    assert sum(got["input_tuple_count_per_path"]) == n
    for key in STAT_KEYS:
        assert got[key] == want[key], key
    for x, y in zip(b.fetch_log(), want_log):
        assert np.array_equal(x, y)
    assert b.steal_stats() == {"chunks_routed": n_chunks, "chunks_stolen": 0, "n_steals": 0}
    a.close()
    b.close()


def test_generic_pipeline_with_thieves(gpu_ctx):
    """star_skew, emitting: 4 executors, grant 2, everything owned by executor 0 (196 chunks: at least one routing step
    per grant of two against one scan of four words for a thief -- something is stolen)"""
    wl, paths, pipe, n, n_chunks, k = star(gpu_ctx)
    P = len(paths)
    ref_out = capi.Output(pipe, 1024, 8192)
    one = capi.DeviceMultiplexer(pipe, "adaptive_reinit")
    capi.run_resident([one], [(0, n_chunks)], out=ref_out, reset=True, finish=True)
    st1 = one.finish()
    want_count = sum(st1["stage_out"][p][k - 1] for p in range(P))
    want_rows = _sorted_rows(ref_out.fetch_ids())
    assert want_count == len(want_rows) > 0
    mpxs = [capi.DeviceMultiplexer(pipe, "adaptive_reinit") for _ in range(4)]
    out = capi.Output(pipe, 1024, 8192)
    capi.run_resident_stealing(mpxs, [(0, n_chunks), (0, 0), (0, 0), (0, 0)], 2, out=out, reset=True, finish=True)
    stats = capi.finish_many(mpxs)
    steal = [m.steal_stats() for m in mpxs]
    print(steal)
    assert sum(sum(st["input_tuple_count_per_path"]) for st in stats) == n
    assert sum(sum(st["stage_out"][p][k - 1] for p in range(P)) for st in stats) == want_count
    assert not out.stats()[2]
    assert np.array_equal(_sorted_rows(out.fetch_ids()), want_rows)
    assert sum(s["chunks_routed"] for s in steal) == n_chunks
    assert all(s["chunks_stolen"] % 2 == 0 for s in steal)
    assert sum(s["chunks_stolen"] for s in steal) > 0
    for m in mpxs + [one]:
        m.close()
    out.close()
    ref_out.close()


def test_repeated_pass_gets_fresh_words(gpu_ctx):
    """the same call twice: the second finds its descriptors on the device (nothing is re-sent) -- the claim words, which
    the first pass has consumed, are initialised again all the same"""
    wl, pipe, joins, n, n_chunks, k = q41(gpu_ctx)
    E = 4
    ranges = [((e * n_chunks) // E, ((e + 1) * n_chunks) // E) for e in range(E)]
    mpxs = [capi.DeviceMultiplexer(pipe, "adaptive_reinit") for _ in range(E)]
    for rep in range(2):
        capi.run_resident_stealing(mpxs, ranges, 16, reset=True, finish=True)
        stats = capi.finish_many(mpxs)
        assert sum(sum(st["input_tuple_count_per_path"]) for st in stats) == n, rep
        assert sum(sum(st["stage_out"][p][k - 1] for p in range(pipe.n_paths)) for st in stats) == GOLD["count_star"], rep
        assert sum(m.steal_stats()["chunks_routed"] for m in mpxs) == n_chunks, rep
    for m in mpxs:
        m.close()


def _fused_setup(ctx, n):
    from test_gpu_engine_matrix import _fused_star
    joins, cols, valid = _fused_star(n=n)
    names = list(cols)
    pcols = list(cols.values())
    pvalid = [valid.get(c) for c in names]
    ght = [j.device(ctx) for j in joins]
    pipe = capi.Pipeline(ctx, pcols, n, [(h, [(-1, j.src)]) for h, j in zip(ght, joins)], [[0, 1], [1, 0]],
                         probe_valid=pvalid)
    return joins, cols, valid, names, ght, pipe


def test_scan_filtered_source(gpu_ctx):
    """scan_filter + use_scan_chunks: chunks of uneven size whose boundaries the router keeps a window of in LDS -- a
    thief jumps to another part of the table and the window follows"""
    n = 300_000
    joins, cols, valid, names, ght, pipe = _fused_setup(gpu_ctx, n)
    n_sel, n_chunks = pipe.scan_filter([(names.index("f"), "<", 60)])
    assert n_sel == int((cols["f"] < 60).sum()) and n_chunks > 200
    one = capi.DeviceMultiplexer(pipe, "adaptive_reinit")
    one.use_scan_chunks()
    capi.run_resident([one], [(0, n_chunks)], reset=True, finish=True)
    st1 = one.finish()
    want_count = sum(st1["stage_out"][p][1] for p in range(2))
    assert sum(st1["input_tuple_count_per_path"]) == n_sel and want_count > 0
    mpxs = [capi.DeviceMultiplexer(pipe, "adaptive_reinit") for _ in range(4)]
    for m in mpxs:
        m.use_scan_chunks()
    ranges = [(0, 7), (7, n_chunks - 40), (0, 0), (n_chunks - 40, n_chunks)]
    capi.run_resident_stealing(mpxs, ranges, 3, reset=True, finish=True)
    stats = capi.finish_many(mpxs)
    steal = [m.steal_stats() for m in mpxs]
    print(steal)
    assert sum(sum(st["input_tuple_count_per_path"]) for st in stats) == n_sel
    assert sum(sum(st["stage_out"][p][1] for p in range(2)) for st in stats) == want_count
    assert sum(s["chunks_routed"] for s in steal) == n_chunks
    assert all(s["chunks_stolen"] % 3 == 0 for s in steal)
    for m in mpxs + [one]:
        m.close()
    pipe.close()
    for h in ght:
        h.close()


def test_fused_sink_under_the_stealing_launch(gpu_ctx):
    """test_fused_sink_matrix's star, shape "two-joins", table source, against the same numpy GROUP BY"""
    from test_gpu_engine_matrix import FUSED_AGGS_SMALL, FUSED_SHAPES, _fused_want
    n = 50_000
    joins, cols, valid, names, ght, pipe = _fused_setup(gpu_ctx, n)
    raw_keys, in_lds = FUSED_SHAPES["two-joins"]
    keys = [(sj, names.index(sc) if sj < 0 else sc, mn, nv) for sj, sc, mn, nv in raw_keys]
    specs = FUSED_AGGS_SMALL
    dspecs = [(fn, sj, 0 if sc is None else (names.index(sc) if sj < 0 else sc)) for fn, sj, sc in specs]
    n_chunks = (n + 1023) // 1024
    want, dropped, n_rows = _fused_want(joins, cols, valid, names, keys, specs, None)
    out = capi.Output(pipe, 1024, 64)
    out.fuse_grouped(keys, dspecs)
    mpxs = [capi.DeviceMultiplexer(pipe, "adaptive_reinit") for _ in range(4)]
    capi.run_resident_stealing(mpxs, [(0, 0), (0, n_chunks - 9), (n_chunks - 9, n_chunks), (0, 0)], 2, out=out, reset=True,
                               finish=True)
    stats = capi.finish_many(mpxs)
    assert sum(sum(st["stage_out"][p][1] for p in range(2)) for st in stats) == n_rows
    vals, counts, got_dropped = out.fused_result()
    assert got_dropped == dropped
    n_groups = int(np.prod([key[3] for key in keys]))
    for q in range(n_groups):
        assert vals[q] == want[q], "group %d" % q
    assert out.stats()[0] == 0
    for m in mpxs:
        m.close()
    out.close()
    pipe.close()
    for h in ght:
        h.close()


def test_refusals_enqueue_nothing(gpu_ctx):
    wl, pipe, joins, n, n_chunks, k = q41(gpu_ctx)
    mpxs = [capi.DeviceMultiplexer(pipe, "adaptive_reinit") for _ in range(3)]
    good = [(0, 400), (400, 800), (800, n_chunks)]
    for ranges, grant, word in (([(0, 400), (399, 800), (800, n_chunks)], 8, "disjoint"),
                                (good, 0, "grant"),
                                ([(0, 400), (400, 800), (800, n_chunks + 1)], 8, "outside")):
        with pytest.raises(capi.PolrError) as e:
            capi.run_resident_stealing(mpxs, ranges, grant, reset=True, finish=True)
        assert e.value.code == capi.E_INVALID
        assert word in str(e.value), str(e.value)
    # nothing was enqueued, and the multiplexers run normally afterwards
    capi.run_resident(mpxs, good, reset=True, finish=True)
    stats = capi.finish_many(mpxs)
    assert sum(sum(st["input_tuple_count_per_path"]) for st in stats) == n
    assert sum(sum(st["stage_out"][p][k - 1] for p in range(pipe.n_paths)) for st in stats) == GOLD["count_star"]
    # ... and a plain run leaves no stealing counters
    for m in mpxs:
        assert m.steal_stats() == {"chunks_routed": 0, "chunks_stolen": 0, "n_steals": 0}
    capi.run_resident_stealing(mpxs, good, 8, reset=True, finish=True)
    stats = capi.finish_many(mpxs)
    assert sum(sum(st["input_tuple_count_per_path"]) for st in stats) == n
    assert sum(m.steal_stats()["chunks_routed"] for m in mpxs) == n_chunks
    capi.run_resident(mpxs, good, reset=True, finish=True)
    capi.finish_many(mpxs)
    for m in mpxs:
        assert m.steal_stats() == {"chunks_routed": 0, "chunks_stolen": 0, "n_steals": 0}
    for m in mpxs:
        m.close()
