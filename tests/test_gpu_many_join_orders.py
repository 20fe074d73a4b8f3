"""The device multiplexer with 9 to 32 join orders against the oracle, on the workloads of tests/manyorders.py (whose
conditions -- every order used, re-initialisations, split chunks, tied resistances -- test_many_join_orders.py asserts on
the CPU), and against the reference's own run with all 24 join orders of SSB-skew Q4.1
(tests/golden/many_join_orders.json).  Everything is compared exactly: path, tuples and intermediates of every routing
round, per-path tuple counts, totals, COUNT(*), output row sets.  Both launches throughout: one launch per routing round
(polr_mpx_run) and the resident pool launch (polr_mpx_run_resident)."""
import numpy as np
import pytest

import common
import manyorders as mo
from common import orc
from mpxreplay import replay
from polr_amd import capi, ssb_skew
from test_many_join_orders import alternate_digest, many_orders_fixture

pytestmark = pytest.mark.gpu

LAUNCHES = ("rounds", "resident")
_state = {}  # build sides, pipelines per (shape, P) and references: kept for the whole session, never closed


def _joins(ctx, shape):
    key = ("joins", shape)
    if key not in _state:
        _state[key] = capi.build_joins(ctx, mo.workload(shape))
        kinds = [j[0].info()["kind"] for j in _state[key]]
        # 1 = KIND_PERFECT, 2 = KIND_S8 (unique keys), 3 = KIND_S16 (repeated keys)
        assert kinds == ([1, 1, 1, 2, 2] if shape == "flat" else [1, 1, 1, 3, 2, 1])
    return _state[key]


def _probe_cols(shape):
    return list(mo.workload(shape)["probe"]["cols"].values())


def pipeline_for(ctx, shape, P):
    key = ("pipe", shape, P)
    if key not in _state:
        pipe = capi.Pipeline(ctx, _probe_cols(shape), mo.N, _joins(ctx, shape), mo.bank(shape, P))
        assert pipe.launch_info(False)["flat"] == (1 if shape == "flat" else 0)
        _state[key] = pipe
    return _state[key]


def expected(*args, **kw):
    """mo.expected, the last one kept: both launches of a case share it"""
    key = (args, tuple(sorted(kw.items())))
    if _state.get("ref_key") != key:
        _state["ref"] = mo.expected(*args, **kw)
        _state["ref_key"] = key
    return _state["ref"]


def _run(mpx, launch, a, b, out=None):
    if launch == "resident":
        mpx.run_resident(a, b, out=out)
    else:
        mpx.run(a, b, out=out)


def _n_chunks(n, chunk):
    return (n + chunk - 1) // chunk


def check_log(mpx, ref, where=None):
    path, tuples, inter = mpx.fetch_log()
    assert np.array_equal(inter, ref["intermediates_per_round"]), where
    assert np.array_equal(path, ref["round_path"]), where
    assert np.array_equal(tuples, ref["round_tuples"]), where
    return inter


def check_stats(st, ref, P, k, alternate=False, where=None):
    assert st["num_intermediates"] == ref["num_intermediates"], where
    assert st["input_tuple_count_per_path"] == ref["input_tuple_count_per_path"][:P], where
    last = [st["stage_out"][p][k - 1] for p in range(P)]
    if alternate:  # every join order sees every tuple and arrives at the same COUNT(*)
        assert last == [ref["num_output_rows"]] * P, where
    else:
        assert sum(last) == ref["num_output_rows"], where


def _trace_cases():
    return [(shape, P, routing, pset, chunk, launch) for shape in mo.SHAPES for P in mo.PS for routing in mo.STRATEGIES
            for pset, chunk in mo.param_cases(routing) for launch in LAUNCHES]


@pytest.mark.parametrize("shape,P,routing,pset,chunk,launch", _trace_cases())
def test_trace_matches_oracle(gpu_ctx, shape, P, routing, pset, chunk, launch):
    """the source in three calls, the cuts inside the first init phase: the routing state carries across calls"""
    kw = mo.routing_kwargs(routing, pset, chunk)
    ref = expected(shape, P, routing, kw, chunk)
    pipe = pipeline_for(gpu_ctx, shape, P)
    mpx = capi.DeviceMultiplexer(pipe, routing, chunk_size=chunk, **kw)
    cuts = mo.init_phase_cuts(P, kw, chunk, _n_chunks(mo.N, chunk))
    for a, b in zip(cuts[:-1], cuts[1:]):
        _run(mpx, launch, a, b)
    st = mpx.finish()
    inter = check_log(mpx, ref)
    if routing == "alternate":
        assert np.array_equal(inter.reshape(-1, P), ref["alt_matrix"])
    check_stats(st, ref, P, pipe.k, alternate=routing == "alternate")
    mpx.close()


def sorted_rows(ids, ojoins):
    """row ids in the oracle's terms (a perfect table numbers its rows by key value), sorted"""
    rows = ids.copy()
    for x, oj in enumerate(ojoins):
        if oj.ht.pht:
            rows[:, 1 + x] = oj.ht.pht_orig_rows()[ids[:, 1 + x]]
    return rows[np.lexsort(rows.T[::-1])]


@pytest.mark.parametrize("launch", LAUNCHES)
@pytest.mark.parametrize("routing", ["adaptive_reinit", "dynamic"])
@pytest.mark.parametrize("P", [25, 32])
@pytest.mark.parametrize("shape", mo.SHAPES)
def test_emitting_run_matches_oracle(gpu_ctx, shape, P, routing, launch):
    """the output row set of a run that changes its join order almost every unit (set B, chunks of 128)"""
    chunk = 128
    kw = mo.routing_kwargs(routing, mo.set_b(routing), chunk)
    ref = expected(shape, P, routing, kw, chunk, collect_output=True)
    ojoins = mo.oracle_side(shape)[2]
    pipe = pipeline_for(gpu_ctx, shape, P)
    mpx = capi.DeviceMultiplexer(pipe, routing, chunk_size=chunk, **kw)
    out = capi.Output(pipe, 1024, 8192)
    _run(mpx, launch, 0, _n_chunks(mo.N, chunk), out=out)
    st = mpx.finish()
    check_log(mpx, ref)
    check_stats(st, ref, P, pipe.k)
    n_rows, _, overflow = out.stats()
    assert not overflow and n_rows == ref["num_output_rows"]
    want = ref["out_rows"]
    assert np.array_equal(sorted_rows(out.fetch_ids(), ojoins), want[np.lexsort(want.T[::-1])])
    out.close()
    mpx.close()


@pytest.mark.parametrize("routing", ["adaptive_reinit", "opportunistic"])
@pytest.mark.parametrize("share", [1, 4])
@pytest.mark.parametrize("shape", mo.SHAPES)
def test_executors_match_oracle_runs_over_their_ranges(gpu_ctx, shape, share, routing):
    """7 executors over disjoint chunk ranges in one launch: each one's log and statistics are those of an oracle run over
    its range's rows.  Chunks of 128 (set B): an executor's some 5 700 tuples hold several init phases of 25 x 64"""
    P, n_exec, chunk = 25, 7, 128
    kw = mo.routing_kwargs(routing, mo.set_b(routing), chunk)
    n_chunks = _n_chunks(mo.N, chunk)
    ranges = [((e * n_chunks) // n_exec, ((e + 1) * n_chunks) // n_exec) for e in range(n_exec)]
    refs = [mo.expected(shape, P, routing, kw, chunk, rows=(a * chunk, min(b * chunk, mo.N))) for a, b in ranges]
    assert all(len(r["round_path"]) > P for r in refs)
    pipe = pipeline_for(gpu_ctx, shape, P)
    mpxs = [capi.DeviceMultiplexer(pipe, routing, chunk_size=chunk, **kw) for _ in range(n_exec)]
    for rep in range(2):  # (the second pass starts from what the first left behind)
        capi.run_resident(mpxs, ranges, reset=True, finish=True, share=share)
        stats = capi.finish_many(mpxs)
        for e in range(n_exec):
            check_log(mpxs[e], refs[e], where=(rep, e))
            check_stats(stats[e], refs[e], P, pipe.k, where=(rep, e))
    for m in mpxs:
        m.close()


@pytest.mark.parametrize("shape", mo.SHAPES)
def test_backpressure_with_25_executors(gpu_ctx, shape):
    """one executor per join order racing for morsels: which one gets a morsel is not fixed, the totals are"""
    P, chunk = 25, 128
    ref = mo.oracle_run(shape, P, "default_path", mo.routing_kwargs("default_path", "A", 1024), chunk)
    pipe = pipeline_for(gpu_ctx, shape, P)
    mpxs = [capi.DeviceMultiplexer(pipe, "backpressure", chunk_size=chunk) for _ in range(P)]
    k = pipe.k
    for _ in range(2):
        capi.run_backpressure(mpxs, 0, _n_chunks(mo.N, chunk), morsel_chunks=5)
        stats = capi.finish_many(mpxs)
        assert sum(sum(st["input_tuple_count_per_path"]) for st in stats) == mo.N
        assert sum(sum(st["stage_out"][p][k - 1] for p in range(P)) for st in stats) == ref["num_output_rows"]
    for m in mpxs:
        m.close()


# --- edges ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("launch", LAUNCHES)
@pytest.mark.parametrize("routing", ["adaptive_reinit", "dynamic"])
@pytest.mark.parametrize("shape", mo.SHAPES)
def test_chunks_of_2048_with_32_orders(gpu_ctx, shape, routing, launch):
    """the largest vector the oracle takes; every chunk of the init phase is split between two join orders"""
    P, chunk = 32, 2048
    kw = {"regret_budget": 0.2, "init_tuple_count": 1024, "atc_multiplier": 1}
    ref = expected(shape, P, routing, kw, chunk)
    assert len(ref["round_path"]) > P
    pipe = pipeline_for(gpu_ctx, shape, P)
    mpx = capi.DeviceMultiplexer(pipe, routing, chunk_size=chunk, **kw)
    _run(mpx, launch, 0, _n_chunks(mo.N, chunk))
    st = mpx.finish()
    check_log(mpx, ref)
    check_stats(st, ref, P, pipe.k)
    mpx.close()


@pytest.mark.parametrize("launch", LAUNCHES)
@pytest.mark.parametrize("routing", mo.ADAPTIVE)
@pytest.mark.parametrize("shape", mo.SHAPES)
def test_source_ends_inside_the_first_init_phase(gpu_ctx, shape, routing, launch):
    """20 chunks over 32 join orders: the run is closed with 12 orders never measured"""
    P, chunk, n_src = 32, 1024, 20
    kw = mo.routing_kwargs(routing, "A", chunk, n=n_src * chunk)
    ref = expected(shape, P, routing, kw, chunk, rows=(0, n_src * chunk))
    assert len(ref["round_path"]) == n_src and ref["input_tuple_count_per_path"].count(0) == P - n_src
    pipe = pipeline_for(gpu_ctx, shape, P)
    mpx = capi.DeviceMultiplexer(pipe, routing, chunk_size=chunk, **kw)
    _run(mpx, launch, 0, n_src)
    st = mpx.finish()
    check_log(mpx, ref)
    check_stats(st, ref, P, pipe.k)
    mpx.close()


SCAN_VECTOR = 128  # scan vectors of 128 rows leave chunks of some 64: with init_tuple_count 64 the init phase of 32 orders ends a tenth into the run


def _scan_reference(shape, P, routing, kw):
    """the oracle over a filtered source (scan chunks of unequal size): its pipeline run and, for path and tuples of every
    round, its multiplexer replayed over the selected rows"""
    key = ("scan", shape, P, routing)
    if key not in _state:
        pcols, pvalid, ojoins = mo.oracle_side(shape)
        flt = [(2, "<=", int(np.median(pcols[2])))]  # on k1
        osel, ooffs = orc.scan_filter(pcols, flt, vector_size=SCAN_VECTOR)
        sizes = np.diff(ooffs.astype(np.int64))
        assert 0 < len(osel) < mo.N and len(set(sizes[:-1].tolist())) > 8  # ragged
        ref = orc.run_pipeline(pcols, ojoins, mo.bank(shape, P), routing=routing, caching=False, collect_output=False,
                               sel=osel, chunk_offsets=ooffs, **kw)
        per_tuple = np.diff(mo.prefix(shape, P), axis=0)[osel]
        pre = np.concatenate([np.zeros((1, P), dtype=np.int64), np.cumsum(per_tuple, axis=0)])
        rounds, slices = replay(orc.Multiplexer(P, routing, **kw), pre, len(osel), chunk_offsets=ooffs)
        assert len(rounds) > P  # (the run goes on past its first init phase)
        assert [s[0] for s in slices] == list(ref["trace_path"]) and [s[1] for s in slices] == list(ref["trace_tuples"])
        assert [r[2] for r in rounds] == list(ref["intermediates_per_round"])
        ref["round_path"] = np.asarray([r[0] for r in rounds], dtype=np.uint32)
        ref["round_tuples"] = np.asarray([r[1] for r in rounds], dtype=np.uint64)
        _state[key] = (flt, osel, ooffs, ref)
    return _state[key]


@pytest.mark.parametrize("launch", LAUNCHES)
@pytest.mark.parametrize("routing", ["adaptive_reinit", "dynamic"])
@pytest.mark.parametrize("shape", mo.SHAPES)
def test_scan_filtered_source_with_32_orders(gpu_ctx, shape, routing, launch):
    P = 32
    kw = mo.routing_kwargs(routing, mo.set_b(routing), SCAN_VECTOR)
    flt, osel, ooffs, ref = _scan_reference(shape, P, routing, kw)
    # (a pipeline of its own: the scan leaves its selection behind)
    pipe = capi.Pipeline(gpu_ctx, _probe_cols(shape), mo.N, _joins(gpu_ctx, shape), mo.bank(shape, P))
    n_sel, n_chunks = pipe.scan_filter(flt, vector_size=SCAN_VECTOR)
    assert n_sel == len(osel) and n_chunks == len(ooffs) - 1
    mpx = capi.DeviceMultiplexer(pipe, routing, chunk_size=SCAN_VECTOR, **kw)
    mpx.use_scan_chunks()
    _run(mpx, launch, 0, n_chunks)
    st = mpx.finish()
    check_log(mpx, ref)
    check_stats(st, ref, P, pipe.k)
    mpx.close()
    pipe.close()


def test_33_orders_are_refused(gpu_ctx):
    shape = "flat"
    paths = np.asarray(mo.legal_orders(shape)[:33], dtype=np.int32)
    with pytest.raises(capi.PolrError) as e:
        capi.Pipeline(gpu_ctx, _probe_cols(shape), mo.N, _joins(gpu_ctx, shape), paths)
    assert e.value.code == capi.E_UNSUPPORTED
    # ... and 32 of them are taken, by a pipeline that works
    kw = mo.routing_kwargs("init_once", "A", 1024)
    pcols, pvalid, ojoins = mo.oracle_side(shape)
    ref = orc.run_pipeline(pcols, ojoins, paths[:32], routing="init_once", caching=False, collect_output=False, **kw)
    pipe = capi.Pipeline(gpu_ctx, _probe_cols(shape), mo.N, _joins(gpu_ctx, shape), paths[:32])
    mpx = capi.DeviceMultiplexer(pipe, "init_once", **kw)
    mpx.run_resident(0, _n_chunks(mo.N, 1024))
    st = mpx.finish()
    assert np.array_equal(mpx.fetch_log()[2], ref["intermediates_per_round"])
    check_stats(st, ref, 32, pipe.k)
    mpx.close()
    pipe.close()


# --- the reference with 24 join orders ------------------------------------------------------------------------------
def _fixture_pipeline(ctx):
    if "gold_pipe" not in _state:
        gold, wl, pcols, ojoins = many_orders_fixture()
        joins = capi.build_joins(ctx, wl, auto=True)
        _state["gold_pipe"] = capi.Pipeline(ctx, pcols, len(pcols[0]), joins, np.asarray(gold["paths"], dtype=np.int32))
    return _state["gold_pipe"]


@pytest.mark.parametrize("launch", LAUNCHES)
def test_device_alternate_matches_reference_at_24_orders(gpu_ctx, launch):
    gold, wl, pcols, ojoins = many_orders_fixture()
    pipe = _fixture_pipeline(gpu_ctx)
    n = len(pcols[0])
    mpx = capi.DeviceMultiplexer(pipe, "alternate")
    _run(mpx, launch, 0, _n_chunks(n, 1024))
    st = mpx.finish()
    inter = mpx.fetch_log()[2]
    assert alternate_digest(inter.reshape(-1, 24)) == gold["alternate"]["digest"]
    assert st["num_intermediates"] == gold["alternate"]["intms"]
    assert [st["stage_out"][p][pipe.k - 1] for p in range(24)] == [gold["count_star"]] * 24
    mpx.close()


@pytest.mark.parametrize("launch", LAUNCHES)
@pytest.mark.parametrize("routing", ["init_once", "opportunistic", "adaptive_reinit", "dynamic", "exponential_backoff",
                                     "default_path"])
def test_device_routing_matches_reference_at_24_orders(gpu_ctx, routing, launch):
    gold, wl, pcols, ojoins = many_orders_fixture()
    g = gold["routing"][routing]
    pipe = _fixture_pipeline(gpu_ctx)
    n = len(pcols[0])
    budget = n / 10240.0 / 10 / 1 if routing == "exponential_backoff" else 0.01  # polar_config.cpp:115-120
    mpx = capi.DeviceMultiplexer(pipe, routing, regret_budget=budget)
    n_chunks = _n_chunks(n, 1024)
    cuts = [0, n_chunks // 3, n_chunks // 3 + 1, n_chunks]
    for a, b in zip(cuts[:-1], cuts[1:]):
        _run(mpx, launch, a, b)
    st = mpx.finish()
    path, tuples, inter = mpx.fetch_log()
    assert list(inter) == g["rounds"]
    assert st["num_intermediates"] == g["intms"]
    assert st["input_tuple_count_per_path"] == g["tuple_counts"]
    assert int(tuples.sum()) == n
    assert sum(st["stage_out"][p][pipe.k - 1] for p in range(24)) == gold["count_star"]
    mpx.close()
