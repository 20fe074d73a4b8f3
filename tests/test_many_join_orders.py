"""The routing code with 9 to 32 join orders, on the CPU: the C++ host mirror (the same polr_routing.h the device routers
compile) against the oracle, on the workloads of tests/manyorders.py -- round log, per-path tuple counts and total, for
every P, strategy and parameter set; the conditions that keep those workloads from being degenerate (every order is
used, ADAPTIVE_REINIT re-initialises, DYNAMIC splits chunks, resistances tie); and the oracle's own routing code against
the reference's run with all 24 join orders of SSB-skew Q4.1 (tests/golden/many_join_orders.json)."""
import hashlib
import itertools

import numpy as np
import pytest

import common
import manyorders as mo
from common import orc
from mpxreplay import replay
from polr_amd import host, ssb_skew


def _host_cases():
    return [(shape, P, routing, pset, chunk) for shape in mo.SHAPES for P in mo.PS for routing in mo.STRATEGIES
            for pset, chunk in mo.param_cases(routing)]


@pytest.mark.parametrize("shape,P,routing,pset,chunk", _host_cases())
def test_host_multiplexer_matches_oracle(shape, P, routing, pset, chunk):
    kw = mo.routing_kwargs(routing, pset, chunk)
    ref = mo.expected(shape, P, routing, kw, chunk)
    mpx = host.HostMultiplexer(P, routing, **kw)
    rounds, slices = replay(mpx, mo.prefix(shape, P), mo.N, chunk)
    lines = mpx.log_csv().strip().splitlines()
    if routing == "alternate":
        assert lines[0] == "".join("path_%d," % i for i in range(P))
        matrix = np.asarray([[int(x) for x in l.rstrip(",").split(",")] for l in lines[1:]], dtype=np.uint64)
        assert np.array_equal(matrix, ref["alt_matrix"])
        logged = [int(x) for x in matrix.reshape(-1)]
    else:
        logged = [int(x) for x in lines[1:]]
    assert logged == list(ref["intermediates_per_round"])
    assert [r[0] for r in rounds] == list(ref["round_path"])
    assert [r[1] for r in rounds] == list(ref["round_tuples"])
    assert mpx.tuple_counts() == ref["input_tuple_count_per_path"]
    assert sum(logged) == ref["num_intermediates"]
    assert sum(mpx.tuple_counts()) == mo.N * (P if routing == "alternate" else 1)  # (ALTERNATE: every order sees every tuple)


@pytest.mark.parametrize("shape", mo.SHAPES)
@pytest.mark.parametrize("P", mo.PS)
def test_banks_are_legal_and_distinct(shape, P):
    paths = mo.bank(shape, P)
    k = 5 if shape == "flat" else 6
    assert paths.shape == (P, k) and list(paths[0]) == list(range(k))
    assert len({tuple(p) for p in paths}) == P
    for p in paths:
        p = list(p)
        assert sorted(p) == list(range(k))
        assert shape == "flat" or p.index(0) < p.index(5)
    assert sum(1 for p in paths if p[0] == mo.MISS_JOIN) >= 4
    # nothing matches join MISS_JOIN in the first quarter, and something does afterwards
    pre = mo.prefix(shape, P)
    first = [i for i, p in enumerate(paths) if p[0] == mo.MISS_JOIN]
    assert all(pre[mo.MISS_END, i] == 0 and pre[-1, i] > 0 for i in first)
    others = [i for i in range(P) if i not in first]
    assert all(pre[mo.MISS_END, i] > 0 for i in others)


@pytest.mark.parametrize("shape", mo.SHAPES)
@pytest.mark.parametrize("P", mo.PS)
@pytest.mark.parametrize("routing", mo.ADAPTIVE)
def test_guard_every_order_receives_tuples(shape, P, routing):
    for pset, chunk in mo.param_cases(routing):
        ref = mo.expected(shape, P, routing, mo.routing_kwargs(routing, pset, chunk), chunk)
        assert min(ref["input_tuple_count_per_path"]) > 0, (pset, chunk)
        # ... and not through the init phase alone, which visits every order whatever follows (INIT_ONCE keeps to one
        # order after it; ADAPTIVE_REINIT has test_guard_adaptive_reinit_has_three_init_phases)
        if routing in ("dynamic", "opportunistic", "exponential_backoff"):
            assert len(set(ref["round_path"][P:].tolist())) >= 2, (pset, chunk)


@pytest.mark.parametrize("shape", mo.SHAPES)
@pytest.mark.parametrize("P", mo.PS)
def test_guard_adaptive_reinit_has_three_init_phases(shape, P):
    for pset, chunk in mo.param_cases("adaptive_reinit"):
        if pset != "B_ar":
            continue
        ref = mo.oracle_run(shape, P, "adaptive_reinit", mo.routing_kwargs("adaptive_reinit", pset, chunk), chunk)
        assert len(ref["intermediates_per_round"]) >= 3 * P, (pset, chunk)


@pytest.mark.parametrize("shape", mo.SHAPES)
@pytest.mark.parametrize("P", mo.PS)
def test_guard_dynamic_splits_chunks_and_carries_small_shares(shape, P):
    """DYNAMIC hands out parts of a chunk that are no multiple of 64 (the table, the chunk sizes and the init_tuple_counts
    all are).  Not asked of set B with chunks of 128: its window is 128 tuples, shares below 64 are carried over, and what
    is left of 128 in shares of at least 64 is 128 or 64 + 64 -- there the rule shows as rounds of 64 and 128 only"""
    for pset, chunk in mo.param_cases("dynamic"):
        if (pset, chunk) == ("B", 128):
            ref = mo.expected(shape, P, "dynamic", mo.routing_kwargs("dynamic", pset, chunk), chunk)
            assert set(int(t) for t in ref["round_tuples"][:-1]) == {64, 128}
            # the carry at work: a window serves two orders at the most, and without the carry an order whose share
            # of 128 is below 64 would never be served -- yet some 8 rounds in a row (4 windows or more, over which
            # the weights hardly move) go to 5 orders or more
            after = ref["round_path"][P:].tolist()
            assert max(len(set(after[i:i + 8])) for i in range(len(after) - 8)) >= 5
            continue
        ref = mo.expected(shape, P, "dynamic", mo.routing_kwargs("dynamic", pset, chunk), chunk)
        assert np.any(ref["round_tuples"][:-1] % 64 != 0), (pset, chunk)


@pytest.mark.parametrize("shape", mo.SHAPES)
@pytest.mark.parametrize("P", mo.PS)
def test_guard_resistances_tie_in_the_all_miss_quarter(shape, P):
    """host mirror's state: with every order measured (DYNAMIC's init phase done, so every later window closes into
    CalculateJoinPathWeights over these values) at least four orders have the same resistance inside the all-miss quarter"""
    kw = mo.routing_kwargs("dynamic", "B", 128)
    seen = []

    def watch(mpx, begin):
        r = mpx.resistances()
        if begin < mo.MISS_END and all(x != 0 for x in r):
            seen.append(mo.largest_tie(r))

    mpx = host.HostMultiplexer(P, "dynamic", **kw)
    replay(mpx, mo.prefix(shape, P), mo.N, 128, watch=watch)
    assert len(seen) >= 8 and max(seen) >= 4


def test_join_path_weights_match_oracle_with_ties():
    """CalculateJoinPathWeights over up to 32 costs with runs of equal values and values 0.001 apart"""
    rng = np.random.default_rng(9)
    for _ in range(300):
        n = int(rng.integers(9, 33))
        pool = np.round(rng.uniform(0.5, 6.0, int(rng.integers(2, 8))), int(rng.integers(1, 4)))
        costs = [float(x) for x in rng.choice(pool, n)]
        for i in rng.choice(n, 3, replace=False):
            costs[i] += 0.001 * int(rng.integers(0, 3))
        b = float(rng.choice([0.01, 0.2, 0.5]))
        assert host.join_path_weights(costs, b) == orc.join_path_weights(costs, b)


# --- the reference with 24 join orders ------------------------------------------------------------------------------
_gold = {}


def many_orders_fixture():
    """(fixture, workload, probe columns, oracle joins)"""
    if not _gold:
        gold = common.load_golden("many_join_orders")
        wl = ssb_skew.workload(gold["query"], **gold["shape"])
        pcols, pvalid, ojoins = common.oracle_joins(wl)
        _gold.update(gold=gold, wl=wl, pcols=pcols, ojoins=ojoins)
    return _gold["gold"], _gold["wl"], _gold["pcols"], _gold["ojoins"]


def alternate_digest(matrix):
    m = np.ascontiguousarray(matrix, dtype=np.uint64)
    return {"n_rows": int(m.shape[0]), "column_sums": [int(x) for x in m.sum(axis=0)],
            "sha1": hashlib.sha1(m.tobytes()).hexdigest()}


def test_fixture_holds_all_24_orders():
    gold, wl, pcols, ojoins = many_orders_fixture()
    assert gold["max_join_orders"] == 24
    assert sorted(tuple(p) for p in gold["paths"]) == sorted(itertools.permutations(range(4)))


def test_oracle_alternate_matches_reference_at_24_orders():
    gold, wl, pcols, ojoins = many_orders_fixture()
    res = orc.run_pipeline(pcols, ojoins, gold["paths"], routing="alternate", caching=False, collect_output=False)
    assert alternate_digest(res["alt_matrix"]) == gold["alternate"]["digest"]
    assert res["num_intermediates"] == gold["alternate"]["intms"]
    assert res["num_output_rows"] == gold["count_star"]


@pytest.mark.parametrize("routing", ["init_once", "opportunistic", "adaptive_reinit", "dynamic", "exponential_backoff",
                                     "default_path"])
def test_oracle_routing_matches_reference_at_24_orders(routing):
    gold, wl, pcols, ojoins = many_orders_fixture()
    g = gold["routing"][routing]
    budget = len(pcols[0]) / 10240.0 / 10 / 1 if routing == "exponential_backoff" else 0.01
    res = orc.run_pipeline(pcols, ojoins, gold["paths"], routing=routing, caching=False, collect_output=False,
                           regret_budget=budget)
    assert list(res["intermediates_per_round"]) == g["rounds"]
    assert res["num_intermediates"] == g["intms"]
    assert res["input_tuple_count_per_path"] == g["tuple_counts"]
    assert res["num_output_rows"] == gold["count_star"]
