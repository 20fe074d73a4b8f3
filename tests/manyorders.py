"""Workloads for the multiplexer with 9 to 32 join orders, and their expected results from the oracle.

Two shapes over 40 000 probe rows with integer keys:
  flat     5 joins, each keyed by a probe column of its own: three perfect tables, two unique-key hash tables
  generic  the same, but join 3's build keys repeat, and a sixth join is keyed by a payload column of join 0 (legal join
           orders have join 0 in front of join 5)
Every join's selectivity drifts along the table, so the best join order changes; in the first quarter of the table join
MISS_JOIN matches nothing, so all join orders that begin with it measure the same resistance (0.5) -- the first quarter,
because a resistance is smoothed with the order's history from its second measurement on, and histories differ.

The bank of P join orders: the original order, then a seeded draw from the legal permutations, four of them from those
that begin with MISS_JOIN (of 120 permutations a plain draw of 8 would hold four such orders once in twenty seeds).

Expected values come from the oracle alone: orc.run_pipeline for the totals, the intermediates of every round and the
output rows; the (path, tuples) of every round from the oracle's Multiplexer driven through mpxreplay.replay with the
oracle's per-tuple intermediates -- and that replay must reproduce the pipeline run's own slices, round log and counts
(asserted in expected())."""
import itertools

import numpy as np

import common
from common import orc
from mpxreplay import replay

N = 40_000
PS = (9, 16, 17, 25, 32)
SHAPES = ("flat", "generic")
STRATEGIES = ("alternate", "adaptive_reinit", "dynamic", "init_once", "opportunistic", "default_path",
              "exponential_backoff")
ADAPTIVE = ("adaptive_reinit", "dynamic", "init_once", "opportunistic", "exponential_backoff")
MISS_JOIN = 2
MISS_END = N // 4  # rows [0, MISS_END): join MISS_JOIN matches nothing
SEED = 20260131

# parameter set -> regret_budget, atc_multiplier, {chunk size: init_tuple_count}
# ADAPTIVE_REINIT runs set B_ar in place of set B.  With a budget of 0.5 a window is some 6 500 tuples here, and as long
# as the best order is one the window has not visited, a new window follows without an init phase in between: 37 rounds
# at P = 32, one re-init.  2.0 gives at least 192 rounds (3 P = 96) on both shapes; 1.0 gives 100 and 98.  With chunks
# (and an init_tuple_count) of 1024 its first init phase covers 32 768 of the 40 000 tuples at P = 32 and no second one
# follows, so B_ar has chunks of 128 only.
PARAM_SETS = {
    "A": (0.01, 1, {1024: 1024}),
    "B": (0.5, 1, {1024: 1024, 128: 64}),
    "B_ar": (2.0, 1, {128: 64}),
    "C": (0.2, 2, {1024: 1024, 128: 128}),
}

_cache = {}


def _rng(*salt):
    return np.random.default_rng(np.random.SeedSequence([SEED] + [int(s) for s in salt]))


def workload(shape):
    key = ("wl", shape)
    if key in _cache:
        return _cache[key]
    rng = _rng(1)
    x = np.arange(N) / N
    fact = {"id": np.arange(N, dtype=np.int32)}
    joins = []
    # (number of key values, stride of the key values, perfect table)
    dims = [(3_000, 1, True), (500, 1, True), (8_000, 1, True), (6_000, 1_009, False), (2_500, 4_003, False)]
    for d, (n_keys, stride, perfect) in enumerate(dims):
        keys = (np.arange(n_keys, dtype=np.int64) * stride + 17 + d).astype(np.int32)
        keep = rng.random(n_keys) < 0.5
        kept, dropped = keys[keep], keys[~keep]
        hit_prob = 0.5 + 0.45 * np.sin(2 * np.pi * (1.3 * x + d / 5.0))
        if d == MISS_JOIN:
            hit_prob[:MISS_END] = 0.0
        hit = rng.random(N) < hit_prob
        fact["k%d" % d] = np.where(hit, kept[rng.integers(0, len(kept), N)],
                                   dropped[rng.integers(0, len(dropped), N)]).astype(np.int32)
        bkeys = kept[rng.permutation(len(kept))]
        if shape == "generic" and d == 3:
            bkeys = np.repeat(bkeys, rng.integers(1, 4, size=len(bkeys)))  # repeated build keys
            bkeys = bkeys[rng.permutation(len(bkeys))]
        payload = {"r%d" % d: rng.integers(0, 50, len(bkeys)).astype(np.int32),
                   "q%d" % d: (bkeys % 251).astype(np.int16)}
        joins.append({"name": "d%d" % d, "keys": [bkeys.astype(np.int32)], "key_names": ["k"], "payload": payload,
                      "key_src": [(-1, 1 + d)], "perfect": (int(keys.min()), int(keys.max())) if perfect else None})
    if shape == "generic":
        k5 = np.arange(40, dtype=np.int32)[rng.permutation(40)]  # 40 of the 50 values of d0.r0
        joins.append({"name": "d5", "keys": [k5], "key_names": ["k"], "payload": {"r5": k5 * 3}, "key_src": [(0, 0)],
                      "perfect": (0, 49)})
    wl = {"name": "many_orders_" + shape, "probe": {"name": "fact", "cols": fact}, "joins": joins}
    _cache[key] = wl
    return wl


def legal_orders(shape):
    k = 5 if shape == "flat" else 6
    perms = [list(p) for p in itertools.permutations(range(k))]
    if shape == "generic":
        perms = [p for p in perms if p.index(0) < p.index(5)]
    return perms


def bank(shape, P):
    """P legal join orders, seeded; order 0 is the original order, four begin with MISS_JOIN"""
    key = ("bank", shape, P)
    if key not in _cache:
        rng = _rng(2, SHAPES.index(shape), P)
        perms = legal_orders(shape)
        original = perms[0]
        assert original == sorted(original)
        miss = [p for p in perms if p[0] == MISS_JOIN]
        rest = [p for p in perms if p[0] != MISS_JOIN and p != original]
        drawn = [miss[i] for i in rng.choice(len(miss), 4, replace=False)]
        drawn += [rest[i] for i in rng.choice(len(rest), P - 5, replace=False)]
        drawn = [drawn[i] for i in rng.permutation(len(drawn))]
        _cache[key] = np.asarray([original] + drawn, dtype=np.int32)
    return _cache[key]


def routing_kwargs(routing, pset, chunk, n=N):
    budget, atc, inits = PARAM_SETS[pset]
    if routing == "exponential_backoff":
        budget = n / 10240.0 / 10 / 1  # polar_config.cpp:115-120: the knob is this strategy's window cap
    return {"regret_budget": budget, "init_tuple_count": inits[chunk], "atc_multiplier": atc}


def set_b(routing):
    """the name of set B for a strategy"""
    return "B_ar" if routing == "adaptive_reinit" else "B"


def param_cases(routing):
    """(parameter set, chunk size) pairs a strategy runs with"""
    skip = "B" if routing == "adaptive_reinit" else "B_ar"
    return [(pset, chunk) for pset, (_b, _a, inits) in PARAM_SETS.items() if pset != skip for chunk in inits]


def oracle_side(shape):
    key = ("orc", shape)
    if key not in _cache:
        _cache[key] = common.oracle_joins(workload(shape))
    return _cache[key]


def prefix(shape, P):
    """prefix[t, p] = intermediates the tuples [0, t) produce on join order p (oracle, ALTERNATE over 1-tuple chunks)"""
    key = ("prefix", shape, P)
    if key not in _cache:
        pcols, pvalid, ojoins = oracle_side(shape)
        res = orc.run_pipeline(pcols, ojoins, bank(shape, P), routing="alternate", caching=False, collect_output=False,
                               chunk_offsets=np.arange(N + 1, dtype=np.uint64))
        m = res["alt_matrix"].astype(np.int64)
        assert m.shape == (N, P)
        _cache[key] = np.concatenate([np.zeros((1, P), dtype=np.int64), np.cumsum(m, axis=0)])
    return _cache[key]


def oracle_run(shape, P, routing, kw, chunk, rows=None, collect_output=False, sel=None, chunk_offsets=None):
    """orc.run_pipeline over probe rows [rows[0], rows[1]) (default: all)"""
    pcols, pvalid, ojoins = oracle_side(shape)
    if rows is not None:
        pcols = [c[rows[0]:rows[1]] for c in pcols]
    return orc.run_pipeline(pcols, ojoins, bank(shape, P), routing=routing, caching=False, vector_size=chunk,
                            collect_output=collect_output, sel=sel, chunk_offsets=chunk_offsets, **kw)


def expected(shape, P, routing, kw, chunk, rows=None, collect_output=False, watch=None):
    """the oracle's pipeline run, plus the (path, tuples, intermediates) of every round from the oracle's own multiplexer
    replayed over the oracle's per-tuple intermediates.  The two must agree wherever they overlap."""
    a, b = rows if rows is not None else (0, N)
    ref = oracle_run(shape, P, routing, kw, chunk, rows=rows, collect_output=collect_output)
    pre = prefix(shape, P)[a:b + 1]
    mpx = orc.Multiplexer(P, routing, **kw)
    rounds, slices = replay(mpx, pre, b - a, chunk, watch=watch)
    assert [s[0] for s in slices] == list(ref["trace_path"]) and [s[1] for s in slices] == list(ref["trace_tuples"])
    assert [r[2] for r in rounds] == list(ref["intermediates_per_round"])
    tuples = [0] * P
    for p, t, _i in rounds:
        tuples[p] += t
    assert tuples == ref["input_tuple_count_per_path"]
    ref["resistances"] = mpx.resistances()  # (after the closing FinalizePathRun)
    ref["round_path"] = np.asarray([r[0] for r in rounds], dtype=np.uint32)
    ref["round_tuples"] = np.asarray([r[1] for r in rounds], dtype=np.uint64)
    return ref


def init_phase_cuts(P, kw, chunk, n_chunks):
    """the source in three calls, the middle one a single chunk inside the first init phase"""
    c1 = max(1, P * kw["init_tuple_count"] // chunk // 3)
    assert c1 + 1 < n_chunks
    return [0, c1, c1 + 1, n_chunks]


def largest_tie(resistances):
    """size of the largest group of equal, measured (non-zero) resistances"""
    r = [x for x in resistances if x != 0]
    return max((r.count(x) for x in set(r)), default=0)
