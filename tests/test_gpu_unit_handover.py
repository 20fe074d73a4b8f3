"""What a probe wave of the flat pool kernel does between two units: the join-order switch (all stage records of the new
order in one batch), the look at its ring's three queues (hi / mid / lo: the tickets it lacks, then one load) and the
arrival (one counter atomic for all stages).  None of it may change a count.

Sources of 64 chunks of 1 024 rows and build sides of about 1 000 keys.  Every run is compared exactly -- the routing
trace, the tuples per join order, the intermediates, COUNT(*), where the routing fixes them the per-position counters
(tests/joinref.py), and the path resistances -- with the oracle and with the host-routed driver (the host mirror's
POLARPipelineExecutor, one launch per path run) over the same chunk range of every executor."""
import numpy as np
import pytest

import poolunits
from common import orc
from joinref import Join, Ref
from polr_amd import capi, host
from test_gpu_engine_matrix import _perfect_join

pytestmark = pytest.mark.gpu

CHUNK = 1024
N_CHUNKS = 64
RANGES = [(-300, 1199), (0, 1499), (-2000, -1), (5, 1604)]


def _bank(rng, k):
    """k joins, join c keyed by probe column c: perfect tables (a = min) with ONE unique-key hash table (a = mask) at
    position 1 next to them"""
    joins = [_perfect_join(rng, np.int32, lo, hi, 1000, c) for c, (lo, hi) in enumerate(RANGES[:k])]
    keys = rng.choice(np.arange(0, 200_000, 2, dtype=np.int32), 1000, replace=False)  # even; odd keys miss
    joins[1] = Join(keys, 1, None, None, [np.arange(len(keys), dtype=np.int32)])
    return joins


def _keys(rng, j, hit):
    n = len(hit)
    if j.perfect is None:
        miss = 2 * rng.integers(0, 100_000, n) + 1
    else:
        lo, hi = j.perfect
        holes = np.setdiff1d(np.arange(lo, hi + 1), j.keys.astype(np.int64))
        miss = np.where(rng.random(n) < 0.5, rng.choice(holes, n), rng.integers(hi + 1, hi + 5000, n))
    return np.where(hit, rng.choice(j.keys.astype(np.int64), n), miss).astype(np.int32)


def _source(rng, joins, n, rates, valid_on=None):
    """probe columns whose rows match join c with probability rates[c]; valid_on: a column that gets a validity array"""
    cols = [_keys(rng, j, rng.random(n) < rates[c]) for c, j in enumerate(joins)]
    pvalid = None
    if valid_on is not None:
        pvalid = [None] * len(joins)
        pvalid[valid_on] = (rng.random(n) > 0.1).astype(np.uint8)
    return cols, pvalid


class Case:
    """one pipeline on the device, its oracle joins and its numpy reference"""

    def __init__(self, ctx, joins, pcols, pvalid, orders, compiled, sel=None):
        self.ctx, self.joins, self.pcols, self.pvalid, self.orders, self.sel = ctx, joins, pcols, pvalid, orders, sel
        self.k = len(joins)
        self.ght = [j.device(ctx) for j in joins]
        assert self.ght[1].info()["kind"] == 2  # the unique-key hash table
        self.pipe = capi.Pipeline(ctx, pcols, len(pcols[0]), [(h, [(-1, j.src)]) for h, j in zip(self.ght, joins)], orders,
                                  probe_valid=pvalid)
        li = self.pipe.launch_info(False)
        assert li["flat"] == 1 and li["compiled_stages"] == compiled, li
        self.ojoins = [j.oracle() for j in joins]
        self.source = np.arange(len(pcols[0]), dtype=np.uint32) if sel is None else sel
        self.n = len(self.source)
        self.n_chunks = (self.n + CHUNK - 1) // CHUNK

    def rows_of(self, a, b):
        return self.source[a * CHUNK:min(self.n, b * CHUNK)]

    def expected(self, ranges, routing, **cfg):
        """per executor: (oracle result, host-routed result, numpy reference over its rows)"""
        want = []
        for a, b in ranges:
            rows = self.rows_of(a, b)
            offs = np.minimum(np.arange(0, len(rows) + CHUNK, CHUNK), len(rows)).astype(np.uint64)
            o = orc.run_pipeline(self.pcols, self.ojoins, self.orders, routing=routing, caching=False, collect_output=False,
                                 sel=rows, chunk_offsets=offs, probe_valid=self.pvalid, **cfg)
            self.pipe.set_selection(rows)
            h = host.run_pipeline(self.pipe, self.orders, routing, len(rows), chunk_offsets=offs, device_routed=False, **cfg)
            want.append((o, h, Ref(self.pcols, self.pvalid, self.joins, rows)))
        self.pipe.set_selection(self.sel)
        return want

    def multiplexers(self, n, routing, **cfg):
        return [capi.DeviceMultiplexer(self.pipe, routing, chunk_size=CHUNK, **cfg) for _ in range(n)]

    def check(self, mpxs, stats, want, routing):
        P, k = len(self.orders), self.k
        for e, (st, (o, h, ref)) in enumerate(zip(stats, want)):
            _, tuples, inter = mpxs[e].fetch_log()
            if routing == "alternate":
                assert np.array_equal(inter.reshape(-1, P), o["alt_matrix"]), e
            else:
                assert list(inter) == list(o["intermediates_per_round"]), e
            assert list(inter) == list(h["rounds"]), e
            assert st["num_intermediates"] == o["num_intermediates"] == h["num_intermediates"], e
            assert st["input_tuple_count_per_path"] == o["input_tuple_count_per_path"][:P] == h["input_tuple_count_per_path"], e
            assert st["path_resistances"] == h["path_resistances"], e
            if routing != "alternate":  # (ALTERNATE forwards path 0 only)
                assert sum(st["stage_out"][p][k - 1] for p in range(P)) == o["num_output_rows"], e
            if routing in ("alternate", "default_path"):
                for p in range(P if routing == "alternate" else 1):
                    assert st["stage_out"][p] == ref.stage_counts(self.orders[p]), (e, p)

    def close(self):
        self.pipe.close()
        for h in self.ght:
            h.close()


def _split(n_chunks, n_exec):
    return [((e * n_chunks) // n_exec, ((e + 1) * n_chunks) // n_exec) for e in range(n_exec)]


SWITCH_CASES = [("k2", 2, 2, None), ("k4", 4, 4, None), ("k3-on-k4", 3, 4, None), ("k4-sel", 4, 4, "sel")]


@pytest.mark.parametrize("name,k,compiled,form", SWITCH_CASES, ids=[c[0] for c in SWITCH_CASES])
def test_path_switch_on_every_unit(gpu_ctx, name, k, compiled, form):
    """ALTERNATE sends every chunk down every join order in turn, a unit each: consecutive units of a wave differ in join
    order.  One stage is the hash table (a = mask) next to perfect tables (a = min), the last join's column -- a deeper
    stage in all orders but one -- has a validity column; k = 3 runs on the K = 4 build (a stage beyond the last join
    stays inert)"""
    rng = np.random.default_rng(4100 + k + (7 if form else 0))
    joins = _bank(rng, k)
    n_tab = N_CHUNKS * CHUNK + (1500 if form else 0)
    pcols, pvalid = _source(rng, joins, n_tab, [0.7, 0.6, 0.8, 0.5][:k], valid_on=k - 1)
    sel = None
    if form:
        sel = np.sort(rng.choice(n_tab - 1, N_CHUNKS * CHUNK - 1, replace=False))
        sel = np.concatenate([sel, [n_tab - 1]]).astype(np.uint32)
    orders = [[(s + c) % k for c in range(k)] for s in range(k)]
    if k == 2:
        orders.append([0, 1])  # (two joins have two orders: the third path repeats the first)
    assert len(orders) >= 3
    case = Case(gpu_ctx, joins, pcols, pvalid, orders, compiled, sel)
    ranges = [(0, case.n_chunks)]
    want = case.expected(ranges, "alternate")
    mpxs = case.multiplexers(1, "alternate")
    capi.run_resident(mpxs, ranges, reset=True, finish=True)
    case.check(mpxs, capi.finish_many(mpxs), want, "alternate")
    for m in mpxs:
        m.close()
    case.close()


def test_a_join_order_whose_first_stage_kills_every_tuple(gpu_ctx):
    """join 0 matches nothing: in the order that starts with it every deeper counter is zero and every unit arrives with
    nothing but its stage-0 count of zero (no counter add at all); in the others the last counter is zero.  The run ends
    and every counter is exact"""
    rng = np.random.default_rng(4200)
    joins = _bank(rng, 4)
    pcols, pvalid = _source(rng, joins, N_CHUNKS * CHUNK, [0.0, 0.6, 0.8, 0.5])
    orders = [[0, 1, 2, 3], [1, 2, 3, 0], [2, 1, 0, 3]]
    case = Case(gpu_ctx, joins, pcols, pvalid, orders, 4)
    ranges = [(0, case.n_chunks)]
    for routing in ("alternate", "default_path"):
        want = case.expected(ranges, routing)
        assert want[0][2].stage_counts(orders[0]) == [0, 0, 0, 0]
        mpxs = case.multiplexers(1, routing)
        capi.run_resident(mpxs, ranges, reset=True, finish=True)
        stats = capi.finish_many(mpxs)
        assert stats[0]["stage_out"][0] == [0, 0, 0, 0]
        case.check(mpxs, stats, want, routing)
        for m in mpxs:
            m.close()
    case.close()


QUEUE_CASES = [("default_path", {}), ("init_once", {}), ("adaptive_reinit", {"init_tuple_count": 1024})]


@pytest.mark.parametrize("routing,cfg", QUEUE_CASES, ids=[c[0] for c in QUEUE_CASES])
def test_the_three_queues_across_passes(gpu_ctx, routing, cfg):
    """DEFAULT_PATH publishes on lo only, INIT_ONCE on hi then lo, ADAPTIVE_REINIT (init_tuple_count 1024) on hi and mid;
    7 executors.  After a first pass, three passes run back to back on the same multiplexers with no host
    synchronisation in between (reset and finish folded into the launches): every wave leaves a pass holding one mid
    ticket and no lo ticket, so the third pass's statistics are the first's"""
    rng = np.random.default_rng(4300)
    joins = _bank(rng, 4)
    pcols, pvalid = _source(rng, joins, N_CHUNKS * CHUNK, [0.7, 0.3, 0.8, 0.5], valid_on=3)
    orders = [[0, 1, 2, 3], [1, 2, 3, 0], [3, 2, 1, 0]]
    case = Case(gpu_ctx, joins, pcols, pvalid, orders, 4)
    ranges = _split(case.n_chunks, 7)
    want = case.expected(ranges, routing, **cfg)
    mpxs = case.multiplexers(7, routing, **cfg)
    hi_tuples = capi.pool_info(mpxs)["hi_tuples"]
    capi.run_resident(mpxs, ranges, reset=True, finish=True)
    first = capi.finish_many(mpxs)
    case.check(mpxs, first, want, routing)
    # the queues this routing publishes on, as far as the round logs tell: a round of up to hi_tuples tuples goes to hi, a
    # bigger one to lo if it is terminal (DEFAULT_PATH always, INIT_ONCE after its init phase) and to mid if its executor
    # waits for its counters (an exploit window of ADAPTIVE_REINIT -- whether or not the source ends behind it; only a
    # strategy that has stopped re-initialising sends it to lo, which the log does not show)
    logs = [m.fetch_log()[1] for m in mpxs]
    small = sum(int((t <= hi_tuples).sum()) for t in logs)
    big_last = sum(int(t[-1] > hi_tuples) for t in logs)
    big_before_more = sum(int((t[:-1] > hi_tuples).sum()) for t in logs)
    print("rounds: %d small, %d big and last, %d big with more behind" % (small, big_last, big_before_more))
    if routing == "default_path":
        assert small == 0 and big_last == 7 and big_before_more == 0  # lo only
    elif routing == "init_once":
        assert small > 0 and big_last == 7  # hi, then lo
    else:
        assert small > 0 and big_last + big_before_more > 0  # hi, and exploit windows (mid)
    for _ in range(3):
        capi.run_resident(mpxs, ranges, reset=True, finish=True)
    third = capi.finish_many(mpxs)
    case.check(mpxs, third, want, routing)
    for a, b in zip(first, third):
        for key in ("num_intermediates", "num_rounds", "input_tuple_count_per_path", "path_resistances", "stage_out"):
            assert a[key] == b[key], key
    for m in mpxs:
        m.close()
    case.close()


@pytest.mark.parametrize("routing", ["default_path", "adaptive_reinit"])
def test_the_smallest_rounds(gpu_ctx, routing):
    """the smallest pool the tuning allows, so that a round's units are no multiple of the rings in use; 64 executors with
    one chunk each (the last one 700 rows) and 5 executors over uneven ranges"""
    rng = np.random.default_rng(4400)
    joins = _bank(rng, 4)
    n = (N_CHUNKS - 1) * CHUNK + 700
    pcols, pvalid = _source(rng, joins, n, [0.7, 0.6, 0.8, 0.5])
    orders = [[0, 1, 2, 3], [2, 3, 0, 1], [3, 0, 1, 2]]
    case = Case(gpu_ctx, joins, pcols, pvalid, orders, 4)
    assert case.n_chunks == N_CHUNKS
    try:
        gpu_ctx.set_pool_tuning(device_share=16, units_x=1)
        for ranges in (_split(N_CHUNKS, N_CHUNKS), [(0, 3), (3, 4), (4, 31), (31, 33), (33, N_CHUNKS)]):
            want = case.expected(ranges, routing)
            mpxs = case.multiplexers(len(ranges), routing)
            info = capi.pool_info(mpxs)
            assert info["flat"] == 1 and info["n_rings"] > 1
            if routing == "default_path":
                # an executor's whole range is ONE round; the small ones (up to hi_tuples tuples) are cut into units of
                # hi_unit tuples whoever else is still routing: unit counts that are no multiple of the rings in use
                rows = [len(case.rows_of(a, b)) for a, b in ranges]
                units = [poolunits.unit_size(r, info["pool_waves"], 1, info["gran"], info["hi_tuples"], info["units_x"],
                                             info["hi_unit"])[1] for r in rows if r <= info["hi_tuples"]]
                assert units and any(u % info["n_rings"] != 0 for u in units), (units, info)
            capi.run_resident(mpxs, ranges, reset=True, finish=True)
            case.check(mpxs, capi.finish_many(mpxs), want, routing)
            for m in mpxs:
                m.close()
    finally:
        gpu_ctx.set_pool_tuning()
    case.close()
