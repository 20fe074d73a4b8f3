"""The flat pool kernel's sweep at every fill level of its slot groups.

A sweep (flat_sweep, polr_flat_device.h) pops up to 64 x flat_sweep_f<K>() entries from every deeper queue and loads keys
and table words for ALL its slots without a branch around any load: a slot that holds no tuple reads what the unit's
FIRST tuple reads (the "safe row") and must never count, push or emit.  Here one executor's DEFAULT_PATH round over a
source of 2 748 or 3 072 tuples runs in units of 1 024 tuples (a small round: hi_unit) on the smallest pool the tuning
allows, and the survivors of stage 0 per unit are constructed to be exactly 0, 1, 63, 64, 65, 255, 256, 257, 512 and 1 024:
empty, partly filled and full slot groups, sweeps while the source is still running and in the drain.  The unit's first
row is once a row that matches every join -- a slot that leaked would add to a count -- and once a row that matches none.

Sources: plain (streamed), a last unit of 700 tuples that ends at the columns' last row, a selection vector (whose last
entry is the table's last row), and validity columns on every join's column with NULLs at the safe row and elsewhere.
Banks: 4 joins and 3 joins on the K = 4 build; all bit tables in LDS, one perfect table too wide for LDS (a range of 2 M
values, 300 build rows) and one unique-key hash table between perfect stages.

Exact comparisons: per-position counters and the emitted row set against tests/joinref.py's Ref; the intermediates,
COUNT(*) and the row set against the oracle."""
import numpy as np
import pytest

import poolunits
from common import orc
from joinref import Join, Ref, chunks_for, device_rows, sort_rows
from polr_amd import capi
from test_gpu_engine_matrix import _perfect_join

pytestmark = pytest.mark.gpu

SMALL_POOL = dict(device_share=16, units_x=1)
UNIT = 1024
LEVELS = [0, 1, 63, 64, 65, 255, 256, 257, 512, 1024]
RANGES = [(-300, 699), (0, 499), (-1000, -1), (5, 1204)]
WIDE = (0, 2_000_000)  # 250 KB of bits: never in LDS


def _bank(rng, k, kind):
    """k joins, join c keyed by probe column c; `kind` replaces the join in the middle of the bank"""
    joins = [_perfect_join(rng, np.int32, lo, hi, hi - lo + 1, c) for c, (lo, hi) in enumerate(RANGES[:k])]
    mid = k // 2
    if kind == "hbm":
        keys = np.unique(np.concatenate([rng.integers(WIDE[0], WIDE[1] + 1, 300), [WIDE[0], WIDE[1]]])).astype(np.int32)
        joins[mid] = Join(rng.permutation(keys), mid, WIDE, None, [(keys % 7).astype(np.int16)])
    elif kind == "hash":
        keys = rng.choice(np.arange(0, 200_000, 2, dtype=np.int32), 400, replace=False)  # even; odd keys miss
        joins[mid] = Join(keys, mid, None, None, [np.arange(len(keys), dtype=np.int32)])
    return joins


def _keys(rng, j, hit):
    """a key column for join j: build keys where `hit`, else holes of its range and values outside it"""
    n = len(hit)
    if j.perfect is None:
        miss = (2 * rng.integers(0, 100_000, n) + 1)
    else:
        lo, hi = j.perfect
        holes = np.setdiff1d(np.arange(lo, hi + 1), j.keys.astype(np.int64))
        assert len(holes) > 10
        miss = np.where(rng.random(n) < 0.5, rng.choice(holes, n), rng.integers(hi + 1, hi + 5000, n))
    return np.where(hit, rng.choice(j.keys.astype(np.int64), n), miss).astype(np.int32)


def _hits(rng, k, n, level, safe):
    """hit[c][t]: does tuple t of the source match join c.  Join 0 (stage 0 of every order run here): exactly
    min(level, unit's tuples) hits per unit of 1024 tuples; the other joins: about 60 %.  The unit's first tuple matches
    every join (safe = "all") or none ("none") -- except that join 0 takes it where the level leaves no choice"""
    hit = [np.zeros(n, bool)] + [rng.random(n) < 0.6 for _ in range(1, k)]
    for lo in range(0, n, UNIT):
        hi = min(n, lo + UNIT)
        want = min(level, hi - lo)
        first = (safe == "all" and want > 0) or want == hi - lo
        hit[0][lo] = first
        hit[0][rng.choice(np.arange(lo + 1, hi), want - int(first), replace=False)] = True
        assert hit[0][lo:hi].sum() == want
        for c in range(1, k):
            hit[c][lo] = safe == "all"
    return hit


def _source(rng, joins, form, level, safe):
    """-> (probe columns, validity or None, selection or None, tuples of the source)"""
    k = len(joins)
    n = 2 * UNIT + 700 if form == "tail" else 3 * UNIT
    hit = _hits(rng, k, n, level, safe)
    cols = [_keys(rng, j, hit[c]) for c, j in enumerate(joins)]
    pvalid, sel = None, None
    if form == "valid":
        # NULL never matches: on join 0's column only where the key misses anyway (the level stays exact), on the others
        # at every unit's first row -- the safe row's KEY may match, the row never does -- and at a tenth of the rest
        pvalid = []
        for c in range(k):
            v = rng.random(n) > 0.1
            if c == 0:
                v |= hit[0]
            else:
                v[::UNIT] = False
            pvalid.append(v.astype(np.uint8))
    if form == "sel":
        # the source is a selection of a longer table; every other row of the table matches every join
        n_tab = n + 1500
        sel = np.sort(rng.choice(n_tab - 1, n - 1, replace=False))
        sel = np.concatenate([sel, [n_tab - 1]]).astype(np.uint32)
        full = [rng.choice(j.keys, n_tab).astype(np.int32) for j in joins]
        for c in range(k):
            full[c][sel] = cols[c]
        cols = full
    return cols, pvalid, sel, n


def _oracle(pcols, pvalid, sel, n, joins, order, ref, want):
    kw = {}
    if sel is not None:
        kw = dict(sel=sel, chunk_offsets=np.minimum(np.arange(0, n + UNIT, UNIT), n).astype(np.uint64))
    o = orc.run_pipeline(pcols, [j.oracle() for j in joins], [order], routing="default_path", probe_valid=pvalid, **kw)
    stage = ref.stage_counts(order)
    assert o["num_intermediates"] == sum(stage) and o["num_output_rows"] == stage[-1]
    assert np.array_equal(sort_rows(o["out_rows"]), want)


CASES = ([("k4-lds", f, s) for f in ("plain", "tail", "sel", "valid") for s in ("all", "none")] +
         [(b, f, s) for b in ("k3-lds", "k4-hbm", "k4-hash") for f in ("plain", "sel") for s in ("all", "none")] +
         [("k4-hbm", "valid", "all"), ("k4-hash", "valid", "all"), ("k3-lds", "tail", "none")])


@pytest.mark.parametrize("bank,form,safe", CASES, ids=["%s-%s-safe-%s" % c for c in CASES])
def test_sweep_fill_levels(gpu_ctx, bank, form, safe):
    k, kind = int(bank[1]), bank.split("-")[1]
    rng = np.random.default_rng(9000 + CASES.index((bank, form, safe)))
    joins = _bank(rng, k, kind)
    orders = [list(range(k)), [0] + list(range(k - 1, 0, -1))]  # join 0 first: the levels are stage 0's survivors
    flat_emit = kind != "hash"  # (an emitting run over a hash table takes the generic kernel)
    try:
        gpu_ctx.set_pool_tuning(**SMALL_POOL)
        ght = [j.device(gpu_ctx) for j in joins]
        if kind == "hash":
            assert ght[k // 2].info()["kind"] == 2
        for level in LEVELS:
            pcols, pvalid, sel, n = _source(rng, joins, form, level, safe)
            ref = Ref(pcols, pvalid, joins, sel)
            want = sort_rows(ref.rows())
            for lo in range(0, n, UNIT):  # the construction: stage 0's survivors of every unit
                rows = np.arange(lo, min(n, lo + UNIT)) if sel is None else sel[lo:lo + UNIT]
                assert ref.counts[0][rows].sum() == min(level, len(rows))
            for x, order in enumerate(orders):
                pipe = capi.Pipeline(gpu_ctx, pcols, ref.n, [(h, [(-1, j.src)]) for h, j in zip(ght, joins)],
                                     [order] + [o for o in orders if o != order], probe_valid=pvalid)
                if sel is not None:
                    pipe.set_selection(sel)
                li = pipe.launch_info(False)
                assert li["flat"] == 1 and li["compiled_stages"] == 4
                assert li["lds_tables"] == k - (kind != "lds")
                stage = ref.stage_counts(order)
                assert stage[0] == sum(min(level, min(n, lo + UNIT) - lo) for lo in range(0, n, UNIT))
                m = capi.DeviceMultiplexer(pipe, "default_path")
                for emit in (False, True):
                    out = capi.Output(pipe, 1024, chunks_for(len(want), 1024)) if emit else None
                    info = capi.pool_info([m], out)
                    assert info["flat"] == int(flat_emit or not emit)
                    if info["flat"]:
                        assert info["share"] == 16 and poolunits.unit_of(n, info) == UNIT, info
                    capi.run_resident([m], [(0, (n + 1023) // 1024)], out=out, reset=True, finish=True)
                    st = m.finish()
                    assert st["stage_out"][0] == stage, "level %d, order %s, emit %d" % (level, order, emit)
                    assert sum(st["input_tuple_count_per_path"]) == n
                    if emit:
                        n_rows, _, over = out.stats()
                        assert not over and n_rows == len(want)
                        assert np.array_equal(sort_rows(device_rows(out.fetch_ids(), joins)), want), \
                            "rows, level %d, order %s" % (level, order)
                        out.close()
                m.close()
                pipe.close()
                if x == 0:
                    _oracle(pcols, pvalid, sel, n, joins, order, ref, want)
        for h in ght:
            h.close()
    finally:
        gpu_ctx.set_pool_tuning()
