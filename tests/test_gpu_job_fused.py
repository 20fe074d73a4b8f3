"""The JOB family through the fused ungrouped sink (polr_amd.job_family.run_fused_device): SELECT COUNT(*), MIN(a), MIN(b), ...
in one pool launch -- the select columns as sorted dictionary codes of their build sides, MIN(code) folded inside the
generic kernel, the winning codes turned back into strings -- against the reference engine's own answers
(tests/golden/job_family.json) and, for the heavy fan-out shapes, against a numpy evaluation of the join tree."""
import numpy as np
import pytest

import common
from polr_amd import capi
from polr_amd import host as phost
from polr_amd import job_family as jf

pytestmark = pytest.mark.gpu

SHAPES = jf.shapes()


def _paths(wl):
    pn = list(wl["probe"]["cols"].keys())
    return phost.generate_join_orders("each_last_once", len(pn), [len(j["payload"]) for j in wl["joins"]],
                                      wl["cond_left_index"], [len(j["keys"][0]) for j in wl["joins"]], max_join_orders=8)[0]


def test_all_113_shapes_against_the_reference(gpu_ctx):
    """the 104 shapes whose select list lies on build sides return the reference's COUNT(*) and MIN strings, with no row id
    written; exactly 9 shapes name a probe-side VARCHAR column and are left to the materialising route"""
    gold = common.load_golden("job_family")
    t = jf.Tables(scale=gold["scale"])
    left_out, with_min = [], 0
    for name in sorted(SHAPES):
        g = gold["queries"][name]
        wl = jf.workload(name, t, SHAPES[name])
        if not jf.fused_select_on_build_sides(wl):
            left_out.append(name)
            assert any(sj < 0 for sj, _c in wl["select"]), name
            continue
        res = jf.run_fused_device(gpu_ctx, wl, _paths(wl))
        assert res["count_star"] == g["count_star"], name
        assert [None if m is None else m.decode() for m in res["select_min"]] == g["select_min"], (name, res["select_min"])
        assert res["rows_written"] == 0, name
        with_min += any(m is not None for m in res["select_min"])
    assert len(left_out) == 9 and len(SHAPES) - len(left_out) == 104, left_out
    # 57 of the 113 shapes have a non-NULL MIN at this scale; 52 of them are among the 104 that ran here
    assert sum(any(m is not None for m in g["select_min"]) for g in gold["queries"].values()) == 57 and with_min == 52


def tree_reference(wl):
    """COUNT(*) and, per select column, the smallest string among the build rows that take part in the result, by numpy
    over the join TREE (a join is keyed by a probe column or by a column of an earlier join): bottom-up the number of
    result tuples below every build row, top-down which rows are reached from a surviving probe row"""
    joins = wl["joins"]
    k = len(joins)
    pcols = list(wl["probe"]["cols"].values())
    children = {j: [] for j in range(-1, k)}
    for j, jn in enumerate(joins):
        children[jn["key_src"][0][0]].append(j)

    def src_col(j):
        sj, sc = joins[j]["key_src"][0]
        return pcols[sc] if sj < 0 else list(joins[sj]["payload"].values())[sc]

    below = {}  # per join: result tuples of its subtree per build row (far inside 64 bits at these scales)
    for j in range(k - 1, -1, -1):
        w = np.ones(len(joins[j]["keys"][0]), dtype=np.int64)
        for c in children[j]:
            w = w * match_weight(src_col(c), joins[c]["keys"][0], below[c])
        below[j] = w
    n = len(pcols[0])
    live = np.zeros(n, bool)
    sel = wl["probe"].get("filter_sel")
    live[sel if sel is not None else slice(None)] = True
    wp = live.astype(np.int64)
    for c in children[-1]:
        wp = wp * match_weight(src_col(c), joins[c]["keys"][0], below[c])
    count = int(wp.sum())
    reached = {-1: wp != 0}
    for j in range(k):
        sj = joins[j]["key_src"][0][0]
        parent_vals = np.unique(src_col(j)[reached[sj]])
        reached[j] = (below[j] != 0) & np.isin(joins[j]["keys"][0], parent_vals)
    mins = []
    for sj, col in wl["select"]:
        vals = [s for s, r in zip(joins[sj]["strings"][col], reached[sj].tolist()) if r]
        mins.append(min(vals) if vals else None)
    return count, mins


def match_weight(src, keys, weight):
    """per source row: the summed weight of the build rows whose key equals the row's value"""
    uk, inv = np.unique(keys, return_inverse=True)
    sums = np.zeros(len(uk), dtype=np.int64)
    np.add.at(sums, inv, weight)
    pos = np.searchsorted(uk, src)
    pos[pos == len(uk)] = 0
    hit = uk[pos] == src if len(uk) else np.zeros(len(src), bool)
    out = np.zeros(len(src), dtype=np.int64)
    out[hit] = sums[pos[hit]]
    return out


_HEAVY = {}


@pytest.mark.parametrize("share_after", [16, 0xFFFFFFFF], ids=["share16", "off"])
def test_heavy_fanout_shapes_with_work_sharing(gpu_ctx, share_after):
    """the JOB shapes whose fan-out joins multiply (25c, 17e, 31a, 19c) at scale 0.05, with work sharing after 16 steps and
    with sharing off: whatever was cut and handed to other waves, COUNT(*) and the MINs are the join tree's"""
    for name in ("25c", "17e", "31a", "19c"):
        if name not in _HEAVY:  # (the workload and its reference once, shared by the two cases and left unchanged)
            wl = jf.workload(name, _HEAVY.setdefault("tables", jf.Tables(scale=0.05)), SHAPES[name])
            _HEAVY[name] = (wl, tree_reference(wl))
        wl, (want_count, want_mins) = _HEAVY[name]
        assert jf.fused_select_on_build_sides(wl), name
        assert (want_count > 0) == (name != "19c")  # (19c's filters leave no result row at this scale: COUNT(*) 0, MINs NULL)
        try:
            gpu_ctx.set_pool_tuning(share_after=share_after)
            res = jf.run_fused_device(gpu_ctx, wl, _paths(wl))
        finally:
            gpu_ctx.set_pool_tuning()
        assert res["count_star"] == want_count, name
        assert res["select_min"] == want_mins and res["rows_written"] == 0, name
