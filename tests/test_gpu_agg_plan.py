"""The aggregate sinks of the library follow their host plan (duckdb-polr_amd/csrc/polr_agg_plan.h): for a dozen refusing
requests across polr_out_aggregate, _aggregate_expr, _aggregate_grouped, _aggregate_hashed_str, _fuse_grouped and
_fuse_aggregate the return code and polr_last_error are what the stand-alone plan program (tests/aggplan/agg_plan_main.cpp,
built here as tests/test_agg_plan.py builds it) answers for the request as described, no device memory stays behind, and a
refused polr_out_fuse_grouped leaves the output usable; one accepted request per family is checked against exact Python over
the row ids.  8 probe rows, one join against a 4-row perfect build side, an output of one chunk: every refusal under test
occurs before any launch, so no larger shape can show more."""
import ctypes as C

import numpy as np
import pytest

from joinref import MAX_WAVE_CHUNKS
from polr_amd import capi
from test_agg_plan import (AGG_CELLS, ALREADY, COUNT, COUNT_STAR, MAX, MIN, MUL, SIGNED, SUM, agg, build, col, expr, key, parse, plan,
                           run, write_requests)

pytestmark = pytest.mark.gpu

PROBE = [np.array([0, 1, 2, 3, 3, 2, 9, 0], np.int32),             # the join key (9: no partner)
         np.array([5, -7, 300, -300, 11, 12, 13, 14], np.int16),
         np.arange(8, dtype=np.uint64),                            # unsigned 8-byte: no sink reads it
         capi.string_cells(["a", "bb", "a", "", "bb", "a", "x", "a"])[0]]
BUILD = [np.array([0, 1, 0, 2], np.int32),                         # a group column: domain [0, 2]
         np.array([2 ** 40, -(2 ** 40), 7, -1], np.int64),
         capi.string_cells(["de", "fr", "de", "it"])[0]]


def describe(src_join, src_col):
    """the column as the library describes it to the plan"""
    cols = PROBE if src_join < 0 else (BUILD if src_join == 0 else [])
    if src_col >= len(cols):
        return col(0, 0, 0)
    return col(1, cols[src_col].dtype.itemsize, SIGNED if cols[src_col].dtype.kind == "i" else 0)


def d_agg(fn, src_join, src_col):
    return agg(fn, src_join, src_col, describe(src_join, src_col))


def d_expr(fn, op, left, right, dtype):
    dt = np.dtype(dtype)
    return expr(fn, op, describe(*left), describe(*right), dt.itemsize, SIGNED if dt.kind == "i" else 0, left + right)


def d_key(src_join, src_col, n_values=0):
    return key(n_values, src_join, src_col, describe(src_join, src_col))


@pytest.fixture(scope="module")
def star(gpu_ctx):
    ht = capi.HashTable.from_columns(gpu_ctx, [np.arange(4, dtype=np.int32)], BUILD)
    assert ht.finalize_perfect(0, 3)
    pipe = capi.Pipeline(gpu_ctx, PROBE, 8, [(ht, [(-1, 0)])], [[0]])
    out = capi.Output(pipe, 64, 1 + MAX_WAVE_CHUNKS)  # (one partially filled chunk per emitting wave)
    mpx = capi.DeviceMultiplexer(pipe, "default_path")

    def fill():
        out.reset()
        capi.run_resident([mpx], [(0, 1)], out=out, reset=True, finish=True)
        mpx.finish()

    fill()
    yield pipe, out, fill
    mpx.close()
    out.close()
    pipe.close()
    ht.close()


def test_the_sinks_answer_as_their_plan(gpu_ctx, star, tmp_path):
    pipe, out, fill = star
    L = gpu_ctx.L
    assert pipe.launch_info(True)["flat"] == 1  # (a perfect table: emitting runs take the flat kernel)
    ids = out.fetch_ids().astype(np.int64)
    assert sorted(ids[:, 0].tolist()) == [0, 1, 2, 3, 4, 5, 7]
    res = (capi.AggValue * 64)()
    gkeys, gnulls = np.zeros(64, np.int64), np.zeros(16, np.uint32)
    n_g, used, oor, dropped = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    arena = np.zeros(256, np.uint8)

    def ungrouped(specs):
        return lambda: L.polr_out_aggregate(out.h, None, capi._agg_specs(specs), len(specs), res)

    def ungrouped_expr(specs):
        return lambda: L.polr_out_aggregate_expr(out.h, None, capi.make_agg_exprs(specs), len(specs), res, C.byref(oor))

    def grouped(keys, specs, n_groups):
        return lambda: L.polr_out_aggregate_grouped(out.h, None, capi._group_keys(keys)[0], len(keys), capi._agg_specs(specs),
                                                    len(specs), res, n_groups, C.byref(dropped))

    def hashed_str(cols, specs, max_groups):
        return lambda: L.polr_out_aggregate_hashed_str(out.h, None, capi._group_keys(cols)[0], len(cols), capi._agg_specs(specs),
                                                       len(specs), max_groups, gkeys.ctypes.data, gnulls.ctypes.data, res,
                                                       C.byref(n_g), arena.ctypes.data, 256, C.byref(used))

    def fuse_grouped(keys, specs):
        return lambda: L.polr_out_fuse_grouped(out.h, capi._group_keys(keys)[0], len(keys), capi._agg_specs(specs), len(specs))

    def fuse_aggregate(specs):
        return lambda: L.polr_out_fuse_aggregate(out.h, capi._agg_specs(specs), len(specs))

    one = [d_agg(SUM, -1, 1)]
    sum1 = [("sum", -1, 1)]
    # name -> (the request as described to the plan program, the call)
    refusing = {
        "u_probe_col_beyond": (plan("ungrouped", aggs=[d_agg(COUNT_STAR, -1, 99), d_agg(SUM, -1, 9)]),
                               ungrouped([("count_star", -1, 99), ("sum", -1, 9)])),
        "u_16_byte_cells": (plan("ungrouped", aggs=[d_agg(MIN, -1, 3)]), ungrouped([("min", -1, 3)])),
        "x_build_col_beyond": (plan("ungrouped", aggs=[d_expr(SUM, MUL, (-1, 1), (0, 7), np.int64)]),
                               ungrouped_expr([("sum", "*", (-1, 1), (0, 7), np.int64)])),
        "x_result_cannot_hold": (plan("ungrouped", aggs=[d_expr(SUM, MUL, (-1, 1), (0, 1), np.int32)]),
                                 ungrouped_expr([("sum", "*", (-1, 1), (0, 1), np.int32)])),
        "g_empty_domain": (plan("grouped", keys=[d_key(0, 0, 3), d_key(-1, 1, 0)], aggs=one),
                           grouped([(0, 0, 0, 3), (-1, 1, 0, 0)], sum1, 0)),
        "g_above_2_20": (plan("grouped", keys=[d_key(0, 0, 1024), d_key(-1, 1, 1025)], aggs=one, n_groups=1024 * 1025),
                         grouped([(0, 0, 0, 1024), (-1, 1, 0, 1025)], sum1, 1024 * 1025)),
        "g_mismatch": (plan("grouped", keys=[d_key(0, 0, 3)], aggs=one, n_groups=4), grouped([(0, 0, 0, 3)], sum1, 4)),
        "h_above_2_24": (plan("hashed", keys=[d_key(0, 2)], aggs=one, strings=1, str_cap=256, max_groups=2 ** 24 + 1),
                         hashed_str([(0, 2)], sum1, 2 ** 24 + 1)),
        "h_unsigned_8": (plan("hashed", keys=[d_key(0, 2), d_key(-1, 2)], aggs=one, strings=1, str_cap=256, max_groups=16),
                         hashed_str([(0, 2), (-1, 2)], sum1, 16)),
        "f_sum_8_bytes": (plan("fuse", keys=[d_key(0, 0, 3)], aggs=[d_agg(COUNT, 0, 1), d_agg(SUM, 0, 1)]),
                          fuse_grouped([(0, 0, 0, 3)], [("count", 0, 1), ("sum", 0, 1)])),
        "f_min": (plan("fuse", keys=[d_key(0, 0, 3)], aggs=[d_agg(MIN, -1, 1)]), fuse_grouped([(0, 0, 0, 3)], [("min", -1, 1)])),
        "f_4097_groups": (plan("fuse", keys=[d_key(0, 0, 3), d_key(-1, 1, 1366)], aggs=one),
                          fuse_grouped([(0, 0, 0, 3), (-1, 1, 0, 1366)], sum1)),
    }
    # ... and with a fused sink attached (below): a second one, and a row-id sink over aggregate cells
    attached = {
        "second_sink_behind_grouped": (plan("fuse", keys=[d_key(0, 0, 3)], aggs=one, already_fused=1), fuse_grouped([(0, 0, 0, 3)], sum1)),
        "second_sink_behind_ungrouped": (plan("fuse", keys=[d_key(0, 0, 3)], aggs=one, already_fused=1, agg_cells=1),
                                         fuse_grouped([(0, 0, 0, 3)], sum1)),
        "row_ids_wanted_of_cells": (plan("ungrouped", aggs=one, agg_cells=1), ungrouped(sum1)),
    }
    path = str(tmp_path / "requests.txt")
    # (polr_out_fuse_aggregate's per-aggregate step is the argument rule alone)
    args = {"a_build_col_beyond": (1, d_agg(MAX, 3, 0), None, None, None)}
    write_requests(path, {n: r for n, (r, _call) in dict(refusing, **attached).items()}, args, {})
    want = parse(run(build(tmp_path, None), path))
    assert all(w["code"] != 0 and w["message"] for w in (want[n] for n in list(refusing) + list(attached) + list(args)))
    assert want["second_sink_behind_ungrouped"]["message"] == ALREADY and want["row_ids_wanted_of_cells"]["message"] == AGG_CELLS

    def check_refused(name, call):
        live = capi.device_bytes_live()
        rc = call()
        assert (rc, L.polr_last_error(gpu_ctx.h).decode()) == (want[name]["code"], want[name]["message"]), name
        assert capi.device_bytes_live() == live, name

    for name, (_r, call) in refusing.items():
        check_refused(name, call)
    check_refused("a_build_col_beyond", fuse_aggregate([("count_star", 0, 0), ("max", 3, 0)]))
    # the refused polr_out_fuse_grouped calls left the output as it was: its row ids, and a row-id run into it
    assert np.array_equal(out.fetch_ids(), ids.astype(np.uint32))
    fill()
    ids = out.fetch_ids().astype(np.int64)
    assert sorted(ids[:, 0].tolist()) == [0, 1, 2, 3, 4, 5, 7]

    # ---- one accepted request per family, against exact Python over the row ids
    p1 = [int(x) for x in PROBE[1][ids[:, 0]]]
    b0 = [int(x) for x in BUILD[0][ids[:, 1]]]
    b1 = [int(x) for x in BUILD[1][ids[:, 1]]]
    names = [bytes(BUILD[2][i].tobytes()[4:6]) for i in ids[:, 1]]
    assert out.aggregate([("count_star", -1, 0), ("sum", -1, 1), ("min", 0, 1), ("max", 0, 1)]) == [7, sum(p1), min(b1), max(b1)]
    prod = [x * y for x, y in zip(p1, b1)]
    assert out.aggregate_expr([("sum", "*", (-1, 1), (0, 1), np.int64), ("min", "*", (-1, 1), (0, 1), np.int64)]) == [sum(prod), min(prod)]
    vals, counts, n_dropped = out.aggregate_grouped([(0, 0, 0, 3)], [("count_star", -1, 0), ("sum", -1, 1)])
    by_group = [[x for x, g in zip(p1, b0) if g == q] for q in range(3)]
    assert n_dropped == 0 and vals == [[len(v), sum(v) if v else None] for v in by_group]
    got = out.aggregate_hashed_str([(0, 2), (0, 0)], [("count", -1, 1), ("max", -1, 1)], 16)
    groups = sorted(set(zip(names, b0)))
    assert got == {(s, g): [len(v), max(v)] for (s, g) in groups for v in [[x for x, n2, g2 in zip(p1, names, b0) if (n2, g2) == (s, g)]]}
    out.fuse_grouped([(0, 0, 0, 3)], [("count_star", -1, 0), ("sum", -1, 1)])
    check_refused("second_sink_behind_grouped", attached["second_sink_behind_grouped"][1])
    fill()
    fvals, _counts, n_dropped = out.fused_result()
    assert n_dropped == 0 and fvals == [[len(v), sum(v) if v else None] for v in by_group]
    out.fuse_grouped(None, None)
    out.fuse_aggregate([("count_star", -1, 0), ("sum", 0, 1), ("min", -1, 1)])
    for name in ("second_sink_behind_ungrouped", "row_ids_wanted_of_cells"):
        check_refused(name, attached[name][1])
    fill()
    assert out.fused_aggregate_result() == [7, sum(b1), min(p1)]
    out.fuse_aggregate(None)
    fill()  # (for whoever shares the fixture: row ids again)
