"""The host-side plan of the aggregate sinks (duckdb-polr_amd/csrc/polr_agg_plan.h), the part that needs no GPU: the header
alone behind a stand-alone host program (tests/aggplan/agg_plan_main.cpp).  Per entry-point family every head refusal with
its code and whole message -- the literals below are transcribed from polr_agg.hip as it stood before the plan existed --,
alone and in pairs (the earlier one wins); the argument rule in its column and its expression form; the group-domain rule of
the perfect-hash and of the fused sink at their limits; the hashed sink's group columns and string mask; the hashed sink's
allocation against the expression it replaces; and the decode.  Built plain and with the address + undefined-behaviour
sanitizers, and run directly."""
import os
import subprocess

import pytest

import common

SRC = os.path.join(common.ROOT, "tests", "aggplan", "agg_plan_main.cpp")
OK, INVALID, UNSUPPORTED = 0, -2, -3
COUNT_STAR, COUNT, SUM, MIN, MAX = range(5)
COLUMN, ADD, SUB, MUL = range(4)
SIGNED = 1  # POLR_COL_SIGNED
M64 = (1 << 64) - 1
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1

AGG_CELLS = "the output has a fused aggregate sink: it holds aggregate cells, no row ids (polr_out_fused_aggregate_result)"
COL_RULE = "only integer columns of up to 8 bytes (signed if 8)"
UNGROUPED_COUNT = "at most 8 aggregates per call"
GROUPED_COUNT = "at most 3 group columns and 8 aggregates"
HASHED_COUNT = "at most 3 group columns, 8 aggregates and 2^24 groups"
FUSE_COUNT = "1..3 group columns and 1..8 aggregates"
FUSE_NOT_FLAT = ("a GROUP BY sink is fused into FLAT pipelines whose joins are all perfect tables (polr_pipeline_launch_info); "
                 "others: polr_out_aggregate_grouped over the emitted row ids")
ALREADY = "the output object already has a fused sink"
FUSE_4096 = "group column %d: a fused sink holds at most 4096 groups"
FUSE_FN = "aggregate %d: a fused sink computes COUNT(*), COUNT and SUM"
FUSE_SUM = "aggregate %d: a fused SUM takes columns of at most 4 bytes"
EMPTY = "group column %d: empty domain"
TOO_MANY = "more than 2^20 groups: not a perfect-hash aggregate"
MISMATCH = "results hold %d groups, the domains span %d"


def col(in_range=1, width=4, flags=SIGNED):
    return (in_range, width, flags)


def agg(fn=SUM, src_join=-1, src_col=0, c=col()):
    """the column form"""
    return (fn, COLUMN, src_join, src_col, 0, 0, 0, 0) + c + col(0, 0, 0)


def expr(fn, op, left=col(), right=col(), rw=8, rflags=SIGNED, src=(-1, 0, 0, 1)):
    return (fn, op, src[0], src[1], src[2], src[3], rw, rflags) + left + right


def key(n_values=4, src_join=0, src_col=0, c=col()):
    return (src_join, src_col, n_values) + c


def plan(family, code=OK, message="", keys=(key(),), aggs=(agg(),), **kw):
    keys, aggs = list(keys), list(aggs)
    groups = 1
    for k in keys:
        groups *= k[2]
    r = dict(family=family, code=code, message=message, keys=keys, aggs=aggs, has_out=1, has_keys=1, has_specs=1, has_results=1,
             has_group_outputs=1, agg_cells=0, n_keys=len(keys), n_aggs=len(aggs), n_groups=groups, max_groups=16, strings=0,
             has_str_used=1, has_str_bytes=1, str_cap=0, flat_emit=1, already_fused=0)
    assert set(kw) <= set(r), kw
    r.update(kw)
    return r


HEAD_FIELDS = ("has_out", "has_keys", "has_specs", "has_results", "has_group_outputs", "agg_cells", "n_keys", "n_aggs", "n_groups",
               "max_groups", "strings", "has_str_used", "has_str_bytes", "str_cap", "flat_emit", "already_fused")


def head_cases():
    c = {}
    # ---- polr_out_aggregate(_expr)
    c["u_ok"] = plan("ungrouped", aggs=[agg(COUNT_STAR), agg(MIN, 0, 1), agg(MAX)])
    for f in ("has_out", "has_specs", "has_results"):
        c["u_null_" + f] = plan("ungrouped", INVALID, "", **{f: 0})
    c["u_no_aggs"] = plan("ungrouped", INVALID, "", aggs=[])
    c["u_agg_cells"] = plan("ungrouped", INVALID, AGG_CELLS, agg_cells=1)
    c["u_nine"] = plan("ungrouped", UNSUPPORTED, UNGROUPED_COUNT, aggs=[], n_aggs=9)  # (no aggregate is looked at)
    c["u_eight"] = plan("ungrouped", aggs=[agg()] * 8)
    c["u_bad_agg"] = plan("ungrouped", INVALID, "aggregate 1: unknown function 5", aggs=[agg(), agg(5)])
    c["u_order_null_before_cells"] = plan("ungrouped", INVALID, "", has_results=0, agg_cells=1, aggs=[], n_aggs=9)
    c["u_order_cells_before_count"] = plan("ungrouped", INVALID, AGG_CELLS, agg_cells=1, aggs=[], n_aggs=9)
    c["u_order_count_before_aggs"] = plan("ungrouped", UNSUPPORTED, UNGROUPED_COUNT, aggs=[], n_aggs=9)
    c["u_order_first_agg_first"] = plan("ungrouped", UNSUPPORTED, "aggregate 0: " + COL_RULE, aggs=[agg(c=col(1, 16, 0)), agg(7)])
    # ---- polr_out_aggregate_grouped(_expr)
    c["g_ok"] = plan("grouped", keys=[key(7), key(25, -1, 2)])
    for f in ("has_out", "has_keys", "has_specs", "has_results"):
        c["g_null_" + f] = plan("grouped", INVALID, "", **{f: 0})
    c["g_no_keys"] = plan("grouped", INVALID, "", keys=[])
    c["g_no_aggs"] = plan("grouped", INVALID, "", aggs=[])
    c["g_agg_cells"] = plan("grouped", INVALID, AGG_CELLS, agg_cells=1)
    c["g_four_keys"] = plan("grouped", UNSUPPORTED, GROUPED_COUNT, keys=[], n_keys=4, n_groups=1)
    c["g_nine_aggs"] = plan("grouped", UNSUPPORTED, GROUPED_COUNT, aggs=[], n_aggs=9)
    c["g_order_null_before_cells"] = plan("grouped", INVALID, "", has_keys=0, agg_cells=1)
    c["g_order_cells_before_count"] = plan("grouped", INVALID, AGG_CELLS, agg_cells=1, keys=[], n_keys=4, n_groups=1)
    c["g_order_count_before_columns"] = plan("grouped", UNSUPPORTED, GROUPED_COUNT, keys=[key(c=col(0))], aggs=[], n_aggs=9)
    c["g_order_columns_before_mismatch"] = plan("grouped", INVALID, EMPTY % 1, keys=[key(2), key(0)], n_groups=99)
    c["g_order_mismatch_before_aggs"] = plan("grouped", INVALID, MISMATCH % (99, 8), keys=[key(2), key(4)], n_groups=99,
                                             aggs=[agg(5)])
    c["g_order_aggs_last"] = plan("grouped", INVALID, "aggregate 0: unknown function 5", aggs=[agg(5)])
    # ---- polr_out_aggregate_hashed(_str, _expr)
    c["h_ok"] = plan("hashed")
    for f in ("has_out", "has_keys", "has_specs", "has_group_outputs", "has_results"):
        c["h_null_" + f] = plan("hashed", INVALID, "", **{f: 0})
    c["h_no_keys"] = plan("hashed", INVALID, "", keys=[])
    c["h_no_aggs"] = plan("hashed", INVALID, "", aggs=[])
    c["h_max_groups_0"] = plan("hashed", INVALID, "", max_groups=0)
    c["h_max_groups_2_24"] = plan("hashed", max_groups=2 ** 24)
    c["h_max_groups_above"] = plan("hashed", UNSUPPORTED, HASHED_COUNT, max_groups=2 ** 24 + 1)
    c["h_str_no_used"] = plan("hashed", INVALID, "", strings=1, has_str_used=0)
    c["h_str_no_bytes_with_cap"] = plan("hashed", INVALID, "", strings=1, has_str_bytes=0, str_cap=8)
    c["h_str_no_bytes_no_cap"] = plan("hashed", strings=1, has_str_bytes=0, str_cap=0)
    c["h_no_strings_ignores_str_args"] = plan("hashed", strings=0, has_str_used=0, has_str_bytes=0, str_cap=8)
    c["h_agg_cells"] = plan("hashed", INVALID, AGG_CELLS, agg_cells=1)
    c["h_four_keys"] = plan("hashed", UNSUPPORTED, HASHED_COUNT, keys=[], n_keys=4)
    c["h_nine_aggs"] = plan("hashed", UNSUPPORTED, HASHED_COUNT, aggs=[], n_aggs=9)
    c["h_order_null_before_cells"] = plan("hashed", INVALID, "", max_groups=0, agg_cells=1)
    c["h_order_cells_before_count"] = plan("hashed", INVALID, AGG_CELLS, agg_cells=1, max_groups=2 ** 24 + 1)
    c["h_order_count_before_columns"] = plan("hashed", UNSUPPORTED, HASHED_COUNT, keys=[key(c=col(0))], max_groups=2 ** 24 + 1)
    c["h_order_columns_before_aggs"] = plan("hashed", INVALID, "group column 0: build column (0,0) out of range",
                                            keys=[key(c=col(0))], aggs=[agg(5)])
    # group columns: any integer column; a 16-byte column where the call allows strings; the string mask
    c["h_key_varchar_allowed"] = plan("hashed", strings=1, keys=[key(c=col(1, 16, 0))])
    c["h_key_varchar_not_allowed"] = plan("hashed", UNSUPPORTED, "group column 0: " + COL_RULE, strings=0, keys=[key(c=col(1, 16, 0))])
    c["h_key_mixed"] = plan("hashed", strings=1, keys=[key(c=col(1, 16, 0)), key(c=col(1, 8, SIGNED)), key(0, -1, 1, col(1, 16, 0))])
    c["h_key_unsigned_8"] = plan("hashed", UNSUPPORTED, "group column 1: " + COL_RULE, strings=1,
                                 keys=[key(c=col(1, 16, 0)), key(c=col(1, 8, 0))])
    c["h_key_probe_out_of_range"] = plan("hashed", INVALID, "group column 1: probe column 9 out of range", strings=1,
                                         keys=[key(), key(4, -1, 9, col(0, 16, 0))])
    # ---- polr_out_fuse_grouped
    c["f_ok"] = plan("fuse", aggs=[agg(COUNT_STAR), agg(COUNT), agg(SUM)])
    c["f_null_out"] = plan("fuse", INVALID, "", has_out=0)
    # un-fuse is never refused, except for a NULL output
    c["f_unfuse_null_keys"] = plan("fuse", has_keys=0, has_specs=0, n_aggs=9, aggs=[], flat_emit=0, already_fused=1, agg_cells=1)
    c["f_unfuse_no_keys"] = plan("fuse", keys=[], aggs=[], flat_emit=0, already_fused=1)
    c["f_unfuse_null_out"] = plan("fuse", INVALID, "", has_out=0, has_keys=0)
    c["f_null_specs"] = plan("fuse", INVALID, FUSE_COUNT, has_specs=0)
    c["f_no_aggs"] = plan("fuse", INVALID, FUSE_COUNT, aggs=[])              # INVALID, where the row-id sinks say UNSUPPORTED
    c["f_nine_aggs"] = plan("fuse", INVALID, FUSE_COUNT, aggs=[], n_aggs=9)
    c["f_four_keys"] = plan("fuse", INVALID, FUSE_COUNT, keys=[], n_keys=4)
    c["f_not_flat"] = plan("fuse", UNSUPPORTED, FUSE_NOT_FLAT, flat_emit=0)
    c["f_already"] = plan("fuse", INVALID, ALREADY, already_fused=1)
    c["f_fn_min"] = plan("fuse", UNSUPPORTED, FUSE_FN % 0, aggs=[agg(MIN)])
    c["f_fn_7"] = plan("fuse", UNSUPPORTED, FUSE_FN % 1, aggs=[agg(), agg(7)])  # (before "unknown function")
    c["f_sum_8_bytes"] = plan("fuse", UNSUPPORTED, FUSE_SUM % 0, aggs=[agg(SUM, c=col(1, 8, SIGNED))])
    c["f_count_8_bytes"] = plan("fuse", aggs=[agg(COUNT, c=col(1, 8, SIGNED))])
    c["f_order_count_before_flat"] = plan("fuse", INVALID, FUSE_COUNT, aggs=[], n_aggs=9, flat_emit=0)
    c["f_order_flat_before_already"] = plan("fuse", UNSUPPORTED, FUSE_NOT_FLAT, flat_emit=0, already_fused=1)
    c["f_order_already_before_columns"] = plan("fuse", INVALID, ALREADY, already_fused=1, keys=[key(0)])
    c["f_order_columns_before_aggs"] = plan("fuse", UNSUPPORTED, FUSE_4096 % 0, keys=[key(0)], aggs=[agg(MIN)])
    c["f_order_fn_before_column"] = plan("fuse", UNSUPPORTED, FUSE_FN % 0, aggs=[agg(MAX, -1, 9, col(0))])
    c["f_order_column_before_sum"] = plan("fuse", UNSUPPORTED, "aggregate 0: " + COL_RULE, aggs=[agg(SUM, c=col(1, 16, 0))])
    return c


def domain_cases():
    c = {}
    # the perfect-hash sink: 2^20 groups
    c["g_2_20"] = plan("grouped", keys=[key(1024), key(1024)])
    c["g_2_20_plus_1"] = plan("grouped", UNSUPPORTED, TOO_MANY, keys=[key(2 ** 20 + 1)])
    c["g_2_20_times_2"] = plan("grouped", UNSUPPORTED, TOO_MANY, keys=[key(1024), key(1024), key(2)])
    c["g_empty"] = plan("grouped", INVALID, EMPTY % 0, keys=[key(0)])
    c["g_empty_behind"] = plan("grouped", INVALID, EMPTY % 2, keys=[key(3), key(3), key(0)])
    c["g_mismatch"] = plan("grouped", INVALID, MISMATCH % (34, 35), keys=[key(7), key(5)], n_groups=34)
    c["g_key_varchar"] = plan("grouped", UNSUPPORTED, "group column 0: " + COL_RULE, keys=[key(c=col(1, 16, 0))])
    c["g_key_out_of_range"] = plan("grouped", INVALID, "group column 1: build column (2,7) out of range",
                                   keys=[key(), key(4, 2, 7, col(0))])
    # three columns of 2^31 values: the product would wrap 64 bits if multiplied blindly (2^93); refused at the column
    # where the limit is first passed
    c["g_wrap"] = plan("grouped", UNSUPPORTED, TOO_MANY, keys=[key(2 ** 31)] * 3, n_groups=0)
    c["g_wrap_second"] = plan("grouped", UNSUPPORTED, TOO_MANY, keys=[key(2 ** 20), key(2 ** 32 - 1), key(2 ** 32 - 1)], n_groups=0)
    # the fused sink: 4096 groups, one code and text for an empty domain and for too many
    c["f_4096"] = plan("fuse", keys=[key(64), key(64)])
    c["f_4097"] = plan("fuse", UNSUPPORTED, FUSE_4096 % 0, keys=[key(4097)])
    c["f_4096_times_2"] = plan("fuse", UNSUPPORTED, FUSE_4096 % 2, keys=[key(64), key(64), key(2)])
    c["f_empty"] = plan("fuse", UNSUPPORTED, FUSE_4096 % 1, keys=[key(3), key(0)])
    c["f_wrap"] = plan("fuse", UNSUPPORTED, FUSE_4096 % 0, keys=[key(2 ** 31)] * 3)
    c["f_wrap_second"] = plan("fuse", UNSUPPORTED, FUSE_4096 % 1, keys=[key(4096), key(2 ** 32 - 1), key(2 ** 32 - 1)])
    c["f_key_varchar"] = plan("fuse", UNSUPPORTED, "group column 0: " + COL_RULE, keys=[key(c=col(1, 16, 0))])
    return c


I8, I16, I32, I64 = col(1, 1, SIGNED), col(1, 2, SIGNED), col(1, 4, SIGNED), col(1, 8, SIGNED)
U8, U16, U32, U64 = col(1, 1, 0), col(1, 2, 0), col(1, 4, 0), col(1, 8, 0)
CANNOT_HOLD = "aggregate %d: a %ssigned %d-byte result cannot hold every value of its %s operand (%ssigned, %d bytes)"


def arg_cases():
    """name -> (index, arg, code, message, accepted (fn, op, lo, hi) or None)"""
    c = {}
    # the column form
    c["col_ok"] = (0, agg(SUM), OK, "", (SUM, COLUMN, 0, 0))
    c["col_unknown_fn"] = (3, agg(5), INVALID, "aggregate 3: unknown function 5", None)
    c["col_count_star_ignores_its_column"] = (0, agg(COUNT_STAR, 5, 99, col(0, 16, 0)), OK, "", (COUNT_STAR, COLUMN, 0, 0))
    c["col_probe_out_of_range"] = (1, agg(MIN, -1, 7, col(0)), INVALID, "aggregate 1: probe column 7 out of range", None)
    c["col_build_out_of_range"] = (2, agg(MAX, 2, 9, col(0)), INVALID, "aggregate 2: build column (2,9) out of range", None)
    c["col_16_bytes"] = (0, agg(MIN, c=col(1, 16, 0)), UNSUPPORTED, "aggregate 0: " + COL_RULE, None)
    c["col_unsigned_8"] = (7, agg(SUM, c=U64), UNSUPPORTED, "aggregate 7: " + COL_RULE, None)
    c["col_signed_8"] = (0, agg(SUM, c=I64), OK, "", (SUM, COLUMN, 0, 0))
    c["col_fn_before_column"] = (0, agg(6, -1, 3, col(0, 16, 0)), INVALID, "aggregate 0: unknown function 6", None)
    c["col_range_before_type"] = (0, agg(SUM, -1, 3, col(0, 16, 0)), INVALID, "aggregate 0: probe column 3 out of range", None)
    # the expression form
    c["expr_ok"] = (0, expr(SUM, MUL, I32, I32, 8, SIGNED), OK, "", (SUM, MUL, I64_MIN, I64_MAX))
    c["expr_column_op_ignores_result"] = (0, expr(SUM, COLUMN, I32, col(0, 16, 0), 3, 0), OK, "", (SUM, COLUMN, 0, 0))
    c["expr_count_star_ignores_all"] = (0, expr(COUNT_STAR, 9, col(0), col(0), 3, 0), OK, "", (COUNT_STAR, COLUMN, 0, 0))
    c["expr_unknown_fn"] = (0, expr(5, 9), INVALID, "aggregate 0: unknown function 5", None)
    c["expr_unknown_op"] = (1, expr(SUM, 4), INVALID, "aggregate 1: unknown operator 4", None)
    c["expr_left_out_of_range"] = (0, expr(SUM, ADD, col(0), col(0), src=(-1, 5, 1, 6)), INVALID,
                                   "aggregate 0: probe column 5 out of range", None)
    c["expr_right_out_of_range"] = (0, expr(SUM, ADD, I32, col(0), src=(-1, 0, 1, 6)), INVALID,
                                    "aggregate 0: build column (1,6) out of range", None)
    c["expr_right_varchar"] = (0, expr(SUM, SUB, I32, col(1, 16, 0)), UNSUPPORTED, "aggregate 0: " + COL_RULE, None)
    c["expr_left_unsigned_8"] = (0, expr(SUM, SUB, U64, I32), UNSUPPORTED, "aggregate 0: " + COL_RULE, None)
    for rw in (0, 3, 16):
        c["expr_width_%d" % rw] = (2, expr(SUM, ADD, I8, I8, rw), INVALID,
                                   "aggregate 2: result width %d (1, 2, 4 or 8 bytes)" % rw, None)
    c["expr_unsigned_8_result"] = (0, expr(SUM, ADD, U32, U32, 8, 0), UNSUPPORTED, "aggregate 0: an 8-byte result type must be signed", None)
    c["expr_width_before_signedness"] = (0, expr(SUM, ADD, I64, I64, 16, 0), INVALID, "aggregate 0: result width 16 (1, 2, 4 or 8 bytes)", None)
    # the lossless-cast rule
    c["cast_signed_into_unsigned"] = (0, expr(SUM, ADD, I8, U8, 4, 0), INVALID, CANNOT_HOLD % (0, "un", 4, "left", "", 1), None)
    c["cast_unsigned_into_same_width_signed"] = (1, expr(MIN, SUB, U32, I32, 4, SIGNED), INVALID,
                                                 CANNOT_HOLD % (1, "", 4, "left", "un", 4), None)
    c["cast_wider_into_narrower"] = (0, expr(MAX, MUL, I64, I32, 4, SIGNED), INVALID, CANNOT_HOLD % (0, "", 4, "left", "", 8), None)
    c["cast_right_operand"] = (0, expr(SUM, MUL, I16, I32, 2, SIGNED), INVALID, CANNOT_HOLD % (0, "", 2, "right", "", 4), None)
    c["cast_right_unsigned_wider"] = (0, expr(SUM, MUL, U8, U16, 1, 0), INVALID, CANNOT_HOLD % (0, "un", 1, "right", "un", 2), None)
    c["cast_left_before_right"] = (0, expr(SUM, ADD, I64, I64, 2, SIGNED), INVALID, CANNOT_HOLD % (0, "", 2, "left", "", 8), None)
    c["cast_unsigned_into_wider_signed"] = (0, expr(SUM, ADD, U32, I8, 8, SIGNED), OK, "", (SUM, ADD, I64_MIN, I64_MAX))
    # lo / hi of the seven result types, as known answers
    bounds = {(1, SIGNED): (-128, 127), (2, SIGNED): (-32768, 32767), (4, SIGNED): (-2147483648, 2147483647),
              (8, SIGNED): (-9223372036854775808, 9223372036854775807), (1, 0): (0, 255), (2, 0): (0, 65535), (4, 0): (0, 4294967295)}
    for (rw, rf), (lo, hi) in bounds.items():
        operand = I8 if rf else U8
        c["bounds_%s%d" % ("i" if rf else "u", 8 * rw)] = (0, expr(MIN, SUB, operand, operand, rw, rf), OK, "", (MIN, SUB, lo, hi))
    return c


CELL, COUNTERS = 40, 128  # sizeof(GroupCell); the counter block: (8 own + 8 out-of-range counters) * 8 bytes


def layout_as_before(capacity, max_groups, n_cols, n_aggs, strings):
    """the expressions of aggregate_hashed before polr_hashagg_layout, restated"""
    rep = 16 if strings else 0
    sizes = [capacity * 4, capacity * 4, COUNTERS, capacity * n_cols * 8, capacity * n_cols * rep, capacity * n_aggs * CELL,
             (max_groups * n_cols * 8 + 15) & ~15, max_groups * n_cols * rep, (max_groups * 4 + 15) & ~15, max_groups * n_aggs * CELL]
    offs, at = [], 0
    for b in sizes:
        offs.append(at)
        at += b
    return offs, sizes, sizes[0] + sizes[1] + sizes[2], at


LAYOUTS = {"small": (8, 3, 2, 1, 0), "strings": (16, 5, 3, 8, 1)}


def decode_cases():
    """name -> (fn, sum, mn, mx, count, want (lo, hi, count, is_null))"""
    d = {}
    d["count_star_0"] = (COUNT_STAR, 0, I64_MAX, I64_MIN, 0, (0, 0, 0, 0))  # COUNT is never NULL
    d["count_0"] = (COUNT, 0, I64_MAX, I64_MIN, 0, (0, 0, 0, 0))
    d["count_7"] = (COUNT, 123, 1, 2, 7, (7, 0, 7, 0))
    d["sum_null"] = (SUM, 0, I64_MAX, I64_MIN, 0, (0, 0, 0, 1))
    d["min_null"] = (MIN, 0, I64_MAX, I64_MIN, 0, (0, 0, 0, 1))             # (the far ends no row replaced are not reported)
    d["max_null"] = (MAX, 0, I64_MAX, I64_MIN, 0, (0, 0, 0, 1))
    d["min_negative"] = (MIN, 0, -5, 9, 2, (-5, -1, 2, 0))                  # sign extension into hi
    d["max_negative"] = (MAX, 0, -9, -5, 2, (-5, -1, 2, 0))
    d["min_positive"] = (MIN, 0, 5, 9, 2, (5, 0, 2, 0))
    d["max_i64_min"] = (MAX, 0, I64_MIN, I64_MIN, 1, (I64_MIN, -1, 1, 0))
    d["sum_66_bits"] = (SUM, 5 * I64_MAX, 0, 0, 5, None)                    # 5 x (2^63 - 1)
    d["sum_66_bits_negative"] = (SUM, 5 * I64_MIN, 0, 0, 5, None)
    d["sum_minus_1"] = (SUM, -1, 0, 0, 1, (-1, -1, 1, 0))
    return d


def write_requests(path, plans, args, decodes):
    with open(path, "w") as f:
        for name, p in plans.items():
            f.write("plan %s %s %s\n" % (p["family"], name, " ".join(str(p[k]) for k in HEAD_FIELDS)))
            for k in p["keys"]:
                f.write("key %d %d %d %d %d %d\n" % k)
            for a in p["aggs"]:
                f.write("agg " + " ".join(map(str, a)) + "\n")
            f.write("end\n")
        for name, (index, a, _c, _m, _w) in args.items():
            f.write("arg %s %d %s\n" % (name, index, " ".join(map(str, a))))
        for name, shape in LAYOUTS.items():
            f.write("layout %s %d %d %d %d %d %d %d\n" % ((name,) + shape + (CELL, COUNTERS)))
        for name, (fn, total, mn, mx, count, _w) in decodes.items():
            hi = (total >> 64)
            f.write("decode %s %d %d %d %d %d %d\n" % (name, fn, hi, total & M64, mn, mx, count))
        for n in (1, 8):
            f.write("words w%d %d\n" % (n, n))


def parse(stdout):
    got, cur = {}, None
    for line in stdout.splitlines():
        if line.startswith("  "):
            k, *rest = line.split()
            cur.setdefault(k, []).append([int(x) for x in rest])
        elif line != "ok" and not line.endswith(" requests"):
            name, code, *msg = line.split(" ", 2)
            cur = got[name] = {"code": int(code), "message": msg[0] if msg else ""}
    return got


def build(tmp_path, sanitize):
    exe = str(tmp_path / "agg_plan")
    flags = ["-fsanitize=" + sanitize, "-fno-sanitize-recover=all"] if sanitize else []
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall"] + flags + [SRC, "-o", exe], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-4000:]
    return exe


def run(exe, path):
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    return r.stdout


@pytest.mark.parametrize("sanitize", [None, "address,undefined"], ids=["plain", "asan-ubsan"])
def test_refusals_rules_layout_and_decode(tmp_path, sanitize):
    exe, path = build(tmp_path, sanitize), str(tmp_path / "requests.txt")
    plans = dict(head_cases(), **domain_cases())
    args, decodes = arg_cases(), decode_cases()
    write_requests(path, plans, args, decodes)
    stdout = run(exe, path)
    assert stdout.strip().splitlines()[-2:] == ["%d requests" % (len(plans) + len(args) + len(LAYOUTS) + len(decodes) + 2), "ok"]
    got = parse(stdout)
    for name, p in plans.items():
        assert got[name]["code"] == p["code"], (name, got[name])
        assert got[name]["message"] == p["message"], (name, got[name])  # the whole message
        head_passed, unfuse = got[name]["flags"][0]
        assert unfuse == int(name.startswith("f_unfuse") and p["code"] == OK), name
        if p["code"] == OK and not unfuse:
            n_aggs, n_groups, str_mask = got[name]["plan"][0]
            assert n_aggs == len(p["aggs"]) and [a[0] for a in got[name]["agg"]] == [a[0] for a in p["aggs"]], name
            if p["family"] in ("grouped", "fuse"):
                assert n_groups == p["n_groups"], name
            if p["family"] == "hashed":
                assert head_passed == 1, name
                assert str_mask == sum(1 << q for q, k in enumerate(p["keys"]) if p["strings"] and k[4] == 16), name
    # the hashed sink resets *str_used once its head is passed, whatever refusal follows
    assert got["h_order_columns_before_aggs"]["flags"] == [[1, 0]] and got["h_key_unsigned_8"]["flags"] == [[1, 0]]
    for name in ("h_null_has_out", "h_max_groups_0", "h_agg_cells", "h_max_groups_above", "h_order_count_before_columns"):
        assert got[name]["flags"] == [[0, 0]], name
    # known answers
    assert got["h_key_mixed"]["plan"][0][2] == 0b101 and got["h_key_varchar_allowed"]["plan"][0][2] == 1
    assert got["h_ok"]["plan"][0][2] == 0
    assert got["g_2_20"]["plan"][0][1] == 2 ** 20 and got["f_4096"]["plan"][0][1] == 4096 and got["g_ok"]["plan"][0][1] == 175
    for name, (_i, _a, code, message, want) in args.items():
        assert (got[name]["code"], got[name]["message"]) == (code, message), (name, got[name])
        if want is not None:
            assert got[name]["agg"] == [list(want)], (name, got[name])
    # the allocation of the hashed sink: every offset as the expressions it replaces give it
    for name, shape in LAYOUTS.items():
        offs, sizes, zero, total = layout_as_before(*shape)
        o = got[name]["offsets"][0]
        assert o[:10] == offs and o[10] == zero and o[11] == total, (name, o)
        assert o[6] % 16 == 0 and o[7] % 16 == 0 and o[9] % 8 == 0, name  # okeys / oreps (uint4) and what lies behind
        if shape[4]:
            assert o[4] % 16 == 0, name                                   # reps (uint4)
        ends = [a + b for a, b in zip(offs, sizes)]
        assert all(ends[i] <= o[i + 1] for i in range(9)) and ends[9] == total, name  # in order, nothing overlaps
    # capacity 8, max_groups 3, 2 columns, 1 aggregate, no strings -- by hand: state 32, nulls 32, counters 128, keys 128,
    # no reps, cells 320; okeys 48, no oreps, onulls 12 -> 16, ocells 120
    assert got["small"]["offsets"] == [[0, 32, 64, 192, 320, 320, 640, 688, 688, 704, 192, 824]]
    for name, (fn, total, _mn, _mx, count, want) in decodes.items():
        lo, hi, n, is_null = got[name]["value"][0]
        if want is None:
            assert (hi << 64) + (lo & M64) == total and (n, is_null) == (count, 0), name
        else:
            assert (lo, hi, n, is_null) == want, name
    assert got["sum_66_bits"]["value"][0][1] == 2 and got["sum_66_bits_negative"]["value"][0][:2] == [I64_MIN, -3]
    assert got["w1"]["words"] == [[3]] and got["w8"]["words"] == [[17]]


def test_the_rules_stand_once():
    """the integer-column rule's text stands in one source file, and the fused GROUP BY sink's words per group in one place"""
    csrc = os.path.join(common.ROOT, "duckdb-polr_amd", "csrc")
    holders = [n for n in sorted(os.listdir(csrc)) if n.endswith((".h", ".hip")) and COL_RULE in open(os.path.join(csrc, n)).read()]
    assert holders == ["polr_agg_plan.h"], holders
    for name in ("polr_agg.hip", "polr_capi.hip", "polr_mpx.hip", "polr_fuseagg_plan.h"):
        assert "2u * n_aggs" not in open(os.path.join(csrc, name)).read().replace("fused_aggs", "n_aggs"), name
