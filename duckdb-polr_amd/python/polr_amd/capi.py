"""ctypes binding of include/polr_hip.h (libpolr_hip.so).

This is the only way Python code (tests, bench.py) reaches the device path: straight through the C
ABI.  There is no fallback: if the shared library is missing or no gfx950 device is visible every
entry point raises.
"""
import ctypes as C
import os

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_PKG))  # duckdb-polr_amd/
LIB_PATH = os.path.join(_ROOT, "libpolr_hip.so")

MAX_JOINS, MAX_PATHS, MAX_KEYS = 8, 32, 4
MAX_PREDS = 4
CMP_PRED = {"=": 0, "==": 0, "<>": 1, "!=": 1, "<": 2, ">": 3, "<=": 4, ">=": 5, "str_eq": 8}  # (8 = POLR_CMP_STR_EQ: string cells)
COL_SIGNED, COL_DEVICE = 1, 2

OK, E_NO_DEVICE, E_INVALID, E_UNSUPPORTED, E_HIP, E_DUPLICATE, E_OVERFLOW = 0, -1, -2, -3, -4, -5, -6
E_RANGE = -7  # an aggregate argument `left OP right` outside its result type (PolrError.count: how many)

ROUTING = {"alternate": 0, "adaptive_reinit": 1, "dynamic": 2, "init_once": 3, "opportunistic": 4,
           "default_path": 5, "backpressure": 6, "exponential_backoff": 7}

EXPORTS = [
    "polr_abi_version", "polr_ctx_create", "polr_ctx_destroy", "polr_last_error", "polr_ctx_sync",
    "polr_ht_upload_rows", "polr_ht_upload_columns", "polr_ht_finalize_hash", "polr_ht_finalize_perfect",
    "polr_pht_upload", "polr_ht_destroy", "polr_ht_get_info", "polr_ht_export", "polr_ht_alloc_like",
    "polr_pipeline_create", "polr_pipeline_set_selection", "polr_pipeline_update_probe", "polr_pipeline_destroy",
    "polr_out_create", "polr_out_reset", "polr_out_stats", "polr_out_fetch_ids", "polr_out_materialize",
    "polr_out_destroy", "polr_probe_rounds", "polr_probe_rounds_async",
    "polr_mpx_create", "polr_mpx_run", "polr_mpx_set_chunk_offsets", "polr_mpx_finish", "polr_mpx_fetch_log",
    "polr_mpx_destroy", "polr_mpx_reset", "polr_mpx_enable_timing", "polr_mpx_kernel_time", "polr_mpx_run_many", "polr_mpx_finish_many", "polr_mpx_run_resident", "polr_mpx_run_resident_ranges", "polr_mpx_run_resident_morsels",
    "polr_ht_finalize_auto", "polr_pipeline_launch_info", "polr_pipeline_scan_filter", "polr_pipeline_fetch_scan", "polr_mpx_use_scan_chunks", "polr_out_aggregate", "polr_out_aggregate_grouped",
    "polr_mpx_run_backpressure", "polr_pipeline_scan_filter_lip", "polr_comm_get_unique_id", "polr_comm_create", "polr_bcast_build", "polr_comm_bytes_broadcast", "polr_comm_destroy",
    "polr_ctx_set_pool_tuning", "polr_ctx_get_stream",
    "polr_ht_set_payload_heap", "polr_pipeline_set_probe_heap", "polr_out_aggregate_string", "polr_ht_set_key_flags",
    "polr_out_fuse_grouped", "polr_out_fused_result", "polr_out_aggregate_hashed",
    "polr_ht_set_payload_heaps", "polr_pipeline_set_probe_heaps", "polr_out_aggregate_hashed_str", "polr_out_column_width",
    "polr_ht_encode_dictionary", "polr_ht_fetch_dictionary",
    "polr_ht_encode_dictionary_ex", "polr_ht_fetch_dictionary_codes",
    "polr_out_aggregate_expr", "polr_out_aggregate_grouped_expr", "polr_out_aggregate_hashed_expr",
    "polr_mpx_run_resident_stealing", "polr_mpx_steal_stats",
    "polr_pipeline_scan_filter_str",
    "polr_pipeline_scan_filter_expr",
    "polr_device_bytes_live",
    "polr_out_materialize_strings",
    "polr_mpx_pool_info",
    "polr_ht_from_output",
    "polr_ht_filter", "polr_ht_fetch_filter_rows",
    "polr_pipeline_from_output",
    "polr_ht_semi_filter",
    "polr_ht_column_stats", "polr_pipeline_column_stats", "polr_ht_finalize_auto_stats", "polr_col_stats_plan_info",
    "polr_out_fuse_aggregate", "polr_out_fused_aggregate_result",
    "polr_pipeline_encode_dictionary", "polr_pipeline_fetch_dictionary", "polr_pipeline_fetch_dictionary_codes",
]


class PolrError(RuntimeError):
    def __init__(self, code, text, count=None):
        super().__init__("polr error %d: %s" % (code, text))
        self.code = code
        self.count = count  # E_RANGE: the arguments out of range (*n_out_of_range)


class Col(C.Structure):
    _fields_ = [("data", C.c_void_p), ("valid", C.c_void_p), ("width", C.c_uint32), ("flags", C.c_uint32)]


KEY_BY_VALUE, KEY_NULL_EQUAL = 1, 2  # polr_ht_set_key_flags
DICT_SORTED, DICT_NULL_INVALID = 1, 2  # polr_ht_encode_dictionary_ex
DICT_SELECTED = 4  # polr_pipeline_encode_dictionary only


class PoolTuning(C.Structure):
    """polr_pool_tuning: 0 = the library's default"""
    _fields_ = [("device_share", C.c_uint32), ("units_x", C.c_uint32), ("hi_unit", C.c_uint32),
                ("hi_lottery", C.c_uint32), ("hi_tuples_p1", C.c_uint32), ("idle_sleep", C.c_uint32),
                ("watchdog_us", C.c_uint32), ("share_after", C.c_uint32)]


class JoinDesc(C.Structure):
    _fields_ = [("ht", C.c_void_p), ("n_keys", C.c_uint32), ("key_src_join", C.c_int32 * MAX_KEYS),
                ("key_src_col", C.c_int32 * MAX_KEYS), ("n_preds", C.c_uint32), ("pred_op", C.c_uint32 * MAX_PREDS),
                ("pred_src_join", C.c_int32 * MAX_PREDS), ("pred_src_col", C.c_int32 * MAX_PREDS),
                ("pred_build_col", C.c_uint32 * MAX_PREDS)]


class Round(C.Structure):
    _fields_ = [("begin", C.c_uint64), ("count", C.c_uint64), ("path", C.c_uint32), ("emit", C.c_uint32)]


class ScanFilter(C.Structure):
    _fields_ = [("col", C.c_uint32), ("op", C.c_uint32), ("constant", C.c_int64)]


class ScanFilterStr(C.Structure):
    """polr_scan_filter_str"""
    _fields_ = [("col", C.c_uint32), ("op", C.c_uint32), ("constant", C.c_int64), ("str", C.c_void_p),
                ("str_len", C.c_uint64)]


class FilterValue(C.Structure):
    """polr_filter_value"""
    _fields_ = [("constant", C.c_int64), ("str", C.c_void_p), ("str_len", C.c_uint64)]


class FilterNode(C.Structure):
    """polr_filter_node"""
    _fields_ = [("kind", C.c_uint32), ("col", C.c_uint32), ("op", C.c_uint32), ("first_value", C.c_uint32),
                ("n_values", C.c_uint32), ("pad", C.c_uint32)]


SEMI_ANTI, MAX_SEMI_FILTERS = 1, 4  # POLR_SEMI_ANTI, POLR_MAX_SEMI_FILTERS


class SemiFilter(C.Structure):
    """polr_semi_filter"""
    _fields_ = [("by", C.c_void_p), ("n_cols", C.c_uint32), ("cols", C.c_uint32 * MAX_KEYS), ("flags", C.c_uint32)]


MAX_STATS_COLS, STATS_SELECTED = 16, 1  # POLR_MAX_STATS_COLS, POLR_STATS_SELECTED


class ColStats(C.Structure):
    """polr_col_stats"""
    _fields_ = [("min_value", C.c_int64), ("max_value", C.c_int64), ("n_rows", C.c_uint64), ("n_valid", C.c_uint64),
                ("n_long", C.c_uint64), ("long_bytes", C.c_uint64), ("width", C.c_uint32), ("flags", C.c_uint32)]


class ColStatsPlan(C.Structure):
    """polr_col_stats_plan"""
    _fields_ = [("cells_per_load", C.c_uint32), ("loads_in_flight", C.c_uint32), ("tile_rows", C.c_uint32),
                ("n_workgroups", C.c_uint32), ("stride_rows", C.c_uint64), ("scratch_bytes", C.c_uint64)]


def _stats_dicts(arr, n):
    return [{f[0]: getattr(arr[i], f[0]) for f in ColStats._fields_} for i in range(n)]


FX = {"cmp": 0, "in": 1, "like": 2, "not": 3, "and": 4, "or": 5}  # POLR_FX_*
MAX_FILTER_NODES, MAX_FILTER_DEPTH, MAX_FILTER_VALUES, MAX_FILTER_BYTES = 64, 32, 64, 16384
CMP = {"=": 0, "==": 0, "!=": 1, "<>": 1, "<": 2, ">": 3, "<=": 4, ">=": 5, "is null": 6, "is not null": 7}
MAX_FILTER_STRING = 4096  # POLR_MAX_FILTER_STRING


def like_pushdown(pattern):
    """What the reference pushes into the table scan for `col LIKE pattern` / prefix(col, pattern) (FilterCombiner,
    src/optimizer/filter_combiner.cpp:450-485) -> [(op, constant)]: nothing for a pattern that begins with a wildcard;
    equality for one without wildcards; else the range [prefix, prefix with its last byte + 1) of the bytes before the first
    wildcard; IS NOT NULL goes with both.  The range is the whole predicate only for a pure prefix pattern ('abc%'):
    anything else stays a filter of the engine behind the scan."""
    p = pattern.encode() if isinstance(pattern, str) else bytes(pattern)
    if not p or p[0] in b"%_":
        return []
    cut = min([i for i in (p.find(b"%"), p.find(b"_")) if i >= 0], default=-1)
    if cut < 0:
        return [("=", p), ("is not null", None)]
    prefix = p[:cut]
    if prefix[-1] == 0xFF:
        raise ValueError("a LIKE prefix that ends in 0xFF has no upper bound one byte up (not UTF-8)")
    return [(">=", prefix), ("<", prefix[:-1] + bytes([prefix[-1] + 1])), ("is not null", None)]


def flatten_filter_expr(expr):
    """a nested filter expression (Pipeline.scan_filter_expr) -> (nodes, values) in postfix order, as
    Pipeline.scan_filter_expr_raw takes them"""
    nodes, values = [], []

    def value(c):
        if isinstance(c, (bytes, bytearray, str)):
            b = c.encode() if isinstance(c, str) else bytes(c)
            values.append((0, b, len(b)))
        else:
            values.append((int(c), None, 0))

    def walk(e):
        kind = e[0]
        if kind in ("and", "or"):
            if len(e) < 3:
                raise ValueError("%s takes two or more operands" % kind)
            walk(e[1])
            for operand in e[2:]:
                walk(operand)
                nodes.append((kind, 0, 0, 0, 0))
        elif kind == "not":
            walk(e[1])
            nodes.append(("not", 0, 0, 0, 0))
        elif kind == "cmp":
            col, op, const = e[1], e[2], e[3] if len(e) > 3 else None  # (IS [NOT] NULL takes no constant)
            code = CMP[op] if isinstance(op, str) else op
            if code >= CMP["is null"]:
                nodes.append(("cmp", col, code, 0, 0))
            else:
                nodes.append(("cmp", col, code, len(values), 1))
                value(const)
        elif kind == "in":
            _, col, members = e
            nodes.append(("in", col, 0, len(values), len(members)))
            for m in members:
                value(m)
        elif kind == "like":
            _, col, pattern = e
            nodes.append(("like", col, 0, len(values), 1))
            value(pattern)
        else:
            raise ValueError("unknown filter expression node %r" % (kind,))

    if expr is not None:
        walk(expr)
    return nodes, values


def _filter_arrays(nodes, values):
    """nodes = [(kind, col, op, first_value, n_values)], values = [(constant, bytes or None, str_len)] -> the
    polr_filter_node and polr_filter_value arrays, and the buffers that keep the values' bytes alive"""
    na, va, keep = (FilterNode * max(len(nodes), 1))(), (FilterValue * max(len(values), 1))(), []
    for i, (kind, col, op, first, n) in enumerate(nodes):
        na[i].kind, na[i].col, na[i].op = FX[kind] if isinstance(kind, str) else kind, col, CMP[op] if isinstance(op, str) else op
        na[i].first_value, na[i].n_values = first, n
    for i, (const, b, blen) in enumerate(values):
        va[i].constant, va[i].str_len = int(const or 0), blen
        if b is not None:
            buf = C.create_string_buffer(bytes(b), max(len(b), 1))
            keep.append(buf)
            va[i].str = C.addressof(buf)
    return na, va, keep


class OutColRef(C.Structure):
    """polr_out_col_ref"""
    _fields_ = [("src_join", C.c_int32), ("src_col", C.c_uint32)]


def _out_col_refs(cols):
    """[(src_join, src_col)] -> polr_out_col_ref array"""
    arr = (OutColRef * max(len(cols), 1))()
    for i, (sj, sc) in enumerate(cols):
        arr[i].src_join, arr[i].src_col = sj, sc
    return arr


class HeapRange(C.Structure):
    _fields_ = [("base", C.c_void_p), ("bytes", C.c_uint64)]


def _heap_ranges(blocks):
    """[uint8 numpy array per heap block] -> polr_heap_range array (keeps the blocks alive with it)"""
    blocks = [np.ascontiguousarray(b, dtype=np.uint8) for b in blocks]
    arr = (HeapRange * max(len(blocks), 1))(*[HeapRange(b.ctypes.data, b.nbytes) for b in blocks])
    arr._keep = blocks
    return arr


def _record(raw, at):
    """the string record at offset `at` of a byte arena, {u32 length, little endian; the bytes} (polr_strrec_plan.h) -> bytes"""
    ln = int.from_bytes(raw[at:at + 4], "little")
    return raw[at + 4:at + 4 + ln]


def _fetch_records(call, cap):
    """call(str_bytes, str_cap, byref(str_used)) -> rc with a byte arena of `cap` bytes (a first guess), repeated once with
    the exact size when the guess was too small -> (rc of the last call, the arena as bytes)"""
    used = C.c_uint64()
    for attempt in (0, 1):
        arena = np.zeros((max(cap, 1),), dtype=np.uint8)
        rc = call(arena.ctypes.data, cap, C.byref(used))
        if not (rc == E_OVERFLOW and attempt == 0 and used.value > cap):
            break
        cap = used.value
    return rc, arena.tobytes()


class AggSpec(C.Structure):
    _fields_ = [("fn", C.c_uint32), ("src_join", C.c_int32), ("src_col", C.c_uint32)]


class AggValue(C.Structure):
    _fields_ = [("lo", C.c_int64), ("hi", C.c_int64), ("count", C.c_uint64), ("is_null", C.c_uint32),
                ("pad", C.c_uint32)]


AGG = {"count_star": 0, "count": 1, "sum": 2, "min": 3, "max": 4}


class AggExpr(C.Structure):
    """polr_agg_expr: an aggregate whose argument is a column or `left OP right`"""
    _fields_ = [("fn", C.c_uint32), ("op", C.c_uint32), ("src_join", C.c_int32 * 2), ("src_col", C.c_uint32 * 2),
                ("result_width", C.c_uint32), ("result_flags", C.c_uint32)]


ARG = {"column": 0, "+": 1, "-": 2, "*": 3}


def make_agg_exprs(specs):
    """[(fn, op, (join, col), (join, col) or None, result_dtype or None)] -> polr_agg_expr array.  op in ARG (or a number);
    result_dtype: anything numpy.dtype() takes, the type the reference's binder gave the expression; with op "column" the
    right operand and the result type are ignored (None will do)"""
    arr = (AggExpr * max(len(specs), 1))()
    for i, (fn, op, left, right, rtype) in enumerate(specs):
        arr[i].fn = AGG[fn] if isinstance(fn, str) else fn
        arr[i].op = ARG[op] if isinstance(op, str) else op
        right = right if right is not None else left
        arr[i].src_join[0], arr[i].src_col[0] = left
        arr[i].src_join[1], arr[i].src_col[1] = right
        if rtype is not None:
            dt = np.dtype(rtype)
            arr[i].result_width = dt.itemsize
            arr[i].result_flags = COL_SIGNED if dt.kind == "i" else 0
    return arr


class LaunchInfo(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("waves_per_workgroup", "workgroups_per_cu", "lds_bytes_per_workgroup",
                                          "compiled_stages", "tuple_slots", "n_cus", "flat", "lds_tables", "lds_table_bytes", "pad")]


class PoolInfo(C.Structure):
    """polr_pool_info"""
    _fields_ = [(n, C.c_uint32) for n in ("n_blocks", "pool_waves", "n_rings", "mixed", "share", "units_x", "hi_unit",
                                          "hi_tuples", "gran", "flat")]


class GroupKey(C.Structure):
    _fields_ = [("src_join", C.c_int32), ("src_col", C.c_uint32), ("min_value", C.c_int64), ("n_values", C.c_uint32),
                ("pad", C.c_uint32)]


def _agg_specs(specs):
    """[(fn, src_join, src_col)] with fn in AGG (or a number) -> polr_agg_spec array"""
    arr = (AggSpec * len(specs))()
    for i, (fn, sj, sc) in enumerate(specs):
        arr[i].fn, arr[i].src_join, arr[i].src_col = AGG[fn] if isinstance(fn, str) else fn, sj, sc
    return arr


def _group_keys(keys):
    """[(src_join, src_col)], or with domains [(src_join, src_col, min, n_values)] -> (polr_group_key array, the number of
    groups the domains span)"""
    arr = (GroupKey * len(keys))()
    n_groups = 1
    for i, (sj, sc, *domain) in enumerate(keys):
        arr[i].src_join, arr[i].src_col = sj, sc
        if domain:
            arr[i].min_value, arr[i].n_values = int(domain[0]), int(domain[1])
            n_groups *= int(domain[1])
    return arr, n_groups


def _agg_int(r):
    """polr_agg_value -> python int (the 128-bit two's complement value), or None for NULL"""
    return None if r.is_null else (r.hi << 64) + (r.lo & 0xFFFFFFFFFFFFFFFF)


def _agg_grid(res, n_groups, na):
    """polr_agg_value[n_groups * na] -> (values[n_groups][na], counts[n_groups][na])"""
    return ([[_agg_int(res[g * na + a]) for a in range(na)] for g in range(n_groups)],
            [[res[g * na + a].count for a in range(na)] for g in range(n_groups)])


class HtInfo(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("n_keys", C.c_uint32), ("n_rows", C.c_uint64), ("capacity", C.c_uint64),
                ("max_run", C.c_uint64), ("device_bytes", C.c_uint64), ("is_dense", C.c_uint32),
                ("has_null", C.c_uint32)]


class MpxConfig(C.Structure):
    _fields_ = [("routing", C.c_uint32), ("chunk_size", C.c_uint32), ("regret_budget", C.c_double),
                ("init_tuple_count", C.c_uint64), ("atc_multiplier", C.c_uint64), ("log_rounds", C.c_uint32),
                ("max_log_rounds", C.c_uint32)]


class MpxStats(C.Structure):
    _fields_ = [("num_tuples_processed", C.c_uint64), ("num_intermediates", C.c_uint64), ("num_rounds", C.c_uint64),
                ("input_tuple_count_per_path", C.c_uint64 * MAX_PATHS), ("path_resistances", C.c_double * MAX_PATHS),
                ("stage_out", (C.c_uint64 * MAX_JOINS) * MAX_PATHS)]


class StealStats(C.Structure):
    _fields_ = [("chunks_routed", C.c_uint64), ("chunks_stolen", C.c_uint64), ("n_steals", C.c_uint32), ("pad", C.c_uint32)]


_lib = None


def load():
    """dlopen libpolr_hip.so and declare prototypes; raises if the library is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PolrError(E_NO_DEVICE, "libpolr_hip.so not built (run __graft_entry__.build())")
    L = C.CDLL(LIB_PATH)
    vp, u32, u64, i32, i64 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int32, C.c_int64
    P = C.POINTER
    L.polr_abi_version.restype = C.c_int
    L.polr_device_bytes_live.argtypes = []
    L.polr_device_bytes_live.restype = u64
    L.polr_ctx_create.argtypes = [C.c_int, P(vp)]
    L.polr_ctx_destroy.argtypes = [vp]
    L.polr_ctx_destroy.restype = None
    L.polr_last_error.argtypes = [vp]
    L.polr_last_error.restype = C.c_char_p
    L.polr_ctx_sync.argtypes = [vp, vp]
    L.polr_ctx_set_pool_tuning.argtypes = [vp, C.POINTER(PoolTuning)]
    L.polr_ctx_get_stream.argtypes = [vp, C.POINTER(C.c_void_p)]
    L.polr_ht_set_payload_heap.argtypes = [vp, C.c_uint32, vp, C.c_uint64]
    L.polr_ht_set_key_flags.argtypes = [vp, C.c_uint32, C.c_uint32]
    L.polr_pipeline_set_probe_heap.argtypes = [vp, C.c_uint32, vp, C.c_uint64]
    L.polr_out_aggregate_string.argtypes = [vp, vp, C.c_uint32, C.c_int32, C.c_uint32, C.c_char_p, C.c_uint32,
                                            C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.polr_ht_upload_rows.argtypes = [vp, vp, u64, u32, vp, vp, vp, u32, u32, P(vp)]
    L.polr_ht_upload_columns.argtypes = [vp, P(Col), u32, P(Col), u32, u64, P(vp)]
    L.polr_ht_from_output.argtypes = [vp, vp, P(OutColRef), u32, P(OutColRef), u32, P(vp)]
    L.polr_ht_filter.argtypes = [vp, vp, P(FilterNode), u32, P(FilterValue), u32, P(u64)]
    L.polr_ht_semi_filter.argtypes = [vp, vp, P(SemiFilter), u32, P(u64)]
    L.polr_pipeline_from_output.argtypes = [vp, vp, P(OutColRef), u32, P(JoinDesc), u32, vp, u32, P(vp)]
    L.polr_ht_column_stats.argtypes = [vp, vp, P(u32), u32, P(ColStats)]
    L.polr_pipeline_column_stats.argtypes = [vp, vp, P(u32), u32, u32, P(ColStats)]
    L.polr_ht_finalize_auto_stats.argtypes = [vp, vp, P(u32), P(ColStats)]
    L.polr_col_stats_plan_info.argtypes = [u64, u32, P(ColStatsPlan)]
    L.polr_ht_fetch_filter_rows.argtypes = [vp, vp, vp, u64]
    L.polr_ht_finalize_hash.argtypes = [vp, vp]
    L.polr_ht_finalize_perfect.argtypes = [vp, i64, i64, vp]
    L.polr_pht_upload.argtypes = [vp, u32, u32, i64, i64, vp, P(Col), u32, P(vp)]
    L.polr_ht_destroy.argtypes = [vp]
    L.polr_ht_destroy.restype = None
    L.polr_ht_get_info.argtypes = [vp, P(HtInfo)]
    L.polr_ht_export.argtypes = [vp, vp, P(u64), P(vp), P(u64), P(u32)]
    L.polr_ht_alloc_like.argtypes = [vp, vp, u64, P(vp)]
    L.polr_pipeline_create.argtypes = [vp, P(Col), u32, u64, P(JoinDesc), u32, vp, u32, P(vp)]
    L.polr_pipeline_set_selection.argtypes = [vp, vp, u64, u32]
    L.polr_pipeline_update_probe.argtypes = [vp, u32, vp, vp, u64]
    L.polr_pipeline_destroy.argtypes = [vp]
    L.polr_pipeline_destroy.restype = None
    L.polr_out_create.argtypes = [vp, u32, u64, P(vp)]
    L.polr_out_reset.argtypes = [vp, vp]
    L.polr_out_stats.argtypes = [vp, vp, P(u64), P(u64), P(u32)]
    L.polr_out_fetch_ids.argtypes = [vp, vp, vp, u64]
    L.polr_out_materialize.argtypes = [vp, vp, i32, u32, vp, vp, u64, u32]
    L.polr_out_materialize_strings.argtypes = [vp, vp, i32, u32, vp, vp, u64, vp, u64, P(u64), u32]
    L.polr_out_destroy.argtypes = [vp]
    L.polr_out_destroy.restype = None
    L.polr_probe_rounds.argtypes = [vp, vp, P(Round), u32, vp, vp]
    L.polr_probe_rounds_async.argtypes = [vp, vp, P(Round), u32, vp, vp]
    L.polr_mpx_create.argtypes = [vp, P(MpxConfig), P(vp)]
    L.polr_mpx_run.argtypes = [vp, vp, u64, u64, vp]
    L.polr_mpx_set_chunk_offsets.argtypes = [vp, vp, u64]
    L.polr_mpx_finish.argtypes = [vp, vp, P(MpxStats)]
    L.polr_mpx_fetch_log.argtypes = [vp, vp, vp, vp, vp, u64, P(u64)]
    L.polr_mpx_destroy.argtypes = [vp]
    L.polr_mpx_destroy.restype = None
    L.polr_mpx_reset.argtypes = [vp, vp]
    L.polr_mpx_run_many.argtypes = [vp, vp, vp, vp, u32, vp]
    L.polr_mpx_finish_many.argtypes = [vp, u32, vp]
    L.polr_pipeline_launch_info.argtypes = [vp, C.c_int, vp]
    L.polr_ht_finalize_auto.argtypes = [vp, C.c_int64, C.c_int64, vp, vp]
    L.polr_pipeline_scan_filter.argtypes = [vp, vp, vp, u32, u32, vp, vp]
    L.polr_pipeline_scan_filter_lip.argtypes = [vp, vp, vp, u32, u32, u32, vp, vp]
    L.polr_pipeline_scan_filter_str.argtypes = [vp, vp, vp, u32, u32, u32, vp, vp]
    L.polr_pipeline_scan_filter_expr.argtypes = [vp, vp, vp, u32, vp, u32, u32, u32, vp, vp]
    L.polr_pipeline_fetch_scan.argtypes = [vp, vp, vp]
    L.polr_mpx_use_scan_chunks.argtypes = [vp]
    L.polr_out_aggregate.argtypes = [vp, vp, vp, u32, vp]
    L.polr_out_aggregate_grouped.argtypes = [vp, vp, vp, u32, vp, u32, vp, C.c_uint64, vp]
    L.polr_out_fuse_grouped.argtypes = [vp, vp, u32, vp, u32]
    L.polr_out_aggregate_hashed.argtypes = [vp, vp, vp, u32, vp, u32, C.c_uint64, vp, vp, vp, vp]
    L.polr_out_column_width.argtypes = [vp, C.c_int32, u32, P(u32)]
    L.polr_out_aggregate_hashed_str.argtypes = [vp, vp, vp, u32, vp, u32, C.c_uint64, vp, vp, vp, vp, vp, C.c_uint64, vp]
    L.polr_out_aggregate_expr.argtypes = [vp, vp, vp, u32, vp, vp]
    L.polr_out_aggregate_grouped_expr.argtypes = [vp, vp, vp, u32, vp, u32, vp, C.c_uint64, vp, vp]
    L.polr_out_aggregate_hashed_expr.argtypes = [vp, vp, vp, u32, vp, u32, C.c_uint64, vp, vp, vp, vp, vp, C.c_uint64, vp, vp]
    L.polr_ht_encode_dictionary.argtypes = [vp, u32, vp, P(u32), P(u32), P(u32)]
    L.polr_ht_fetch_dictionary.argtypes = [vp, u32, vp, vp, u64, vp, u64, P(u64)]
    L.polr_ht_encode_dictionary_ex.argtypes = [vp, u32, u32, vp, P(u32), P(u32), P(u32)]
    L.polr_ht_fetch_dictionary_codes.argtypes = [vp, u32, vp, vp, u64, vp, vp, u64, P(u64)]
    L.polr_pipeline_encode_dictionary.argtypes = [vp, u32, u32, vp, P(u32), P(u32), P(u32)]
    L.polr_pipeline_fetch_dictionary.argtypes = [vp, u32, vp, vp, u64, vp, u64, P(u64)]
    L.polr_pipeline_fetch_dictionary_codes.argtypes = [vp, u32, vp, vp, u64, vp, vp, u64, P(u64)]
    L.polr_out_fused_result.argtypes = [vp, vp, vp, C.c_uint64, vp]
    L.polr_out_fuse_aggregate.argtypes = [vp, vp, u32]
    L.polr_out_fused_aggregate_result.argtypes = [vp, vp, vp, u32]
    L.polr_mpx_run_resident.argtypes = [vp, vp, vp, vp, u32, vp, u32]
    L.polr_mpx_pool_info.argtypes = [vp, u32, vp, u32, P(PoolInfo)]
    L.polr_mpx_run_resident_ranges.argtypes = [vp, vp, vp, vp, u32, u32, vp, u32]
    L.polr_mpx_run_resident_morsels.argtypes = [vp, vp, C.c_uint64, C.c_uint64, u32, u32, vp, u32]
    L.polr_mpx_run_resident_stealing.argtypes = [vp, vp, vp, vp, u32, u32, vp, u32]
    L.polr_mpx_steal_stats.argtypes = [vp, vp]
    L.polr_mpx_run_backpressure.argtypes = [vp, vp, C.c_uint64, C.c_uint64, u32, vp, u32]
    L.polr_mpx_enable_timing.argtypes = [vp, C.c_int]
    L.polr_mpx_kernel_time.argtypes = [vp, P(C.c_double), P(u64)]
    L.polr_comm_get_unique_id.argtypes = [vp]
    L.polr_comm_create.argtypes = [vp, vp, C.c_int, C.c_int, P(vp)]
    L.polr_bcast_build.argtypes = [vp, P(vp), C.c_int, vp]
    L.polr_comm_bytes_broadcast.argtypes = [vp, P(u64)]
    L.polr_comm_destroy.argtypes = [vp]
    L.polr_comm_destroy.restype = None
    _lib = L
    return L


def device_bytes_live():
    """polr_device_bytes_live: bytes of device memory the library owns right now, over all contexts and handles"""
    return int(load().polr_device_bytes_live())


def col_stats_plan_info(n_rows, width):
    """polr_col_stats_plan_info: what a statistics call plans for one aligned column of n_rows rows (launches nothing)"""
    L = load()
    i = ColStatsPlan()
    rc = L.polr_col_stats_plan_info(int(n_rows), int(width), C.byref(i))
    if rc != OK:
        raise PolrError(rc, "polr_col_stats_plan_info(%d, %d)" % (n_rows, width))
    return {f[0]: getattr(i, f[0]) for f in ColStatsPlan._fields_}


def _np_col(arr, valid=None):
    arr = np.ascontiguousarray(arr)
    width = arr.dtype.itemsize
    flags = COL_SIGNED if arr.dtype.kind == "i" else 0
    c = Col(arr.ctypes.data, None, width, flags)
    c._keep = [arr]
    if valid is not None:
        valid = np.ascontiguousarray(valid, dtype=np.uint8)
        c.valid = valid.ctypes.data
        c._keep.append(valid)
    return c


def dev_col(ptr, width, signed=False, valid_ptr=None):
    """column descriptor for memory that is already on the device (e.g. a torch tensor's data_ptr())"""
    return Col(ptr, valid_ptr, width, COL_DEVICE | (COL_SIGNED if signed else 0))


def string_cells(values):
    """VARCHAR column -> (cells, heap): cells = one 16-byte string_t per value (string_type.hpp:23-28: length, then up to 12
    characters inline, or a 4-byte prefix and a pointer), heap = the bytes the pointers of the long ones point into (a numpy
    array: keep it alive until the heap has been handed over with set_payload_heap / set_probe_heap).  values: bytes / str."""
    vals = [v.encode() if isinstance(v, str) else bytes(v) for v in values]
    heap = np.frombuffer(b"".join(v for v in vals if len(v) > 12) or b"\0", dtype=np.uint8).copy()
    base = heap.ctypes.data
    cells = np.zeros((len(vals), 16), dtype=np.uint8)
    off = 0
    for i, v in enumerate(vals):
        cells[i, 0:4] = np.frombuffer(np.uint32(len(v)).tobytes(), dtype=np.uint8)
        if len(v) <= 12:
            cells[i, 4:4 + len(v)] = np.frombuffer(v, dtype=np.uint8)
        else:
            cells[i, 4:8] = np.frombuffer(v[:4], dtype=np.uint8)
            cells[i, 8:16] = np.frombuffer(np.uint64(base + off).tobytes(), dtype=np.uint8)
            off += len(v)
    return cells.reshape(-1).view("V16"), heap


def string_hashes(values, bits=64):
    """a 64-bit hash per string, as an engine hands over for a VARCHAR join key (JoinHashTable::Hash): the KEY column of
    such a join on both sides; the strings themselves ride along as a "str_eq" condition.  bits < 64 keeps only the low bits
    (tests: collisions on purpose, so that the verifying comparison has something to reject)"""
    import xxhash
    vals = [v.encode() if isinstance(v, str) else bytes(v) for v in values]
    h = np.array([xxhash.xxh64_intdigest(v) for v in vals], dtype=np.uint64)
    return h if bits >= 64 else (h & np.uint64((1 << bits) - 1))


def _col_array(cols):
    arr = (Col * max(len(cols), 1))(*cols)
    arr._keep = cols
    return arr


class Context:
    def __init__(self, device_id=0):
        self.L = load()
        h = C.c_void_p()
        rc = self.L.polr_ctx_create(device_id, C.byref(h))
        if rc != OK:
            raise PolrError(rc, "polr_ctx_create(%d) failed: no gfx950 device visible" % device_id)
        self.h = h

    def check(self, rc):
        if rc != OK:
            raise PolrError(rc, self.L.polr_last_error(self.h).decode())

    def check_range(self, rc, n_out_of_range):
        """check() for the *_expr sinks: POLR_E_RANGE carries the count of arguments out of range"""
        if rc == E_RANGE:
            raise PolrError(rc, self.L.polr_last_error(self.h).decode(), count=n_out_of_range.value)
        self.check(rc)

    def sync(self, stream=None):
        self.check(self.L.polr_ctx_sync(self.h, stream))

    def stream(self):
        """the context's own stream (polr_ctx_get_stream), to pass to run_resident so that a run is in line with
        Output.reset before it and the aggregates behind it"""
        st = C.c_void_p()
        self.check(self.L.polr_ctx_get_stream(self.h, C.byref(st)))
        return st

    def set_pool_tuning(self, **kw):
        """polr_ctx_set_pool_tuning; no arguments = every default.  hi_tuples=N is passed as hi_tuples_p1 = N + 1"""
        if not kw:
            self.check(self.L.polr_ctx_set_pool_tuning(self.h, None))
            return
        if "hi_tuples" in kw:
            kw["hi_tuples_p1"] = int(kw.pop("hi_tuples")) + 1
        t = PoolTuning(**{k: int(v) for k, v in kw.items()})
        self.check(self.L.polr_ctx_set_pool_tuning(self.h, C.byref(t)))

    def close(self):
        if self.h:
            self.L.polr_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HashTable:
    """A build side resident in HBM."""

    def __init__(self, ctx, handle):
        self.ctx = ctx
        self.h = handle

    @classmethod
    def from_columns(cls, ctx, keys, payload=(), key_valid=None, payload_valid=None):
        """keys/payload: numpy arrays or pre-built Col descriptors (device memory)"""
        kv = key_valid or [None] * len(keys)
        pv = payload_valid or [None] * len(payload)
        kc = [k if isinstance(k, Col) else _np_col(k, v) for k, v in zip(keys, kv)]
        pc = [p if isinstance(p, Col) else _np_col(p, v) for p, v in zip(payload, pv)]
        n = len(keys[0]) if not isinstance(keys[0], Col) else None
        return cls.from_cols(ctx, kc, pc, n)

    @classmethod
    def from_cols(cls, ctx, key_cols, payload_cols, n_rows):
        h = C.c_void_p()
        ctx.check(ctx.L.polr_ht_upload_columns(ctx.h, _col_array(key_cols), len(key_cols), _col_array(payload_cols),
                                               len(payload_cols), n_rows, C.byref(h)))
        return cls(ctx, h)

    @classmethod
    def from_output(cls, out, keys, payload=(), stream=None):
        """polr_ht_from_output: the rows of Output `out` as an un-finalized build side, built on the device.  keys / payload:
        [(src_join, src_col)] as the sinks take them (-1 = probe table).  Build row r of the new table is output row r of
        `out` (the order of fetch_ids); the table owns all its memory, `out` and its sources may be closed afterwards."""
        ctx = out.ctx
        keys, payload = list(keys), list(payload)
        h = C.c_void_p()
        ctx.check(ctx.L.polr_ht_from_output(out.h, stream, _out_col_refs(keys), len(keys), _out_col_refs(payload), len(payload),
                                            C.byref(h)))
        return cls(ctx, h)

    def filter(self, expr, stream=None):
        """polr_ht_filter (before encode_dictionary and finalize): keep the rows for which `expr` is TRUE and compact the
        table on the device -> the kept count.  expr: the nested tuples of Pipeline.scan_filter_expr; its columns number the
        table's, keys first, then payload.  None keeps every row.  Build row r is afterwards the r-th kept row:
        filter_rows() maps build ids back to the rows as uploaded."""
        nodes, values = flatten_filter_expr(expr)
        return self.filter_raw(nodes, values, stream)

    def filter_raw(self, nodes, values, stream=None, n_nodes=None, n_values=None):
        """polr_ht_filter with the struct fields as given (Pipeline.scan_filter_expr_raw) -> the kept count"""
        na, va, keep = _filter_arrays(nodes, values)
        kept = C.c_uint64()
        self.ctx.check(self.ctx.L.polr_ht_filter(self.h, stream, na if nodes else None, len(nodes) if n_nodes is None else n_nodes,
                                                 va if values else None, len(values) if n_values is None else n_values,
                                                 C.byref(kept)))
        self._n_kept = kept.value
        return kept.value

    def semi_filter(self, filters, stream=None):
        """polr_ht_semi_filter (before encode_dictionary and finalize): thin the table by SEMI / ANTI joins against finalized
        tables and compact it on the device -> the kept count.  filters: [(by, cols, anti)] -- `by` a finalized HashTable, cols
        the columns of this table (keys first, then payload) paired with by's keys, anti True keeps the rows WITHOUT a match
        (NOT EXISTS; rows whose key is NULL among them).  A row is kept iff every filter keeps it; [] keeps every row.
        Allowed after filter() or another semi_filter(): filter_rows() is then the composed list."""
        fl = [SemiFilter(by.h if by is not None else None, len(cols), (C.c_uint32 * MAX_KEYS)(*list(cols)[:MAX_KEYS]),
                         (SEMI_ANTI if anti is True else int(anti))) for by, cols, anti in filters]
        return self.semi_filter_raw(fl, stream)

    def semi_filter_raw(self, filters, stream=None, n_filters=None):
        """polr_ht_semi_filter with SemiFilter structs as given -> the kept count"""
        arr = (SemiFilter * max(len(filters), 1))(*filters)
        kept = C.c_uint64()
        self.ctx.check(self.ctx.L.polr_ht_semi_filter(self.h, stream, arr if filters else None,
                                                      len(filters) if n_filters is None else n_filters, C.byref(kept)))
        self._n_kept = kept.value
        return kept.value

    def filter_rows(self, stream=None):
        """polr_ht_fetch_filter_rows: the uploaded row number of every build row of a filtered table, ascending"""
        n = getattr(self, "_n_kept", 0)  # (not filtered through this object: the call refuses)
        rows = np.zeros((max(n, 1),), dtype=np.uint32)
        self.ctx.check(self.ctx.L.polr_ht_fetch_filter_rows(self.h, stream, rows.ctypes.data, n))
        return rows[:n]

    def set_key_flags(self, key_col, flags):
        """polr_ht_set_key_flags (before finalize): KEY_BY_VALUE = the probe side may read another integer type (a CAST'ed
        key), KEY_NULL_EQUAL = IS NOT DISTINCT FROM"""
        self.ctx.check(self.ctx.L.polr_ht_set_key_flags(self.h, key_col, flags))

    def set_payload_heap(self, payload_col, heap):
        """polr_ht_set_payload_heap: the string heap the cells of payload column `payload_col` point into (before finalize)"""
        heap = np.ascontiguousarray(heap, dtype=np.uint8)
        self.ctx.check(self.ctx.L.polr_ht_set_payload_heap(self.h, payload_col, heap.ctypes.data, heap.nbytes))
        return self

    def set_payload_heaps(self, payload_col, blocks):
        """polr_ht_set_payload_heaps: a heap made of several blocks (one range each; before finalize)"""
        L = self.ctx.L
        L.polr_ht_set_payload_heaps.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(HeapRange), C.c_uint32]
        self.ctx.check(L.polr_ht_set_payload_heaps(self.h, payload_col, _heap_ranges(blocks), len(blocks)))
        return self

    def encode_dictionary(self, payload_col, stream=None, sorted=False, null_invalid=False, flags=None):
        """polr_ht_encode_dictionary (before finalize): VARCHAR payload column `payload_col` -> one more payload column of
        4-byte codes, 0 .. n_codes - 1 in order of first appearance, NULL rows n_codes -> (code_col, n_codes, has_null).
        sorted / null_invalid (polr_ht_encode_dictionary_ex: DICT_SORTED, DICT_NULL_INVALID; `flags`: the word itself): codes
        that rise with the strings; a validity array for the code column, copied from the source column's"""
        col, n, null = C.c_uint32(), C.c_uint32(), C.c_uint32()
        if flags is None:
            flags = (DICT_SORTED if sorted else 0) | (DICT_NULL_INVALID if null_invalid else 0)
        if flags:
            self.ctx.check(self.ctx.L.polr_ht_encode_dictionary_ex(self.h, payload_col, flags, stream, C.byref(col), C.byref(n),
                                                                   C.byref(null)))
        else:
            self.ctx.check(self.ctx.L.polr_ht_encode_dictionary(self.h, payload_col, stream, C.byref(col), C.byref(n),
                                                                C.byref(null)))
        self.__dict__.setdefault("_n_codes", {})[col.value] = n.value  # (dictionary() sizes its offsets by it)
        return col.value, n.value, null.value

    def dictionary(self, code_col, str_cap=4096, stream=None):
        """polr_ht_fetch_dictionary: the strings of code column `code_col` (as encode_dictionary of this object returned
        it), [bytes] indexed by code.  The byte arena is sized here (str_cap: a first guess) and the call repeated once
        with the exact size when the guess was too small."""
        n_codes = getattr(self, "_n_codes", {}).get(code_col, 0)  # (not encoded through this object: the call refuses)
        offs = np.zeros((max(n_codes, 1),), dtype=np.uint64)
        rc, raw = _fetch_records(lambda *arena: self.ctx.L.polr_ht_fetch_dictionary(self.h, code_col, stream, offs.ctypes.data,
                                                                                    n_codes, *arena), str_cap)
        self.ctx.check(rc)
        return [_record(raw, at) for at in offs[:n_codes].tolist()]

    def dictionary_strings(self, code_col, codes, str_cap=4096, stream=None):
        """polr_ht_fetch_dictionary_codes: the strings of the listed codes of code column `code_col`, [bytes] in list order
        (duplicates included); one retry with the exact size when str_cap was too small"""
        codes = np.ascontiguousarray(codes, dtype=np.uint32)
        n = len(codes)
        offs = np.zeros((max(n, 1),), dtype=np.uint64)
        rc, raw = _fetch_records(lambda *arena: self.ctx.L.polr_ht_fetch_dictionary_codes(self.h, code_col, stream, codes.ctypes.data,
                                                                                          n, offs.ctypes.data, *arena), str_cap)
        self.ctx.check(rc)
        return [_record(raw, at) for at in offs[:n].tolist()]

    @classmethod
    def from_rows(cls, ctx, rows, n_rows, row_width, col_offset, col_width, col_signed, n_keys, n_payload):
        rows = np.ascontiguousarray(rows, dtype=np.uint8)
        off = np.ascontiguousarray(col_offset, dtype=np.uint32)
        wid = np.ascontiguousarray(col_width, dtype=np.uint32)
        flg = np.ascontiguousarray([COL_SIGNED if s else 0 for s in col_signed], dtype=np.uint32)
        h = C.c_void_p()
        ctx.check(ctx.L.polr_ht_upload_rows(ctx.h, rows.ctypes.data, n_rows, row_width, off.ctypes.data,
                                            wid.ctypes.data, flg.ctypes.data, n_keys, n_payload, C.byref(h)))
        return cls(ctx, h)

    @classmethod
    def from_perfect(cls, ctx, key_width, key_signed, min_value, max_value, bitmap, payload=(), payload_valid=None):
        bitmap = np.ascontiguousarray(bitmap, dtype=np.uint8)
        pv = payload_valid or [None] * len(payload)
        pc = [_np_col(p, v) for p, v in zip(payload, pv)]
        h = C.c_void_p()
        ctx.check(ctx.L.polr_pht_upload(ctx.h, key_width, COL_SIGNED if key_signed else 0, int(min_value),
                                        int(max_value), bitmap.ctypes.data, _col_array(pc), len(pc), C.byref(h)))
        return cls(ctx, h)

    def finalize_hash(self, stream=None):
        self.ctx.check(self.ctx.L.polr_ht_finalize_hash(self.h, stream))
        return self

    def finalize_perfect(self, min_value, max_value, stream=None):
        """returns False on a duplicate key (caller falls back to finalize_hash)"""
        rc = self.ctx.L.polr_ht_finalize_perfect(self.h, int(min_value), int(max_value), stream)
        if rc == E_DUPLICATE:
            return False
        self.ctx.check(rc)
        return True

    def finalize_auto(self, min_value, max_value, stream=None):
        """polr_ht_finalize_auto: perfect table for a dense unique integer key, hash table otherwise -> kind"""
        kind = C.c_uint32()
        self.ctx.check(self.ctx.L.polr_ht_finalize_auto(self.h, int(min_value), int(max_value), stream, C.byref(kind)))
        return kind.value

    def column_stats(self, cols, stream=None):
        """polr_ht_column_stats (before finalize): min / max / counts of the table's columns cols[] -- keys first, then
        payload, as filter() numbers them -- in one pass on the device -> a list of dicts with the fields of polr_col_stats.
        A VARCHAR column: min / max of the LENGTHS, n_long / long_bytes of the strings beyond 12 bytes."""
        cols = list(cols)
        return self.column_stats_raw(cols, len(cols), stream)

    def column_stats_raw(self, cols, n_cols, stream=None, stats=None):
        """polr_ht_column_stats with cols (a list or None) and n_cols as given; stats: a ColStats array to fill"""
        ca = (C.c_uint32 * max(len(cols), 1))(*cols) if cols is not None else None
        st = (ColStats * max(n_cols, 1))() if stats is None else stats
        self.ctx.check(self.ctx.L.polr_ht_column_stats(self.h, stream, ca, n_cols, st))
        return _stats_dicts(st, n_cols)

    def finalize_auto_stats(self, stream=None):
        """polr_ht_finalize_auto_stats: finalize_auto with the min / max of key column 0 taken on the device -> (kind,
        key_stats: the dict of column_stats for key column 0)"""
        kind, st = C.c_uint32(), (ColStats * 1)()
        self.ctx.check(self.ctx.L.polr_ht_finalize_auto_stats(self.h, stream, C.byref(kind), st))
        return kind.value, _stats_dicts(st, 1)[0]

    def info(self):
        i = HtInfo()
        self.ctx.check(self.ctx.L.polr_ht_get_info(self.h, C.byref(i)))
        return {f[0]: getattr(i, f[0]) for f in HtInfo._fields_}

    def export(self):
        """(meta bytes, [(device ptr, nbytes)]) of the finalized table, for a broadcast"""
        L = self.ctx.L
        mb, nb = C.c_uint64(0), C.c_uint32(0)
        self.ctx.check(L.polr_ht_export(self.h, None, C.byref(mb), None, None, C.byref(nb)))
        meta = (C.c_uint8 * mb.value)()
        ptrs = (C.c_void_p * nb.value)()
        sizes = (C.c_uint64 * nb.value)()
        self.ctx.check(L.polr_ht_export(self.h, meta, C.byref(mb), ptrs, sizes, C.byref(nb)))
        return bytes(meta), [(ptrs[i], sizes[i]) for i in range(nb.value)]

    @classmethod
    def alloc_like(cls, ctx, meta):
        buf = (C.c_uint8 * len(meta)).from_buffer_copy(meta)
        h = C.c_void_p()
        ctx.check(ctx.L.polr_ht_alloc_like(ctx.h, buf, len(meta), C.byref(h)))
        return cls(ctx, h)

    def close(self):
        if self.h:
            self.ctx.L.polr_ht_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Pipeline:
    def __init__(self, ctx, probe_cols, n_probe_rows, joins, paths, probe_valid=None):
        """probe_cols: numpy arrays or Col descriptors; joins: [(HashTable, [(src_join, src_col)])]"""
        self.ctx = ctx
        pv = probe_valid or [None] * len(probe_cols)
        pc = [c if isinstance(c, Col) else _np_col(c, v) for c, v in zip(probe_cols, pv)]
        self.k = len(joins)
        self._hts = [j[0] for j in joins]
        jd = self._join_descs(joins)
        paths = np.ascontiguousarray(np.asarray(paths, dtype=np.int32).reshape(-1, self.k))
        self.n_paths = len(paths)
        h = C.c_void_p()
        ctx.check(ctx.L.polr_pipeline_create(ctx.h, _col_array(pc), len(pc), n_probe_rows, jd, self.k,
                                             paths.ctypes.data, self.n_paths, C.byref(h)))
        self.h = h
        self.scan = (0, 0)  # (n_selected, n_chunks) of the last scan_filter: what fetch_scan sizes its arrays by

    @staticmethod
    def _join_descs(joins):
        """[(HashTable, [(src_join, src_col)])] -> polr_join_desc array"""
        jd = (JoinDesc * max(len(joins), 1))()
        for i, (ht, key_src) in enumerate(joins):
            jd[i].ht = ht.h
            jd[i].n_keys = len(key_src)
            for c, (sj, sc) in enumerate(key_src):
                jd[i].key_src_join[c] = sj
                jd[i].key_src_col[c] = sc
            # non-equality conditions of the join ride on the table object: ht.preds = [(op, (src_join, src_col),
            # payload column index)] (build_joins sets it from the workload's "preds")
            preds = getattr(ht, "preds", None) or []
            jd[i].n_preds = len(preds)
            for c, (op, (sj, sc), bc) in enumerate(preds[:MAX_PREDS]):
                jd[i].pred_op[c] = CMP_PRED[op] if isinstance(op, str) else op
                jd[i].pred_src_join[c] = sj
                jd[i].pred_src_col[c] = sc
                jd[i].pred_build_col[c] = bc
        return jd

    @classmethod
    def from_output(cls, out, cols, joins, paths, stream=None):
        """polr_pipeline_from_output: the rows of Output `out` as the source of a new pipeline, gathered on the device.
        cols: [(src_join, src_col)] as the sinks take them (-1 = probe table) -- cols[i] becomes probe column i; joins and
        paths as for Pipeline().  Probe row r of the new pipeline is output row r of `out` (the order of fetch_ids), so slot 0
        of its outputs indexes out.fetch_ids().  The pipeline owns its columns: `out`, its pipeline and that pipeline's
        tables may be closed afterwards."""
        ctx = out.ctx
        self = cls.__new__(cls)
        self.ctx = ctx
        cols, joins = list(cols), list(joins)
        self.k = len(joins)
        self._hts = [j[0] for j in joins]
        paths = np.ascontiguousarray(np.asarray(paths, dtype=np.int32).reshape(-1, max(self.k, 1)))
        self.n_paths = len(paths)
        self.h = None
        h = C.c_void_p()
        ctx.check(ctx.L.polr_pipeline_from_output(out.h, stream, _out_col_refs(cols), len(cols), cls._join_descs(joins), self.k,
                                                  paths.ctypes.data, self.n_paths, C.byref(h)))
        self.h = h
        self.scan = (0, 0)
        return self

    def set_probe_heap(self, probe_col, heap):
        """polr_pipeline_set_probe_heap: the string heap the cells of probe column `probe_col` point into"""
        heap = np.ascontiguousarray(heap, dtype=np.uint8)
        self.ctx.check(self.ctx.L.polr_pipeline_set_probe_heap(self.h, probe_col, heap.ctypes.data, heap.nbytes))

    def set_probe_heaps(self, probe_col, blocks):
        """polr_pipeline_set_probe_heaps: a heap made of several blocks (one range each)"""
        L = self.ctx.L
        L.polr_pipeline_set_probe_heaps.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(HeapRange), C.c_uint32]
        self.ctx.check(L.polr_pipeline_set_probe_heaps(self.h, probe_col, _heap_ranges(blocks), len(blocks)))

    def set_selection(self, sel, device=False, n=None):
        if sel is None:
            self.ctx.check(self.ctx.L.polr_pipeline_set_selection(self.h, None, 0, 0))
        elif device:
            self.ctx.check(self.ctx.L.polr_pipeline_set_selection(self.h, sel, n, COL_DEVICE))
        else:
            sel = np.ascontiguousarray(sel, dtype=np.uint32)
            self.ctx.check(self.ctx.L.polr_pipeline_set_selection(self.h, sel.ctypes.data, len(sel), 0))

    def encode_dictionary(self, probe_col, sorted=False, null_invalid=False, selected=False, stream=None, flags=None):
        """polr_pipeline_encode_dictionary: VARCHAR probe column `probe_col` -> one more probe column of 4-byte codes, by the
        rules of HashTable.encode_dictionary -> (code_col, n_codes, has_null).  selected (DICT_SELECTED): only the rows of the
        selection in force are read and coded; every other row gets n_codes.  `flags`: the word itself."""
        col, n, null = C.c_uint32(), C.c_uint32(), C.c_uint32()
        if flags is None:
            flags = (DICT_SORTED if sorted else 0) | (DICT_NULL_INVALID if null_invalid else 0) | (DICT_SELECTED if selected else 0)
        self.ctx.check(self.ctx.L.polr_pipeline_encode_dictionary(self.h, probe_col, flags, stream, C.byref(col), C.byref(n),
                                                                  C.byref(null)))
        self.__dict__.setdefault("_n_codes", {})[col.value] = n.value  # (dictionary() sizes its offsets by it)
        return col.value, n.value, null.value

    def dictionary(self, code_col, str_cap=4096, stream=None):
        """polr_pipeline_fetch_dictionary: the strings of code column `code_col`, [bytes] indexed by code; one retry with the
        exact size when str_cap was too small"""
        n_codes = getattr(self, "_n_codes", {}).get(code_col, 0)  # (not encoded through this object: the call refuses)
        offs = np.zeros((max(n_codes, 1),), dtype=np.uint64)
        rc, raw = _fetch_records(lambda *arena: self.ctx.L.polr_pipeline_fetch_dictionary(self.h, code_col, stream, offs.ctypes.data,
                                                                                          n_codes, *arena), str_cap)
        self.ctx.check(rc)
        return [_record(raw, at) for at in offs[:n_codes].tolist()]

    def dictionary_strings(self, code_col, codes, str_cap=4096, stream=None):
        """polr_pipeline_fetch_dictionary_codes: the strings of the listed codes of code column `code_col`, [bytes] in list
        order (duplicates included); one retry with the exact size when str_cap was too small"""
        codes = np.ascontiguousarray(codes, dtype=np.uint32)
        n = len(codes)
        offs = np.zeros((max(n, 1),), dtype=np.uint64)
        rc, raw = _fetch_records(lambda *arena: self.ctx.L.polr_pipeline_fetch_dictionary_codes(
            self.h, code_col, stream, codes.ctypes.data, n, offs.ctypes.data, *arena), str_cap)
        self.ctx.check(rc)
        return [_record(raw, at) for at in offs[:n].tolist()]

    def column_stats(self, cols, selected=False, stream=None):
        """polr_pipeline_column_stats: min / max / counts of the probe columns cols[] in one pass on the device, over all
        probe rows or, selected=True, over the rows of the selection in force -> a list of dicts (polr_col_stats)"""
        cols = list(cols)
        return self.column_stats_raw(cols, len(cols), STATS_SELECTED if selected else 0, stream)

    def column_stats_raw(self, cols, n_cols, flags=0, stream=None, stats=None):
        """polr_pipeline_column_stats with cols (a list or None), n_cols and flags as given; stats: a ColStats array to fill"""
        ca = (C.c_uint32 * max(len(cols), 1))(*cols) if cols is not None else None
        st = (ColStats * max(n_cols, 1))() if stats is None else stats
        self.ctx.check(self.ctx.L.polr_pipeline_column_stats(self.h, stream, ca, n_cols, flags, st))
        return _stats_dicts(st, n_cols)

    def launch_info(self, materialize=False):
        i = LaunchInfo()
        self.ctx.check(self.ctx.L.polr_pipeline_launch_info(self.h, int(materialize), C.byref(i)))
        return {f[0]: getattr(i, f[0]) for f in LaunchInfo._fields_}

    def scan_filter(self, filters, vector_size=1024, stream=None, lip_joins=0):
        """polr_pipeline_scan_filter(_lip): filters = [(col, op, constant)] with op in CMP; lip_joins: bit j = also
        apply join j's filter at the source (LIP); the selection and the chunk boundaries stay on the device ->
        (n_selected, n_chunks).  A bytes / str constant is a VARCHAR one (polr_pipeline_scan_filter_str): any such
        constant sends the whole call through that entry point."""
        n = len(filters)
        ns, nc = C.c_uint64(), C.c_uint64()
        if any(isinstance(f[2], (bytes, bytearray, str)) for f in filters):
            raw = []
            for col, op, const in filters:
                if isinstance(const, (bytes, bytearray, str)):
                    b = const.encode() if isinstance(const, str) else bytes(const)
                    raw.append((col, op, 0, b, len(b)))
                else:
                    raw.append((col, op, const, None, 0))
            return self.scan_filter_str_raw(raw, vector_size, stream, lip_joins)
        arr = (ScanFilter * max(n, 1))()
        for i, (col, op, const) in enumerate(filters):
            arr[i].col, arr[i].op, arr[i].constant = col, CMP[op] if isinstance(op, str) else op, int(const or 0)
        self.ctx.check(self.ctx.L.polr_pipeline_scan_filter_lip(self.h, stream, arr if n else None, n, int(lip_joins),
                                                                vector_size, C.byref(ns), C.byref(nc)))
        self.scan = (ns.value, nc.value)
        return self.scan

    def scan_filter_str_raw(self, filters, vector_size=1024, stream=None, lip_joins=0):
        """polr_pipeline_scan_filter_str with the struct fields as given: filters = [(col, op code, constant, bytes or
        None, str_len)] -- the edges of the contract (a length without bytes, bytes against an integer column)"""
        n = len(filters)
        arr, keep = (ScanFilterStr * max(n, 1))(), []
        for i, (col, op, const, b, blen) in enumerate(filters):
            arr[i].col, arr[i].op, arr[i].constant, arr[i].str_len = col, CMP[op] if isinstance(op, str) else op, int(const or 0), blen
            if b is not None:
                buf = C.create_string_buffer(bytes(b), max(len(b), 1))
                keep.append(buf)
                arr[i].str = C.addressof(buf)
        ns, nc = C.c_uint64(), C.c_uint64()
        self.ctx.check(self.ctx.L.polr_pipeline_scan_filter_str(self.h, stream, arr if n else None, n, int(lip_joins),
                                                                vector_size, C.byref(ns), C.byref(nc)))
        self.scan = (ns.value, nc.value)
        return self.scan

    def scan_filter_expr(self, expr, vector_size=1024, stream=None, lip_joins=0):
        """polr_pipeline_scan_filter_expr: expr is a nested tuple -- ("and" | "or", a, b, ...), ("not", a), and the leaves
        ("cmp", col, op, constant), ("in", col, [members]), ("like", col, pattern); a bytes / str constant is a VARCHAR
        one; None: every row passes.  Flattened to postfix (an "and" / "or" of more than two operands left to right);
        sets self.scan and returns it."""
        nodes, values = flatten_filter_expr(expr)
        return self.scan_filter_expr_raw(nodes, values, vector_size, stream, lip_joins)

    def scan_filter_expr_raw(self, nodes, values, vector_size=1024, stream=None, lip_joins=0, n_nodes=None, n_values=None):
        """polr_pipeline_scan_filter_expr with the struct fields as given: nodes = [(kind, col, op, first_value,
        n_values)], values = [(constant, bytes or None, str_len)]; n_nodes / n_values: the counts to pass, when they are
        not the lists' lengths -- the edges of the contract"""
        na, va, keep = _filter_arrays(nodes, values)
        ns, nc = C.c_uint64(), C.c_uint64()
        self.ctx.check(self.ctx.L.polr_pipeline_scan_filter_expr(
            self.h, stream, na if nodes else None, len(nodes) if n_nodes is None else n_nodes, va if values else None,
            len(values) if n_values is None else n_values, int(lip_joins), vector_size, C.byref(ns), C.byref(nc)))
        self.scan = (ns.value, nc.value)
        return self.scan

    def fetch_scan(self):
        ns, nc = self.scan
        sel = np.zeros((ns,), dtype=np.uint32)
        offs = np.zeros((nc + 1,), dtype=np.uint64)
        self.ctx.check(self.ctx.L.polr_pipeline_fetch_scan(self.h, sel.ctypes.data, offs.ctypes.data))
        return sel, offs

    def probe_rounds(self, rounds, out=None, stream=None):
        """rounds: [(begin, count, path, emit)] -> counts ndarray [n_rounds, k]"""
        n = len(rounds)
        arr = (Round * n)()
        for i, (b, c, p, e) in enumerate(rounds):
            arr[i].begin, arr[i].count, arr[i].path, arr[i].emit = int(b), int(c), int(p), int(e)
        counts = np.zeros((n, self.k), dtype=np.uint64)
        rc = self.ctx.L.polr_probe_rounds(self.h, stream, arr, n, out.h if out else None, counts.ctypes.data)
        if rc == E_OVERFLOW:
            raise PolrError(rc, self.ctx.L.polr_last_error(self.ctx.h).decode())
        self.ctx.check(rc)
        return counts

    def probe_rounds_async(self, rounds_struct, n, counts_dev_ptr, out=None, stream=None):
        self.ctx.check(self.ctx.L.polr_probe_rounds_async(self.h, stream, rounds_struct, n, out.h if out else None,
                                                          counts_dev_ptr))

    def close(self):
        if self.h:
            self.ctx.L.polr_pipeline_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def make_rounds(rounds):
    arr = (Round * len(rounds))()
    for i, (b, c, p, e) in enumerate(rounds):
        arr[i].begin, arr[i].count, arr[i].path, arr[i].emit = int(b), int(c), int(p), int(e)
    return arr


class Output:
    def __init__(self, pipe, chunk_capacity=1024, max_chunks=1024):
        self.pipe = pipe
        self.ctx = pipe.ctx
        h = C.c_void_p()
        self.ctx.check(self.ctx.L.polr_out_create(pipe.h, chunk_capacity, max_chunks, C.byref(h)))
        self.h = h
        self._fused_aggs = 0  # aggregates of the fused ungrouped sink attached through fuse_aggregate (0: none)

    def reset(self, stream=None):
        self.ctx.check(self.ctx.L.polr_out_reset(self.h, stream))

    def stats(self, stream=None):
        n, c, o = C.c_uint64(), C.c_uint64(), C.c_uint32()
        self.ctx.check(self.ctx.L.polr_out_stats(self.h, stream, C.byref(n), C.byref(c), C.byref(o)))
        return n.value, c.value, bool(o.value)

    def fetch_ids(self, stream=None):
        n, _, _ = self.stats(stream)
        out = np.zeros((n, 1 + self.pipe.k), dtype=np.uint32)
        self.ctx.check(self.ctx.L.polr_out_fetch_ids(self.h, stream, out.ctypes.data, n))
        return out

    def aggregate(self, specs, stream=None):
        """polr_out_aggregate: specs = [(fn, src_join, src_col)] with fn in AGG -> [python int or None]
        (ungrouped COUNT(*) / COUNT / SUM / MIN / MAX over the output, reduced on the device)"""
        res = (AggValue * len(specs))()
        self.ctx.check(self.ctx.L.polr_out_aggregate(self.h, stream, _agg_specs(specs), len(specs), res))
        return [_agg_int(r) for r in res]

    def aggregate_grouped(self, keys, specs, stream=None):
        """polr_out_aggregate_grouped: keys = [(src_join, src_col, min, n_values)], specs as in aggregate() ->
        (values[n_groups][n_aggs] of python int / None, counts[n_groups][n_aggs], n_dropped)"""
        ka, n_groups = _group_keys(keys)
        na = len(specs)
        res = (AggValue * (n_groups * na))()
        dropped = C.c_uint64()
        self.ctx.check(self.ctx.L.polr_out_aggregate_grouped(self.h, stream, ka, len(keys), _agg_specs(specs), na, res,
                                                             n_groups, C.byref(dropped)))
        return _agg_grid(res, n_groups, na) + (dropped.value,)

    def aggregate_hashed(self, cols, specs, max_groups, stream=None):
        """polr_out_aggregate_hashed: GROUP BY over group columns of any integer domain.  cols = [(src_join, src_col)],
        specs as in aggregate() -> {group key tuple (None = NULL): [value per aggregate (python int / None)]}"""
        return self._hashed(self.ctx.L.polr_out_aggregate_hashed, cols, _agg_specs(specs), len(specs), max_groups, stream)

    def _col_width(self, src_join, src_col):
        """polr_out_column_width: cell width of a probe column (src_join < 0) or of a payload column of join src_join"""
        w = C.c_uint32()
        self.ctx.check(self.ctx.L.polr_out_column_width(self.h, src_join, src_col, C.byref(w)))
        return w.value

    def _hashed(self, entry, cols, sa, na, max_groups, stream, strings=False, str_cap=None, ranged=False):
        """one of the three polr_out_aggregate_hashed* entry points -> {group key tuple: [value per aggregate]}.  strings: the
        entry point takes the byte arena of the groups' strings, sized here (str_cap: a first guess) and the call repeated
        once with the exact size when the guess was too small; ranged: it reports arguments out of range"""
        nk = len(cols)
        ka, _ = _group_keys(cols)
        keys = np.zeros((max_groups, nk), dtype=np.int64)
        nulls = np.zeros((max_groups,), dtype=np.uint32)
        res = (AggValue * (max_groups * na))()
        n, oor = C.c_uint64(), C.c_uint64()
        cap = (max(4096, 24 * max_groups) if str_cap is None else int(str_cap)) if strings else 0

        def call(*arena):  # (repeated where the strings did not fit; the groups did)
            tail = (arena if strings else ()) + ((C.byref(oor),) if ranged else ())
            return entry(self.h, stream, ka, nk, sa, na, max_groups, keys.ctypes.data, nulls.ctypes.data, res, C.byref(n), *tail)

        rc, raw = _fetch_records(call, cap)
        self.ctx.check_range(rc, oor)
        is_str = [strings and self._col_width(sj, sc) == 16 for sj, sc in cols]
        out = {}
        for g in range(n.value):
            key = []
            for c in range(nk):
                if (nulls[g] >> c) & 1:
                    key.append(None)
                elif is_str[c]:
                    key.append(_record(raw, int(keys[g, c])))
                else:
                    key.append(int(keys[g, c]))
            out[tuple(key)] = [_agg_int(res[g * na + a]) for a in range(na)]
        return out

    def aggregate_hashed_str(self, cols, specs, max_groups, str_cap=None, stream=None):
        """polr_out_aggregate_hashed_str: the general GROUP BY whose group columns may be VARCHAR (width-16 string_t
        columns, grouped by the strings' bytes) or integer, in any mix.  cols / specs as in aggregate_hashed ->
        {group key tuple: [value per aggregate]} with bytes for a VARCHAR column, int for an integer one, None for NULL.
        The byte arena of the groups' strings is sized here (str_cap: a first guess) and the call repeated once with the
        exact size when the guess was too small."""
        return self._hashed(self.ctx.L.polr_out_aggregate_hashed_str, cols, _agg_specs(specs), len(specs), max_groups, stream,
                            strings=True, str_cap=str_cap)

    def aggregate_expr(self, specs, stream=None):
        """polr_out_aggregate_expr: ungrouped aggregates whose argument is a column or `left OP right`.  specs = [(fn, op,
        (join, col), (join, col), result_dtype)] (make_agg_exprs) -> [python int or None]; an argument outside result_dtype
        for some output row: PolrError with code E_RANGE and .count"""
        res = (AggValue * len(specs))()
        oor = C.c_uint64()
        self.ctx.check_range(self.ctx.L.polr_out_aggregate_expr(self.h, stream, make_agg_exprs(specs), len(specs), res,
                                                                C.byref(oor)), oor)
        return [_agg_int(r) for r in res]

    def aggregate_grouped_expr(self, keys, specs, stream=None):
        """polr_out_aggregate_grouped_expr: keys as in aggregate_grouped, specs as in aggregate_expr -> (values, counts,
        n_dropped) as aggregate_grouped"""
        ka, n_groups = _group_keys(keys)
        na = len(specs)
        res = (AggValue * (n_groups * na))()
        dropped, oor = C.c_uint64(), C.c_uint64()
        self.ctx.check_range(self.ctx.L.polr_out_aggregate_grouped_expr(self.h, stream, ka, len(keys), make_agg_exprs(specs), na,
                                                                        res, n_groups, C.byref(dropped), C.byref(oor)), oor)
        return _agg_grid(res, n_groups, na) + (dropped.value,)

    def aggregate_hashed_expr(self, cols, specs, max_groups, str_cap=None, stream=None):
        """polr_out_aggregate_hashed_expr: the general GROUP BY (integer and VARCHAR group columns, as aggregate_hashed_str)
        with specs as in aggregate_expr -> {group key tuple: [value per aggregate]}"""
        return self._hashed(self.ctx.L.polr_out_aggregate_hashed_expr, cols, make_agg_exprs(specs), len(specs), max_groups,
                            stream, strings=True, str_cap=str_cap, ranged=True)

    def fuse_grouped(self, keys, specs):
        """polr_out_fuse_grouped: fold the join result into group cells inside the run (flat pipelines of perfect tables;
        COUNT(*) / COUNT / SUM).  keys / specs as in aggregate_grouped; keys=None un-fuses.  reset() zeroes the cells."""
        if keys is None:
            self.ctx.check(self.ctx.L.polr_out_fuse_grouped(self.h, None, 0, None, 0))
            self._fused = None
            return
        ka, n_groups = _group_keys(keys)
        self.ctx.check(self.ctx.L.polr_out_fuse_grouped(self.h, ka, len(keys), _agg_specs(specs), len(specs)))
        self._fused = (n_groups, len(specs))

    def fuse_aggregate(self, specs):
        """polr_out_fuse_aggregate: fold the join result into ungrouped aggregate cells inside the run (any pipeline; the
        generic pool kernel; COUNT(*) / COUNT / SUM / MIN / MAX over integer columns).  specs as in aggregate(); specs=None
        un-fuses.  reset() returns the cells to "no rows"; every pool run with this output adds to them."""
        if not specs:
            self.ctx.check(self.ctx.L.polr_out_fuse_aggregate(self.h, None, 0))
            self._fused_aggs = 0
            return
        self.ctx.check(self.ctx.L.polr_out_fuse_aggregate(self.h, _agg_specs(specs), len(specs)))
        self._fused_aggs = len(specs)

    def fused_aggregate_result(self, stream=None):
        """polr_out_fused_aggregate_result -> [python int or None], as aggregate()"""
        na = self._fused_aggs  # (0, no sink attached through this object: the call refuses)
        res = (AggValue * max(na, 1))()
        self.ctx.check(self.ctx.L.polr_out_fused_aggregate_result(self.h, stream, res, na))
        return [_agg_int(r) for r in res[:na]]

    def fused_result(self, stream=None):
        """polr_out_fused_result -> (values[n_groups][n_aggs], counts[n_groups][n_aggs], n_dropped), as aggregate_grouped"""
        n_groups, na = self._fused
        res = (AggValue * (n_groups * na))()
        dropped = C.c_uint64()
        self.ctx.check(self.ctx.L.polr_out_fused_result(self.h, stream, res, n_groups, C.byref(dropped)))
        return _agg_grid(res, n_groups, na) + (dropped.value,)

    def aggregate_string(self, fn, src_join, src_col, stream=None, cap=4096):
        """polr_out_aggregate_string: MIN / MAX of a VARCHAR column over the output rows -> bytes, or None (no non-NULL row)"""
        buf = C.create_string_buffer(cap)
        n, null = C.c_uint32(), C.c_uint32()
        self.ctx.check(self.ctx.L.polr_out_aggregate_string(self.h, stream, AGG[fn] if isinstance(fn, str) else fn, src_join,
                                                            src_col, buf, cap, C.byref(n), C.byref(null)))
        if null.value:
            return None
        if n.value > cap:
            return self.aggregate_string(fn, src_join, src_col, stream, cap=n.value)
        return buf.raw[:n.value]

    def materialize(self, src_join, src_col, dtype, stream=None):
        n, _, _ = self.stats(stream)
        data = np.zeros((n,), dtype=dtype)
        valid = np.ones((n,), dtype=np.uint8)
        self.ctx.check(self.ctx.L.polr_out_materialize(self.h, stream, src_join, src_col, data.ctypes.data,
                                                       valid.ctypes.data, n, 0))
        return data, valid

    def materialize_strings_raw(self, src_join, src_col, stream=None, heap_cap=None, device=False):
        """polr_out_materialize_strings -> (cells, valid, heap, heap_used): one string_t cell per output row (a V16 array),
        the validity bytes, and the packed heap the long cells point into.  heap_cap=None: the sizing call first, then one
        retry with the exact size; a heap_cap that is too small raises PolrError(E_OVERFLOW).  device=True: the three
        arrays are uint8 torch tensors on the context's device (cells [n, 16]) and the cells' pointers are device
        addresses inside `heap`; otherwise numpy arrays, the pointers host addresses inside `heap`."""
        n, _, _ = self.stats(stream)
        used = C.c_uint64()
        if device:
            import torch
            dev = torch.device("cuda", torch.cuda.current_device())

            def alloc(shape, fill=0):
                t = torch.full(shape, fill, dtype=torch.uint8, device=dev)
                torch.cuda.synchronize()
                return t, t.data_ptr()
        else:
            def alloc(shape, fill=0):
                a = np.full(shape, fill, dtype=np.uint8)
                return a, a.ctypes.data
        cells, p_cells = alloc((n, 16))
        valid, p_valid = alloc((n,), 1)
        sizing = heap_cap is None
        for cap in (0, None) if sizing else (int(heap_cap),):
            if cap is None:
                cap = used.value
            heap, p_heap = alloc((cap,))
            rc = self.ctx.L.polr_out_materialize_strings(self.h, stream, src_join, src_col, p_cells, p_valid, n,
                                                         p_heap if cap else None, cap, C.byref(used),
                                                         COL_DEVICE if device else 0)
            if not (sizing and cap == 0 and rc == E_OVERFLOW):  # (the sizing call said how much: once more, with that)
                break
        self.ctx.check(rc)
        return (cells if device else cells.reshape(-1).view("V16")), valid, heap, used.value

    def materialize_strings(self, src_join, src_col, stream=None):
        """a VARCHAR column over the output rows -> [bytes or None (NULL)], decoded from the cells: inline strings from the
        cell, long ones through the pointer relative to the heap's address"""
        cells, valid, heap, used = self.materialize_strings_raw(src_join, src_col, stream)
        raw = cells.view(np.uint8).reshape(-1, 16)
        words = raw.view(np.uint32).reshape(-1, 4)
        ptr = raw.view(np.uint64).reshape(-1, 2)[:, 1]
        base, blob = heap.ctypes.data, heap.tobytes()
        out = []
        for i in range(len(raw)):
            if not valid[i]:
                out.append(None)
                continue
            ln = int(words[i, 0])
            if ln <= 12:
                out.append(raw[i, 4:4 + ln].tobytes())
            else:
                at = int(ptr[i]) - base
                if at < 0 or at + ln > used:
                    raise PolrError(E_INVALID, "row %d: cell points outside the heap" % i)
                out.append(blob[at:at + ln])
        return out

    def close(self):
        if self.h:
            self.ctx.L.polr_out_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceMultiplexer:
    def __init__(self, pipe, routing, chunk_size=1024, regret_budget=0.01, init_tuple_count=1024, atc_multiplier=1,
                 log_rounds=True, max_log_rounds=1 << 20):
        self.pipe = pipe
        self.ctx = pipe.ctx
        cfg = MpxConfig(ROUTING[routing] if isinstance(routing, str) else routing, chunk_size, regret_budget,
                        init_tuple_count, atc_multiplier, int(log_rounds), max_log_rounds)
        h = C.c_void_p()
        self.ctx.check(self.ctx.L.polr_mpx_create(pipe.h, C.byref(cfg), C.byref(h)))
        self.h = h
        self.max_log_rounds = max_log_rounds

    def set_chunk_offsets(self, offsets):
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        self.ctx.check(self.ctx.L.polr_mpx_set_chunk_offsets(self.h, offsets.ctypes.data, len(offsets) - 1))

    def use_scan_chunks(self):
        """source chunks = the pipeline's scan_filter result (device-resident boundaries)"""
        self.ctx.check(self.ctx.L.polr_mpx_use_scan_chunks(self.h))

    def run(self, chunk_begin, chunk_end, out=None, stream=None):
        self.ctx.check(self.ctx.L.polr_mpx_run(self.h, stream, chunk_begin, chunk_end, out.h if out else None))

    def run_resident(self, chunk_begin, chunk_end, out=None):
        """the same run as one launch (polr_mpx_run_resident with this single executor)"""
        run_resident([self], [(chunk_begin, chunk_end)], out)

    def finish(self, stream=None):
        st = MpxStats()
        self.ctx.check(self.ctx.L.polr_mpx_finish(self.h, stream, C.byref(st)))
        return _stats_dict(st, self.pipe.n_paths, self.pipe.k)

    def steal_stats(self):
        """polr_mpx_steal_stats: this executor's counters of its last run, after finish / finish_many (zeros unless that
        run was a run_resident_stealing)"""
        st = StealStats()
        self.ctx.check(self.ctx.L.polr_mpx_steal_stats(self.h, C.byref(st)))
        return {"chunks_routed": st.chunks_routed, "chunks_stolen": st.chunks_stolen, "n_steals": st.n_steals}

    def reset(self, stream=None):
        self.ctx.check(self.ctx.L.polr_mpx_reset(self.h, stream))

    def enable_timing(self, on=True):
        self.ctx.check(self.ctx.L.polr_mpx_enable_timing(self.h, int(on)))

    def kernel_time(self):
        ms, n = C.c_double(), C.c_uint64()
        self.ctx.check(self.ctx.L.polr_mpx_kernel_time(self.h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def fetch_log(self, stream=None):
        n = C.c_uint64()
        cap = self.max_log_rounds
        path = np.zeros((cap,), dtype=np.uint32)
        tuples = np.zeros((cap,), dtype=np.uint64)
        inter = np.zeros((cap,), dtype=np.uint64)
        self.ctx.check(self.ctx.L.polr_mpx_fetch_log(self.h, stream, path.ctypes.data, tuples.ctypes.data,
                                                     inter.ctypes.data, cap, C.byref(n)))
        m = n.value
        return path[:m].copy(), tuples[:m].copy(), inter[:m].copy()

    def close(self):
        if self.h:
            self.ctx.L.polr_mpx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def run_many(mpxs, ranges, out=None):
    """polr_mpx_run_many: mpxs[i] routes chunks ranges[i] = (begin, end) concurrently (own streams)"""
    n = len(mpxs)
    hs = _handles(mpxs)
    b = np.ascontiguousarray([r[0] for r in ranges], dtype=np.uint64)
    e = np.ascontiguousarray([r[1] for r in ranges], dtype=np.uint64)
    ctx = mpxs[0].ctx
    ctx.check(ctx.L.polr_mpx_run_many(hs, None, b.ctypes.data, e.ctypes.data, n, out.h if out else None))


def _stats_dict(st, P, k):
    return {"num_tuples_processed": st.num_tuples_processed, "num_intermediates": st.num_intermediates,
            "num_rounds": st.num_rounds,
            "input_tuple_count_per_path": [st.input_tuple_count_per_path[i] for i in range(P)],
            "path_resistances": [st.path_resistances[i] for i in range(P)],
            "stage_out": [[st.stage_out[i][j] for j in range(k)] for i in range(P)]}


RUN_RESET, RUN_FINISH = 1, 2


def _handles(mpxs):
    """the handle array the polr_mpx_*_many / _run_resident* entry points take"""
    return (C.c_void_p * len(mpxs))(*[m.h for m in mpxs])


def _run_flags(reset, finish, share):
    """POLR_RUN_RESET | POLR_RUN_FINISH | POLR_RUN_SHARE(share)"""
    return (RUN_RESET if reset else 0) | (RUN_FINISH if finish else 0) | ((share & 0xFF) << 8 if share > 1 else 0)


def run_resident(mpxs, ranges, out=None, reset=False, finish=False, share=1, stream=None):
    """polr_mpx_run_resident: the same run as ONE launch (device-resident routing loop);
    reset / finish fold polr_mpx_reset / the closing FinalizePathRun into the same launch"""
    ctx = mpxs[0].ctx
    n = len(mpxs)
    hs = _handles(mpxs)
    b = np.ascontiguousarray([r[0] for r in ranges], dtype=np.uint64)
    e = np.ascontiguousarray([r[1] for r in ranges], dtype=np.uint64)
    ctx.check(ctx.L.polr_mpx_run_resident(hs, stream, b.ctypes.data, e.ctypes.data, n, out.h if out else None,
                                          _run_flags(reset, finish, share)))


def pool_info(mpxs, out=None, share=1):
    """polr_mpx_pool_info: what run_resident*(mpxs, .., out=out, share=share) would plan under the context's tuning (grid,
    probe waves, the numbers that cut a round into units); launches nothing"""
    ctx = mpxs[0].ctx
    i = PoolInfo()
    ctx.check(ctx.L.polr_mpx_pool_info(_handles(mpxs), len(mpxs), out.h if out else None, _run_flags(False, False, share),
                                       C.byref(i)))
    return {f[0]: getattr(i, f[0]) for f in PoolInfo._fields_}


def run_resident_ranges(mpxs, range_lists, out=None, reset=False, finish=False, share=1):
    """polr_mpx_run_resident_ranges: range_lists[i] = [(begin, end), ...] of executor i (the same number for every one)"""
    ctx = mpxs[0].ctx
    n = len(mpxs)
    r = len(range_lists[0])
    hs = _handles(mpxs)
    flat = [x for lst in range_lists for x in lst]
    b = (C.c_uint64 * (n * r))(*[x[0] for x in flat])
    e = (C.c_uint64 * (n * r))(*[x[1] for x in flat])
    ctx.check(ctx.L.polr_mpx_run_resident_ranges(hs, None, b, e, r, n, out.h if out else None,
                                                 _run_flags(reset, finish, share)))


def run_resident_morsels(mpxs, chunk_begin, chunk_end, morsel_chunks=120, out=None, reset=False, finish=False, share=1):
    """polr_mpx_run_resident_morsels: the executors share [chunk_begin, chunk_end) and pull morsels from one cursor"""
    ctx = mpxs[0].ctx
    n = len(mpxs)
    hs = _handles(mpxs)
    ctx.check(ctx.L.polr_mpx_run_resident_morsels(hs, None, chunk_begin, chunk_end, morsel_chunks, n,
                                                  out.h if out else None,
                                                  _run_flags(reset, finish, share)))


def run_resident_stealing(mpxs, ranges, grant_chunks, out=None, reset=False, finish=False, share=1):
    """polr_mpx_run_resident_stealing: mpxs[i] owns the chunks ranges[i] = (begin, end) (pairwise disjoint, may be empty)
    and takes them grant_chunks at a time; an executor that has run dry steals the far half of whoever has most left"""
    ctx = mpxs[0].ctx
    n = len(mpxs)
    hs = _handles(mpxs)
    b = np.ascontiguousarray([r[0] for r in ranges], dtype=np.uint64)
    e = np.ascontiguousarray([r[1] for r in ranges], dtype=np.uint64)
    ctx.check(ctx.L.polr_mpx_run_resident_stealing(hs, None, b.ctypes.data, e.ctypes.data, grant_chunks, n,
                                                   out.h if out else None,
                                                   _run_flags(reset, finish, share)))


def run_backpressure(mpxs, chunk_begin, chunk_end, morsel_chunks=120, out=None, reset=True, finish=True):
    """polr_mpx_run_backpressure: one executor per join order racing for morsels of the source"""
    ctx = mpxs[0].ctx
    n = len(mpxs)
    hs = _handles(mpxs)
    ctx.check(ctx.L.polr_mpx_run_backpressure(hs, None, chunk_begin, chunk_end, morsel_chunks, out.h if out else None,
                                              _run_flags(reset, finish, 1)))


def finish_many_raw(mpxs):
    """polr_mpx_finish_many: settles the run(s) of these multiplexers and returns their statistics as the C structs
    (stats_dicts() turns them into dictionaries -- host-side bookkeeping a measurement keeps outside its clock)"""
    n = len(mpxs)
    hs = _handles(mpxs)
    stats = (MpxStats * n)()
    ctx = mpxs[0].ctx
    ctx.check(ctx.L.polr_mpx_finish_many(hs, n, stats))
    return stats


def stats_dicts(stats, mpxs):
    return [_stats_dict(stats[i], mpxs[i].pipe.n_paths, mpxs[i].pipe.k) for i in range(len(mpxs))]


def finish_many(mpxs):
    return stats_dicts(finish_many_raw(mpxs), mpxs)


COMM_ID_BYTES = 128


def comm_unique_id():
    """polr_comm_get_unique_id: 128 bytes made on ONE rank, to be shipped to the others out of band"""
    L = load()
    buf = (C.c_uint8 * COMM_ID_BYTES)()
    rc = L.polr_comm_get_unique_id(buf)
    if rc != OK:
        raise PolrError(rc, "polr_comm_get_unique_id failed (is librccl.so present?)")
    return bytes(buf)


class Comm:
    """RCCL communicator of the library (one rank per GPU) for polr_bcast_build, the path's one exchange step"""

    def __init__(self, ctx, unique_id, world_size, rank):
        self.ctx = ctx
        buf = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(unique_id)
        h = C.c_void_p()
        ctx.check(ctx.L.polr_comm_create(ctx.h, buf, world_size, rank, C.byref(h)))
        self.h = h
        self.rank = rank

    def bcast_build(self, ht, root=0, stream=None):
        """root: ht is the finalized HashTable to send (returned unchanged); other ranks: pass None, get a new one"""
        h = C.c_void_p(ht.h.value if ht is not None else None)
        self.ctx.check(self.ctx.L.polr_bcast_build(self.h, C.byref(h), root, stream))
        return ht if self.rank == root else HashTable(self.ctx, h)

    def bytes_broadcast(self):
        n = C.c_uint64()
        self.ctx.check(self.ctx.L.polr_comm_bytes_broadcast(self.h, C.byref(n)))
        return n.value

    def close(self):
        if self.h:
            self.ctx.L.polr_comm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def string_payload_index(j, col):
    """payload column number of VARCHAR column `col` of workload join `j` as build_joins uploads it"""
    return len(j["payload"]) + list(j.get("strings", {}).keys()).index(col)


def dictionary_payload_index(j, col):
    """(payload column number of the code column of VARCHAR column `col` of workload join `j`, (n_codes, has_null)) as
    build_joins made it for j["dictionary"]"""
    return j["dictionary_cols"][col]


def build_joins(ctx, wl, auto=False):
    """upload + finalize the build sides of a workload dict.  auto=False: the way the reference's planner would
    (perfect table where the plan allows it and the build has no duplicate, hash table otherwise);
    auto=True: polr_ht_finalize_auto with the key column's min/max statistics (dense unique keys of any range
    become perfect tables)."""
    joins = []
    for j in wl["joins"]:
        pv = [j.get("payload_valid", {}).get(n) for n in j["payload"].keys()]
        # VARCHAR payload columns (j["strings"]: name -> bytes per build row) go behind the fixed-width ones, as 16-byte
        # string_t cells + one heap each (string_payload_index gives their column number); j["strings_valid"]: name ->
        # validity bytes of such a column (absent: no NULLs)
        strs = [string_cells(v) for v in j.get("strings", {}).values()]
        ht = HashTable.from_columns(ctx, j["keys"], list(j["payload"].values()) + [c for c, _h in strs],
                                    key_valid=j.get("key_valid"),
                                    payload_valid=pv + [j.get("strings_valid", {}).get(n) for n in j.get("strings", {})])
        for i, (_c, heap) in enumerate(strs):
            ht.set_payload_heap(len(j["payload"]) + i, heap)
        # j["dictionary"]: names of j["strings"] columns to dictionary-encode (HashTable.encode_dictionary: one code column
        # each, behind all the others; dictionary_payload_index gives its column number and (n_codes, has_null))
        if j.get("dictionary"):
            j["dictionary_cols"] = {}
            # j["dictionary_flags"] = {name: DICT_SORTED | DICT_NULL_INVALID}: the flags of polr_ht_encode_dictionary_ex
            for col in j["dictionary"]:
                flags = (j.get("dictionary_flags") or {}).get(col, 0)
                if flags:
                    code_col, n_codes, has_null = ht.encode_dictionary(string_payload_index(j, col), flags=flags)
                else:
                    code_col, n_codes, has_null = ht.encode_dictionary(string_payload_index(j, col))
                j["dictionary_cols"][col] = (code_col, (n_codes, has_null))
        # j["key_flags"]: per key column KEY_BY_VALUE (the probe side reads another integer type: a CAST'ed key) and / or
        # KEY_NULL_EQUAL (IS NOT DISTINCT FROM)
        for c, f in enumerate(j.get("key_flags", [])):
            if f:
                ht.set_key_flags(c, f)
        done = False
        if auto and not any(j.get("key_flags", [])) and len(j["keys"]) == 1 and j["keys"][0].dtype.kind in "iu" and len(j["keys"][0]):
            kv = j.get("key_valid")
            kk = j["keys"][0] if not kv or kv[0] is None else j["keys"][0][kv[0].astype(bool)]
            if len(kk):
                ht.finalize_auto(int(kk.min()), int(kk.max()))
                done = True
        if not done and j.get("perfect") is not None:
            done = ht.finalize_perfect(*j["perfect"])
        if not done:
            ht.finalize_hash()
        # conditions: (op, (src_join, src_col), build column NAME) -- a fixed-width payload column, or for "str_eq" one of the
        # join's VARCHAR columns (their column numbers: string_payload_index)
        names = list(j["payload"].keys())
        ht.preds = [(op, src, names.index(col) if col in names else string_payload_index(j, col))
                    for op, src, col in j.get("preds", [])]
        joins.append((ht, j["key_src"]))
    return joins
