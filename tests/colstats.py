"""The numpy twin of polr_ht_column_stats / polr_pipeline_column_stats (include/polr_hip.h): what the device must return for
a column, as the dict capi.HashTable.column_stats gives.  A few lines per width and kind; tests/test_colstats_abi.py checks
it against hand-written cases, the GPU tests compare every device result with it."""
import numpy as np

SIGNED = 1  # POLR_COL_SIGNED


def as_i64(x):
    """a Python integer as the int64 bit pattern the ABI returns it in"""
    x = int(x) & (2 ** 64 - 1)
    return x - 2 ** 64 if x >= 2 ** 63 else x


def lengths(cells):
    """the length words of a VARCHAR column (capi.string_cells: one V16 cell per value)"""
    return np.ascontiguousarray(cells).view(np.uint8).reshape(-1, 16)[:, :4].copy().view(np.uint32).reshape(-1)


def reference(col, valid=None, rows=None):
    """col: an integer numpy array (its dtype is the column's type) or V16 string cells; valid: validity bytes or None; rows:
    the selection (row numbers, any order, repeats allowed) or None for every row"""
    col = np.ascontiguousarray(col)
    is_str = col.dtype.itemsize == 16
    vals = lengths(col) if is_str else col
    ok = np.ones(len(vals), dtype=bool) if valid is None else np.asarray(valid).astype(bool)
    if rows is not None:
        rows = np.asarray(rows, dtype=np.int64)
        vals, ok = vals[rows], ok[rows]
    live = vals[ok]  # compared in the dtype's own order: signed as signed, unsigned as unsigned
    st = {"min_value": 0, "max_value": 0, "n_rows": len(vals), "n_valid": len(live), "n_long": 0, "long_bytes": 0,
          "width": col.dtype.itemsize, "flags": SIGNED if col.dtype.kind == "i" else 0}
    if len(live):
        st["min_value"], st["max_value"] = as_i64(live.min()), as_i64(live.max())  # (an unsigned 8-byte value: its bit pattern)
    if is_str:
        long = live[live > 12]
        st["n_long"], st["long_bytes"] = len(long), int(long.astype(np.uint64).sum())
    return st
