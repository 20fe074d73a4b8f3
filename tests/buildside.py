"""The three routes by which a build side reaches the device without HashTable.from_columns, restated in plain numpy for
tests/test_gpu_build_routes.py (and checked against the oracle, without a GPU, by tests/test_buildside_helpers.py):

  row_blob        the reference's row format (oracle/polr_oracle.c, orc_ht_build2), what polr_ht_upload_rows takes
  perfect_arrays  what PerfectHashJoinExecutor leaves (bool bitmap, re-ordered payload cells), what polr_pht_upload takes
  clone           export -> alloc_like -> a device-to-device copy of every buffer, what polr_bcast_build does on a
                  receiving rank

and key_codes: composite keys, NULL = NULL columns included, reduced to one integer code per row, so that joinref.Ref
(one key column per join) is the reference of those joins too."""
import ctypes as C

import numpy as np

from joinref import U64
from polr_amd import capi

TRAILER = 8  # bytes behind the last cell of a row: the chain pointer of the reference's table, a host address


def _ok(valid, n):
    return np.ones(n, bool) if valid is None else np.asarray(valid).astype(bool)


def _flags(null_equal, n_keys):
    return [bool(null_equal[c]) if c < len(null_equal) else False for c in range(n_keys)]


def row_blob(keys, key_valid, payload, payload_valid, null_equal=()):
    """-> (blob uint8[kept * row_width], row_width, col_offset[n_cols], kept_rows).  Per row: (n_cols + 1 + 7) // 8 validity
    bytes, all ones but the bits of the NULL cells; key cells, then payload cells, unaligned, NULL cells zeroed; 8 trailing
    bytes (never zero here: the device must not read them).  null_equal: one flag per key column (missing: False); a row
    with a NULL key in a column without the flag is left out, kept_rows[blob ordinal] = input row."""
    keys = [np.ascontiguousarray(k) for k in keys]
    payload = [np.ascontiguousarray(p) for p in payload]
    n = len(keys[0])
    kv = [_ok(v, n) for v in (key_valid or [None] * len(keys))]
    pv = [_ok(v, n) for v in (payload_valid or [None] * len(payload))]
    keep = np.ones(n, bool)
    for ok, ne in zip(kv, _flags(null_equal, len(keys))):
        if not ne:
            keep &= ok
    kept = np.nonzero(keep)[0]
    cols, oks = keys + payload, kv + pv
    flag_bytes = (len(cols) + 1 + 7) // 8
    col_offset, w = [], flag_bytes
    for col in cols:
        col_offset.append(w)
        w += col.dtype.itemsize
    row_width = w + TRAILER
    blob = np.zeros((len(kept), row_width), np.uint8)
    blob[:, :flag_bytes] = 0xFF
    for c, (col, ok) in enumerate(zip(cols, oks)):
        width = col.dtype.itemsize
        ok = ok[kept]
        cells = np.ascontiguousarray(col[kept]).view(np.uint8).reshape(len(kept), width)
        blob[:, col_offset[c]:col_offset[c] + width] = np.where(ok[:, None], cells, 0)
        blob[~ok, c >> 3] &= 0xFF ^ (1 << (c & 7))
    blob[:, w:] = np.arange(0xA1, 0xA1 + TRAILER, dtype=np.uint8)
    return blob.reshape(-1), row_width, col_offset, kept


def col_shape(cols):
    """(col_width, col_signed) of numpy columns, as HashTable.from_rows takes them"""
    return [c.dtype.itemsize for c in cols], [c.dtype.kind == "i" for c in cols]


def perfect_arrays(keys, key_valid, payload, payload_valid, lo, hi):
    """-> (bitmap uint8[range + 1], cells per payload column, cell_valid per payload column, id_to_row int64[range + 1]).
    Slot key - lo of every valid key inside [lo, hi] is set and holds that row's payload cells (a NULL cell: zero and
    invalid); unset slots are zero, invalid, and id_to_row -1.  A uint64 range is given as int64 bit patterns (lo and hi
    are reduced modulo 2^64).  The keys are unique."""
    keys = np.ascontiguousarray(keys)
    n = len(keys)
    size = ((int(hi) - int(lo)) & U64) + 1
    off = keys.astype(np.uint64) - np.uint64(int(lo) & U64)  # (modulo 2^64, whatever the key's sign)
    inside = _ok(key_valid, n) & (off < np.uint64(size))
    rows = np.nonzero(inside)[0]
    idx = off[rows].astype(np.int64)
    assert len(np.unique(idx)) == len(idx), "a perfect table takes unique keys"
    bitmap = np.zeros(size, np.uint8)
    bitmap[idx] = 1
    id_to_row = np.full(size, -1, np.int64)
    id_to_row[idx] = rows
    cells, cell_valid = [], []
    for p, v in zip(payload, payload_valid or [None] * len(payload)):
        p = np.ascontiguousarray(p)
        ok = _ok(v, n)[rows]
        c = np.zeros(size, p.dtype)
        c[idx[ok]] = p[rows[ok]]
        cv = np.zeros(size, np.uint8)
        cv[idx] = ok
        cells.append(c)
        cell_valid.append(cv)
    return bitmap, cells, cell_valid, id_to_row


def _d2d(dst, src, n):
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(dst, src, n, 3) == 0


def clone(ctx, ht):
    """export -> alloc_like -> every buffer copied device to device: a table that shares nothing with `ht`"""
    meta, bufs = ht.export()
    twin = capi.HashTable.alloc_like(ctx, meta)
    meta2, bufs2 = twin.export()
    assert len(meta2) == len(meta)
    assert [n for _, n in bufs2] == [n for _, n in bufs]
    for (src, n), (dst, _) in zip(bufs, bufs2):
        assert src and dst and dst != src
        _d2d(dst, src, n)
    return twin


def key_codes(build_keys, build_valid, probe_keys, probe_valid, null_equal=()):
    """Composite keys -> one int64 code per row: (build codes, build row takes part, probe codes, probe row takes part).
    Equal codes = equal keys, column by column and by value; in a null_equal column NULL is a value of its own, in any
    other a NULL takes the row out.  (Columns of one key are compared as int64, a uint64 column by its bit pattern.)"""
    nb, npr = len(build_keys[0]), len(probe_keys[0])
    ne = _flags(null_equal, len(build_keys))
    bok, pok = np.ones(nb, bool), np.ones(npr, bool)
    parts = []
    for c, (b, p) in enumerate(zip(build_keys, probe_keys)):
        bv = _ok(build_valid[c] if build_valid else None, nb)
        pv = _ok(probe_valid[c] if probe_valid else None, npr)
        if not ne[c]:
            bok &= bv
            pok &= pv
        null = np.concatenate([~bv, ~pv])
        both = np.concatenate([np.asarray(b).astype(np.int64), np.asarray(p).astype(np.int64)])
        parts += [null.astype(np.int64), np.where(null, 0, both)]
    _, inv = np.unique(np.column_stack(parts), axis=0, return_inverse=True)
    inv = inv.reshape(-1).astype(np.int64)
    return inv[:nb], bok, inv[nb:], pok
