"""SEMI / ANTI filters over a build side, restated in plain numpy: the reference of tests/test_gpu_ht_semi_filter.py, held to
the reference's own answers (tests/golden/semi_build.json) by tests/test_htsemi_golden.py.

  matches   does a row's key find at least one row of `by` -- np.isin over per-row key codes, with the NULL rules of the
            contract (include/polr_hip.h, polr_ht_semi_filter): a NULL never matches unless the column is NULL = NULL, a key
            that repeats in `by` counts once
  kept      the rows a list of filters keeps: SEMI the matching rows, ANTI the rest (rows whose key is NULL among them)
  fixture_tables / run_query   the tables of the fixture (seeded) and its query specs evaluated with the two above"""
import hashlib

import numpy as np

FIXTURE_SEED, FIXTURE_ROWS = 20261020, 2000
_WORDS = ["Japan", "Tokyo", "(voice)", "(uncredited)", "character-name-in-title", "", "J", "München"]


def _ok(valid, n):
    return np.ones(n, bool) if valid is None else np.asarray(valid).astype(bool)


def _codes(a, by_value):
    """a column as (high, low) int64 pairs that are equal iff the cells are: by value whatever the two types, or bit for bit"""
    a = np.ascontiguousarray(a)
    if by_value:
        high = (a > np.uint64(2 ** 63 - 1)) if a.dtype == np.uint64 else np.zeros(len(a), bool)
        return high.astype(np.int64), a.astype(np.int64)
    bits = a.view("u%d" % a.dtype.itemsize).astype(np.uint64).view(np.int64)
    return np.zeros(len(a), np.int64), bits


def matches(cols, valid, by_keys, by_valid=None, null_equal=(), by_value=()):
    """-> bool[n]: row r of the table (key columns `cols`, validity `valid`: a list of arrays or None) matches `by` (key
    columns by_keys).  null_equal / by_value: one flag per key column of `by` (missing: False)."""
    n, nb, nk = len(cols[0]), len(by_keys[0]), len(by_keys)
    assert len(cols) == nk
    ne = [bool(null_equal[c]) if c < len(null_equal) else False for c in range(nk)]
    bv_ = [bool(by_value[c]) if c < len(by_value) else False for c in range(nk)]
    t_ok, b_ok, parts = np.ones(n, bool), np.ones(nb, bool), []
    for c in range(nk):
        tv = _ok(valid[c] if valid else None, n)
        bv = _ok(by_valid[c] if by_valid else None, nb)
        if not ne[c]:
            t_ok &= tv
            b_ok &= bv
        null = np.concatenate([~bv, ~tv])
        bh, bl = _codes(by_keys[c], bv_[c])
        th, tl = _codes(cols[c], bv_[c])
        parts += [null.astype(np.int64), np.where(null, 0, np.concatenate([bh, th])), np.where(null, 0, np.concatenate([bl, tl]))]
    _, inv = np.unique(np.column_stack(parts), axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    return t_ok & np.isin(inv[nb:], inv[:nb][b_ok])


def kept(n, filters):
    """filters: [(cols, valid, by_keys, by_valid, anti, null_equal, by_value)] (the last two optional) -> bool[n]: kept by all"""
    keep = np.ones(n, bool)
    for f in filters:
        m = matches(f[0], f[1], f[2], f[3], *f[5:7])
        keep &= ~m if f[4] else m
    return keep


# ---- the fixture: d(id, k, k2, s) and the subquery tables a(x, y) -- repeated keys, one NULL key -- and b(x, y)
def fixture_tables(seed=FIXTURE_SEED, n=FIXTURE_ROWS):
    """-> {table: {column: (values, valid)}}; a VARCHAR column is a list of bytes"""
    rng = np.random.default_rng(seed)
    d = {"id": (np.arange(n, dtype=np.int32), np.ones(n, np.uint8)),
         "k": (rng.integers(0, 300, n).astype(np.int32), (rng.random(n) >= 0.05).astype(np.uint8)),
         "k2": (rng.integers(0, 20, n).astype(np.int32), (rng.random(n) >= 0.05).astype(np.uint8)),
         "s": ([_WORDS[i].encode() for i in rng.integers(0, len(_WORDS), n)], np.ones(n, np.uint8))}
    na, nb = 150, 120
    ax_valid = np.ones(na, np.uint8)
    ax_valid[17] = 0
    a = {"x": (rng.integers(0, 400, na).astype(np.int32), ax_valid),
         "y": (rng.integers(0, 20, na).astype(np.int32), np.ones(na, np.uint8))}
    a["x"][0][40:60] = a["x"][0][0:20]  # repeated keys for certain
    b = {"x": (rng.permutation(400)[:nb].astype(np.int32), np.ones(nb, np.uint8)),
         "y": (rng.integers(0, 20, nb).astype(np.int32), np.ones(nb, np.uint8))}
    return {"d": d, "a": a, "b": b}


def tables_digest(tables):
    h = hashlib.sha1()
    for t in sorted(tables):
        for c in sorted(tables[t]):
            values, valid = tables[t][c]
            h.update(b"".join(values) if isinstance(values, list) else np.ascontiguousarray(values).tobytes())
            h.update(np.ascontiguousarray(valid).tobytes())
    return h.hexdigest()


_CMP = {"<": np.less, "<=": np.less_equal, ">": np.greater, ">=": np.greater_equal, "=": np.equal, "<>": np.not_equal}


def const_mask(table, conds):
    """conds: [[column, op, constant] or [column, "is not null"]], all of them TRUE (a comparison with NULL is not)"""
    n = len(next(iter(table.values()))[0])
    keep = np.ones(n, bool)
    for cond in conds:
        values, valid = table[cond[0]]
        keep &= valid.astype(bool)
        if cond[1] != "is not null":
            keep &= _CMP[cond[1]](values, cond[2])
    return keep


def subquery_rows(tables, f):
    """the rows of filter f's subquery table that its WHERE keeps"""
    return np.nonzero(const_mask(tables[f["by"]], f.get("by_where", [])))[0]


def run_query(tables, q):
    """a query spec of the fixture -> the ascending ids of d it keeps.  q: {"const": conds over d, "filters": [{"by": table,
    "cols": columns of d, "by_cols": columns of the subquery table, "anti": bool, "by_where": conds over it}]}"""
    d = tables["d"]
    n = len(d["id"][0])
    keep = const_mask(d, q.get("const", []))
    fl = []
    for f in q["filters"]:
        rows = subquery_rows(tables, f)
        by = tables[f["by"]]
        fl.append(([d[c][0] for c in f["cols"]], [d[c][1] for c in f["cols"]], [by[c][0][rows] for c in f["by_cols"]],
                   [by[c][1][rows] for c in f["by_cols"]], bool(f.get("anti"))))
    return np.nonzero(keep & kept(n, fl))[0]
