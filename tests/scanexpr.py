"""What the expression-filter tests share (polr_pipeline_scan_filter_expr): the tests' own evaluator of a filter expression
-- SQL three-valued logic in numpy, IN by bytes equality, LIKE through a bytes regular expression ('%' -> '.*', '_' -> '.',
the rest escaped; DOTALL, fullmatch: '_' is one BYTE) -- and the pattern / string edge set of LIKE.  The evaluator is pinned
against the reference engine by tests/test_scan_expr_golden.py.  Expressions are the nested tuples of
polr_amd.capi.Pipeline.scan_filter_expr; a column is a list of bytes / None (VARCHAR) or (ndarray, validity or None)."""
import re

import numpy as np

import scanstr
from scanstr import cells, chunks_of, fixture_column, rows_digest  # noqa: F401  (what the tests take from here)

_S12, _S40 = scanstr._S12, scanstr._S40

LIKE_STRINGS = list(scanstr.EDGES) + [
    b"abab", b"ababab", b"aab", b"aba", b"Munchen", "München".encode(), "日本語".encode(),
    b"(2006) (USA) (TV) (worldwide)", b"(as Metro-Goldwyn-Mayer Pictures)", b"(voice: Japanese version) (uncredited)",
    b"(2007) (worldwide) (all media)", b"(presents) (2001) (USA) (DVD)", b"(USA) (2003) (co-production)",
]
LIKE_PATTERNS = [
    b"", b"%", b"%%", b"_", b"__", b"%_", b"_%",
    b"a%", b"%a", b"%a%", b"a%a", b"%ab%ab", b"%ab%b", b"a_c",
    b"%_b_%",
    b"abcd%", b"abcde%", b"0123%", b"0123X%",           # front-anchored literals of 4 and 5 bytes: the prefix word of a long cell
    _S12 + b"!",                                        # 13 bytes, no wildcard
    b"%" + _S12 + b"!" + b"%",
    b"y" * 301, b"%" + b"y" * 301,                      # longer than every string
    b"M_nchen", b"M__nchen",                            # against München: '_' is a byte
    "%語%".encode(),
    b"%abcde%",                                         # bytes 10-14 of the 40-byte string: straddles byte 12
    b"%ABCD%", b"%D",                                   # occurs only at the very end
    b"%ab", b"ab%ab",                                   # the segment occurs twice, only the second occurrence ends the string
    b"%(200%)%", b"%(USA)%", b"%(200_) (USA)%", b"(%) (%)", b"%\\%", b"ab\x01",
]
LIKE_EDGES = {"patterns": LIKE_PATTERNS, "strings": LIKE_STRINGS}


def like_regex(pattern):
    out = b""
    for b in bytes(pattern):
        ch = bytes([b])
        out += b".*" if ch == b"%" else b"." if ch == b"_" else re.escape(ch)
    return re.compile(out, re.DOTALL)


def like(value, pattern):
    """value LIKE pattern on bytes (no ESCAPE); None for a NULL"""
    if value is None:
        return None
    return like_regex(pattern).fullmatch(value) is not None


def _bytes(c):
    return c.encode() if isinstance(c, str) else bytes(c)


def _str_leaf(col, fn):
    """(true, null) arrays of a VARCHAR leaf: fn(bytes) -> bool, evaluated once per distinct string"""
    memo = {}
    t = np.zeros(len(col), bool)
    n = np.zeros(len(col), bool)
    for i, v in enumerate(col):
        if v is None:
            n[i] = True
            continue
        r = memo.get(v)
        if r is None:
            r = memo[v] = bool(fn(v))
        t[i] = r
    return t, n


_STR_OPS = {0: lambda a, b: a == b, 1: lambda a, b: a != b, 2: lambda a, b: a < b, 3: lambda a, b: a > b,
            4: lambda a, b: a <= b, 5: lambda a, b: a >= b}
_CODES = {"=": 0, "==": 0, "!=": 1, "<>": 1, "<": 2, ">": 3, "<=": 4, ">=": 5, "is null": 6, "is not null": 7}


def _validity(col):
    if isinstance(col, tuple):
        data, valid = col
        return np.ones(len(data), bool) if valid is None else np.asarray(valid).astype(bool)
    return np.array([v is not None for v in col], bool)


def evaluate(expr, cols):
    """-> (true, null): two bool arrays over the rows; a row passes a WHERE when `true`"""
    kind = expr[0]
    if kind == "not":
        t, n = evaluate(expr[1], cols)
        return ~t & ~n, n
    if kind in ("and", "or"):
        t, n = evaluate(expr[1], cols)
        for e in expr[2:]:
            t2, n2 = evaluate(e, cols)
            if kind == "and":
                false = (~t & ~n) | (~t2 & ~n2)
                t, n = t & t2, (n | n2) & ~false
            else:
                t = t | t2
                n = (n | n2) & ~t
        return t, n
    col = cols[expr[1]]
    valid = _validity(col)
    if kind == "cmp":
        op = _CODES[expr[2]] if isinstance(expr[2], str) else expr[2]
        if op == 6:
            return ~valid, np.zeros(len(valid), bool)
        if op == 7:
            return valid, np.zeros(len(valid), bool)
        if isinstance(col, tuple):
            a, c = col[0], expr[3]
            t = {0: a == c, 1: a != c, 2: a < c, 3: a > c, 4: a <= c, 5: a >= c}[op]
            return np.asarray(t, bool) & valid, ~valid
        c = _bytes(expr[3])
        return _str_leaf(col, lambda v: _STR_OPS[op](v, c))
    if kind == "in":
        if isinstance(col, tuple):
            return np.isin(col[0], np.asarray(list(expr[2]), dtype=col[0].dtype)) & valid, ~valid
        members = {_bytes(m) for m in expr[2]}
        return _str_leaf(col, lambda v: v in members)
    if kind == "like":
        rx = like_regex(_bytes(expr[2]))
        return _str_leaf(col, lambda v: rx.fullmatch(v) is not None)
    raise ValueError(kind)


def passing(expr, cols, n_rows):
    """the rows (ascending uint32) on which expr is TRUE; None: every row"""
    if expr is None:
        return np.arange(n_rows, dtype=np.uint32)
    return np.nonzero(evaluate(expr, cols)[0])[0].astype(np.uint32)


# ---- the tests/golden/scan_expr.json fixture: t(id INTEGER, s VARCHAR, i INTEGER) ----------------------------------------
def fixture_int(seed=scanstr.FIXTURE_SEED + 1, n=scanstr.FIXTURE_ROWS):
    """the fixture's integer column -> (int32 values 0..99, validity uint8 with about 10 % NULLs of its own)"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 100, n).astype(np.int32), (rng.random(n) >= 0.1).astype(np.uint8)


def bind(expr, columns):
    """a fixture expression (JSON: nested lists, column names, text constants) -> the nested tuples the evaluator and
    Pipeline.scan_filter_expr take, with columns[name] in place of every column name and text as UTF-8 bytes"""
    def const(c):
        return c.encode() if isinstance(c, str) else c
    kind = expr[0]
    if kind in ("and", "or", "not"):
        return (kind,) + tuple(bind(e, columns) for e in expr[1:])
    if kind == "cmp":
        return ("cmp", columns[expr[1]], expr[2]) + ((const(expr[3]),) if len(expr) > 3 else (None,))
    if kind == "in":
        return ("in", columns[expr[1]], [const(m) for m in expr[2]])
    return ("like", columns[expr[1]], const(expr[2]))
