"""What the VARCHAR scan-filter tests share: the edge strings of the comparison, the seeded string column of the
tests/golden/scan_varchar.json fixture (the fixture stores the seed and the answers, never the strings), and the tests' own
reference -- Python's bytes comparison, which is memcmp over the shorter length with the shorter string first on a tie,
the order of the reference's StringComparisonOperators (comparison_operators.hpp:157-227)."""
import hashlib
import struct

import numpy as np

_S12 = b"twelve bytes"
_S40 = b"0123456789abcdefghijklmnopqrstuvwxyzABCD"
assert len(_S12) == 12 and len(_S40) == 40

# every ordered pair of these is compared (tests/test_str_compare.py on the host, tests/test_gpu_scan_varchar.py on the device)
EDGES = [
    b"", b"\0", b"a", b"ab", b"ab\0", b"ab\0\1", b"ab\1", b"abc", b"abcd", b"abcd\0", b"abcde",
    _S12, _S12 + b"!",                                  # 12 bytes inline; the same plus one byte: the first heap form
    _S12[:11] + b"zA", _S12[:11] + b"zB",               # two 13-byte strings that differ only in byte 12
    b"0123X" + _S40[5:], b"0123Y" + _S40[5:],           # 40 bytes: four bytes shared, different at byte 4
    _S40[:39] + b"y", _S40[:39] + b"z",                 # 40 bytes: different at the last byte
    _S40, _S40 + b"E",                                  # 40 bytes, a prefix of 41
    b"\x7f", b"\x80", b"\xff", b"\xff" * 5,
    bytes((i * 7 + 3) % 251 for i in range(300)),       # 300 bytes
]
OPS = ["=", "<>", "<", ">", "<=", ">="]


def holds(value, op, const):
    """value OP const on bytes; a NULL (None) passes nothing"""
    if value is None:
        return False
    return {"=": value == const, "<>": value != const, "<": value < const, ">": value > const, "<=": value <= const,
            ">=": value >= const}[op]


def passing(values, filters):
    """rows of `values` (bytes or None) that pass every (op, const) of filters (AND); "is null" / "is not null" too"""
    out = []
    for i, v in enumerate(values):
        ok = True
        for op, c in filters:
            ok = ok and ((v is None) if op == "is null" else (v is not None) if op == "is not null" else holds(v, op, c))
        if ok:
            out.append(i)
    return np.asarray(out, dtype=np.uint32)


def chunks_of(sel, n_rows, vector_size):
    """the scan's chunk boundaries for a selection: one chunk per vector with a survivor -> offsets[n_chunks + 1]"""
    counts = np.bincount(np.asarray(sel, dtype=np.int64) // vector_size, minlength=(n_rows + vector_size - 1) // vector_size)
    counts = counts[counts > 0]
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)


def rows_digest(rows):
    """how the fixture records a row set: count and SHA-1 of the ascending row ids as little-endian uint32"""
    rows = np.asarray(rows, dtype="<u4")
    return {"count": int(len(rows)), "sha1": hashlib.sha1(rows.tobytes()).hexdigest()}


def column_digest(values):
    """SHA-1 over a column (bytes or None per row): tells a drifted generator from a wrong comparison"""
    return hashlib.sha1(b"".join(b"\xff" if v is None else struct.pack("<I", len(v)) + v for v in values)).hexdigest()


def write_edges(path, strings=EDGES):
    """u32 n, then n x (u32 length, bytes): what tests/strcmp/str_cmp_main.cpp reads"""
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(strings)))
        for s in strings:
            f.write(struct.pack("<I", len(s)) + s)


# ---- the fixture's column ----------------------------------------------------------------------------------------
FIXTURE_SEED, FIXTURE_ROWS = 20261018, 5000
_STEMS = ["Japan", "Jap", "Japanese", "Jamaica", "J", "Tokyo", "Tok", "tokyo", "München", "Mün", "Zürich", "日本", "日本語",
          "東京都", "naïve", "😀", "😀😁", "A", "", "character-name-in-title", "character", "char", "Ünited", "(voice)",
          "(voice: English version)", "(uncredited)"]
_FILL = ["a", "b", "z", " ", "é", "ü", "語", "😀", "0", "-"]


def fixture_column(seed=FIXTURE_SEED, n=FIXTURE_ROWS):
    """-> [bytes or None] * n: valid UTF-8 with 2-, 3- and 4-byte sequences, lengths 0..60 clustered around 4, 12 and 13,
    many shared prefixes, about 5 % NULLs"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        if rng.random() < 0.05:
            out.append(None)
            continue
        target = [4, 12, 13, int(rng.integers(0, 61))][int(rng.integers(0, 4))] + int(rng.integers(-1, 2))
        target = min(max(target, 0), 60)
        s = _STEMS[int(rng.integers(0, len(_STEMS)))]
        while len(s.encode()) < target:
            s += _FILL[int(rng.integers(0, len(_FILL)))]
        b = s.encode()
        while len(b) > target:  # cut back to whole characters
            s = s[:-1]
            b = s.encode()
        out.append(b)
    return out


def cells(values, n_blocks=1, null_cell=b"ab", dirty_seed=None):
    """string_t cells for a column (bytes or None per row) -> (V16 cells, validity uint8 or None, [heap blocks]): the long
    strings go to n_blocks separate host arrays in turn (hand them over with Pipeline.set_probe_heaps).  A NULL row holds
    `null_cell` -- bytes: that string as an inline cell; a V16 scalar: that cell -- so a scan that read NULL cells would pass
    rows it must not.  dirty_seed: the padding of every inline cell is filled with non-zero garbage."""
    parts, sizes, where = [[] for _ in range(n_blocks)], [0] * n_blocks, {}
    n_long = 0
    for i, v in enumerate(values):
        if v is not None and len(v) > 12:
            b = n_long % n_blocks
            n_long += 1
            where[i] = (b, sizes[b])
            parts[b].append(v)
            sizes[b] += len(v)
    blocks = [np.frombuffer(b"".join(p) + b"\x00", np.uint8).copy() for p in parts]  # (+1: never empty)
    bases = [b.ctypes.data for b in blocks]
    garbage = np.random.default_rng(dirty_seed).integers(1, 256, 12 * len(values), dtype=np.uint8).tobytes() \
        if dirty_seed is not None else bytes(12 * len(values))
    raw = bytearray()
    for i, v in enumerate(values):
        if v is None and not isinstance(null_cell, bytes):
            raw += bytes(null_cell)
            continue
        s = null_cell if v is None else v
        if len(s) <= 12:
            raw += struct.pack("<I", len(s)) + s + garbage[12 * i + len(s):12 * i + 12]
        else:
            b, off = where[i]
            raw += struct.pack("<I4sQ", len(s), s[:4], bases[b] + off)
    raw = np.frombuffer(bytes(raw), np.uint8).copy()
    valid = None if all(v is not None for v in values) else np.array([v is not None for v in values], np.uint8)
    return raw.reshape(-1).view("V16"), valid, blocks
