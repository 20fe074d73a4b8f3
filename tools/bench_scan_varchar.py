"""Times the device source scan with pushed-down VARCHAR filters (polr_pipeline_scan_filter_str) against the integer scan
on the same pipeline.
usage: python tools/bench_scan_varchar.py <duckdb-polr_amd tree> <tag> [log2 rows, default 26]   -> one JSON line per case
(host clock around the C call, which ends in a synchronise: 3 warm-up calls, then 9 timed ones; median, min, max; bytes/s =
the algorithmic bytes of DESIGN section 4 over the median).  The tree is where the library AND its binding are taken from,
so that the integer case -- the yardstick -- also runs on a build from before the VARCHAR filters, which skips the
string cases.  (alg_bytes and GBps are those of this tree's scan -- every column once, plus the pass bits --, also
when the tree named is an older one that reads its columns twice: compare the times.)  To compare two builds, run it on each, alternating, one process each.  Cases:
  int8_lt        one filter on an 8-byte integer column (the yardstick)
  inline_eq      = on an inline-only VARCHAR column, about 1 % of the rows pass (first without a heap handed over: the call
                 then counts the column's long cells before it scans; then with one)
  like_heap      a LIKE range on a column where 30 % of the rows are 24-byte heap strings that share the constant's first four
                 bytes, every row with its own heap copy
n_selected of every case is checked against the count computed from the vocabulary.  Results: profiles/README.md"""
import json
import os
import sys
import time

import numpy as np

TREE = os.path.abspath(sys.argv[1])
TAG = sys.argv[2]
LOG2 = int(sys.argv[3]) if len(sys.argv) > 3 else 26
sys.path.insert(0, os.path.join(TREE, "python"))
from polr_amd import capi  # noqa: E402

assert os.path.dirname(capi.LIB_PATH) == TREE, capi.LIB_PATH
REPS, WARM = 9, 3
HAS_STR = hasattr(capi, "like_pushdown")


def vocab_cells(words):
    """inline cells of a vocabulary (every word <= 12 bytes) -> (len(words), 16) uint8"""
    out = np.zeros((len(words), 16), np.uint8)
    for i, w in enumerate(words):
        assert len(w) <= 12
        out[i, 0:4] = np.frombuffer(np.uint32(len(w)).tobytes(), np.uint8)
        out[i, 4:4 + len(w)] = np.frombuffer(w, np.uint8)
    return out


def timed(fn):
    for _ in range(WARM):
        fn()
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return {"median_ms": round(ts[len(ts) // 2], 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4)}


def report(case, n, n_sel, alg_bytes, t, **more):
    print(json.dumps(dict({"tag": TAG, "case": case, "rows": n, "n_selected": int(n_sel), "alg_bytes": int(alg_bytes),
                           "GBps": round(alg_bytes / (t["median_ms"] * 1e-3) / 1e9, 1)}, **t, **more)), flush=True)


def main():
    n = 1 << LOG2
    rng = np.random.default_rng(26)
    pk = rng.integers(0, 1000, n).astype(np.int32)
    i8 = rng.integers(0, 1 << 40, n).astype(np.int64)
    # inline-only column: 100 words of 3..12 bytes, uniform -> one word is 1 % of the rows
    words = [b"w%02d" % i + b"abcdefghi"[:(i * 7) % 10] for i in range(100)]
    assert len(set(words)) == 100
    pick = rng.integers(0, 100, n)
    s_inline = vocab_cells(words)[pick].reshape(-1).view("V16")
    # heap column: 30 % of the rows are one of 64 strings of 24 bytes that begin with "Japa", each row with its own heap copy;
    # the rest the inline words
    longs = [b"Japa" + bytes([ord("m") + i % 3]) + b"-%02d-long-heap-string" % i for i in range(64)]
    longs = [w[:24] for w in longs]
    assert all(len(w) == 24 for w in longs)
    is_long = rng.random(n) < 0.30
    n_long = int(is_long.sum())
    lpick = rng.integers(0, 64, n_long)
    heap = np.frombuffer(b"".join(longs), np.uint8).reshape(64, 24)[lpick].reshape(-1).copy()
    s_heap = vocab_cells(words)[pick]
    lc = np.zeros((n_long, 16), np.uint8)
    lc[:, 0:4] = np.frombuffer(np.uint32(24).tobytes(), np.uint8)
    lc[:, 4:8] = np.frombuffer(b"Japa", np.uint8)
    lc[:, 8:16] = (np.uint64(heap.ctypes.data) + np.arange(n_long, dtype=np.uint64) * np.uint64(24)).view(np.uint8).reshape(-1, 8)
    s_heap[is_long] = lc
    s_heap = s_heap.reshape(-1).view("V16")
    ctx = capi.Context(0)
    ht = capi.HashTable.from_columns(ctx, [np.arange(1000, dtype=np.int32)], []).finalize_hash()
    pipe = capi.Pipeline(ctx, [pk, i8, s_inline, s_heap], n, [(ht, [(-1, 0)])], [[0]])
    pipe.set_probe_heaps(3, [heap])

    cut = 1 << 33  # 1 / 128 of the rows
    want = int((i8 < cut).sum())
    t = timed(lambda: pipe.scan_filter([(1, "<", cut)]))
    assert pipe.scan[0] == want, (pipe.scan, want)
    bits = 2 * n // 8  # the pass bits: written once, read once
    report("int8_lt", n, want, 8 * n + bits + 4 * want, t)
    if not HAS_STR:
        return
    word = words[37]
    want = int((pick == 37).sum())
    for case in ("inline_eq_no_heap_handed_over", "inline_eq"):
        if case == "inline_eq":
            pipe.set_probe_heaps(2, [np.zeros(1, np.uint8)])
        t = timed(lambda: pipe.scan_filter([(2, "=", word)]))
        assert pipe.scan[0] == want, (pipe.scan, want)
        guard = 4 * n if case != "inline_eq" else 0  # (the length words of the guard pass)
        report(case, n, want, 16 * n + bits + guard + 4 * want, t, constant=word.decode())
    f = capi.like_pushdown(b"Japan%")
    lo, hi = f[0][1], f[1][1]
    per_long = np.bincount(lpick, minlength=64)
    want = sum(int(c) for w, c in zip(longs, per_long) if lo <= w < hi) + \
        sum(int(c) for w, c in zip(words, np.bincount(pick[~is_long], minlength=100)) if lo <= w < hi)
    t = timed(lambda: pipe.scan_filter([(3, op, c) for op, c in f]))
    assert pipe.scan[0] == want, (pipe.scan, want)
    # heap bytes: both constants are 5 bytes long and tie with every long cell's prefix, so byte 4 decides: one byte per
    # constant (what the memory system moves for it is a whole sector of a row's own heap copy)
    report("like_heap", n, want, 16 * n + 2 * n_long + bits + 4 * want, t, pattern="Japan%", heap_rows=n_long)


if __name__ == "__main__":
    main()
