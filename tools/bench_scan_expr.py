"""Times the device source scan with a filter expression (polr_pipeline_scan_filter_expr: OR / NOT trees, IN lists, LIKE)
and, as the yardstick, the AND-only programs that polr_pipeline_scan_filter_str evaluates too, on the same pipeline in the
same process.
usage: python tools/bench_scan_expr.py <duckdb-polr_amd tree> <tag> [log2 rows, default 26]   -> one JSON line per case
(host clock around the C call, which ends in a synchronise: 3 warm-up calls, then 9 timed ones; median, min, max; bytes/s =
the algorithmic bytes of DESIGN section 4 over the median).  The tree is where the library AND its binding are taken from,
so that the yardstick cases also run on a build from before the expression scan, which skips the rest.  (alg_bytes and
GBps are those of this tree's scan -- every column once, plus the pass bits --, also when the tree named is an older one
whose yardstick entry points read their columns twice: compare the times.)  To compare two
builds, run it on each, alternating, one process each.  Cases:
  inline_eq/str, like_heap/str   the cases of tools/bench_scan_varchar.py through scan_filter_str (the yardstick)
  inline_eq/expr, like_heap/expr the same filters as AND-only programs
  contains_heap   LIKE '%(200%)%' on a column where 30 % of the rows are 24-40-byte heap notes, every row with its own copy
  in8_inline      IN of 8 inline members on the inline-only column
  job19a          the mc.note and mi.info predicates of JOB 19a as one expression over two columns:
                  note IS NOT NULL AND (note LIKE '%(USA)%' OR note LIKE '%(worldwide)%') AND
                  info IS NOT NULL AND (info LIKE 'Japan:%200%' OR info LIKE 'USA:%200%')
n_selected of every case is checked against the count computed from the vocabulary.  Results: profiles/README.md"""
import json
import os
import re
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
HAS_EXPR = hasattr(capi.Pipeline, "scan_filter_expr")


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


def column(vocab, pick, stride):
    """cells of vocab[pick]: words of up to 12 bytes inline, longer ones as a pointer to the row's own copy in a heap of
    `stride` bytes per long row -> (V16 cells, heap, the long rows' mask)"""
    n_words = len(vocab)
    cells = np.zeros((n_words, 16), np.uint8)
    padded = np.zeros((n_words, stride), np.uint8)
    for i, w in enumerate(vocab):
        assert len(w) <= stride
        cells[i, 0:4] = np.frombuffer(np.uint32(len(w)).tobytes(), np.uint8)
        head = w if len(w) <= 12 else w[:4]
        cells[i, 4:4 + len(head)] = np.frombuffer(head, np.uint8)
        padded[i, :len(w)] = np.frombuffer(w, np.uint8)
    word_long = np.array([len(w) > 12 for w in vocab])
    out = cells[pick]
    is_long = word_long[pick]
    n_long = int(is_long.sum())
    heap = padded[pick[is_long]].reshape(-1).copy() if n_long else np.zeros(1, np.uint8)
    ptr = np.uint64(heap.ctypes.data) + np.arange(n_long, dtype=np.uint64) * np.uint64(stride)
    out[is_long, 8:16] = ptr.view(np.uint8).reshape(-1, 8)
    return out.reshape(-1).view("V16"), heap, is_long


def like_count(vocab, pick, pattern):
    rx = re.compile(b"".join(b".*" if c == 37 else b"." if c == 95 else re.escape(bytes([c])) for c in pattern), re.DOTALL)
    per_word = np.bincount(pick, minlength=len(vocab))
    return rx, sum(int(c) for w, c in zip(vocab, per_word) if rx.fullmatch(w))


def main():
    n = 1 << LOG2
    rng = np.random.default_rng(26)
    pk = rng.integers(0, 1000, n).astype(np.int32)
    # inline-only column: 100 words of 3..12 bytes, uniform -> one word is 1 % of the rows (tools/bench_scan_varchar.py)
    words = [b"w%02d" % i + b"abcdefghi"[:(i * 7) % 10] for i in range(100)]
    pick = rng.integers(0, 100, n)
    s_inline, _, _ = column(words, pick, 12)
    # heap column of that tool: 30 % of the rows one of 64 strings of 24 bytes that begin with "Japa"
    longs = [(b"Japa" + bytes([ord("m") + i % 3]) + b"-%02d-long-heap-string" % i)[:24] for i in range(64)]
    is_long = rng.random(n) < 0.30
    hpick = np.where(is_long, 100 + rng.integers(0, 64, n), pick)
    s_heap, heap, _ = column(words + longs, hpick, 24)
    # notes (mc.note): 30 % of the rows one of 64 notes of 24..40 bytes, the rest NULL-free inline words
    years = [b"(1994)", b"(2001)", b"(2006)", b"(2007)", b"(1987)", b"(2010)", b"(1999)", b"(2003)"]
    places = [b"(USA)", b"(worldwide)", b"(Japan)", b"(Germany)"]
    media = [b"(TV)", b"(DVD)", b"(theatrical)", b"(all media)"]
    extras = [b"", b" (presents)", b" (co-production)"]
    notes = [b" ".join((a, b) if o else (b, a)) + b" " + m + x for o in (0, 1) for a in years for b in places for m in media
             for x in extras]
    notes = sorted(w for w in set(notes) if 24 <= len(w) <= 40)
    notes = notes[::len(notes) // 64][:64]
    assert len(notes) == 64
    npick = np.where(rng.random(n) < 0.30, 100 + rng.integers(0, len(notes), n), pick)
    s_note, note_heap, _ = column(words + notes, npick, 40)
    # info (mi.info): country:date strings of 8..24 bytes, about half of them longer than 12
    infos = [c + b":" + d for c in (b"USA", b"Japan", b"Germany", b"Sweden") for d in
             (b"2004", b"12 May 2004", b"1999", b"3 March 2001", b"1987", b"21 June 1987", b"2008", b"7 July 2005")]
    ipick = rng.integers(0, len(infos), n)
    s_info, info_heap, _ = column(infos, ipick, 24)
    ctx = capi.Context(0)
    ht = capi.HashTable.from_columns(ctx, [np.arange(1000, dtype=np.int32)], []).finalize_hash()
    pipe = capi.Pipeline(ctx, [pk, s_inline, s_heap, s_note, s_info], n, [(ht, [(-1, 0)])], [[0]])
    pipe.set_probe_heaps(1, [np.zeros(1, np.uint8)])
    pipe.set_probe_heaps(2, [heap])
    pipe.set_probe_heaps(3, [note_heap])
    pipe.set_probe_heaps(4, [info_heap])
    n_long = int(is_long.sum())

    word = words[37]
    want_eq = int((pick == 37).sum())
    f = capi.like_pushdown(b"Japan%")
    lo, hi = f[0][1], f[1][1]
    want_like = sum(int(c) for w, c in zip(words + longs, np.bincount(hpick, minlength=164)) if lo <= w < hi)
    bits = 2 * n // 8  # the pass bits: written once, read once
    t = timed(lambda: pipe.scan_filter([(1, "=", word)]))
    assert pipe.scan[0] == want_eq, (pipe.scan, want_eq)
    report("inline_eq/str", n, want_eq, 16 * n + bits + 4 * want_eq, t, constant=word.decode())
    t = timed(lambda: pipe.scan_filter([(2, op, c) for op, c in f]))
    assert pipe.scan[0] == want_like, (pipe.scan, want_like)
    report("like_heap/str", n, want_like, 16 * n + 2 * n_long + bits + 4 * want_like, t, pattern="Japan%",
           heap_rows=n_long)
    if not HAS_EXPR:
        return
    t = timed(lambda: pipe.scan_filter_expr(("cmp", 1, "=", word)))
    assert pipe.scan[0] == want_eq, (pipe.scan, want_eq)
    report("inline_eq/expr", n, want_eq, 16 * n + bits + 4 * want_eq, t, constant=word.decode())
    e = ("and",) + tuple(("cmp", 2, op, c) for op, c in f)
    t = timed(lambda: pipe.scan_filter_expr(e))
    assert pipe.scan[0] == want_like, (pipe.scan, want_like)
    report("like_heap/expr", n, want_like, 16 * n + 2 * n_long + bits + 4 * want_like, t, pattern="Japan%", heap_rows=n_long)

    vocab = words + notes
    _, want = like_count(vocab, npick, b"%(200%)%")
    n_notes = int((npick >= 100).sum())
    note_bytes = int(sum(len(vocab[i]) for i in range(100, len(vocab))) / len(notes) * n_notes)
    t = timed(lambda: pipe.scan_filter_expr(("like", 3, b"%(200%)%")))
    assert pipe.scan[0] == want and 0 < want < n, (pipe.scan, want)
    report("contains_heap", n, want, 16 * n + note_bytes + bits + 4 * want, t, pattern="%(200%)%", heap_rows=n_notes)

    members = [words[i] for i in (3, 17, 29, 41, 53, 67, 79, 97)]
    want = int(np.isin(pick, (3, 17, 29, 41, 53, 67, 79, 97)).sum())
    t = timed(lambda: pipe.scan_filter_expr(("in", 1, members)))
    assert pipe.scan[0] == want, (pipe.scan, want)
    report("in8_inline", n, want, 16 * n + bits + 4 * want, t)

    rx = [like_count(vocab, npick, p)[0] for p in (b"%(USA)%", b"%(worldwide)%")]
    ry = [like_count(infos, ipick, p)[0] for p in (b"Japan:%200%", b"USA:%200%")]
    note_ok = np.array([bool(rx[0].fullmatch(w) or rx[1].fullmatch(w)) for w in vocab])
    info_ok = np.array([bool(ry[0].fullmatch(w) or ry[1].fullmatch(w)) for w in infos])
    want = int((note_ok[npick] & info_ok[ipick]).sum())
    e = ("and", ("cmp", 3, "is not null", None), ("or", ("like", 3, b"%(USA)%"), ("like", 3, b"%(worldwide)%")),
         ("cmp", 4, "is not null", None), ("or", ("like", 4, b"Japan:%200%"), ("like", 4, b"USA:%200%")))
    info_bytes = int(sum(len(infos[i]) for i in ipick[:100000] if len(infos[i]) > 12) / 100000 * n)
    t = timed(lambda: pipe.scan_filter_expr(e))
    assert pipe.scan[0] == want and 0 < want < n, (pipe.scan, want)
    report("job19a", n, want, 2 * 16 * n + note_bytes + info_bytes + bits + 4 * want, t, heap_rows=n_notes)


if __name__ == "__main__":
    main()
