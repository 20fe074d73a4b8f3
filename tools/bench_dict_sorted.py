#!/usr/bin/env python3
"""Encode time of a dictionary of N distinct 20-byte strings, first-appearance codes against sorted codes
(polr_ht_encode_dictionary_ex without and with POLR_DICT_SORTED), on the GPU.

    python tools/bench_dict_sorted.py [--n 1000000] [--reps 5]

Prints one JSON line: the median wall time of the call (it returns after the codes are complete) per variant, the
difference -- what the device sort costs -- and a check of the sorted dictionary against Python's sorted().  Every
repetition uploads a fresh table; the upload is outside the clock."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "duckdb-polr_amd", "python"))
from polr_amd import capi  # noqa: E402


def cells_of(strs, width):
    """string_t cells + heap of equally long strings (longer than 12 bytes), vectorised"""
    n = len(strs)
    heap = np.frombuffer(b"".join(strs), np.uint8).copy()
    cells = np.zeros((n, 16), np.uint8)
    cells[:, 0:4] = np.frombuffer(np.uint32(width).tobytes(), np.uint8)
    cells[:, 4:8] = heap.reshape(n, width)[:, :4]
    ptr = heap.ctypes.data + np.arange(n, dtype=np.uint64) * np.uint64(width)
    cells[:, 8:16] = ptr.view(np.uint8).reshape(n, 8)
    return cells.reshape(-1).view("V16"), heap


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    rng = np.random.default_rng(7)
    ids = rng.permutation(a.n)
    strs = [b"title-%014d" % i for i in ids.tolist()]  # 20 bytes, shuffled
    assert len(strs[0]) == 20
    cells, heap = cells_of(strs, 20)
    keys = np.arange(a.n, dtype=np.int32)
    ctx = capi.Context(0)
    times = {False: [], True: []}
    checked = False
    for rep in range(a.reps + 1):  # (the first repetition warms up: code objects, allocator)
        for is_sorted in (False, True):
            ht = capi.HashTable.from_columns(ctx, [keys], [cells])
            ht.set_payload_heap(0, heap)
            ctx.sync()
            t0 = time.perf_counter()
            code_col, n_codes, _null = ht.encode_dictionary(0, sorted=is_sorted)
            dt = time.perf_counter() - t0
            assert n_codes == a.n
            if rep:
                times[is_sorted].append(dt)
            if is_sorted and not checked:
                assert ht.dictionary(code_col, str_cap=24 * a.n) == sorted(strs)
                checked = True
            ht.close()
    plain, srt = statistics.median(times[False]), statistics.median(times[True])
    print(json.dumps({"n_distinct": a.n, "string_bytes": 20, "reps": a.reps, "encode_unsorted_ms": round(plain * 1e3, 3),
                      "encode_sorted_ms": round(srt * 1e3, 3), "sort_ms": round((srt - plain) * 1e3, 3),
                      "sorted_dictionary_equals_python_sorted": checked}))


if __name__ == "__main__":
    main()
