#!/usr/bin/env python3
"""What a probe-side dictionary costs and what it buys (polr_pipeline_encode_dictionary), on the GPU.

    python tools/bench_probe_dictionary.py [--rows 30000000] [--reps 5] [--selectivities 64,16,4,1]

A probe table of --rows rows -- two join keys, a filter column and a VARCHAR column of 20-byte strings with 7 and with
1 000 000 distinct values, all in device memory before the clock starts -- under a pipeline of two perfect joins that
every row passes.  Per repetition a fresh pipeline per shape, the shapes alternating inside the repetition; the first
repetition warms up and is dropped.  Median [min, max] of the wall time of the calls, which return when their results are
complete:

  (a) encode_all       the encode over all rows
  (b) encode_selected  POLR_DICT_SELECTED after a scan that keeps 1/16 of the rows
  (c) the query SELECT COUNT(*), MIN(col) end to end after the scan, per selectivity 1/s of --selectivities, two ways:
        string_route   counting run + emitting run into a sized output + polr_out_aggregate_string
        code_route     encode SORTED | NULL_INVALID | SELECTED + one fused pool launch + one dictionary_strings

Prints one JSON line.  algorithmic_bytes: what the encode must move -- per inserted position its selection word, the cell,
the 20 string bytes and its slot word; per table row the slot words the rank and assign steps read (twice and once) and the
code written, and through a selection the "no slot" fill: 56 B a row over all rows, 44 B a selected position + 20 B a table
row through a selection.  scratch_bytes: the encoder's one scratch allocation (polr_pdict_plan.h), without the sort's."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "duckdb-polr_amd", "python"))
from polr_amd import capi  # noqa: E402

WIDTH = 20


def r16(x):
    return (x + 15) & ~15


def scratch_bytes(n_rows, n_insert):
    cap = 1024
    while cap < 2 * n_insert:
        cap *= 2
    return 36 * cap + r16(4 * n_rows) + r16(4 * n_insert) + r16(4 * max(1, -(-n_rows // 1024))) + 64


def algorithmic_bytes(n_rows, n_insert, selected):
    return n_insert * 44 + n_rows * 20 if selected else n_rows * 56


def device_strings(n, d, rng):
    """a VARCHAR column of n rows over d distinct 20-byte strings, on the device: (cells tensor, heap tensor, the strings)"""
    strs = [b"title-%014d" % i for i in rng.permutation(d).tolist()]
    heap = torch.from_numpy(np.frombuffer(b"".join(strs), np.uint8).copy()).cuda()
    pick = rng.integers(0, d, n)
    cells = np.zeros((n, 16), np.uint8)
    cells[:, 0:4] = np.frombuffer(np.uint32(WIDTH).tobytes(), np.uint8)
    cells[:, 4:8] = heap.cpu().numpy().reshape(d, WIDTH)[pick, :4]
    ptr = np.uint64(heap.data_ptr()) + pick.astype(np.uint64) * np.uint64(WIDTH)
    cells[:, 8:16] = ptr.view(np.uint8).reshape(n, 8)
    return torch.from_numpy(cells).cuda(), heap, strs, pick


def summary(ts):
    return {"median_ms": round(statistics.median(ts) * 1e3, 3), "min_ms": round(min(ts) * 1e3, 3), "max_ms": round(max(ts) * 1e3, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=30_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--selectivities", default="64,16,4,1", help="the scan keeps 1/s of the rows, per s (powers of two up to 64)")
    a = ap.parse_args()
    n = a.rows
    sels = [int(s) for s in a.selectivities.split(",")]
    rng = np.random.default_rng(11)
    ctx = capi.Context(0)
    k1 = torch.from_numpy(rng.integers(0, 1000, n).astype(np.int32)).cuda()
    k2 = torch.from_numpy(rng.integers(0, 1000, n).astype(np.int32)).cuda()
    f_host = rng.integers(0, 64, n).astype(np.int32)
    f = torch.from_numpy(f_host).cuda()
    columns = {d: device_strings(n, d, rng) for d in (7, 1_000_000)}
    torch.cuda.synchronize()
    hts = []
    for _ in range(2):
        ht = capi.HashTable.from_columns(ctx, [np.arange(1000, dtype=np.int32)])
        assert ht.finalize_perfect(0, 999)
        hts.append(ht)

    def pipeline(d):
        cells = columns[d][0]
        cols = [capi.dev_col(k1.data_ptr(), 4, True), capi.dev_col(k2.data_ptr(), 4, True), capi.dev_col(f.data_ptr(), 4, True),
                capi.dev_col(cells.data_ptr(), 16)]
        return capi.Pipeline(ctx, cols, n, [(hts[0], [(-1, 0)]), (hts[1], [(-1, 1)])], [[0, 1], [1, 0]])

    def timed(call):
        ctx.sync()
        t0 = time.perf_counter()
        res = call()
        ctx.sync()
        return time.perf_counter() - t0, res

    def pool(pipe, n_chunks, out):
        mpx = capi.DeviceMultiplexer(pipe, "adaptive_reinit")
        mpx.use_scan_chunks()
        capi.run_resident([mpx], [(0, n_chunks)], out=out, reset=True, finish=True)
        st = mpx.finish()
        mpx.close()
        return sum(st["stage_out"][p][1] for p in range(2))

    def string_route(pipe, n_chunks):
        n_out = pool(pipe, n_chunks, None)
        out = capi.Output(pipe, 1024, n_out // 1024 + 1 + 8192)
        pool(pipe, n_chunks, out)
        res = (out.stats()[0], out.aggregate_string("min", -1, 3))
        out.close()
        return res

    def code_route(pipe, n_chunks):
        code_col = pipe.encode_dictionary(3, sorted=True, null_invalid=True, selected=True)[0]
        out = capi.Output(pipe, 1024, 1)
        out.fuse_aggregate([("count_star", -1, 0), ("min", -1, code_col)])
        pool(pipe, n_chunks, out)
        count, code = out.fused_aggregate_result()
        out.close()
        return count, None if code is None else pipe.dictionary_strings(code_col, [code])[0]

    times = {}
    checks = []
    for rep in range(a.reps + 1):
        for d in columns:
            strs, pick = columns[d][2], columns[d][3]
            # (a) all rows
            pipe = pipeline(d)
            dt, (_col, n_codes, _null) = timed(lambda: pipe.encode_dictionary(3))
            assert n_codes == len(np.unique(pick))
            times.setdefault(("encode_all", d), []).append(dt)
            pipe.close()
            # (b) 1/16 selected by a scan
            pipe = pipeline(d)
            n_sel, _ = pipe.scan_filter([(2, "<", 4)])
            dt, (_col, n_codes, _null) = timed(lambda: pipe.encode_dictionary(3, selected=True))
            if rep == 0:
                assert n_sel == int((f_host < 4).sum()) and n_codes == len(np.unique(pick[f_host < 4]))
            times.setdefault(("encode_selected", d), []).append(dt)
            times[("n_selected", d)] = n_sel
            pipe.close()
            # (c) the query, both routes, per selectivity
            for s in sels:
                answers = []
                for route in (string_route, code_route):
                    pipe = pipeline(d)
                    n_sel, n_chunks = pipe.scan_filter([(2, "<", 64 // s)])
                    dt, res = timed(lambda: route(pipe, n_chunks))
                    times.setdefault((route.__name__, d, s), []).append(dt)
                    answers.append(res)
                    pipe.close()
                assert answers[0] == answers[1], answers
                if rep == 0:
                    want = min(strs[i] for i in np.unique(pick[f_host < 64 // s]).tolist())
                    assert answers[0] == (n_sel, want), (answers[0], n_sel, want)
                    checks.append((d, s))
    res = {"rows": n, "string_bytes": WIDTH, "reps": a.reps, "checked_against_numpy": len(checks)}
    for d in columns:
        n_sel = times[("n_selected", d)]
        res["distinct_%d" % d] = {
            "encode_all": dict(summary(times[("encode_all", d)][1:]), algorithmic_bytes=algorithmic_bytes(n, n, False),
                               scratch_bytes=scratch_bytes(n, n)),
            "encode_selected_16th": dict(summary(times[("encode_selected", d)][1:]), n_selected=n_sel,
                                         algorithmic_bytes=algorithmic_bytes(n, n_sel, True), scratch_bytes=scratch_bytes(n, n_sel)),
            "query": {"1/%d" % s: {"string_route": summary(times[("string_route", d, s)][1:]),
                                   "code_route": summary(times[("code_route", d, s)][1:])} for s in sels},
        }
    print(json.dumps(res))
    for ht in hts:
        ht.close()


if __name__ == "__main__":
    main()
