"""polr_pipeline_from_output (Pipeline.from_output): the output of pipeline A as the SOURCE of pipeline B, gathered on the
device.

How the gathered columns are read back: B gets one join, a perfect table over the whole domain of an all-valid int32
column of A that is carried along, so every probe row of B meets exactly one build row and slot 0 of B's output is a
permutation of A's output rows.  polr_out_materialize(-1, i) of B's output, put back into A's row order, must then equal the
composed route -- polr_out_materialize of A's output for the source column -- bit for bit, cells and validity (a NULL cell
is zero on both routes).  VARCHAR columns are compared as raw cells where they hold no pointer (inline and NULL cells) and
as decoded strings everywhere.  Row sets of two-stage queries are composed through fetch_ids of both outputs down to
base-table rows and compared against the numpy join of all tables (joinref.Ref); intermediates against the oracle.

Every GPU step runs once; nothing retries.  The refusal of an output of 2^32 - 16 rows or more is checked where it is
decided, in tests/test_pipesrc_plan.py: such an output would take minutes to produce."""
import ctypes as C

import numpy as np
import pytest

import jobchain
from common import orc
from joinref import MAX_WAVE_CHUNKS, Join, Ref, device_rows, sort_rows
from polr_amd import capi, job_family
from test_gpu_from_output import DTS, POOL, Source, edge_source, string_source
from test_gpu_sink_matrix import DevBuf

pytestmark = pytest.mark.gpu


def identity_table(ctx, lo, hi):
    ht = capi.HashTable.from_columns(ctx, [np.arange(lo, hi + 1, dtype=np.int32)], [])
    assert ht.finalize_perfect(lo, hi)
    return ht


def run_all(pipe, n, cap=64, fan=1):
    """every probe row of `pipe` through join order 0, emitting -> (Output, counts)"""
    out = capi.Output(pipe, cap, fan * n // cap + 1 + MAX_WAVE_CHUNKS)
    counts = pipe.probe_rounds([(0, n, 0, 1)], out=out) if n else np.zeros((1, pipe.k), np.uint64)
    return out, counts


def read_back(ctx, src, cols, ident, lo, hi, close_src=False):
    """B = from_output(A's output, cols + [ident]) x the identity join on `ident` -> ([(data or raw string tuple, valid)] per
    column in A's output-row order, as B's output materialises them; the composed route's answer for the same columns)"""
    n = len(src.rows)
    want = []
    for r in cols:
        vals = src.cols[r][0]
        if isinstance(vals, list):
            want.append((src.out.materialize_strings_raw(*r)[:2], src.out.materialize_strings(*r)))
        else:
            want.append(src.out.materialize(r[0], r[1], vals.dtype))
    ht = identity_table(ctx, lo, hi)
    pipe = capi.Pipeline.from_output(src.out, list(cols) + [ident], [(ht, [(-1, len(cols))])], [[0]])
    assert pipe.scan_filter([])[0] == n  # one probe row per output row
    pipe.set_selection(None)
    if close_src:
        src.close()
    out, counts = run_all(pipe, n)
    assert int(counts.sum()) == n
    ids = out.fetch_ids().astype(np.int64)
    assert np.array_equal(np.sort(ids[:, 0]), np.arange(n))
    back = np.empty(n, np.int64)
    back[ids[:, 0]] = np.arange(n)  # A's output row r is B's output row back[r]
    got = []
    for i, r in enumerate(cols):
        vals = src.cols[r][0]
        if isinstance(vals, list):
            cells, valid = out.materialize_strings_raw(-1, i)[:2]
            strs = out.materialize_strings(-1, i)
            got.append(((cells[back], valid[back]), [strs[j] for j in back.tolist()]))
        else:
            d, v = out.materialize(-1, i, vals.dtype)
            got.append((d[back], v[back]))
    out.close()
    return pipe, ht, got, want


def assert_same_columns(src, cols, got, want):
    for r, g, w in zip(cols, got, want):
        if isinstance(src.cols[r][0], list):
            (gc, gv), gs = g
            (wc, wv), ws = w
            assert gs == ws and np.array_equal(gv, wv), r
            graw, wraw = gc.view(np.uint8).reshape(-1, 16), wc.view(np.uint8).reshape(-1, 16)
            no_ptr = (gv == 0) | (graw.view(np.uint32).reshape(-1, 4)[:, 0] <= 12)
            assert np.array_equal(graw[no_ptr], wraw[no_ptr]), r  # inline cells zero-padded, NULL cells all-zero: the same bits
            assert np.array_equal(graw[~no_ptr, :8], wraw[~no_ptr, :8]), r  # long cells: length and prefix (the pointers differ)
            assert not graw[gv == 0].any(), r
        else:
            assert g[0].dtype == w[0].dtype and np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]), r
            assert not g[0][g[1] == 0].any(), r  # NULL cells are zero


# ---- 1. gather edges --------------------------------------------------------------------------------------------------------
_SRC = {}


@pytest.fixture(scope="module", autouse=True)
def _close_sources():
    yield
    for s in _SRC.values():
        s.close()
    _SRC.clear()


def fanout_source(ctx):
    """a 2-join first pipeline: join 0 repeats every key 1..4 times (output rows exceed probe rows, row ids repeat), join 1 is
    a perfect table.  Probe columns: two keys, the row number, then every width signed and unsigned without (3..10) and with
    (11..18) a validity array; both joins carry payload of several widths with and without validity.  chunk_capacity 64."""
    if "fan" not in _SRC:
        rng = np.random.default_rng(11)
        n, nk, nb1 = 700, 120, 90
        k0 = rng.permutation(np.repeat(np.arange(nk, dtype=np.int32), rng.integers(1, 5, nk)))
        j0 = Join(k0, 0, payload=[rng.integers(-100, 100, len(k0)).astype(np.int8), rng.integers(0, 1 << 40, len(k0)).astype(np.uint64),
                                  rng.integers(0, 60000, len(k0)).astype(np.uint16)],
                  payload_valid=[(rng.random(len(k0)) > 0.2).astype(np.uint8), None, (rng.random(len(k0)) > 0.2).astype(np.uint8)])
        j1 = Join(rng.permutation(nb1).astype(np.int32), 1, (0, nb1 - 1),
                  payload=[rng.integers(-(1 << 30), 1 << 30, nb1).astype(np.int32), rng.integers(-(1 << 60), 1 << 60, nb1).astype(np.int64)],
                  payload_valid=[None, (rng.random(nb1) > 0.2).astype(np.uint8)])
        pcols = [rng.integers(-5, nk + 5, n).astype(np.int32), rng.integers(-5, nb1 + 5, n).astype(np.int32), np.arange(n, dtype=np.int32)]
        pvalid = [None, None, None]
        for with_valid in (False, True):
            for dt in DTS:
                info = np.iinfo(dt)
                pcols.append(rng.integers(info.min, info.max, n, dtype=dt, endpoint=True))
                pvalid.append((rng.random(n) > 0.15).astype(np.uint8) if with_valid else None)
        _SRC["fan"] = Source(ctx, pcols, pvalid, [j0, j1], cap=64)
    return _SRC["fan"]


def test_gather_every_width_slot_and_validity(gpu_ctx):
    src = fanout_source(gpu_ctx)
    n = len(src.rows)
    assert n > 700 and np.bincount(src.rows[:, 0]).max() >= 2  # fan-out: probe rows repeat among the output rows
    n_rows, n_chunks, _ = src.out.stats()
    assert n_rows == n and n_chunks * 64 > n_rows  # (several partially filled chunks)
    # columns from slot 0 and from every join slot, scrambled; (0, 1) and (-1, 13) named twice
    cols = [(1, 0)] + [(-1, 3 + i) for i in range(16)] + [(0, 0), (0, 1), (1, 1), (0, 2), (0, 1), (-1, 13), (-1, 0)]
    pipe, ht, got, want = read_back(gpu_ctx, src, cols, (-1, 2), 0, 699)
    assert_same_columns(src, cols, got, want)
    assert any(not g[1].all() for g in got) and any(g[1].all() for g in got)
    # ... and against the host: A's fetch_ids index A's source columns
    for r, g in zip(cols, got):
        vals, ok = src.host(r)
        assert np.array_equal(g[1], ok) and np.array_equal(g[0], vals * ok.astype(vals.dtype)), r
    # an ordinary pipeline: the launch is planned like any other, its width and signedness are the sources'
    assert pipe.launch_info()["flat"] == 1
    pipe.close()
    ht.close()


EDGES = {"one-row": (1, 64), "one-chunk": (64, 64), "one-chunk-plus-1": (65, 64), "cap65": (1000, 65), "cap1000": (2500, 1000)}


@pytest.mark.parametrize("case", list(EDGES))
def test_gather_chunk_edges(gpu_ctx, case):
    n, cap = EDGES[case]
    src = edge_source(gpu_ctx, n, cap)
    assert len(src.rows) == n
    n_rows, n_chunks, _ = src.out.stats()
    assert n_rows == n and n_chunks >= (n + cap - 1) // cap
    cols = [(0, 0), (-1, 0), (-1, 1)]
    pipe, ht, got, want = read_back(gpu_ctx, src, cols, (-1, 1), 0, n - 1, close_src=True)
    assert_same_columns(src, cols, got, want)
    pipe.close()
    ht.close()


def test_gather_chunks_of_1_63_64_and_1_rows(gpu_ctx):
    """every probe_rounds call starts chunks of its own: chunks that hold 1, 63, 64 and (65 as) 64 + 1 rows"""
    src = edge_source(gpu_ctx, 1 + 63 + 64 + 65, 64, rounds=[(0, 1), (1, 63), (64, 64), (128, 65)])
    n_rows, n_chunks, _ = src.out.stats()
    assert n_rows == 193 and n_chunks >= 5
    cols = [(-1, 0), (0, 0)]
    pipe, ht, got, want = read_back(gpu_ctx, src, cols, (-1, 1), 0, 192)
    assert_same_columns(src, cols, got, want)
    pipe.close()
    ht.close()
    src.close()


@pytest.mark.parametrize("filled", [True, False], ids=["zero-rows", "never-filled"])
def test_empty_output_gives_a_pipeline_of_no_rows(gpu_ctx, filled):
    """as polr_pipeline_create with n_probe_rows = 0: a valid pipeline; scans select nothing, runs count nothing"""
    live0 = capi.device_bytes_live()
    src = edge_source(gpu_ctx, 500, 64, hit=False, run=filled)
    ht = identity_table(gpu_ctx, 0, 499)
    pipe = capi.Pipeline.from_output(src.out, [(0, 0), (-1, 1)], [(ht, [(-1, 1)])], [[0]])
    twin = capi.Pipeline(gpu_ctx, [np.zeros(0, np.int32), np.zeros(0, np.int32)], 0, [(ht, [(-1, 1)])], [[0]])
    src.close()
    one = np.zeros(1, np.int32)
    infos = []
    for p in (pipe, twin):
        infos.append((p.launch_info(), p.launch_info(True)))
        out = capi.Output(p, 64, 64)
        assert out.stats()[0] == 0 and len(out.fetch_ids()) == 0
        # zero probe rows: an update of one row does not fit
        rc = gpu_ctx.L.polr_pipeline_update_probe(p.h, 0, one.ctypes.data, None, 1)
        assert rc == capi.E_INVALID and "2 columns, 0 rows" in gpu_ctx.L.polr_last_error(gpu_ctx.h).decode()
        out.close()
        p.close()
    assert infos[0] == infos[1] and infos[0][0]["flat"] == 1
    ht.close()
    assert capi.device_bytes_live() == live0


# ---- 2. VARCHAR -------------------------------------------------------------------------------------------------------------
def test_varchar_columns_cells_heaps_and_string_sink(gpu_ctx):
    """inline strings with dirty padding, long ones (a 5000-byte string, heaps of two and three blocks), NULLs; from the probe
    table and from a fan-out build side; the string MIN / MAX sink over a second-stage output reads the pipeline's own heap"""
    live0 = capi.device_bytes_live()
    src = string_source(gpu_ctx, 80)
    n = len(src.rows)
    assert np.bincount(src.rows[:, 1]).max() >= 2  # one build row behind many output rows: each gets its own heap copy
    cols = [(-1, 2), (0, 0), (0, 1), (0, 0)]
    host = [src.host(r) for r in cols]
    for vals, ok in host[:2]:
        assert any(o and len(v) == 5000 for v, o in zip(vals, ok)) and any(o and len(v) <= 12 for v, o in zip(vals, ok)) and not all(ok)
    live1 = capi.device_bytes_live()
    pipe, ht, got, want = read_back(gpu_ctx, src, cols, (-1, 1), 0, 299)
    assert_same_columns(src, cols, got, want)
    for (vals, ok), g in zip(host[:2], got[:2]):
        assert g[1] == [v if o else None for v, o in zip(vals, ok)]
    # every byte is accounted for: one allocation of cells + validity (+ descriptors), a packed heap per VARCHAR column
    def up(x):
        return (x + 255) // 256 * 256

    heap = [sum(len(v) for v, o in zip(*h) if o and len(v) > 12) for h in (host[0], host[1], host[3])]
    own = sum(up(n * w) + up(n) for w in (16, 16, 4, 16, 4)) + sum(heap)
    grew = capi.device_bytes_live() - live1 - ht.info()["device_bytes"]
    assert own < grew  # (the pipeline's stage descriptors and scan buffers come on top)
    # the column counts as rebased: a heap of the caller's is refused
    with pytest.raises(capi.PolrError) as e:
        pipe.set_probe_heap(0, np.zeros(64, np.uint8))
    assert e.value.code == capi.E_INVALID and "device heap already" in str(e.value)
    # the sources go; the second stage still reads its own cells and heaps
    src.close()
    src.keep.clear()
    out, _ = run_all(pipe, n)
    for c in (0, 1):
        live = [v for v in got[c][1] if v is not None]
        assert out.aggregate_string("min", -1, c, cap=8192) == min(live) and out.aggregate_string("max", -1, c, cap=8192) == max(live)
    # a pushed-down VARCHAR filter over the gathered column
    n_sel, _ = pipe.scan_filter([(0, "=", b"UNITED STATES")])
    assert n_sel == sum(v == b"UNITED STATES" for v in got[0][1]) > 0
    out.close()
    pipe.close()
    ht.close()
    assert capi.device_bytes_live() == live0


def test_varchar_from_caller_device_memory(gpu_ctx):
    """a POLR_COL_DEVICE source: cells that point into the caller's HBM; the new pipeline owns copies"""
    rng = np.random.default_rng(81)
    n, nb = 600, 50
    vals = [POOL[i] for i in rng.integers(0, len(POOL), n)]
    ok = (rng.random(n) > 0.2).astype(np.uint8)
    heap = np.frombuffer(b"".join(vals), np.uint8)
    d_heap, d_cells, d_ok = DevBuf(heap.nbytes), DevBuf(16 * n), DevBuf(n)
    cells = np.zeros((n, 16), np.uint8)
    at = 0
    for i, v in enumerate(vals):
        cells[i, :4] = np.frombuffer(np.uint32(len(v)).tobytes(), np.uint8)
        if len(v) <= 12:
            cells[i, 4:4 + len(v)] = np.frombuffer(v, np.uint8)
        else:
            cells[i, 4:8] = np.frombuffer(v[:4], np.uint8)
            cells[i, 8:] = np.frombuffer(np.uint64(d_heap.ptr + at).tobytes(), np.uint8)
        at += len(v)
    d_heap.upload(heap)
    d_cells.upload(cells)
    d_ok.upload(ok)
    key = rng.integers(0, nb, n).astype(np.int32)
    rowno = np.arange(n, dtype=np.int32)
    j = Join(np.arange(nb, dtype=np.int32), 0, (0, nb - 1))
    h0 = j.device(gpu_ctx)
    a = capi.Pipeline(gpu_ctx, [key, rowno, capi.dev_col(d_cells.ptr, 16, valid_ptr=d_ok.ptr)], n, [(h0, [(-1, 0)])], [[0]])
    out_a, _ = run_all(a, n)
    ids_a = out_a.fetch_ids()
    ht = identity_table(gpu_ctx, 0, n - 1)
    b = capi.Pipeline.from_output(out_a, [(-1, 2), (-1, 1)], [(ht, [(-1, 1)])], [[0]])
    out_a.close()
    a.close()
    h0.close()
    for d in (d_heap, d_cells, d_ok):  # the caller's memory goes too
        d.free()
    out_b, _ = run_all(b, n)
    ids_b = out_b.fetch_ids()
    strs = out_b.materialize_strings(-1, 0)
    rows = ids_a[ids_b[:, 0], 0]
    assert strs == [vals[r] if ok[r] else None for r in rows.tolist()] and len(strs) == n
    assert any(v is not None and len(v) > 12 for v in strs) and None in strs
    out_b.close()
    b.close()
    ht.close()


def test_varchar_heap_never_came(gpu_ctx):
    live0 = capi.device_bytes_live()
    src = string_source(gpu_ctx, 82, heaps=False)
    ht = identity_table(gpu_ctx, 0, 299)
    live1 = capi.device_bytes_live()
    for ref in [(-1, 2), (0, 0)]:
        rc, h = raw_call(gpu_ctx, src.out.h, [(-1, 1), ref], 2, [(ht, [(-1, 0)])], 1, [[0]], 1)
        assert rc == capi.E_INVALID and not h
        assert "heap was never put on the device" in gpu_ctx.L.polr_last_error(gpu_ctx.h).decode()
        assert capi.device_bytes_live() == live1
    src.close()
    # the same columns holding inline strings only need no heap
    src = string_source(gpu_ctx, 83, heaps=False, pool=[v for v in POOL if len(v) <= 12])
    cols = [(-1, 2), (0, 0)]
    pipe, ht2, got, want = read_back(gpu_ctx, src, cols, (-1, 1), 0, 299, close_src=True)
    assert_same_columns(src, cols, got, want)
    pipe.close()
    ht2.close()
    ht.close()
    assert capi.device_bytes_live() == live0


# ---- 3. second stage runs: 8 + 4 joins --------------------------------------------------------------------------------------
class TwoStage:
    """a 12-join query cut after 8 joins.  Stage 1: a probe table with key columns 0..7 (and 8..11 for the star tail) x 8
    perfect tables; table j of the first four carries payload column 0, the key of tail join 8 + j in the DEPENDENT variant.
    Stage 2 = from_output(carried key columns) x 4 tail tables: all perfect (flat), or with one repeated-key hash table
    (generic)."""

    def __init__(self, ctx, dependent, repeated_tail, seed):
        rng = np.random.default_rng(seed)
        self.ctx, self.dependent = ctx, dependent
        n, nb, nt = 4000, 64, 80
        pcols = [rng.integers(0, nb + 3, n).astype(np.int32) for _ in range(8)] + [rng.integers(0, nt + 10, n).astype(np.int32) for _ in range(4)]
        head = []
        for j in range(8):
            pay = [rng.integers(0, nt + 10, nb).astype(np.int32)] if j < 4 else []
            head.append(Join(rng.permutation(nb).astype(np.int32), j, (0, nb - 1), payload=pay, payload_valid=[None] * len(pay)))
        self.src = Source(ctx, pcols, None, head, cap=64, engine="pool")
        assert len(self.src.rows) > 1000
        self.tail = []
        for j in range(4):
            if repeated_tail and j == 2:
                self.tail.append(Join(rng.permutation(np.repeat(np.arange(nt, dtype=np.int32), 2)), j))
            else:
                self.tail.append(Join(rng.permutation(nt).astype(np.int32), j, (0, nt - 1)))
        self.hts = [t.device(ctx) for t in self.tail]
        self.carry = [(j, 0) for j in range(4)] if dependent else [(-1, 8 + j) for j in range(4)]
        self.paths = [[0, 1, 2, 3], [3, 2, 1, 0], [1, 3, 0, 2]]
        self.pipe = capi.Pipeline.from_output(self.src.out, self.carry, [(h, [(-1, j)]) for j, h in enumerate(self.hts)], self.paths)
        # the numpy join of all thirteen tables, as base-table rows
        self.host_cols = [self.src.host(r)[0] for r in self.carry]
        self.n2 = len(self.src.rows)
        self.ref2 = Ref(self.host_cols, None, self.tail)
        r2 = self.ref2.rows()
        self.want = sort_rows(np.column_stack([self.src.rows[r2[:, 0]], r2[:, 1:]]))
        assert len(self.want) > 200

    def composed(self, out2):
        ids2 = device_rows(out2.fetch_ids(), self.tail)
        return sort_rows(np.column_stack([self.src.rows[ids2[:, 0]], ids2[:, 1:]]))

    def oracle(self, routing="default_path"):
        return orc.run_pipeline(self.host_cols, [t.oracle() for t in self.tail], self.paths, routing=routing, caching=False)

    def close(self):
        self.pipe.close()
        for h in self.hts:
            h.close()
        self.src.close()


@pytest.mark.parametrize("shape", ["star", "dependent"])
@pytest.mark.parametrize("tail", ["flat", "generic"])
def test_second_stage_runs(gpu_ctx, shape, tail):
    q = TwoStage(gpu_ctx, shape == "dependent", tail == "generic", seed=31 + (shape == "dependent") + 2 * (tail == "generic"))
    info = q.pipe.launch_info()
    # after the cut a key that was a build column of an earlier join is a plain probe column: the tail qualifies for the flat kernel
    assert info["flat"] == (1 if tail == "flat" else 0)
    n2, k = q.n2, 4
    fan = 2 if tail == "generic" else 1
    ref = q.oracle()
    # (a) polr_probe_rounds, every join order: intermediates per stage, and the row set through the first order
    out = capi.Output(q.pipe, 64, fan * n2 // 64 + 1 + MAX_WAVE_CHUNKS)
    for p, path in enumerate(q.paths):
        counts = q.pipe.probe_rounds([(0, n2, p, int(p == 0))], out=out if p == 0 else None)
        assert [int(x) for x in counts[0]] == q.ref2.stage_counts(path), (p, path)
    assert int(q.pipe.probe_rounds([(0, n2, 0, 0)])[0].sum()) == ref["num_intermediates"]
    assert np.array_equal(q.composed(out), q.want)
    # (b) polr_mpx_run: host-routed rounds
    n_chunks = (n2 + 1023) // 1024
    for engine in ("mpx_run", "pool"):
        out.reset()
        gpu_ctx.sync()
        mx = capi.DeviceMultiplexer(q.pipe, "default_path")
        if engine == "mpx_run":
            mx.run(0, n_chunks, out=out)
        else:
            # (c) the pool launch: the flat kernel where the pipeline is flat and every table perfect, else the generic one
            capi.run_resident([mx], [(0, n_chunks)], out=out, reset=True, finish=True)
        st = mx.finish()
        _, _, inter = mx.fetch_log()
        assert st["num_intermediates"] == ref["num_intermediates"], engine
        assert list(inter) == list(ref["intermediates_per_round"]), engine
        assert st["stage_out"][0][k - 1] == ref["num_output_rows"] == len(q.want), engine
        assert np.array_equal(q.composed(out), q.want), engine
        mx.close()
    # (d) a counting pool run (no output): the flat kernel's counting variant
    mx = capi.DeviceMultiplexer(q.pipe, "default_path")
    capi.run_resident([mx], [(0, n_chunks)], reset=True, finish=True)
    assert mx.finish()["stage_out"][0][k - 1] == len(q.want)
    mx.close()
    out.close()
    q.close()


# ---- 4. a scan filter across tables of the first pipeline -------------------------------------------------------------------
def test_scan_filter_expression_across_first_stage_tables(gpu_ctx):
    src = fanout_source(gpu_ctx)
    n = len(src.rows)
    # (0, 0): int8 payload of join 0 with NULLs; (1, 0): int32 payload of join 1; (-1, 7): a probe column
    cols = [(0, 0), (1, 0), (-1, 7), (-1, 2)]
    ht = identity_table(gpu_ctx, 0, 699)
    pipe = capi.Pipeline.from_output(src.out, cols, [(ht, [(-1, 3)])], [[0]])
    (a, a_ok), (b, _), (c, _) = [src.host(r) for r in cols[:3]]
    expr = ("or", ("and", ("cmp", 0, "<", 10), ("cmp", 1, ">", 0)), ("and", ("cmp", 0, "is null"), ("cmp", 2, "<=", int(np.median(c)))))
    a_ok = a_ok.astype(bool)
    keep = (a_ok & (a < 10) & (b > 0)) | (~a_ok & (c <= int(np.median(c))))
    n_sel, n_chunks = pipe.scan_filter_expr(expr)
    sel, offs = pipe.fetch_scan()
    assert np.array_equal(sel, np.nonzero(keep)[0]) and 0 < n_sel < n and (~a_ok & keep).any() and (a_ok & keep).any()
    # the filtered source runs: the kept rows, each once, composed down to the first pipeline's rows
    mx = capi.DeviceMultiplexer(pipe, "default_path")
    mx.use_scan_chunks()
    out = capi.Output(pipe, 64, n // 64 + 1 + MAX_WAVE_CHUNKS)
    capi.run_resident([mx], [(0, n_chunks)], out=out, reset=True, finish=True)
    mx.finish()
    ids = out.fetch_ids()
    assert np.array_equal(np.sort(ids[:, 0]), np.nonzero(keep)[0])
    mx.close()
    out.close()
    pipe.close()
    ht.close()


# ---- 5. ownership and refusals ----------------------------------------------------------------------------------------------
def test_ownership_sources_destroyed_before_stage_two(gpu_ctx):
    live0 = capi.device_bytes_live()
    results = []
    for destroy_first in (False, True):
        q = TwoStage(gpu_ctx, True, True, seed=40)
        want, tail, rows1, n2 = q.want, q.tail, q.src.rows, q.n2
        if destroy_first:
            q.src.close()  # output A, its pipeline, its eight tables
        out = capi.Output(q.pipe, 64, 2 * n2 // 64 + 1 + MAX_WAVE_CHUNKS)
        counts = q.pipe.probe_rounds([(0, n2, 1, 1)], out=out)
        ids2 = device_rows(out.fetch_ids(), tail)
        got = sort_rows(np.column_stack([rows1[ids2[:, 0]], ids2[:, 1:]]))
        assert np.array_equal(got, want)
        results.append((counts.copy(), got))
        out.close()
        q.pipe.close()
        for h in q.hts:
            h.close()
        if not destroy_first:
            q.src.close()
        assert capi.device_bytes_live() == live0
    assert np.array_equal(results[0][0], results[1][0]) and np.array_equal(results[0][1], results[1][1])


def raw_call(ctx, out_h, cols, n_cols, joins, k, paths, n_paths, want_out=True, null_joins=False, null_paths=False):
    h = C.c_void_p(0xDEAD)
    jd = capi.Pipeline._join_descs(joins)
    pa = np.ascontiguousarray(np.asarray(paths, dtype=np.int32).reshape(-1))
    rc = ctx.L.polr_pipeline_from_output(out_h, None, None if cols is None else capi._out_col_refs(cols), n_cols,
                                         None if null_joins else jd, k, None if null_paths else pa.ctypes.data, n_paths,
                                         C.byref(h) if want_out else None)
    return rc, h.value


def test_refusals_leave_nothing_behind(gpu_ctx):
    src = fanout_source(gpu_ctx)
    ht = identity_table(gpu_ctx, 0, 699)
    raw = capi.HashTable.from_columns(gpu_ctx, [np.arange(10, dtype=np.int32)], [])  # never finalized
    one, p1 = [(ht, [(-1, 0)])], [[0]]
    c = [(-1, 2)]
    live0 = capi.device_bytes_live()
    cases = {
        "NULL output": ((None, c, 1, one, 1, p1, 1), capi.E_INVALID, None),
        "NULL cols": ((src.out.h, None, 1, one, 1, p1, 1), capi.E_INVALID, "cols is NULL"),
        "no columns": ((src.out.h, c, 0, one, 1, p1, 1), capi.E_INVALID, "no columns"),
        "67 columns": ((src.out.h, c * 67, 67, one, 1, p1, 1), capi.E_UNSUPPORTED, "67 columns"),
        "column out of range": ((src.out.h, c + [(-1, 19)], 2, one, 1, p1, 1), capi.E_INVALID, "column 1"),
        "join out of range": ((src.out.h, [(2, 0)], 1, one, 1, p1, 1), capi.E_INVALID, "column 0"),
        "payload column out of range": ((src.out.h, c + [(1, 2)], 2, one, 1, p1, 1), capi.E_INVALID, "column 1"),
        "nine joins": ((src.out.h, c, 1, one * 9, 9, [list(range(9))], 1), capi.E_UNSUPPORTED, "9 multiplexed joins"),
        "no joins": ((src.out.h, c, 1, one, 0, p1, 1), capi.E_UNSUPPORTED, "0 multiplexed joins"),
        "33 join orders": ((src.out.h, c, 1, one, 1, p1 * 33, 33), capi.E_UNSUPPORTED, "33 join orders"),
        "table not finalized": ((src.out.h, c, 1, [(raw, [(-1, 0)])], 1, p1, 1), capi.E_INVALID, "not finalized"),
        "not a permutation": ((src.out.h, c, 1, one * 2, 2, [[1, 1]], 1), capi.E_INVALID, "not a permutation"),
        "key column out of range": ((src.out.h, c, 1, [(ht, [(-1, 1)])], 1, p1, 1), capi.E_INVALID, "probe column 1 out of range"),
        "key width differs": ((src.out.h, [(-1, 9)], 1, one, 1, p1, 1), capi.E_INVALID, "probe key is 8 bytes"),
        # the order: a bad reference is found before nine joins are, no columns before a bad reference could be
        "bad reference before nine joins": ((src.out.h, [(-1, 19)], 1, one * 9, 9, [list(range(9))], 1), capi.E_INVALID, "column 0"),
    }
    for what, (args, code, text) in cases.items():
        rc, h = raw_call(gpu_ctx, *args)
        assert rc == code and not h, what
        if text:
            assert text in gpu_ctx.L.polr_last_error(gpu_ctx.h).decode(), what
        assert capi.device_bytes_live() == live0, what
    for kw in ({"want_out": False}, {"null_joins": True}, {"null_paths": True}):
        rc, h = raw_call(gpu_ctx, src.out.h, c, 1, one, 1, p1, 1, **kw)
        assert rc == capi.E_INVALID and (not h or not kw.get("want_out", True)) and capi.device_bytes_live() == live0
    # the limits themselves are fine: 66 columns, 8 joins, 32 join orders
    pipe = capi.Pipeline.from_output(src.out, [(-1, 2)] + [(-1, 3 + i % 16) for i in range(65)], one * 8, [list(range(8)), list(range(8))[::-1]] * 16)
    assert pipe.launch_info(True)["tuple_slots"] == 9
    pipe.close()
    assert capi.device_bytes_live() == live0
    raw.close()
    ht.close()


def test_refuses_an_output_with_a_fused_sink(gpu_ctx):
    rng = np.random.default_rng(8)
    n, nb = 2000, 100
    j0 = Join(rng.permutation(nb).astype(np.int32), 0, (0, nb - 1), payload=[rng.integers(0, 8, nb).astype(np.int32)], payload_valid=[None])
    j1 = Join(rng.permutation(nb).astype(np.int32), 1, (0, nb - 1), payload=[rng.integers(0, 8, nb).astype(np.int32)], payload_valid=[None])
    pcols = [rng.integers(0, nb, n).astype(np.int32), rng.integers(0, nb, n).astype(np.int32)]
    src = Source(gpu_ctx, pcols, None, [j0, j1], run=False)
    fused = capi.Output(src.pipe, 1024, 64)
    fused.fuse_grouped([(0, 0, 0, 8)], [("count_star", -1, 0)])
    ht = identity_table(gpu_ctx, 0, nb - 1)
    live0 = capi.device_bytes_live()
    rc, h = raw_call(gpu_ctx, fused.h, [(-1, 0)], 1, [(ht, [(-1, 0)])], 1, [[0]], 1)
    assert rc == capi.E_INVALID and not h and capi.device_bytes_live() == live0
    assert "fused GROUP BY sink" in gpu_ctx.L.polr_last_error(gpu_ctx.h).decode()
    ht.close()
    fused.close()
    src.close()


def test_outputs_of_the_new_pipeline_chain_on(gpu_ctx):
    """polr_ht_from_output and polr_pipeline_from_output of a second-stage output: a third stage reads what the second carried"""
    src = edge_source(gpu_ctx, 1000, 64)
    ht = identity_table(gpu_ctx, 0, 999)
    b = capi.Pipeline.from_output(src.out, [(0, 0), (-1, 1)], [(ht, [(-1, 1)])], [[0]])
    pay, rowno = src.host((0, 0))[0], src.host((-1, 1))[0]
    src.close()
    out_b, _ = run_all(b, 1000)
    c = capi.Pipeline.from_output(out_b, [(-1, 0), (-1, 1)], [(ht, [(-1, 1)])], [[0]])
    new = capi.HashTable.from_output(out_b, [(-1, 1)], [(-1, 0)])
    ids_b = out_b.fetch_ids()
    out_b.close()
    b.close()
    out_c, _ = run_all(c, 1000)
    ids_c = out_c.fetch_ids()
    d, v = out_c.materialize(-1, 0, np.int32)
    assert v.all() and np.array_equal(d, pay[ids_b[ids_c[:, 0], 0]])
    d, v = out_c.materialize(-1, 1, np.int32)
    assert np.array_equal(d, rowno[ids_b[ids_c[:, 0], 0]]) and np.array_equal(np.sort(d), np.arange(1000))
    assert new.info()["n_keys"] == 1
    new.finalize_hash()
    assert new.info()["n_rows"] == 1000
    new.close()
    out_c.close()
    c.close()
    ht.close()


# ---- 6. whole queries -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_tables", sorted(jobchain.SHAPES))
def test_whole_queries_through_the_chain_runner(gpu_ctx, n_tables):
    """a JOB shape of 10, 12, 14 and 17 tables with EVERY table joined: the chain runner on the device against the direct numpy
    join of all tables and against the same chain run stage by stage through the oracle (tests/test_job_chain.py)"""
    q, plan, data = jobchain.instance(n_tables)
    assert sum(len(st["joins"]) for st in plan["stages"]) == n_tables - 1 and len(plan["stages"]) >= 2
    want = jobchain.reference(plan, data)
    cpu = job_family.run_chain_host(plan, data, jobchain.oracle_stage)
    assert want["count"] >= 1 and all(r > jobchain.CHUNK for r in cpu["stage_rows"][:-1])
    live0 = capi.device_bytes_live()
    got = job_family.run_chain_device(gpu_ctx, plan, data, chunk_capacity=jobchain.CHUNK)
    assert got["count"] == want["count"] == cpu["count"]
    assert got["mins"] == want["mins"] == cpu["mins"]
    assert got["int_mins"] == want["int_mins"] == cpu["int_mins"]
    assert got["stage_rows"] == cpu["stage_rows"] and got["intermediates"] == cpu["intermediates"]
    assert capi.device_bytes_live() == live0
