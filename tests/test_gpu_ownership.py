"""Who owns device memory (duckdb-polr_amd/csrc/polr_devbuf.h): every handle frees what it allocated, every grow path
replaces its buffer and keeps answering right, and a refused call releases what it took.  Each test makes its own Context,
reads capi.device_bytes_live() -- the library's own count of the bytes it owns, exact where the device's free memory also
moves with other tenants -- before it and asserts the SAME value after everything it made is destroyed (not 0: session
fixtures of other tests may be alive).  The answers in between are checked against the numpy join of tests/joinref.py and
the filter evaluators of tests/scanstr.py / tests/scanexpr.py, like the tests of those paths do.

Shapes are the smallest that reach each path (ownership does not depend on size): build sides of 1 000 rows, a probe side
of 4 096 rows (pk INTEGER, pv BIGINT, ps VARCHAR), two joins in two join orders."""
import gc

import numpy as np
import pytest

import scanexpr
import scanstr
from joinref import Join, Ref, device_rows, sort_rows
from polr_amd import capi
from test_gpu_sink_matrix import py_agg, string_blocks

pytestmark = pytest.mark.gpu

N, NB, CAP = 4096, 1000, 64
MAX_WAVE_CHUNKS = 8192  # one partially filled chunk per emitting wave (polr_out_create)
PK, PV, PS, PU = 0, 1, 2, 3  # probe columns
WORDS = [b"", b"J", b"Japan", b"Jamaica", b"twelve bytes", b"thirteen byte", b"a string that lives in the heap",
         b"a string that lives in the heap too", b"Tokyo", b"zz" * 40]


def live_bytes():
    """the count, after the wrappers earlier tests left to the garbage collector are gone (so that none goes mid-test)"""
    gc.collect()
    return capi.device_bytes_live()


def refused(call, *args):
    with pytest.raises(capi.PolrError) as e:
        call(*args)
    return e.value.code


class Data:
    """the inputs and the numpy reference, shared by the tests and never changed"""

    def __init__(self):
        rng = np.random.default_rng(4242)
        self.pk = rng.integers(-20, NB + 20, N).astype(np.int32)
        self.pv = rng.integers(-(1 << 40), 1 << 40, N).astype(np.int64)
        self.ps = [None if rng.random() < 0.1 else WORDS[i] for i in rng.integers(0, len(WORDS), N)]
        # P: dense unique keys (finalize_auto makes a perfect table); payload a_g INTEGER, a_s VARCHAR
        self.p_keys = rng.permutation(NB).astype(np.int32)
        self.a_g = rng.integers(0, 5, NB).astype(np.int32)
        self.a_s = [WORDS[i] for i in rng.integers(0, len(WORDS), NB)]
        self.a_s_valid = (rng.random(NB) > 0.08).astype(np.uint8)
        # U: unique sparse 4-byte keys (8-byte slots); R: every key twice (16-byte slots + row ids); payload r_v BIGINT
        self.u_keys = (rng.permutation(1 << 20)[:NB] * 1021 + 7).astype(np.int32)
        self.pu = np.where(rng.random(N) < 0.7, self.u_keys[rng.integers(0, NB, N)], rng.integers(0, 1 << 30, N)).astype(np.int32)
        self.r_keys = rng.permutation(np.repeat(np.arange(NB // 2, dtype=np.int32), 2))
        self.r_v = rng.integers(-1000, 1000, NB).astype(np.int64)
        self.pcols = [self.pk, self.pv, None, self.pu]  # (the VARCHAR column: cells are made per pipeline)
        self.joins = [Join(self.p_keys, PK, (0, NB - 1)), Join(self.r_keys, PK)]
        self.ref = Ref([self.pk], None, self.joins)
        self.rows = sort_rows(self.ref.rows())
        self.u_join = Join(self.u_keys, PU)
        self.u_ref = Ref(self.pcols, None, [self.u_join])
        self.expr_cols = {PK: (self.pk, None), PV: (self.pv, None), PS: self.ps, PU: (self.pu, None)}
        d = {}
        for s, ok in zip(self.a_s, self.a_s_valid):
            if ok:
                d.setdefault(s, len(d))
        self.a_words = list(d)  # first-appearance dictionary of a_s; NULL rows get the code len(a_words)
        self.a_codes = np.array([d[s] if ok else len(d) for s, ok in zip(self.a_s, self.a_s_valid)], np.uint32)

    def stage_counts(self, ref, path, tuples):
        """the reference's tuples after every stage of `path` for the source rows `tuples`"""
        prod = np.ones(len(tuples), np.int64)
        out = []
        for j in path:
            prod = prod * ref.counts[j][tuples]
            out.append(int(prod.sum()))
        return out


@pytest.fixture(scope="module")
def data():
    d = Data()
    assert len(d.rows) > N // 4 and not d.a_s_valid.all() and any(s is None for s in d.ps)
    return d


class Bank:
    """tables P, U, R and the pipeline (P, R) in two join orders, made on a context of the test's own.  `made` lists the
    handles in creation order"""

    def __init__(self, ctx, data, dictionary=True):
        d = self.d = data
        self.ctx, self.made = ctx, []
        a_cells, self.a_heap = string_blocks(d.a_s, d.a_s_valid, 2, 1)
        self.P = capi.HashTable.from_columns(ctx, [d.p_keys], [d.a_g, a_cells], payload_valid=[None, d.a_s_valid])
        self.P.set_payload_heaps(1, self.a_heap)
        self.code_col = None
        if dictionary:
            self.code_col, n_codes, has_null = self.P.encode_dictionary(1)
            assert (self.code_col, n_codes, has_null) == (2, len(d.a_words), 1)
        assert self.P.finalize_auto(0, NB - 1) == 1  # perfect
        self.U = capi.HashTable.from_columns(ctx, [d.u_keys]).finalize_hash()
        assert self.U.info()["kind"] == 2  # 8-byte slots
        self.R = capi.HashTable.from_columns(ctx, [d.r_keys], [d.r_v]).finalize_hash()
        assert self.R.info()["kind"] == 3  # 16-byte slots
        ps_cells, ps_valid, self.ps_heap = scanstr.cells(d.ps, 2)
        self.pipe = capi.Pipeline(ctx, [d.pk, d.pv, ps_cells, d.pu], N, [(self.P, [(-1, PK)]), (self.R, [(-1, PK)])],
                                  [[0, 1], [1, 0]], probe_valid=[None, None, ps_valid, None])
        self.pipe.set_probe_heaps(PS, self.ps_heap)
        self.made += [self.P, self.U, self.R, self.pipe]

    def output(self, pipe=None, n_rows=None):
        out = capi.Output(pipe or self.pipe, CAP, (len(self.d.rows) if n_rows is None else n_rows) // CAP + 1 + MAX_WAVE_CHUNKS)
        self.made.append(out)
        return out

    def mpx(self, pipe=None, routing="adaptive_reinit"):
        m = capi.DeviceMultiplexer(pipe or self.pipe, routing)
        self.made.append(m)
        return m

    def close(self, order):
        for h in order:
            h.close()


def whole_life(ctx, d):
    """everything a query makes, with the answers checked -> the Bank, not yet closed"""
    b = Bank(ctx, d)
    # the third table answers through a pipeline of its own: one round of the path kernel
    u_pipe = capi.Pipeline(ctx, [d.pk, d.pv, d.pv, d.pu], N, [(b.U, [(-1, PU)])], [[0]])
    b.made.append(u_pipe)
    assert u_pipe.probe_rounds([(0, N, 0, 0)])[0].tolist() == d.u_ref.stage_counts([0])
    out, m = b.output(), b.mpx()
    capi.run_resident([m], [(0, N // 1024)], out=out, reset=True, finish=True)
    st = m.finish()
    assert sum(st["input_tuple_count_per_path"]) == N
    assert sum(st["stage_out"][p][1] for p in range(2)) == len(d.rows)
    ids = out.fetch_ids()
    dev = device_rows(ids, d.joins)  # (in the order the sinks and materialize see the rows)
    assert np.array_equal(sort_rows(dev), d.rows)
    pr, ar, rr = dev[:, 0], dev[:, 1], dev[:, 2]
    ones = np.ones(len(dev), np.uint8)
    # polr_out_aggregate
    specs = [("count_star", -1, 0), ("sum", -1, PV), ("min", 0, 0), ("max", 0, 0), ("sum", 1, 0)]
    want = [len(dev), py_agg("sum", d.pv[pr], ones), py_agg("min", d.a_g[ar], ones), py_agg("max", d.a_g[ar], ones),
            py_agg("sum", d.r_v[rr], ones)]
    assert out.aggregate(specs) == want
    # the grouped sink, keyed by a_g and by the dictionary codes of a_s (NULL is the code after the last)
    nv = len(d.a_words) + 1
    vals, _counts, dropped = out.aggregate_grouped([(0, 0, 0, 5), (0, b.code_col, 0, nv)], [("count_star", -1, 0), ("sum", -1, PV)])
    assert dropped == 0 and len(vals) == 5 * nv
    for g in range(5):
        for c in range(nv):
            member = (d.a_g[ar] == g) & (d.a_codes[ar] == c)
            assert vals[g * nv + c][0] == int(member.sum()), (g, c)
            if member.any():
                assert vals[g * nv + c][1] == py_agg("sum", d.pv[pr][member], ones[member]), (g, c)
    # polr_out_aggregate_string over the probe column and the build column (both with a heap)
    ps_rows = [d.ps[i] for i in pr.tolist() if d.ps[i] is not None]
    as_rows = [d.a_s[i] for i in ar.tolist() if d.a_s_valid[i]]
    assert out.aggregate_string("min", -1, PS) == min(ps_rows) and out.aggregate_string("max", -1, PS) == max(ps_rows)
    assert out.aggregate_string("min", 0, 1) == min(as_rows) and out.aggregate_string("max", 0, 1) == max(as_rows)
    # polr_out_materialize to the host
    got, ok = out.materialize(-1, PV, np.int64)
    assert ok.all() and np.array_equal(got, d.pv[pr])
    got, ok = out.materialize(0, b.code_col, np.uint32)
    assert ok.all() and np.array_equal(got, d.a_codes[ar])
    got, ok = out.materialize(1, 0, np.int64)
    assert ok.all() and np.array_equal(got, d.r_v[rr])
    assert b.P.dictionary(b.code_col) == d.a_words
    return b


def test_whole_life_destroyed_in_creation_order(data):
    before = live_bytes()
    ctx = capi.Context(0)
    b = whole_life(ctx, data)
    assert capi.device_bytes_live() > before
    b.close(b.made)
    ctx.close()
    assert live_bytes() == before


def test_whole_life_context_destroyed_first(data):
    """polr_ctx_destroy first, then the children in reverse order: they keep the context alive and free what they own"""
    before = live_bytes()
    ctx = capi.Context(0)
    b = whole_life(ctx, data)
    ctx.close()
    assert capi.device_bytes_live() > before
    b.close(b.made[::-1])
    assert live_bytes() == before


def check_scan(pipe, want, V, what):
    sel, offs = pipe.fetch_scan()
    want_offs = scanstr.chunks_of(want, N, V)
    assert pipe.scan == (len(want), len(want_offs) - 1), what
    assert np.array_equal(sel, want) and np.array_equal(offs, want_offs), what


def test_every_grow_path_twice(data):
    d = data
    before = live_bytes()
    ctx = capi.Context(0)
    b = Bank(ctx, d)
    pipe = b.pipe
    all_rows = np.arange(N)

    def check_probe(sel, what):
        """one round over the whole source on each join order against the reference restricted to `sel`"""
        counts = pipe.probe_rounds([(0, len(sel), 0, 0), (0, len(sel), 1, 0)])
        assert counts[0].tolist() == d.stage_counts(d.ref, [0, 1], sel), what
        assert counts[1].tolist() == d.stage_counts(d.ref, [1, 0], sel), what

    # the scan buffers: 4 vectors, then 2 048
    cut = int(np.median(d.pv))
    want = np.nonzero(d.pv <= cut)[0].astype(np.uint32)
    for V in (1024, 2):
        assert pipe.scan_filter([(PV, "<=", cut)], vector_size=V) == (len(want), len(scanstr.chunks_of(want, N, V)) - 1)
        check_scan(pipe, want, V, V)
        check_probe(want, V)
    # the string tails: a VARCHAR constant longer than 12 bytes (twice: the second call finds the buffer)
    for op, const in ((">=", b"a string that lives in the heap too"), ("<", b"thirteen bytes")):
        pipe.scan_filter([(PS, op, const)])
        check_scan(pipe, scanstr.passing(d.ps, [(op, const)]), 1024, (op, const))
    # the pass bits (4 x 16 words, then 64 x 1) and the program buffer (its floor of 8 192 bytes, then 12 000 bytes of constants)
    small = ("or", ("cmp", PK, "<", 100), ("like", PS, b"J%"), ("not", ("in", PV, [int(x) for x in d.pv[:5]])))
    large = ("and", small) + tuple(("cmp", PS, "<>", bytes([65 + i]) * 4000) for i in range(3))
    for expr, V in ((small, 1024), (small, 64), (large, 64), (small, 1024)):
        pipe.scan_filter_expr(expr, vector_size=V)
        want = scanexpr.passing(expr, d.expr_cols, N)
        check_scan(pipe, want, V, (len(expr), V))
    check_probe(want, "expr")
    # a host selection, a scan, a host selection again: the selection in use switches between its two owners
    sel_a = np.nonzero(d.pk % 3 == 0)[0].astype(np.uint32)
    sel_b = np.nonzero(d.pk % 5 == 1)[0].astype(np.uint32)
    pipe.set_selection(sel_a)
    check_probe(sel_a, "host selection")
    want = np.nonzero(d.pv > cut)[0].astype(np.uint32)
    pipe.scan_filter([(PV, ">", cut)])
    check_scan(pipe, want, 1024, "scan after a host selection")
    check_probe(want, "scan after a host selection")
    pipe.set_selection(sel_b)
    check_probe(sel_b, "host selection after a scan")
    pipe.set_selection(None)
    check_probe(all_rows, "no selection")
    # the launch scratch of polr_probe_rounds: 1 round, then 80 (over the floor of 64), then 1 again
    for n_rounds in (1, 80, 1):
        step = N // n_rounds
        rounds = [(r * step, step, r % 2, 0) for r in range(n_rounds)]
        counts = pipe.probe_rounds(rounds)
        for r, (begin, count, path, _e) in enumerate(rounds):
            assert counts[r].tolist() == d.stage_counts(d.ref, [[0, 1], [1, 0]][path], all_rows[begin:begin + count]), (n_rounds, r)
    # resident runs led by one multiplexer: alone, then 4 and 9 executors of a stealing run (executor block, rings, share
    # records, stealing words)
    out = b.output()
    mpxs = [b.mpx() for _ in range(9)]
    n_chunks = N // 1024
    for n_exec in (1, 4, 9):
        out.reset()
        ctx.sync()
        ranges = [(e, e + 1) if e < n_chunks else (0, 0) for e in range(n_exec)] if n_exec > 1 else [(0, n_chunks)]
        if n_exec == 1:
            capi.run_resident(mpxs[:1], ranges, out=out, reset=True, finish=True)
        else:
            capi.run_resident_stealing(mpxs[:n_exec], ranges, 1, out=out, reset=True, finish=True)
        stats = capi.finish_many(mpxs[:n_exec])
        assert sum(sum(st["input_tuple_count_per_path"]) for st in stats) == N, n_exec
        assert sum(st["stage_out"][p][1] for st in stats for p in range(2)) == len(d.rows), n_exec
        assert np.array_equal(sort_rows(device_rows(out.fetch_ids(), d.joins)), d.rows), n_exec
    # polr_out_fuse_grouped twice on one output (a flat pipeline of perfect tables): fused, un-fused, fused again
    flat = capi.Pipeline(ctx, [d.pk, d.pv], N, [(b.P, [(-1, PK)]), (b.P, [(-1, PK)])], [[0, 1], [1, 0]])
    b.made.append(flat)
    assert flat.launch_info(True)["flat"] == 1
    fout = b.output(flat, n_rows=N)
    fm = b.mpx(flat)
    hit = (d.pk >= 0) & (d.pk < NB)
    g_of_row = d.a_g[np.argsort(d.p_keys)][np.clip(d.pk, 0, NB - 1)]  # a_g of the build row a probe key finds
    for keys, n_groups in (([(0, 0, 0, 5)], 5), ([(0, 0, 0, 5), (1, 0, 0, 5)], 25)):
        fout.fuse_grouped(keys, [("count_star", -1, 0), ("sum", -1, PK)])
        assert refused(fout.fuse_grouped, keys, [("count_star", -1, 0)]) == capi.E_INVALID  # (fused already)
        capi.run_resident([fm], [(0, n_chunks)], out=fout, reset=True, finish=True)
        fm.finish()
        vals, _counts, dropped = fout.fused_result()
        assert dropped == 0 and len(vals) == n_groups
        for g in range(5):
            member = hit & (g_of_row == g)
            cell = vals[g] if n_groups == 5 else vals[g * 5 + g]  # (both joins find the same build row)
            assert cell == [int(member.sum()), int(d.pk[member].astype(np.int64).sum())], (n_groups, g)
        assert sum(v[0] for v in vals) == int(hit.sum())
        fout.fuse_grouped(None, None)
    b.close(b.made[::-1])
    ctx.close()
    assert live_bytes() == before


def test_refused_calls_release_what_they_took(data):
    """ordinary error returns, each after the call had allocated something: the count is what it was before the call"""
    d = data
    before = live_bytes()
    ctx = capi.Context(0)
    # a 16-byte key column: refused after the columns were uploaded
    cells, _heap = string_blocks(d.a_s, d.a_s_valid, 1)
    assert refused(capi.HashTable.from_columns, ctx, [cells], [d.a_g]) == capi.E_UNSUPPORTED
    assert capi.device_bytes_live() == before
    # a duplicate key: the perfect attempt changes nothing, the hash build on the same handle answers right
    dup = Join(d.r_keys, PK)
    ht = capi.HashTable.from_columns(ctx, [d.r_keys], [d.r_v])
    uploaded = capi.device_bytes_live()
    info = ht.info()
    assert ht.finalize_perfect(0, NB // 2 - 1) is False
    assert capi.device_bytes_live() == uploaded and ht.info() == info and info["kind"] == 0
    ht.finalize_hash()
    assert ht.info()["kind"] == 3
    ps_cells, ps_valid, ps_heap = scanstr.cells(d.ps, 2)
    pipe = capi.Pipeline(ctx, [d.pk, d.pv, ps_cells], N, [(ht, [(-1, PK)])], [[0]], probe_valid=[None, None, ps_valid])
    ref = Ref([d.pk], None, [dup])
    assert pipe.probe_rounds([(0, N, 0, 0)])[0].tolist() == ref.stage_counts([0])
    # a string cell that points outside the ranges given (the second heap block is withheld)
    made = capi.device_bytes_live()
    assert refused(pipe.set_probe_heaps, PS, ps_heap[:1]) == capi.E_INVALID
    assert capi.device_bytes_live() == made
    pipe.set_probe_heaps(PS, ps_heap)  # (the column was left as it was: the whole heap is still accepted)
    # a column out of range, with rows in the output
    out = capi.Output(pipe, CAP, len(ref.rows()) // CAP + 1 + MAX_WAVE_CHUNKS)
    pipe.probe_rounds([(0, N, 0, 1)], out=out)
    assert out.stats()[0] == len(ref.rows()) > 0
    made = capi.device_bytes_live()
    assert refused(out.materialize, 0, 7, np.int64) == capi.E_INVALID
    assert refused(out.materialize, -1, 3, np.int64) == capi.E_INVALID
    assert capi.device_bytes_live() == made
    got, ok = out.materialize(0, 0, np.int64)
    assert ok.all() and np.array_equal(np.sort(got), np.sort(d.r_v[ref.rows()[:, 1]]))
    out.close()
    pipe.close()
    ht.close()
    ctx.close()
    assert live_bytes() == before
