"""LIP in the source scan (polr_pipeline_scan_filter_lip) against np.isin: the scan kernels keep a slot-by-slot probe of
their own (lip_contains, csrc/polr_scan.hip), a hand-written copy of the rule build and probe share -- perfect tables
sign-extend the key, hash tables zero-extend it, a NULL never joins, the all-ones 8-byte key lives beside an S16 table.

The reference: a source row survives join j's filter when its key is valid and equal to a valid build key (np.isin over
the two columns in their own type); several joins and the table filters AND.  Chunk boundaries as numpy_scan computes them
(common.chunk_bounds).  The run over the scan's chunks is held to joinref.Ref restricted to the expected rows and to
the unfiltered run: LIP thins the source, never the output."""
import numpy as np
import pytest

from common import chunk_bounds
from joinref import KEY_CASES, U64, Join, Ref, _key_case, chunks_for, device_rows, sort_rows
from polr_amd import capi

pytestmark = pytest.mark.gpu


def member(j, pcols, pvalid):
    """rows of the source whose key for join j is valid and equal to a valid build key"""
    bk = j.keys if j.valid is None else j.keys[j.valid.astype(bool)]
    ok = np.isin(pcols[j.src], bk)
    if pvalid is not None and pvalid[j.src] is not None:
        ok &= pvalid[j.src].astype(bool)
    return ok


def run_both(pipe, joins, path, n_chunks, n_rows, scan):
    """one DEFAULT_PATH multiplexer, a counting and an emitting run_resident -> per-position counts, sorted row set"""
    m = capi.DeviceMultiplexer(pipe, "default_path")
    if scan:
        m.use_scan_chunks()
    capi.run_resident([m], [(0, n_chunks)], reset=True, finish=True)
    counts = m.finish()["stage_out"][0]
    out = capi.Output(pipe, 1024, chunks_for(n_rows, 1024))
    capi.run_resident([m], [(0, n_chunks)], out=out, reset=True, finish=True)
    assert m.finish()["stage_out"][0] == counts
    rows = sort_rows(device_rows(out.fetch_ids(), joins))
    out.close()
    m.close()
    return counts, rows


def check_lip(ctx, joins, pcols, pvalid, path, filters=(), keep=None, masks=None, V=1024):
    """for every mask of joins: sel, n_selected and chunk_offsets of the scan == the reference, exactly; the counting run
    over the scan's chunks == Ref over the expected rows; for the full mask the emitting run too, and both end where the
    unfiltered run ends.  keep: what the table filters leave (None: everything) -> the expected selection of the full mask"""
    n = len(pcols[0])
    k = len(joins)
    ght = [j.device(ctx) for j in joins]
    pipe = capi.Pipeline(ctx, pcols, n, [(h, [(-1, j.src)]) for h, j in zip(ght, joins)], [path], probe_valid=pvalid)
    keep = np.ones(n, bool) if keep is None else keep
    plain = Ref(pcols, pvalid, joins, np.nonzero(keep)[0])
    want_rows = sort_rows(plain.rows())
    base_counts, base_rows = run_both(pipe, joins, path, (n + 1023) // 1024, len(want_rows), scan=False)
    if not filters:
        assert base_counts == plain.stage_counts(path) and np.array_equal(base_rows, want_rows)
    members = [member(j, pcols, pvalid) for j in joins]
    expect = None
    for mask in masks or range(1, 1 << k):
        ok = keep.copy()
        for x in range(k):
            if (mask >> x) & 1:
                ok &= members[x]
        expect, want_offs = chunk_bounds(np.nonzero(ok)[0].astype(np.uint32), n, V)
        n_sel, n_chunks = pipe.scan_filter(list(filters), vector_size=V, lip_joins=mask)
        sel, offs = pipe.fetch_scan()
        assert n_sel == len(expect) and n_chunks == len(want_offs) - 1, mask
        assert np.array_equal(sel, expect), mask
        assert np.array_equal(offs, want_offs), mask
        ref = Ref(pcols, pvalid, joins, expect)
        assert ref.stage_counts(path)[-1] == len(want_rows)  # (the reference agrees: LIP never changes the output)
        if mask == (1 << k) - 1:
            counts, rows = run_both(pipe, joins, path, n_chunks, len(want_rows), scan=True)
            assert np.array_equal(rows, sort_rows(ref.rows())) and np.array_equal(rows, want_rows)
            if not filters:
                assert np.array_equal(rows, base_rows)
        else:
            m = capi.DeviceMultiplexer(pipe, "default_path")
            m.use_scan_chunks()
            capi.run_resident([m], [(0, n_chunks)], reset=True, finish=True)
            counts = m.finish()["stage_out"][0]
            m.close()
        assert counts == ref.stage_counts(path), mask
        assert counts[-1] == len(want_rows)
        if not filters:
            assert counts[-1] == base_counts[-1]
    pipe.close()
    for h in ght:
        h.close()
    return expect, want_rows


@pytest.mark.parametrize("dt,kind", KEY_CASES, ids=["%s-%s" % (np.dtype(d).name, k) for d, k in KEY_CASES])
def test_lip_key_types(gpu_ctx, dt, kind):
    """every key dtype x perfect (ranges at the type's low end, middle, high end) / unique-hash / repeated-hash table: type
    min, max, 0, -1, the range's edges and their neighbours, NULLs on both sides"""
    j, pcols, pvalid = _key_case(dt, kind, seed=500 + KEY_CASES.index((dt, kind)))
    expect, want_rows = check_lip(gpu_ctx, [j], pcols, pvalid, [0])
    assert 100 < len(expect) < len(pcols[0]) and len(want_rows) >= len(expect)


@pytest.mark.parametrize("dt", [np.int64, np.uint64], ids=["int64", "uint64"])
@pytest.mark.parametrize("present", [True, False], ids=["with-build-rows", "without"])
def test_lip_all_ones_key(gpu_ctx, dt, present):
    """the key whose 64 bits are all ones (int64 -1, uint64 max) is the empty marker of an S16 table's slots: its build
    rows are kept beside the table.  Source rows with that key, valid and NULL, survive the scan exactly when a valid
    build row has it -- a NULL build row with those bits does not count"""
    rng = np.random.default_rng(700 + int(present))
    info = np.iinfo(dt)
    ones = np.array([U64], dtype=np.uint64).astype(dt)[0]
    distinct = np.unique(rng.integers(info.min, info.max, 2000, dtype=dt, endpoint=True))
    distinct = distinct[distinct != ones]
    bk = np.repeat(distinct, 1 + np.arange(len(distinct)) % 3)
    bvalid = (rng.random(len(bk)) > 0.03).astype(np.uint8)
    extra = [(ones, 0), (ones, 0)] + ([(ones, 1)] * 3 if present else [])
    bk = np.concatenate([bk, np.array([e[0] for e in extra], dtype=dt)])
    bvalid = np.concatenate([bvalid, np.array([e[1] for e in extra], dtype=np.uint8)])
    perm = rng.permutation(len(bk))
    j = Join(bk[perm], 0, None, bvalid[perm], [np.arange(len(bk), dtype=np.int32)])
    ht = j.device(gpu_ctx)
    assert ht.info()["kind"] == 3
    ht.close()
    n = 20_000
    pk = np.concatenate([np.full(n // 4, ones, dtype=dt), rng.choice(distinct, n // 2),
                         rng.integers(info.min, info.max, n - n // 4 - n // 2, dtype=dt, endpoint=True)])
    pk = rng.permutation(pk)
    pvalid = [(rng.random(n) > 0.1).astype(np.uint8)]
    with_ones = pk == ones
    assert (with_ones & (pvalid[0] == 1)).sum() > 1000 and (with_ones & (pvalid[0] == 0)).sum() > 100
    expect, _ = check_lip(gpu_ctx, [j], [pk], pvalid, [0])
    survivors = with_ones[expect]
    if present:
        assert survivors.sum() == (with_ones & (pvalid[0] == 1)).sum()
    else:
        assert not survivors.any()


def _three_joins(rng, n):
    """join 0: S16 (repeated int64 keys, the largest), join 1: perfect over int16 (the smallest), join 2: S8 (unique int32):
    ordered by size the scan tests 1, 2, 0.  The int16 and the int32 probe columns are nullable."""
    d0 = np.unique(rng.integers(-2**62, 2**62, 6000, dtype=np.int64))
    k0 = rng.permutation(np.repeat(d0, 2))
    j0 = Join(k0, 0, None, (rng.random(len(k0)) > 0.02).astype(np.uint8), [np.arange(len(k0), dtype=np.int64)])
    k1 = np.arange(-200, 800, dtype=np.int16)
    k1 = rng.permutation(k1[k1 % 7 != 3])
    j1 = Join(k1, 1, (-200, 799), None, [])
    k2 = rng.choice(np.arange(-10**9, 10**9, 977, dtype=np.int64), 1500, replace=False).astype(np.int32)
    j2 = Join(k2, 2, None, (rng.random(len(k2)) > 0.02).astype(np.uint8), [np.arange(len(k2), dtype=np.int32)])
    pcols = [np.where(rng.random(n) < 0.8, rng.choice(d0, n), rng.integers(-2**62, 2**62, n, dtype=np.int64)),
             rng.integers(-260, 860, n).astype(np.int16),
             np.where(rng.random(n) < 0.8, rng.choice(k2, n), rng.integers(-10**9, 10**9, n)).astype(np.int32),
             rng.integers(0, 100, n).astype(np.int32)]
    pvalid = [None, (rng.random(n) > 0.05).astype(np.uint8), (rng.random(n) > 0.05).astype(np.uint8), None]
    return [j0, j1, j2], pcols, pvalid


def test_lip_three_joins_of_three_kinds(gpu_ctx):
    """a perfect, an S8 and an S16 table on probe columns of 2, 4 and 8 bytes in one scan, with two table filters (one of
    them on a nullable LIP key column): every non-empty mask of the three joins against the AND of the single expectations;
    the tables' sizes put the joins in another order in the scan than in the pipeline"""
    rng = np.random.default_rng(710)
    n = 30_000
    joins, pcols, pvalid = _three_joins(rng, n)
    ght = [j.device(gpu_ctx) for j in joins]
    infos = [h.info() for h in ght]
    for h in ght:
        h.close()
    assert [i["kind"] for i in infos] == [3, 1, 2]
    assert infos[1]["device_bytes"] < infos[2]["device_bytes"] < infos[0]["device_bytes"]
    filters = [(1, ">=", 10), (3, "<", 70)]
    keep = (pcols[1] >= 10) & pvalid[1].astype(bool) & (pcols[3] < 70)
    expect, want_rows = check_lip(gpu_ctx, joins, pcols, pvalid, [0, 1, 2], filters=filters, keep=keep)
    assert 1000 < len(expect) < keep.sum() and len(want_rows) > 1000


def test_lip_refusals_leave_the_previous_scan(gpu_ctx):
    """a mask bit beyond the pipeline's joins, a two-key join, a join that compares its key by value and one with
    NULL = NULL (packed form) are refused; after each, the scan before it is what fetch_scan returns and what its
    multiplexer runs over"""
    rng = np.random.default_rng(720)
    n = 20_000
    k0 = rng.choice(np.arange(0, 10**6, 7, dtype=np.int64), 2000, replace=False).astype(np.int32)
    a = rng.integers(0, 40, 600).astype(np.int32)
    b = rng.integers(0, 40, 600).astype(np.int32)
    pair = np.unique(a.astype(np.int64) * 64 + b)
    a, b = (pair // 64).astype(np.int32), (pair % 64).astype(np.int32)
    k2 = rng.permutation(np.arange(0, 300, dtype=np.int64))[:250]
    k3 = rng.permutation(np.arange(0, 500, dtype=np.int32))[:400]
    pcols = [np.where(rng.random(n) < 0.8, rng.choice(k0, n), rng.integers(0, 10**6, n)).astype(np.int32),
             rng.integers(0, 40, n).astype(np.int32), rng.integers(0, 40, n).astype(np.int32),
             rng.integers(0, 300, n).astype(np.int64), rng.integers(0, 500, n).astype(np.int32),
             rng.integers(0, 100, n).astype(np.int32)]
    hts = [capi.HashTable.from_columns(gpu_ctx, [k0], []).finalize_hash(),
           capi.HashTable.from_columns(gpu_ctx, [a, b], []).finalize_hash()]
    for keys, flag in ((k2, capi.KEY_BY_VALUE), (k3, capi.KEY_NULL_EQUAL)):
        h = capi.HashTable.from_columns(gpu_ctx, [keys], [])
        h.set_key_flags(0, flag)
        hts.append(h.finalize_hash())
    pipe = capi.Pipeline(gpu_ctx, pcols, n, [(hts[0], [(-1, 0)]), (hts[1], [(-1, 1), (-1, 2)]), (hts[2], [(-1, 3)]),
                                             (hts[3], [(-1, 4)])], [[0, 1, 2, 3]])
    # the reference sees the two-key join as one over the pair's number
    ref_cols = [pcols[0], pcols[1].astype(np.int64) * 64 + pcols[2], pcols[3], pcols[4]]
    ref_joins = [Join(k0, 0), Join(pair, 1), Join(k2, 2), Join(k3, 3)]
    flt = [(5, "<", 60)]
    n_sel, n_chunks = pipe.scan_filter(flt, vector_size=64, lip_joins=1)
    sel0, offs0 = pipe.fetch_scan()
    expect, want_offs = chunk_bounds(np.nonzero((pcols[5] < 60) & np.isin(pcols[0], k0))[0].astype(np.uint32), n, 64)
    assert np.array_equal(sel0, expect) and np.array_equal(offs0, want_offs)
    m = capi.DeviceMultiplexer(pipe, "default_path")
    m.use_scan_chunks()
    want = Ref(ref_cols, None, ref_joins, expect).stage_counts([0, 1, 2, 3])
    assert want[-1] > 100

    def previous_scan_intact():
        sel, offs = pipe.fetch_scan()
        assert np.array_equal(sel, sel0) and np.array_equal(offs, offs0)
        capi.run_resident([m], [(0, n_chunks)], reset=True, finish=True)
        assert m.finish()["stage_out"][0] == want

    previous_scan_intact()
    for mask, code in [(1 << 4, capi.E_INVALID), (1 | 1 << 4, capi.E_INVALID), (1 | 1 << 1, capi.E_INVALID),
                       (1 << 2, capi.E_UNSUPPORTED), (1 | 1 << 3, capi.E_UNSUPPORTED)]:
        with pytest.raises(capi.PolrError) as e:
            pipe.scan_filter(flt, vector_size=64, lip_joins=mask)
        assert e.value.code == code and "LIP" in str(e.value), mask
        previous_scan_intact()
    m.close()
    pipe.close()
    for h in hts:
        h.close()
