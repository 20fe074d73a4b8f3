"""polr_ht_semi_filter (HashTable.semi_filter): an un-finalized build side thinned by SEMI / ANTI joins against finalized tables
and compacted on the device.

The reference is never the code under test.  htsemi.kept over the host columns gives the kept rows (np.isin with the NULL
rules of the contract; it is pinned to the reference engine by tests/golden/semi_build.json); a TWIN table is built with
HashTable.from_columns from the numpy-filtered host columns (the Side of tests/test_gpu_ht_filter.py).  Then filter_rows()
must equal the expected rows, every payload column materialised through a one-join probe pipeline must equal the twin's, and
the pipeline's row set -- build id -> filter_rows -> uploaded row -- must equal the twin's and joinref.Ref over the filtered
build side (check_downstream of that file).  SEMI and ANTI of one filter must partition the table, the rows whose key is NULL
on the ANTI side.

Tiles are 1024 rows, a pass-bit word 64, the prefix over the tile counts takes 1024 tiles a step (and the counting kernel's
other build gives a lane one row of each of four consecutive words): the row counts are the edges of all of them."""
import json
import os

import numpy as np
import pytest

import buildside
import common
import htsemi
import scanexpr
import scanstr
from joinref import MAX_WAVE_CHUNKS, Join, Ref, sort_rows
from polr_amd import capi
from test_gpu_from_output import probe_b
from test_gpu_ht_filter import DTS, Side, check_downstream, finalize, raw_columns, string_side

pytestmark = pytest.mark.gpu

BY_VALUE, NULL_EQUAL = capi.KEY_BY_VALUE, capi.KEY_NULL_EQUAL
PERFECT, S8, S16 = 1, 2, 3


class By:
    """a `by` table on the host: keys, validity, how it is finalized, its key flags; kind: the index it must come out as"""

    def __init__(self, keys, valid=None, how="hash", flags=None, kind=None):
        self.keys = [np.ascontiguousarray(k) for k in keys]
        self.valid = list(valid) if valid else [None] * len(self.keys)
        self.how, self.flags, self.kind = how, list(flags) if flags else [0] * len(self.keys), kind

    def device(self, ctx):
        ht = capi.HashTable.from_columns(ctx, self.keys, key_valid=self.valid)
        for c, fl in enumerate(self.flags):
            if fl:
                ht.set_key_flags(c, fl)
        kind = finalize(ht, self.how)
        assert self.kind is None or kind == self.kind, (kind, self.kind)
        return ht

    def rows(self):
        """the rows the index can hold: a perfect table skips the keys outside its range"""
        if self.how != "hash" and self.how[0] == "perfect":
            return np.nonzero((self.keys[0] >= self.how[1]) & (self.keys[0] <= self.how[2]))[0]
        return np.arange(len(self.keys[0]))


def spec(side, by, cols, anti=False):
    c, keep = side.cols(), by.rows()
    return ([c[x][0] for x in cols], [c[x][1] for x in cols], [k[keep] for k in by.keys],
            [None if v is None else v[keep] for v in by.valid], anti, [f & NULL_EQUAL for f in by.flags], [f & BY_VALUE for f in by.flags])


def want_rows(side, filters):
    return np.nonzero(htsemi.kept(side.n, [spec(side, *f) for f in filters]))[0].astype(np.uint32)


def semi(ctx, side, filters, ht=None, how="hash", downstream=True, want=None, **upload):
    """upload, thin by filters [(By, cols, anti)] in ONE call, check -> the kept rows"""
    want = want_rows(side, filters) if want is None else want
    own = ht is None
    ht = ht or side.upload(ctx, **upload)
    bys = {id(f[0]): f[0].device(ctx) for f in filters}
    assert ht.semi_filter([(bys[id(b)], cols, anti) for b, cols, anti in filters]) == len(want)
    for b in bys.values():
        b.close()  # (`by` is only read and may be destroyed after the call)
    if downstream:
        check_downstream(ctx, side, want, ht, how)
    else:
        assert np.array_equal(ht.filter_rows(), want)
    if own:
        ht.close()
    return want


def partition(ctx, side, by, cols, downstream=False, **kw):
    """SEMI and ANTI of one filter on fresh tables: disjoint, together every row, the NULL-key rows on the ANTI side"""
    s = semi(ctx, side, [(by, cols, False)], downstream=downstream, **kw)
    a = semi(ctx, side, [(by, cols, True)], downstream=downstream, **kw)
    assert len(np.intersect1d(s, a)) == 0 and np.array_equal(np.union1d(s, a), np.arange(side.n))
    c, null = side.cols(), np.zeros(side.n, bool)
    for x, fl in zip(cols, by.flags):
        if not fl & NULL_EQUAL and c[x][1] is not None:
            null |= c[x][1] == 0
    assert np.isin(np.nonzero(null)[0], a).all()
    return s, a


# ---- 1. shapes: row counts x kept-row patterns ------------------------------------------------------------------------------
def patterns(n):
    i = np.arange(n)
    return {"none": np.zeros(n, bool), "all": np.ones(n, bool), "alternate": i % 2 == 1, "word": (i // 64) % 2 == 1,
            "lane_rows": (i // 64) % 4 == 2}  # every fourth word only (the third of a lane's rows in the four-row build)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1023, 1024, 1025, 4097])
def test_row_counts_and_patterns(gpu_ctx, n):
    rng = np.random.default_rng(n)
    key = rng.permutation(n).astype(np.int32)
    pay = rng.integers(-(1 << 40), 1 << 40, n).astype(np.int64)
    by = By([np.array([7], np.int32)], kind=S8)
    for name, keep in patterns(n).items():
        side = Side([key], [np.where(keep, 7, 3).astype(np.int32), pay], pvalid=[None, (rng.random(n) > 0.3).astype(np.uint8)])
        s, a = partition(gpu_ctx, side, by, [1], downstream=name == "alternate")
        assert np.array_equal(s, np.nonzero(keep)[0]), name
    side = Side([key], [pay])
    assert len(semi(gpu_ctx, side, [])) == n  # n_filters == 0 keeps every row, compacts and sets the row list


def test_more_tiles_than_one_prefix_step(gpu_ctx):
    """1026 tiles: the prefix over the tile counts carries from its first step of 1024 tiles into the second"""
    n = 1024 * 1024 + 1025
    i = np.arange(n)
    flag = ((i % 3 == 0) | (i >= n - 1500) | ((i // 1024) == 1023)).astype(np.uint8)
    flag[1024 * 1024 - 700:1024 * 1024] = 0
    side = Side([i.astype(np.int32)], [flag])
    want = np.nonzero(flag)[0].astype(np.uint32)
    by = By([np.array([1, 1, 9], np.uint8)], kind=S16).device(gpu_ctx)
    ht = side.upload(gpu_ctx)
    assert ht.semi_filter([(by, [1], False)]) == len(want)
    rows = ht.filter_rows()
    assert np.array_equal(rows, want)
    ht.finalize_hash()
    rng = np.random.default_rng(5)
    pk = np.concatenate([rng.integers(0, n, 4000), np.arange(n - 2100, n), np.arange(1024 * 1024 - 1100, 1024 * 1024 + 100)]).astype(np.int32)
    ids, mats = probe_b(gpu_ctx, ht, [pk], None, [np.uint8])
    hit = flag[pk].astype(bool)
    assert np.array_equal(ids[:, 0], np.nonzero(hit)[0]) and np.array_equal(rows[ids[:, 1]], pk[hit]) and mats[0][0].all()
    ht.close()
    by.close()


# ---- 2. every kind of `by` ---------------------------------------------------------------------------------------------------
def keyed_side(key, valid=None, seed=0):
    rng = np.random.default_rng(seed)
    n = len(key)
    return Side([np.arange(n, dtype=np.int32)], [key, rng.integers(0, 1000, n).astype(np.int16)], None, [valid, None])


def test_perfect_by_with_a_negative_minimum(gpu_ctx):
    rng = np.random.default_rng(1)
    keys = np.concatenate([rng.integers(-70, 70, 2500), [-51, -50, 49, 50, -2 ** 31, 2 ** 31 - 1]]).astype(np.int32)
    side = keyed_side(keys, (rng.random(len(keys)) > 0.1).astype(np.uint8))
    held = np.arange(-50, 50, 2, dtype=np.int32)  # every second value of [-50, 48], and the range's last value 49
    by = By([np.concatenate([held, [49, -60, 90]]).astype(np.int32)], how=("perfect", -50, 49), kind=PERFECT)
    s, a = partition(gpu_ctx, side, by, [1], downstream=True)
    vals = set(keys[s].tolist())
    assert {-50, 49} <= vals and not vals & {-51, 50, -60, 90, -2 ** 31, 2 ** 31 - 1} and len(s) > 300
    # an unsigned perfect table, and the one polr_pht_upload makes
    ukeys = rng.integers(0, 300, 2000).astype(np.uint16)
    uside = keyed_side(ukeys)
    partition(gpu_ctx, uside, By([np.arange(100, 200, dtype=np.uint16)], how=("perfect", 100, 199), kind=PERFECT), [1])
    pht = capi.HashTable.from_perfect(gpu_ctx, 2, False, 100, 199, (np.arange(100) % 3 == 0).astype(np.uint8))
    ht = uside.upload(gpu_ctx)
    want = np.nonzero((ukeys >= 100) & (ukeys <= 199) & ((ukeys.astype(np.int64) - 100) % 3 == 0))[0]
    assert ht.semi_filter([(pht, [1], False)]) == len(want) and np.array_equal(ht.filter_rows(), want)
    ht.close()
    pht.close()


def test_unique_key_hash_by(gpu_ctx):
    rng = np.random.default_rng(2)
    keys = rng.integers(-500, 2500, 3000).astype(np.int32)
    side = keyed_side(keys, (rng.random(3000) > 0.1).astype(np.uint8))
    by = By([rng.permutation(4000)[:1000].astype(np.int32) - 600], [(rng.random(1000) > 0.05).astype(np.uint8)], kind=S8)
    s, a = partition(gpu_ctx, side, by, [1], downstream=True)
    assert 300 < len(s) < 2000


def test_run_hash_by_and_the_all_ones_key(gpu_ctx):
    """repeated keys count once; the all-ones 8-byte key lives beside the slots, and is found or missed there"""
    rng = np.random.default_rng(3)
    ones = np.uint64(2 ** 64 - 1)
    keys = rng.integers(0, 600, 3000).astype(np.uint64)
    keys[::50] = ones
    side = keyed_side(keys, (rng.random(3000) > 0.1).astype(np.uint8))
    rep = np.repeat(rng.permutation(600)[:200].astype(np.uint64), 3)
    with_ones = By([np.concatenate([rep, [ones, ones]])], kind=S16)
    without = By([rep], kind=S16)
    s, _ = partition(gpu_ctx, side, with_ones, [1], downstream=True)
    t, _ = partition(gpu_ctx, side, without, [1])
    assert (keys[s] == ones).sum() > 10 and not (keys[t] == ones).any() and len(t) > 300
    # signed 8-byte keys: -1 is the same bit pattern
    skeys = rng.integers(-3, 3, 1000).astype(np.int64)
    s, _ = partition(gpu_ctx, keyed_side(skeys), By([np.array([-1, -1, 2], np.int64)], kind=S16), [1])
    assert set(skeys[s].tolist()) == {-1, 2}


def test_empty_and_all_null_by(gpu_ctx):
    rng = np.random.default_rng(4)
    keys = rng.integers(0, 50, 1500).astype(np.int32)
    side = keyed_side(keys, (rng.random(1500) > 0.1).astype(np.uint8))
    for by in (By([np.zeros(0, np.int32)]), By([np.arange(40, dtype=np.int32)], [np.zeros(40, np.uint8)]),
               By([np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32)])):
        cols = [1] * len(by.keys)
        s, a = partition(gpu_ctx, side, by, cols)
        assert len(s) == 0 and len(a) == side.n  # SEMI keeps none, ANTI keeps all


def test_tiny_tables_and_colliding_absent_keys(gpu_ctx):
    """<= 8 build rows: the probe sequences of thousands of absent keys start at every slot of the table, run over slot-group
    boundaries and wrap at its end"""
    rng = np.random.default_rng(5)
    for dt, kind in ((np.int32, S8), (np.int64, S16)):
        held = rng.permutation(1 << 20)[:8].astype(dt)
        keys = np.concatenate([rng.integers(0, 1 << 20, 6000), held, held]).astype(dt)
        s, a = partition(gpu_ctx, keyed_side(keys), By([held], kind=kind), [1])
        assert np.array_equal(np.sort(np.unique(keys[s])), np.sort(held)) and len(s) >= 16
        rep = np.repeat(held[:4], 2)  # a run hash table of four keys, each twice
        s, a = partition(gpu_ctx, keyed_side(keys), By([rep], kind=S16), [1])
        assert np.array_equal(np.sort(np.unique(keys[s])), np.sort(held[:4]))


# ---- 3. key forms ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS, ids=[np.dtype(d).name for d in DTS])
def test_key_widths_signed_and_unsigned(gpu_ctx, dt):
    rng = np.random.default_rng(np.dtype(dt).itemsize * 2 + (np.dtype(dt).kind == "i"))
    info = np.iinfo(dt)
    lo, hi = max(int(info.min), -100), min(int(info.max), 100)
    keys = rng.integers(lo, hi, 2200, dtype=dt, endpoint=True)
    keys[:4] = [info.min, info.max, info.min, info.max]
    valid = (rng.random(2200) > 0.1).astype(np.uint8)
    # the column as a KEY of the table, and as its payload
    as_key = Side([keys], [rng.integers(0, 9, 2200).astype(np.int8)], [valid], None)
    as_pay = keyed_side(keys, valid)
    held = np.concatenate([rng.integers(lo, hi, 60, dtype=dt, endpoint=True), [info.max]]).astype(dt)
    by = By([held])
    s, _ = partition(gpu_ctx, as_key, by, [0], downstream=True)
    t, _ = partition(gpu_ctx, as_pay, by, [1])
    assert np.array_equal(s, t) and 0 < len(s) < 2200 and int(info.max) in keys[s].tolist()
    assert set(keys[s].tolist()) == set(held.tolist()) & set(keys[valid != 0].tolist())
    uniq = np.unique(held[held != info.max])
    partition(gpu_ctx, as_pay, By([uniq], how=("perfect", lo, hi), kind=PERFECT), [1])


def test_two_keys_in_plain_form(gpu_ctx):
    rng = np.random.default_rng(6)
    n = 2500
    k0, k1 = rng.integers(-8, 8, n).astype(np.int32), rng.integers(0, 12, n).astype(np.uint16)
    side = Side([k0], [k1, rng.integers(0, 99, n).astype(np.int64)], [(rng.random(n) > 0.1).astype(np.uint8)], [(rng.random(n) > 0.1).astype(np.uint8), None])
    b0, b1 = rng.integers(-8, 8, 60).astype(np.int32), rng.integers(0, 12, 60).astype(np.uint16)
    by = By([b0, b1], [None, (rng.random(60) > 0.1).astype(np.uint8)], kind=S16)
    s, a = partition(gpu_ctx, side, by, [0, 1], downstream=True)
    assert 100 < len(s) < n - 100
    # the same pair the other way round: the columns are paired with by's keys in the order of cols[]
    partition(gpu_ctx, side, By([b1, b0], kind=S16), [1, 0])


@pytest.mark.parametrize("n_keys", [3, 4])
def test_packed_keys(gpu_ctx, n_keys):
    rng = np.random.default_rng(7 + n_keys)
    n = 2400
    dts = [np.int8, np.int32, np.uint16, np.int64][:n_keys]
    cols = [rng.integers(-3, 4, n).astype(dt) if np.dtype(dt).kind == "i" else rng.integers(0, 5, n).astype(dt) for dt in dts]
    valid = [(rng.random(n) > 0.05).astype(np.uint8) if c % 2 == 0 else None for c in range(n_keys)]
    side = Side([np.arange(n, dtype=np.int32)], cols, None, valid)
    bk = [rng.integers(-2, 3, 90).astype(dt) if np.dtype(dt).kind == "i" else rng.integers(1, 4, 90).astype(dt) for dt in dts]
    by = By(bk, [(rng.random(90) > 0.05).astype(np.uint8)] + [None] * (n_keys - 1), kind=S16)
    s, a = partition(gpu_ctx, side, by, list(range(1, 1 + n_keys)), downstream=True)
    assert 50 < len(s) < n - 50  # (values outside by's per-column ranges among the rest: -3, 3, 0, 4)


def test_keys_compared_by_value(gpu_ctx):
    """POLR_KEY_BY_VALUE with a narrower and a wider column on the table's side, values the other width cannot hold"""
    rng = np.random.default_rng(8)
    n = 2000
    narrow = rng.integers(-128, 127, n, endpoint=True).astype(np.int8)
    wide = np.concatenate([rng.integers(-200, 400, n - 6), [255, 256, -1, 2 ** 40, -2 ** 40, 65535]]).astype(np.int64)
    unsigned = rng.integers(0, 65535, n, endpoint=True).astype(np.uint16)
    narrow[:4], unsigned[:4] = [-1, 0, 7, -56], [65535, 255, 127, 300]
    side = Side([np.arange(n, dtype=np.int32)], [narrow, wide, unsigned])
    held16 = np.concatenate([rng.integers(-200, 300, 80), [255, -1, 127, -128]]).astype(np.int16)
    by16 = By([held16], flags=[BY_VALUE], kind=S16)
    s, _ = partition(gpu_ctx, side, by16, [1], downstream=True)   # int8 column against an int16 key
    t, _ = partition(gpu_ctx, side, by16, [2])                    # int64 column: 2^40, 256 < ... never match a value it lacks
    u, _ = partition(gpu_ctx, side, by16, [3])                    # uint16 column: 65535 is not -1
    assert set(narrow[s].tolist()) == set(held16.tolist()) & set(narrow.tolist())
    assert set(wide[t].tolist()) == set(held16.tolist()) & set(wide.tolist()) and 2 ** 40 not in wide[t].tolist()
    assert 65535 not in unsigned[u].tolist() and 255 in unsigned[u].tolist()
    held8 = np.array([255, 0, 7, 200], np.uint8)
    v, _ = partition(gpu_ctx, side, By([held8], flags=[BY_VALUE], kind=S16), [1])  # int8 -1 is not uint8 255
    assert set(narrow[v].tolist()) == {0, 7}
    # without the flag the widths must agree
    ht, by = side.upload(gpu_ctx), By([held16]).device(gpu_ctx)
    with pytest.raises(capi.PolrError) as e:
        ht.semi_filter([(by, [1], False)])
    assert e.value.code == capi.E_INVALID and "column 1 is 1 bytes, the key of `by` 2 bytes" in str(e.value)
    ht.close()
    by.close()


def test_null_equals_null(gpu_ctx):
    """POLR_KEY_NULL_EQUAL: a NULL row matches iff `by` kept a NULL key"""
    rng = np.random.default_rng(9)
    n = 1800
    keys, valid = rng.integers(0, 40, n).astype(np.int32), (rng.random(n) > 0.15).astype(np.uint8)
    side = keyed_side(keys, valid)
    held = rng.integers(0, 40, 12).astype(np.int32)
    hv = np.ones(12, np.uint8)
    without_null = By([held], [hv.copy()], flags=[NULL_EQUAL], kind=S16)
    hv[3] = 0
    with_null = By([held], [hv], flags=[NULL_EQUAL], kind=S16)
    s, a = partition(gpu_ctx, side, with_null, [1], downstream=True)
    t, b = partition(gpu_ctx, side, without_null, [1])
    null = np.nonzero(valid == 0)[0]
    assert np.isin(null, s).all() and np.isin(null, b).all() and len(null) > 100
    # two keys, NULL = NULL on the second only
    k2, v2 = rng.integers(0, 3, n).astype(np.int8), (rng.random(n) > 0.2).astype(np.uint8)
    side2 = Side([np.arange(n, dtype=np.int32)], [keys, k2], None, [valid, v2])
    by2 = By([held, rng.integers(0, 3, 12).astype(np.int8)], [None, hv], flags=[0, NULL_EQUAL], kind=S16)
    s2, a2 = semi(gpu_ctx, side2, [(by2, [1, 2], False)], downstream=False), semi(gpu_ctx, side2, [(by2, [1, 2], True)], downstream=False)
    assert len(s2) > 0 and (v2[s2] == 0).any() and valid[s2].all() and len(s2) + len(a2) == n


# ---- 4. several filters, composition ------------------------------------------------------------------------------------------
def four_filters(rng, n):
    side = Side([rng.integers(0, 400, n).astype(np.int32)],
                [rng.integers(0, 60, n).astype(np.int16), rng.integers(0, 30, n).astype(np.uint64), rng.integers(0, 9, n).astype(np.int8)],
                [(rng.random(n) > 0.05).astype(np.uint8)], [(rng.random(n) > 0.05).astype(np.uint8), None, None])
    filters = [(By([np.arange(0, 400, 3, dtype=np.int32)], how=("perfect", 0, 399), kind=PERFECT), [0], False),
               (By([rng.integers(0, 60, 25).astype(np.int16)], kind=S16), [1], True),
               (By([rng.permutation(30)[:22].astype(np.uint64)], kind=S16), [2], False),
               (By([np.arange(0, 400, 2, dtype=np.int32), np.repeat(np.arange(8, dtype=np.int8), 25)], kind=S16), [0, 3], True)]
    return side, filters


@pytest.mark.parametrize("n_filters", [1, 2, 4])
def test_filters_in_one_call_equal_successive_calls(gpu_ctx, n_filters):
    rng = np.random.default_rng(20)
    side, filters = four_filters(rng, 3000)
    filters = filters[:n_filters]
    want = semi(gpu_ctx, side, filters)
    assert 0 < len(want) < side.n
    ht = side.upload(gpu_ctx)
    for by, cols, anti in filters:  # one call each: the row list composes
        d = by.device(gpu_ctx)
        ht.semi_filter([(d, cols, anti)])
        d.close()
    check_downstream(gpu_ctx, side, want, ht)
    ht.close()
    # the order of the filters in the call changes nothing
    assert np.array_equal(semi(gpu_ctx, side, filters[::-1], downstream=False), want)


def test_constant_filter_then_semi_filter(gpu_ctx):
    """polr_ht_filter first: filter_rows() is the composed list against the rows as uploaded"""
    rng = np.random.default_rng(21)
    side, filters = four_filters(rng, 3000)
    expr = ("and", ("cmp", 3, "<", 6), ("cmp", 1, "is not null"))
    first = scanexpr.passing(expr, side.cols(), side.n)
    keep = np.zeros(side.n, bool)
    keep[first] = True
    want = np.nonzero(keep & htsemi.kept(side.n, [spec(side, *f) for f in filters[:2]]))[0].astype(np.uint32)
    ht = side.upload(gpu_ctx)
    assert ht.filter(expr) == len(first)
    semi(gpu_ctx, side, filters[:2], ht=ht, want=want)
    assert 0 < len(want) < len(first)
    ht.close()
    # ... and an empty call on a filtered table keeps every row and the list
    ht = side.upload(gpu_ctx)
    ht.filter(expr)
    assert ht.semi_filter([]) == len(first) and np.array_equal(ht.filter_rows(), first)
    ht.close()


def test_constant_filter_after_a_semi_filter_is_refused(gpu_ctx):
    rng = np.random.default_rng(22)
    side, filters = four_filters(rng, 2000)
    ht = side.upload(gpu_ctx)
    want = semi(gpu_ctx, side, filters[:1], ht=ht, downstream=False)
    live1, info1 = capi.device_bytes_live(), ht.info()
    with pytest.raises(capi.PolrError) as e:
        ht.filter(("cmp", 3, "<", 6))
    assert e.value.code == capi.E_INVALID and "the table was filtered already (once per table)" in str(e.value)
    assert capi.device_bytes_live() == live1 and ht.info() == info1
    check_downstream(gpu_ctx, side, want, ht)
    ht.close()


GOLD = json.load(open(os.path.join(common.ROOT, "tests", "golden", "semi_build.json"), encoding="utf-8"))


def test_fixture_of_the_reference_engine(gpu_ctx):
    """every query of tests/golden/semi_build.json on the device: the constant conditions through polr_ht_filter, each
    subquery's rows as a finalized table, then one polr_ht_semi_filter -- the kept ids are the recorded row sets"""
    tables = htsemi.fixture_tables(GOLD["seed"], GOLD["n_rows"])
    assert htsemi.tables_digest(tables) == GOLD["tables_sha1"]
    d = tables["d"]
    names = ["id", "k", "k2"]
    cells, ok, blocks = scanstr.cells(d["s"][0], n_blocks=1)
    for q in GOLD["queries"]:
        ht = capi.HashTable.from_columns(gpu_ctx, [d["id"][0]], [d["k"][0], d["k2"][0], cells],
                                         payload_valid=[d["k"][1], d["k2"][1], ok])
        ht.set_payload_heaps(2, blocks)
        if q.get("const"):
            conds = [("cmp", names.index(c[0]), c[1]) + tuple(c[2:]) for c in q["const"]]
            ht.filter(conds[0] if len(conds) == 1 else ("and",) + tuple(conds))
        filters, bys = [], []
        for f in q["filters"]:
            rows = htsemi.subquery_rows(tables, f)
            by = tables[f["by"]]
            b = capi.HashTable.from_columns(gpu_ctx, [by[c][0][rows] for c in f["by_cols"]], key_valid=[by[c][1][rows] for c in f["by_cols"]])
            b.finalize_hash()
            bys.append(b)
            filters.append((b, [names.index(c) for c in f["cols"]], f["anti"]))
        kept = ht.semi_filter(filters)
        assert kept == q["count"] and scanstr.rows_digest(ht.filter_rows()) == {"count": q["count"], "sha1": q["sha1"]}, q["where"]
        for h in bys + [ht]:
            h.close()


# ---- 5. everything else survives ----------------------------------------------------------------------------------------------
def test_every_width_as_payload_and_the_cells_themselves(gpu_ctx):
    rng = np.random.default_rng(30)
    n = 1500
    key = rng.integers(0, 90, n).astype(np.int32)
    payload, pvalid = [], []
    for x, dt in enumerate(DTS):
        ii = np.iinfo(dt)
        payload.append(rng.integers(int(ii.min), int(ii.max), n, dtype=dt, endpoint=True))
        pvalid.append((rng.random(n) > 0.25).astype(np.uint8) if x % 2 else None)
    payload.append([None if rng.random() < 0.2 else bytes(rng.integers(97, 100, int(rng.integers(0, 30)), dtype=np.uint8)) for _ in range(n)])
    pvalid.append(None)
    side = Side([key], payload, [(rng.random(n) > 0.1).astype(np.uint8)], pvalid)
    by = By([rng.permutation(90)[:40].astype(np.int32)], kind=S8)
    want = semi(gpu_ctx, side, [(by, [0], True)], null_cell=b"xxabxx", dirty_seed=3)
    assert 0 < len(want) < n
    # kept NULL rows whose source cells hold garbage come out zero, kept valid cells bit for bit, and a column has a
    # validity array afterwards iff it had one before
    ht = side.upload(gpu_ctx, heaps=False, null_cell=b"xxabxx", dirty_seed=3)
    cols, valid, _ = ht._keep
    semi(gpu_ctx, side, [(by, [0], True)], ht=ht, downstream=False)
    ht.finalize_hash()
    for (cells, ok), src, sv in zip(raw_columns(ht, [c.dtype.itemsize for c in cols]), cols, valid):
        assert (ok is None) == (sv is None)
        w = src.dtype.itemsize
        src = np.ascontiguousarray(src).view(np.uint8).reshape(n, w)[want]
        alive = np.ones(len(want), bool) if sv is None else sv[want].astype(bool)
        assert np.array_equal(cells, np.where(alive[:, None], src, 0))
        assert ok is None or np.array_equal(ok, sv[want])
    ht.close()


def test_varchar_payload_and_a_heap_set_afterwards(gpu_ctx):
    side = string_side(2000, 41)
    by = By([np.arange(0, 2000, 3, dtype=np.int32)], kind=S8)
    want = want_rows(side, [(by, [0], False)])
    assert any(s is not None and len(s) > 12 for s in side.take(want).payload[2])
    ht = side.upload(gpu_ctx, heaps=[0])  # the heap of payload column 2 has not come yet
    semi(gpu_ctx, side, [(by, [0], False)], ht=ht, downstream=False)
    ht.set_payload_heaps(2, ht._keep[2][2])
    check_downstream(gpu_ctx, side, want, ht)
    ht.close()
    # a 16-byte column is no key
    ht, d = side.upload(gpu_ctx), By([np.arange(9, dtype=np.int64)]).device(gpu_ctx)
    with pytest.raises(capi.PolrError) as e:
        ht.semi_filter([(d, [1], False)])
    assert e.value.code == capi.E_UNSUPPORTED and "column 1 holds 16-byte cells" in str(e.value)
    ht.close()
    d.close()


# ---- 6. every route to a table ------------------------------------------------------------------------------------------------
def test_table_from_rows(gpu_ctx):
    rng = np.random.default_rng(50)
    n = 2500
    key = rng.permutation(n).astype(np.int32)
    payload = [rng.integers(-100, 100, n).astype(np.int16), rng.integers(0, 1 << 60, n).astype(np.uint64)]
    pvalid = [(rng.random(n) > 0.2).astype(np.uint8), None]
    blob, row_width, offs, kept_rows = buildside.row_blob([key], [None], payload, pvalid)
    widths, signed = buildside.col_shape([key] + payload)
    ht = capi.HashTable.from_rows(gpu_ctx, blob, n, row_width, offs, widths, signed, 1, 2)
    side = Side([key], payload, [np.ones(n, np.uint8)], [pvalid[0], np.ones(n, np.uint8)])
    semi(gpu_ctx, side, [(By([np.arange(-100, 100, 2, dtype=np.int16)], how=("perfect", -100, 99), kind=PERFECT), [1], False)], ht=ht)
    ht.close()


def test_table_from_output(gpu_ctx):
    rng = np.random.default_rng(51)
    n, nb = 3000, 400
    j = Join(rng.permutation(nb).astype(np.int32), 0, payload=[rng.integers(0, 50, nb).astype(np.int32)], payload_valid=[None])
    pk = rng.integers(-20, nb + 20, n).astype(np.int32)
    tag = rng.permutation(n).astype(np.int64)
    hj = j.device(gpu_ctx)
    pipe = capi.Pipeline(gpu_ctx, [pk, tag], n, [(hj, [(-1, 0)])], [[0]])
    out = capi.Output(pipe, 64, n // 64 + 1 + MAX_WAVE_CHUNKS)
    pipe.probe_rounds([(0, n, 0, 1)], out=out)
    a = out.fetch_ids().astype(np.int64)
    live0 = capi.device_bytes_live()
    ht = capi.HashTable.from_output(out, [(-1, 1)], [(0, 0), (-1, 0)])
    side = Side([tag[a[:, 0]]], [j.payload[0][a[:, 1]], pk[a[:, 0]]], [np.ones(len(a), np.uint8)], [np.ones(len(a), np.uint8)] * 2)
    before = ht.info()["device_bytes"]
    want = semi(gpu_ctx, side, [(By([np.array([3, 4, 5, 6, 7, 40, 40], np.int32)], kind=S16), [1], False)], ht=ht, downstream=False)
    assert 0 < len(want) < len(a) // 2
    assert capi.device_bytes_live() - live0 == ht.info()["device_bytes"] < before  # (the allocation from_output made is gone)
    check_downstream(gpu_ctx, side, want, ht)
    ht.close()
    assert capi.device_bytes_live() == live0
    for h in (out, pipe, hj):
        h.close()


def test_device_columns_are_left_alone(gpu_ctx):
    import torch
    rng = np.random.default_rng(52)
    n = 5000
    key = rng.integers(0, 700, n).astype(np.int32)
    pay = rng.integers(-(1 << 50), 1 << 50, n).astype(np.int64)
    pval = (rng.random(n) > 0.3).astype(np.uint8)
    t_key, t_pay, t_val = (torch.from_numpy(a).to("cuda:0") for a in (key, pay, pval))
    live0 = capi.device_bytes_live()
    ht = capi.HashTable.from_cols(gpu_ctx, [capi.dev_col(t_key.data_ptr(), 4, True)],
                                  [capi.dev_col(t_pay.data_ptr(), 8, True, t_val.data_ptr())], n)
    side = Side([key], [pay], None, [pval])
    want = semi(gpu_ctx, side, [(By([np.arange(0, 700, 5, dtype=np.int32)], kind=S8), [0], True)], ht=ht, downstream=False)
    torch.cuda.synchronize()
    assert np.array_equal(t_key.cpu().numpy(), key) and np.array_equal(t_pay.cpu().numpy(), pay) and np.array_equal(t_val.cpu().numpy(), pval)
    t_key.fill_(-1)
    t_pay.fill_(-1)
    t_val.fill_(0)
    del t_key, t_pay, t_val
    torch.cuda.empty_cache()
    check_downstream(gpu_ctx, side, want, ht)
    ht.close()
    assert capi.device_bytes_live() == live0


# ---- 7. afterwards --------------------------------------------------------------------------------------------------------------
def test_finalize_on_thinned_tables(gpu_ctx):
    """a range that only the kept rows keep duplicate-free finalizes perfect where the whole table is a duplicate"""
    rng = np.random.default_rng(60)
    n = 4000
    key = np.concatenate([rng.permutation(3000), rng.integers(0, 3000, 1000)]).astype(np.int32)
    first = np.concatenate([np.ones(3000, np.uint8), np.zeros(1000, np.uint8)])
    order = rng.permutation(n)
    side = Side([key[order]], [first[order], rng.integers(0, 9, n).astype(np.int16)])
    by = By([np.array([1], np.uint8)], kind=S16)
    for how in ("hash", ("perfect", 0, 2999), ("auto", 0, 2999)):
        ht = side.upload(gpu_ctx)
        want = semi(gpu_ctx, side, [(by, [1], False)], ht=ht, how=how)
        assert len(want) == 3000 and ht.info()["kind"] == (2 if how == "hash" else 1) and ht.info()["n_rows"] == 3000
        ht.close()


def test_dictionary_after_the_semi_filter(gpu_ctx):
    """the codes are sized by the survivors"""
    rng = np.random.default_rng(61)
    n = 3000
    nation = rng.integers(0, 25, n)
    side = Side([np.arange(n, dtype=np.int32)], [nation.astype(np.int32), [b"NATION %02d of twenty-five" % x for x in nation]])
    ht = side.upload(gpu_ctx)
    want = semi(gpu_ctx, side, [(By([np.arange(5, 10, dtype=np.int32)], kind=S8), [1], False)], ht=ht, downstream=False)
    code_col, n_codes, has_null = ht.encode_dictionary(1)
    kept = [side.payload[1][r] for r in want.tolist()]
    assert (code_col, n_codes, has_null) == (2, 5, 0) and sorted(ht.dictionary(code_col)) == sorted(set(kept))
    d = By([np.arange(3, dtype=np.int32)]).device(gpu_ctx)
    with pytest.raises(capi.PolrError) as e:  # filter first, then encode
        ht.semi_filter([(d, [1], False)])
    assert e.value.code == capi.E_INVALID and "payload column 1 is dictionary-encoded: filter first, then encode" in str(e.value)
    d.close()
    ht.finalize_hash()
    ids, mats = probe_b(gpu_ctx, ht, [np.arange(n, dtype=np.int32)], None, [np.int32, None, np.uint32])
    assert np.array_equal(ids[:, 0], want) and mats[1] == kept
    names = ht.dictionary(code_col)
    assert [names[c] for c in mats[2][0].tolist()] == kept
    ht.close()


def test_resident_run_over_a_thinned_table(gpu_ctx):
    """a two-join pipeline with one thinned table, run by the pool launch: the row set of the twin's and of joinref.Ref"""
    rng = np.random.default_rng(62)
    n, nb = 20000, 1500
    j0 = Join(rng.permutation(nb).astype(np.int32), 0, payload=[rng.integers(0, 5, nb).astype(np.int32)], payload_valid=[None])
    j1 = Join(np.repeat(np.arange(300, dtype=np.int32), 2), 1)
    side = Side([j0.keys], [j0.payload[0]])
    by = By([np.array([1, 3, 3], np.int32)], kind=S16)
    want = want_rows(side, [(by, [1], False)])
    pcols = [rng.integers(-10, nb + 10, n).astype(np.int32), rng.integers(-5, 320, n).astype(np.int32)]
    results = []
    for thinned_here in (True, False):
        ht0 = side.upload(gpu_ctx) if thinned_here else side.take(want).upload(gpu_ctx)
        if thinned_here:
            semi(gpu_ctx, side, [(by, [1], False)], ht=ht0, downstream=False)
        ht0.finalize_hash()
        ht1 = j1.device(gpu_ctx)
        pipe = capi.Pipeline(gpu_ctx, pcols, n, [(ht0, [(-1, 0)]), (ht1, [(-1, 1)])], [[0, 1], [1, 0]])
        out = capi.Output(pipe, 1024, 64 + MAX_WAVE_CHUNKS)
        mx = capi.DeviceMultiplexer(pipe, "adaptive_reinit")
        capi.run_resident([mx], [(0, (n + 1023) // 1024)], out=out, reset=True, finish=True)
        mx.finish()
        ids = out.fetch_ids().astype(np.int64)
        ids[:, 1] = want[ids[:, 1]]
        results.append(sort_rows(ids))
        for h in (mx, out, pipe, ht0, ht1):
            h.close()
    ref = Ref(pcols, None, [Join(j0.keys[want], 0), j1]).rows()
    ref[:, 1] = want[ref[:, 1]]
    assert len(ref) > 0 and np.array_equal(results[0], results[1]) and np.array_equal(results[0], sort_rows(ref))


# ---- 8. refusals and atomicity ------------------------------------------------------------------------------------------------
def test_refusals_leave_the_table_as_it_was(gpu_ctx):
    import gc
    gc.collect()
    rng = np.random.default_rng(70)
    n = 1200
    side = Side([rng.permutation(n).astype(np.int32)], [rng.integers(0, 10, n).astype(np.int32), rng.integers(0, 10, n).astype(np.int64)])
    L = gpu_ctx.L
    live0 = capi.device_bytes_live()
    assert L.polr_ht_semi_filter(None, None, None, 0, None) == capi.E_INVALID  # NULL ht
    ht = side.upload(gpu_ctx)
    by = By([np.arange(5, dtype=np.int32)]).device(gpu_ctx)
    by2 = By([np.arange(5, dtype=np.int32), np.arange(5, dtype=np.int32)]).device(gpu_ctx)
    raw = capi.HashTable.from_columns(gpu_ctx, [np.arange(5, dtype=np.int32)])  # not finalized
    other_ctx = capi.Context(0)
    elsewhere = capi.HashTable.from_columns(other_ctx, [np.arange(5, dtype=np.int32)]).finalize_hash()
    live1, info1 = capi.device_bytes_live(), ht.info()

    def refused(code, text, *call):
        with pytest.raises(capi.PolrError) as e:
            call[0](*call[1:])
        assert e.value.code == code and text in str(e.value), str(e.value)
        assert capi.device_bytes_live() == live1 and ht.info() == info1

    one = (by, [1], False)
    refused(capi.E_UNSUPPORTED, "5 filters (at most 4 in one call)", ht.semi_filter, [one] * 5)
    refused(capi.E_INVALID, "filters is NULL", ht.semi_filter_raw, [], None, 2)
    refused(capi.E_INVALID, "filter 1: `by` is NULL", ht.semi_filter, [one, (None, [1], False)])
    refused(capi.E_INVALID, "filter 0: `by` is not finalized", ht.semi_filter, [(raw, [1], False)])
    # (the table itself is un-finalized, so the refusal before "`by` is the table itself" answers: tests/test_htsemi_plan.py)
    refused(capi.E_INVALID, "filter 0: `by` is not finalized", ht.semi_filter, [(ht, [0], False)])
    refused(capi.E_INVALID, "filter 0: `by` lives on another device or context", ht.semi_filter, [(elsewhere, [1], False)])
    refused(capi.E_INVALID, "filter 2: flags 0x2 (0 or POLR_SEMI_ANTI)", ht.semi_filter, [one, one, (by, [1], 2)])
    refused(capi.E_INVALID, "filter 0: 1 columns for a 2-key table", ht.semi_filter, [(by2, [1], False)])
    refused(capi.E_INVALID, "filter 0 key 1: column 3 out of range", ht.semi_filter, [(by2, [1, 3], False)])
    refused(capi.E_INVALID, "filter 0 key 0: column 2 is 8 bytes, the key of `by` 4 bytes", ht.semi_filter, [(by, [2], False)])
    # ... after which a filter behaves as if the refused calls had never been made: the cells are those of the twin
    want = want_rows(side, [(By([np.arange(5, dtype=np.int32)]), [1], True)])
    assert ht.semi_filter([(by, [1], True)]) == len(want)
    info2 = ht.info()
    assert capi.device_bytes_live() - live1 == info2["device_bytes"] - info1["device_bytes"] < 0  # (the table shrank)
    check_downstream(gpu_ctx, side, want, ht)
    live1, info1 = capi.device_bytes_live(), ht.info()
    refused(capi.E_INVALID, "the table is finalized", ht.semi_filter, [one])
    for h in (ht, by, by2, raw, elsewhere):
        h.close()
    other_ctx.close()
    assert capi.device_bytes_live() == live0


def test_live_bytes_are_at_their_baseline(gpu_ctx):
    """every table of this file was closed: nothing a call allocated is left (a fresh table, thinned twice and closed)"""
    import gc
    gc.collect()
    live0 = capi.device_bytes_live()
    side = Side([np.arange(5000, dtype=np.int32)], [np.arange(5000, dtype=np.int64)], None, [np.ones(5000, np.uint8)])
    ht = side.upload(gpu_ctx)
    before, live1 = ht.info()["device_bytes"], capi.device_bytes_live()
    by = By([np.arange(100, dtype=np.int32)]).device(gpu_ctx)
    live1 = capi.device_bytes_live()
    f = capi.SemiFilter(by.h, 1, (capi.C.c_uint32 * 4)(0, 0, 0, 0), 0)
    assert gpu_ctx.L.polr_ht_semi_filter(ht.h, None, capi.C.byref(f), 1, None) == 0  # (n_kept may be NULL)
    assert capi.device_bytes_live() - live1 == ht.info()["device_bytes"] - before < 0
    ht._n_kept = 100
    assert np.array_equal(ht.filter_rows(), np.arange(100))
    assert ht.semi_filter([(by, [0], True)]) == 0 and len(ht.filter_rows()) == 0
    ht.close()
    by.close()
    assert capi.device_bytes_live() == live0
