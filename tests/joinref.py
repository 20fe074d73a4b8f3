"""The plain numpy reference of an equi-join that the GPU matrices check the device against (tests/test_gpu_engine_matrix.py,
tests/test_gpu_sink_matrix.py, tests/test_gpu_scan_lip.py): the build keys sorted, np.searchsorted for each probe row's
run of matching build rows, NULL never matching on either side; the row set expanded join by join.  And the key cases
(8 key types x perfect / unique / repeated tables) the engine matrix and the LIP scan tests share."""
import numpy as np

from common import orc
from polr_amd import capi

U64 = 0xFFFFFFFFFFFFFFFF


class Join:
    """one build side: key column (+ validity), optional payload, probe column it is keyed by, perfect range or hash"""

    def __init__(self, keys, src, perfect=None, valid=None, payload=(), payload_valid=None):
        self.keys = np.ascontiguousarray(keys)
        self.src = src
        self.perfect = perfect
        self.valid = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint8)
        self.payload = [np.ascontiguousarray(p) for p in payload]
        self.payload_valid = payload_valid or [None] * len(self.payload)
        ok = np.ones(len(self.keys), bool) if self.valid is None else self.valid.astype(bool)
        rows = np.nonzero(ok)[0]
        self.order = rows[np.argsort(self.keys[rows], kind="stable")].astype(np.int64)
        self.sorted = self.keys[self.order]
        if perfect is not None:
            # device build id of a perfect table = key - min (modulo 2^64: min may be a uint64's int64 bit pattern); back
            # to the build row, as pht_orig_rows() maps it.  Every build key lies inside [min, max].
            off = self.keys[rows].astype(np.uint64) - np.uint64(perfect[0] & U64)
            size = ((perfect[1] - perfect[0]) & U64) + 1
            assert (off < np.uint64(size)).all()
            self.id_to_row = np.full(size, -1, np.int64)
            self.id_to_row[off.astype(np.int64)] = rows

    def device(self, ctx):
        ht = capi.HashTable.from_columns(ctx, [self.keys], self.payload, key_valid=[self.valid],
                                         payload_valid=self.payload_valid)
        if self.perfect is not None:
            assert ht.finalize_perfect(*self.perfect)
            assert ht.info()["kind"] == 1
        else:
            ht.finalize_hash()
        return ht

    def oracle(self):
        oht = orc.HashTable([self.keys], self.payload, key_valid=[self.valid], payload_valid=self.payload_valid)
        if self.perfect is not None:
            assert oht.make_perfect(*self.perfect)
        return orc.JoinSpec(oht, [(-1, self.src)])


class Ref:
    """the join result of probe columns x joins, restricted to the probe rows in `sel` (None: all)"""

    def __init__(self, pcols, pvalid, joins, sel=None):
        self.pcols, self.joins = pcols, joins
        n = len(pcols[0])
        self.n = n
        insel = np.ones(n, bool)
        if sel is not None:
            insel[:] = False
            insel[sel] = True
        self.starts, self.counts = [], []
        for j in joins:
            pk = pcols[j.src]
            left = np.searchsorted(j.sorted, pk, "left")
            right = np.searchsorted(j.sorted, pk, "right")
            cnt = (right - left).astype(np.int64)
            if pvalid is not None and pvalid[j.src] is not None:
                cnt[~pvalid[j.src].astype(bool)] = 0  # NULL never matches
            cnt[~insel] = 0
            self.starts.append(left.astype(np.int64))
            self.counts.append(cnt)

    def stage_counts(self, path):
        prod = np.ones(self.n, np.int64)
        out = []
        for j in path:
            prod = prod * self.counts[j]
            out.append(int(prod.sum()))
        return out

    def rows(self):
        """(n_rows, 1 + k) int64: probe row, then the build row of every join in the original join order"""
        live = np.ones(self.n, bool)
        for c in self.counts:
            live &= c > 0
        t = np.nonzero(live)[0].astype(np.int64)[:, None]
        for x, j in enumerate(self.joins):
            r = t[:, 0]
            c = self.counts[x][r]
            rep = np.repeat(np.arange(len(t)), c)
            within = np.arange(len(rep)) - np.repeat(np.cumsum(c) - c, c)
            b = j.order[np.repeat(self.starts[x][r], c) + within]
            t = np.column_stack([t[rep], b])
        return t


def sort_rows(a):
    a = np.asarray(a, dtype=np.int64)
    return a[np.lexsort(a.T[::-1])] if len(a) else a.reshape(0, a.shape[1] if a.ndim == 2 else 1)


def device_rows(ids, joins):
    """device row ids -> build rows (perfect tables report key offsets)"""
    rows = ids.astype(np.int64)
    for x, j in enumerate(joins):
        if j.perfect is not None:
            rows[:, 1 + x] = j.id_to_row[rows[:, 1 + x]]
    return rows


# ---- key types x table kinds (tests/test_gpu_engine_matrix.py::test_key_types, tests/test_gpu_scan_lip.py) ---------------------
DTYPES = [np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.int64, np.uint64]
MAX_WAVE_CHUNKS = 8192  # one partially filled chunk per emitting wave (polr_out_create)


def chunks_for(n_rows, cap):
    return (n_rows + cap - 1) // cap + MAX_WAVE_CHUNKS


def _perfect_ranges(dt):
    info = np.iinfo(dt)
    if info.bits <= 16:
        return {"perfect": (int(info.min), int(info.max))}  # the whole domain (type min, max, 0 and -1 inside)
    R = 3000
    if info.min < 0:
        return {"perfect_lo": (int(info.min), int(info.min) + R), "perfect_mid": (-R // 2, R // 2),
                "perfect_hi": (int(info.max) - R, int(info.max))}
    hi = (int(info.max) - R, int(info.max))
    if info.bits == 64:  # above 2^63: min and max passed as their int64 bit patterns
        hi = (hi[0] - (1 << 64), -1)
    return {"perfect_lo": (0, R), "perfect_hi": hi}


KEY_CASES = [(dt, kind) for dt in DTYPES for kind in list(_perfect_ranges(dt)) + ["unique", "repeated"]]


def _specials(dt):
    info = np.iinfo(dt)
    return [int(info.min), int(info.max), 0, -1 if info.min < 0 else int(info.max), 1]


def _key_case(dt, kind, seed, n_probe=20_000):
    rng = np.random.default_rng(seed)
    info = np.iinfo(dt)
    lo_t, hi_t = int(info.min), int(info.max)

    def arr(vals):
        return np.array([int(v) for v in vals], dtype=np.uint64 if dt == np.uint64 else np.int64).astype(dt)

    def rand(lo, hi, n):  # python ints in [lo, hi], any width
        return [lo + x % (hi - lo + 1) for x in rng.integers(0, 2**64, n, dtype=np.uint64).tolist()]

    if kind.startswith("perfect"):
        lo, hi = _perfect_ranges(dt)[kind]
        ulo, uhi = (lo & U64, hi & U64) if dt == np.uint64 else (lo, hi)
        inner = sorted(set(rand(ulo, uhi, min(2000, uhi - ulo + 1))))
        must = [ulo, ulo + 1, uhi - 1, uhi] + [s for s in (0, -1) if ulo <= s <= uhi]
        bk = sorted(set(inner + must))
        bk = [v for v in bk if v not in (ulo + 2, uhi - 2)]  # holes next to both ends
        edges = [ulo - 1, ulo, ulo + 1, ulo + 2, uhi - 2, uhi - 1, uhi, uhi + 1]
        near = rand(max(lo_t, ulo - 40), min(hi_t, uhi + 40), n_probe // 2)
        perfect = (lo, hi)
    else:
        n_b = 150 if info.bits == 8 else 3000
        vals = list(dict.fromkeys(_specials(dt) + rand(lo_t, hi_t, 4 * n_b)))[:n_b]
        bk = vals if kind == "unique" else [v for i, v in enumerate(vals) for _ in range(1 + i % 3)]
        edges = []
        near = [bk[i] for i in rng.integers(0, len(bk), n_probe // 2)]
        perfect = None
    pk = _specials(dt) + [e for e in edges if lo_t <= e <= hi_t] + near
    pk += rand(lo_t, hi_t, n_probe - len(pk))
    bk, pk = rng.permutation(arr(bk)), rng.permutation(arr(pk))
    bvalid = (rng.random(len(bk)) > 0.03).astype(np.uint8)
    pvalid = (rng.random(len(pk)) > 0.03).astype(np.uint8)
    pay = (np.arange(len(bk)) % 97).astype(np.int32)
    return Join(bk, 0, perfect, bvalid, [pay]), [pk], [pvalid]


# ---- the inputs of tests/golden/hash_groupby.json (tests/golden/make_golden_hashagg.py) -----------------------------------------
HASHAGG_SQL = ("SELECT g1, g2, COUNT(*), COUNT(x), SUM(x), MIN(x), MAX(x) FROM fact JOIN dim ON fk = dk GROUP BY g1, g2 "
               "ORDER BY g1 NULLS FIRST, g2 NULLS FIRST")


def hashagg_inputs(seed, n_fact, n_dim):
    """fact(fk INTEGER, g1 BIGINT, x BIGINT) and dim(dk INTEGER, g2 BIGINT): group values wide and sparse (about +-10^12, so
    the reference plans a hash aggregate), NULL in both group columns and in x; x of large magnitude with the sign of the g1
    group, so that group sums leave the int64 range on both sides -> (fact cols, fact valid, dim cols, dim valid)"""
    rng = np.random.default_rng(seed)
    d1 = rng.integers(-10**12, 10**12, 12)
    d2 = rng.integers(-10**12, 10**12, 10)
    assert len(np.unique(d1)) == len(d1) and len(np.unique(d2)) == len(d2)
    i1 = rng.integers(0, len(d1), n_fact)
    big = rng.integers(1 << 61, (1 << 63) - 1, n_fact, dtype=np.int64)
    x = np.where(rng.random(n_fact) < 0.2, rng.integers(-1000, 1000, n_fact), np.where(i1 % 2 == 0, big, -big - 1))
    fact = {"fk": rng.integers(0, n_dim + n_dim // 10, n_fact).astype(np.int32), "g1": d1[i1].astype(np.int64),
            "x": x.astype(np.int64)}
    fact_valid = {"g1": (rng.random(n_fact) > 0.05).astype(np.uint8), "x": (rng.random(n_fact) > 0.08).astype(np.uint8)}
    dim = {"dk": rng.permutation(n_dim).astype(np.int32), "g2": d2[rng.integers(0, len(d2), n_dim)].astype(np.int64)}
    dim_valid = {"g2": (rng.random(n_dim) > 0.05).astype(np.uint8)}
    return fact, fact_valid, dim, dim_valid


def hashagg_groups(g1, g1_ok, g2, g2_ok, x, x_ok):
    """GROUP BY g1, g2 over joined rows -> {(g1, g2) with None = NULL: [COUNT(*), COUNT(x), SUM(x), MIN(x), MAX(x)]}"""
    groups = {}
    for a, ao, b, bo, v, vo in zip(g1.tolist(), g1_ok.tolist(), g2.tolist(), g2_ok.tolist(), x.tolist(), x_ok.tolist()):
        w = groups.setdefault((a if ao else None, b if bo else None), [0, 0, None, None, None])
        w[0] += 1
        if vo:
            w[1] += 1
            w[2] = v if w[2] is None else w[2] + v
            w[3] = v if w[3] is None else min(w[3], v)
            w[4] = v if w[4] is None else max(w[4], v)
    return groups
