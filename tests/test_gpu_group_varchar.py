"""GROUP BY over VARCHAR columns in the general hash aggregate sink (polr_out_aggregate_hashed_str, Output.aggregate_hashed_str)
against exact Python: the numpy join result of tests/joinref.py, group keys as Python bytes / int / None, aggregates as
Python ints -- never anything the code under test computed.  Every case asserts which engine produced the row ids it
groups (`launch_info(True)["flat"]`), as tests/test_gpu_sink_matrix.py does:

  path     the path kernel (probe_rounds) over a repeated-key hash table
  generic  the generic pool (run_resident) over the same table
  flat     the emitting flat pool (run_resident) over a perfect table (string heap set before finalize_perfect)
"""
import ctypes as C

import numpy as np
import pytest

import strref
from joinref import Join, Ref, device_rows, sort_rows
from polr_amd import capi
from test_gpu_sink_matrix import MAX_WAVE_CHUNKS, py_agg, random_strings, string_blocks

pytestmark = pytest.mark.gpu

ENGINES = ["path", "generic", "flat"]

# every string edge in ONE column: the inline / heap boundary with the same first 12 bytes, the same length and first four
# bytes but different later (inline and heap), a difference in the last of 100 bytes only, the empty string, prefixes of
# one another around the 12-byte boundary
EDGES = [b"", b"\x00", b"\xff" * 12, b"\xff" * 13, b"\x00" * 12, b"\x00" * 13, b"ABCDxxxx", b"ABCDxxxy", b"ABCDyxxx",
         b"ABCD" + b"q" * 16, b"ABCD" + b"q" * 15 + b"r", b"ABCDr" + b"q" * 15, b"Q" * 99 + b"a", b"Q" * 99 + b"b",
         b"UNITED STATES", b"UNITED KINGDOM", b"UNITED ST", b"UNITED STATE", b"UNITED STATES "]
assert len(set(EDGES)) == len(EDGES) and {len(e) for e in EDGES} >= {0, 1, 12, 13, 100}


def string_pool(rng, extra=120):
    pool = list(dict.fromkeys(EDGES + random_strings(rng, extra)))  # (distinct, order kept)
    assert {len(v) for v in pool} >= {0, 1, 4, 5, 11, 12, 13, 16, 100}
    return pool


def big_values(rng, n):
    """int64 of large magnitude, both signs: group sums leave the int64 range"""
    big = rng.integers(1 << 61, (1 << 63) - 1, n, dtype=np.int64)
    return np.where(rng.random(n) < 0.5, -big - 1, big)


def dirty_padding(cells, values, valid, rng):
    """fill the unused inline bytes of every non-NULL cell of at most 11 bytes with random non-zero bytes: the padding of
    an inline cell is not part of the string (string_blocks leaves it zero)"""
    raw = cells.view(np.uint8).reshape(-1, 16)
    for i, v in enumerate(values):
        if valid[i] and len(v) < 12:
            raw[i, 4 + len(v):] = rng.integers(1, 256, 12 - len(v))


class Bank:
    """probe (pk, p_s VARCHAR, p_i int16, p_big int64) x one join (repeated-key hash table; perfect for `flat`) with payload
    (b_s VARCHAR, b_i int32, b_big int64); NULLs in every column but pk; the probe heap goes up in probe_blocks blocks, the
    payload heap in build_blocks blocks (heaps=False: no heap is handed over at all)."""
    PROBE = {"p_s": 1, "p_i": 2, "p_big": 3}
    BUILD = {"b_s": 0, "b_i": 1, "b_big": 2}

    def __init__(self, ctx, engine, seed, n=20_000, nb=3000, probe_blocks=1, build_blocks=3, p_strs=None, b_strs=None, heaps=True,
                 p_valid=None, p_big=None, cap=64, dirty=False):
        rng = np.random.default_rng(seed)
        self.engine = engine
        if engine == "flat":
            bk = rng.permutation(np.arange(0, nb, dtype=np.int32))
        else:
            bk = rng.permutation(np.repeat(np.arange(0, nb, 2, dtype=np.int32), 2))
        self.join = Join(bk, 0, (0, nb - 1) if engine == "flat" else None)
        pk = rng.integers(-nb // 30, nb + nb // 30, n).astype(np.int32)
        pool = string_pool(rng)
        self.p_s = p_strs if p_strs is not None else [pool[i] for i in rng.integers(0, len(pool), n)]
        self.b_s = b_strs if b_strs is not None else [pool[i] for i in rng.integers(0, 40, len(bk))]
        self.cols = {"p_s": self.p_s, "p_i": rng.integers(-3, 4, n).astype(np.int16),
                     "p_big": big_values(rng, n) if p_big is None else p_big,
                     "b_s": self.b_s, "b_i": rng.choice(np.array([-(1 << 31), -1, 0, 1, (1 << 31) - 1], np.int32), len(bk)),
                     "b_big": big_values(rng, len(bk))}
        self.valid = {c: (rng.random(len(v)) > 0.08).astype(np.uint8) for c, v in self.cols.items()}
        if p_valid is not None:
            self.valid["p_s"] = p_valid
        p_cells, p_heap = string_blocks(self.p_s, self.valid["p_s"], probe_blocks, seed)
        b_cells, b_heap = string_blocks(self.b_s, self.valid["b_s"], build_blocks, seed + 1)
        if dirty:
            dirty_padding(p_cells, self.p_s, self.valid["p_s"], rng)
            dirty_padding(b_cells, self.b_s, self.valid["b_s"], rng)
        self.keep = (p_cells, p_heap, b_cells, b_heap)  # (host heaps stay alive as long as the bank)
        self.ht = capi.HashTable.from_columns(ctx, [bk], [b_cells, self.cols["b_i"], self.cols["b_big"]],
                                              payload_valid=[self.valid[c] for c in ("b_s", "b_i", "b_big")])
        if heaps:
            self.ht.set_payload_heaps(0, b_heap)
        if engine == "flat":
            assert self.ht.finalize_perfect(0, nb - 1)
        else:
            self.ht.finalize_hash()
        self.pipe = capi.Pipeline(ctx, [pk, p_cells, self.cols["p_i"], self.cols["p_big"]], n, [(self.ht, [(-1, 0)])], [[0]],
                                  probe_valid=[None] + [self.valid[c] for c in ("p_s", "p_i", "p_big")])
        if heaps:
            self.pipe.set_probe_heaps(1, p_heap)
        assert self.pipe.launch_info(True)["flat"] == int(engine == "flat")  # which engine emits the row ids
        self.rows = sort_rows(Ref([pk], None, [self.join]).rows())
        self.out = capi.Output(self.pipe, cap, len(self.rows) // cap + 1 + MAX_WAVE_CHUNKS)
        if engine == "path":
            self.pipe.probe_rounds([(0, n, 0, 1)], out=self.out)
        else:
            mx = capi.DeviceMultiplexer(self.pipe, "default_path")
            capi.run_resident([mx], [(0, (n + 1023) // 1024)], out=self.out, reset=True, finish=True)
            mx.finish()
            mx.close()
        assert np.array_equal(sort_rows(device_rows(self.out.fetch_ids(), [self.join])), self.rows)

    def col(self, name):
        return (-1, self.PROBE[name]) if name in self.PROBE else (0, self.BUILD[name])

    def column(self, name):
        """(python values, validity) of a column over the reference's join rows"""
        r = self.rows[:, 0] if name in self.PROBE else self.rows[:, 1]
        v = self.cols[name]
        vals = [v[i] for i in r.tolist()] if isinstance(v, list) else v[r].tolist()
        return vals, self.valid[name][r].astype(bool).tolist()

    def want(self, group_names, specs):
        """exact Python GROUP BY: {key tuple (bytes / int / None): [aggregate values]}"""
        keys = [self.column(c) for c in group_names]
        members = {}
        for i in range(len(self.rows)):
            members.setdefault(tuple(v[i] if ok[i] else None for v, ok in keys), []).append(i)
        aggs = {}
        for fn, name in specs:
            if name is not None and name not in aggs:
                v, ok = self.column(name)
                aggs[name] = (np.array(v, dtype=object), np.array(ok, dtype=bool))
        out = {}
        for key, idx in members.items():
            out[key] = [len(idx) if fn == "count_star" else py_agg(fn, aggs[name][0][idx], aggs[name][1][idx])
                        for fn, name in specs]
        return out

    def specs(self, specs):
        return [(fn, -1, 0) if name is None else (fn, *self.col(name)) for fn, name in specs]

    def close(self):
        self.out.close()
        self.pipe.close()
        self.ht.close()


ALL_AGGS = [("count_star", None), ("count", "b_big"), ("sum", "b_big"), ("min", "p_big"), ("max", "p_big"), ("sum", "p_big"),
            ("sum", "p_i"), ("max", "b_i")]
SHAPES = {
    "probe-string": ["p_s"],                 # every string edge in one column
    "build-string": ["b_s"],                 # a hash table's payload / a perfect table's re-ordered payload
    "string+int": ["b_s", "p_i"],
    "2strings+int": ["p_s", "b_s", "b_i"],   # SSB Q3: c_city, s_city, d_year
    "int+string": ["b_i", "p_s"],
}
CASES = [(e, s) for e in ENGINES for s in SHAPES]


@pytest.mark.parametrize("engine,shape", CASES, ids=["%s-%s" % c for c in CASES])
def test_group_by_strings(gpu_ctx, engine, shape):
    """1-3 group columns, VARCHAR and integer mixed, from the probe row and from a hash / perfect table's payload; heaps in 1
    and in 3 blocks (which side has which alternates with the case); the key set exactly, then every cell of 8 aggregates
    (sums beyond int64); NULL rows hold garbage cells; every row's long string has its own heap copy"""
    k = CASES.index((engine, shape))
    b = Bank(gpu_ctx, engine, seed=300 + k, probe_blocks=1 + 2 * (k % 2), build_blocks=3 - 2 * (k % 2))
    want = b.want(SHAPES[shape], ALL_AGGS)
    got = b.out.aggregate_hashed_str([b.col(c) for c in SHAPES[shape]], b.specs(ALL_AGGS), max(1024, 2 * len(want)))
    assert set(got) == set(want)
    for key in want:
        assert got[key] == want[key], key
    assert any(v[2] is not None and abs(v[2]) > (1 << 64) for v in want.values())
    if shape == "probe-string":
        # each edge is a group of its own: four groups at the inline / heap boundary, the empty string and NULL apart,
        # same length + same first four bytes apart, a last-byte difference apart, prefixes apart
        assert {(e,) for e in EDGES} | {(None,)} <= set(got)
        longs = [v for v, ok in zip(*b.column("p_s")) if ok and len(v) > 12]
        assert len(longs) > 20 * len(set(longs))  # one long string, many heap copies: ONE group each
    if shape == "2strings+int":
        assert any(key[0] is None and key[1] is None for key in got) and any(key[2] is None for key in got)
    b.close()


@pytest.mark.parametrize("engine", ENGINES)
def test_padding_of_inline_cells_is_not_part_of_the_string(gpu_ctx, engine):
    """every non-NULL inline cell carries random non-zero bytes behind its string, different from row to row: the groups
    are those of the strings all the same (hash and comparison mask the padding), and the strings come back without it"""
    b = Bank(gpu_ctx, engine, seed=320 + ENGINES.index(engine), dirty=True)
    raw = b.keep[0].view(np.uint8).reshape(-1, 16)
    one = [i for i, (v, ok) in enumerate(zip(b.p_s, b.valid["p_s"])) if ok and v == b"\x00"]
    assert len({raw[i, 5:].tobytes() for i in one}) > 10  # (one string, many paddings)
    want = b.want(["p_s", "b_s"], ALL_AGGS)
    got = b.out.aggregate_hashed_str([b.col("p_s"), b.col("b_s")], b.specs(ALL_AGGS), max(1024, 2 * len(want)))
    assert set(got) == set(want)
    for key in want:
        assert got[key] == want[key], key
    assert [b.out._col_width(*b.col(c)) for c in ("p_s", "p_i", "p_big", "b_s", "b_i", "b_big")] == [16, 2, 8, 16, 4, 8]
    b.close()


@pytest.mark.parametrize("engine", ENGINES)
def test_integer_columns_only_equal_the_integer_sink(gpu_ctx, engine):
    """integer group columns through the new entry point: exactly aggregate_hashed on the same output (and Python)"""
    b = Bank(gpu_ctx, engine, seed=330 + ENGINES.index(engine), n=8000)
    cols, specs = [b.col("p_i"), b.col("b_i")], b.specs(ALL_AGGS)
    got = b.out.aggregate_hashed_str(cols, specs, 1024)
    assert got == b.out.aggregate_hashed(cols, specs, 1024) == b.want(["p_i", "b_i"], ALL_AGGS)
    b.close()


@pytest.mark.parametrize("engine", ENGINES)
def test_hot_group(gpu_ctx, engine):
    """~90 % of the rows in one group of a long string (every lane of a wave on one slot), ~5 % in a second one; the hot
    group's SUM is far above int64, the second one's far below"""
    rng = np.random.default_rng(340)
    n = 30_000
    u = rng.random(n)
    pool = string_pool(rng)
    hot, cold = b"UNITED STATES", b"UNITED STATES MINOR OUTLYING ISLANDS"
    strs = [hot if x < 0.9 else (cold if x < 0.95 else pool[int(x * 1e6) % len(pool)]) for x in u.tolist()]
    big = rng.integers(1 << 61, (1 << 63) - 1, n, dtype=np.int64)
    vals = np.where(u < 0.9, big, np.where(u < 0.95, -big - 1, rng.integers(-1000, 1000, n)))
    b = Bank(gpu_ctx, engine, seed=341 + ENGINES.index(engine), n=n, p_strs=strs, p_big=vals)
    specs = [("count_star", None), ("sum", "p_big"), ("min", "p_big"), ("max", "p_big"), ("count", "p_big")]
    want = b.want(["p_s"], specs)
    got = b.out.aggregate_hashed_str([b.col("p_s")], b.specs(specs), 1024)
    assert set(got) == set(want)
    for key in want:
        assert got[key] == want[key], key
    assert got[(hot,)][0] > 0.8 * len(b.rows) and got[(hot,)][1] > (1 << 66) and got[(cold,)][1] < -(1 << 64)
    b.close()


def distinct_strings(n):
    """n different strings: inline ones, 20-byte ones that differ in the tail only, and 100-byte ones that differ in the
    last bytes only"""
    out = []
    for i in range(n):
        if i % 3 == 0:
            out.append(b"%d" % i)
        elif i % 3 == 1:
            out.append(b"distinct-str-%07d" % i)
        else:
            out.append(b"P" * 90 + b"%010d" % i)
    return out


def distinct_bank(ctx, n=50_000):
    rng = np.random.default_rng(350)
    j = Join(np.arange(0, n, dtype=np.int32), 0, (0, n - 1))
    ht = j.device(ctx)
    pk = rng.permutation(n).astype(np.int32)
    strs = distinct_strings(n)
    val = big_values(rng, n)
    cells, heap = string_blocks(strs, np.ones(n, np.uint8), 2, 7)
    pipe = capi.Pipeline(ctx, [pk, cells, val], n, [(ht, [(-1, 0)])], [[0]])
    pipe.set_probe_heaps(1, heap)
    assert pipe.launch_info(True)["flat"] == 1
    out = capi.Output(pipe, 1024, n // 1024 + 1 + MAX_WAVE_CHUNKS)
    pipe.probe_rounds([(0, n, 0, 1)], out=out)
    assert out.stats()[0] == n
    return ht, pipe, out, strs, val, (cells, heap)


def raw_call(ctx, out, cols, specs, max_groups, str_cap):
    """polr_out_aggregate_hashed_str as the C ABI has it -> (rc, n_groups, str_used, keys, nulls, arena)"""
    ka = (capi.GroupKey * len(cols))()
    for i, (sj, sc) in enumerate(cols):
        ka[i].src_join, ka[i].src_col = sj, sc
    sa = (capi.AggSpec * len(specs))(*[capi.AggSpec(capi.AGG[fn], sj, sc) for fn, sj, sc in specs])
    keys = np.full((max_groups, len(cols)), -7, np.int64)
    nulls = np.full(max_groups, 0xABABABAB, np.uint32)
    res = (capi.AggValue * (max_groups * len(specs)))()
    arena = np.full(max(str_cap, 1), 0xEE, np.uint8)
    n_groups, used = C.c_uint64(), C.c_uint64()
    rc = ctx.L.polr_out_aggregate_hashed_str(out.h, None, ka, len(cols), sa, len(specs), max_groups, keys.ctypes.data,
                                             nulls.ctypes.data, res, C.byref(n_groups), arena.ctypes.data, str_cap,
                                             C.byref(used))
    return rc, n_groups.value, used.value, keys, nulls, arena


def test_all_distinct_and_the_capacity_contract(gpu_ctx):
    """groups = rows (50 000 different strings): the key set exactly and every cell; exactly max_groups succeeds and
    max_groups - 1 is POLR_E_OVERFLOW; str_cap one byte short is POLR_E_OVERFLOW with *n_groups and *str_used exact and
    nothing written, and the retry with *str_used succeeds; an empty output has 0 groups"""
    n = 50_000
    ht, pipe, out, strs, val, _keep = distinct_bank(gpu_ctx, n)
    specs = [("count_star", -1, 0), ("sum", -1, 2), ("min", -1, 2)]
    got = out.aggregate_hashed_str([(-1, 1)], specs, n)
    assert len(got) == n and set(got) == {(s,) for s in strs}
    for s, v in zip(strs, val.tolist()):
        assert got[(s,)] == [1, v, v]
    need = sum(4 + len(s) for s in strs)
    rc, n_groups, used, keys, nulls, arena = raw_call(gpu_ctx, out, [(-1, 1)], specs, n - 1, need)
    assert rc == capi.E_OVERFLOW and n_groups >= n - 1
    rc, n_groups, used, keys, nulls, arena = raw_call(gpu_ctx, out, [(-1, 1)], specs, n, need - 1)
    assert rc == capi.E_OVERFLOW and n_groups == n and used == need
    assert (keys == -7).all() and (nulls == 0xABABABAB).all() and (arena == 0xEE).all()  # nothing half-written
    rc, n_groups, used, keys, nulls, arena = raw_call(gpu_ctx, out, [(-1, 1)], specs, n, used)
    assert rc == capi.OK and n_groups == n and used == need and not nulls.any()
    raw = arena.tobytes()
    back = set()
    for at in keys[:, 0].tolist():
        ln = int.from_bytes(raw[at:at + 4], "little")
        back.add(raw[at + 4:at + 4 + ln])
    assert back == set(strs)
    assert len(out.aggregate_hashed_str([(-1, 1)], specs, n, str_cap=16)) == n  # (the binding's one retry)
    out.reset()
    assert out.aggregate_hashed_str([(-1, 1)], specs, 16) == {}
    rc, n_groups, used, *_ = raw_call(gpu_ctx, out, [(-1, 1)], specs, 16, 0)
    assert rc == capi.OK and n_groups == 0 and used == 0
    out.close()
    pipe.close()
    ht.close()


def test_columns_whose_heap_never_came(gpu_ctx):
    """a VARCHAR column whose cells were never rebased onto a device heap: all-inline strings are legal and grouped; one
    long non-NULL cell among the output rows is POLR_E_INVALID -- found by the pass that reads only the cells' length words,
    before any kernel that follows a pointer is enqueued; the old entry point still refuses a width-16 group column"""
    rng = np.random.default_rng(360)
    n = 6000
    short = [bytes(rng.integers(65, 70, k).astype(np.uint8).tolist()) for k in rng.integers(0, 13, n)]
    b = Bank(gpu_ctx, "path", seed=361, n=n, p_strs=short, b_strs=[s[:12] for s in string_pool(rng)[:40] * 75][:3000], heaps=False)
    specs = [("count_star", None), ("sum", "p_big")]
    want = b.want(["p_s", "b_s"], specs)
    assert b.out.aggregate_hashed_str([b.col("p_s"), b.col("b_s")], b.specs(specs), 1 << 16) == want
    live = [v for v, ok in zip(*b.column("p_s")) if ok]
    assert b.out.aggregate_string("min", *b.col("p_s")) == min(live) and b.out.aggregate_string("max", *b.col("p_s")) == max(live)
    with pytest.raises(capi.PolrError) as e:
        b.out.aggregate_hashed([b.col("p_s")], b.specs(specs), 1024)
    assert e.value.code == capi.E_UNSUPPORTED
    b.close()
    # the same with ONE long non-NULL string on a probe row that is in the join result
    probe = Bank(gpu_ctx, "path", seed=361, n=n, p_strs=short, heaps=False, p_valid=np.ones(n, np.uint8))
    hit = int(probe.rows[len(probe.rows) // 2, 0])
    probe.close()
    long_one = list(short)
    long_one[hit] = b"thirteen byte"
    b = Bank(gpu_ctx, "path", seed=361, n=n, p_strs=long_one, heaps=False, p_valid=np.ones(n, np.uint8))
    with pytest.raises(capi.PolrError) as e:
        b.out.aggregate_hashed_str([b.col("p_s")], b.specs(specs), 1 << 16)
    assert e.value.code == capi.E_INVALID
    with pytest.raises(capi.PolrError) as e:  # (the MIN / MAX sink has the same guard)
        b.out.aggregate_string("max", *b.col("p_s"))
    assert e.value.code == capi.E_INVALID
    b.close()


# ---- SSB-skew Q4.1 with a real VARCHAR c_nation against the reference's own answer (tests/golden/ssb_q41_varchar.json) ----
@pytest.mark.parametrize("engine", ["generic", "flat"])
@pytest.mark.parametrize("run", ["rows", "rows_nulls"])
def test_q41_with_varchar_nation_against_the_reference(gpu_ctx, engine, run):
    """the device is handed c_nation as string_t cells + heap (names of tests/strref.py) and returns the reference's rows:
    GROUP BY d_year, c_nation with profit = SUM(lo_revenue) - SUM(lo_supplycost); `rows_nulls`: c_nation NULL for every
    37th customer, the reference's NULL group among the rows.  Reads the fixture and the regenerated instance only."""
    import common
    from polr_amd import ssb_skew
    gold = common.load_golden("ssb_q41_varchar")
    want = {(r[0], None if r[1] is None else r[1].encode()): r[2] for r in gold[run]}
    assert len(want) == len(gold[run])
    wl = ssb_skew.workload("q4.1", **gold["shape"])
    inst = wl["instance"]
    m = inst.lineorder(0, inst.n_lo, cols=["lo_revenue", "lo_supplycost"])
    names = list(wl["probe"]["cols"].keys()) + ["lo_revenue", "lo_supplycost"]
    cols = list(wl["probe"]["cols"].values()) + [m["lo_revenue"], m["lo_supplycost"]]
    n = len(cols[0])
    cust = wl["joins"][0]
    assert cust["name"] == "customer" and wl["joins"][3]["name"] == "date"
    cust["strings"] = {"c_nation_name": strref.nation_names(cust["payload"]["c_nation"])}
    if run == "rows_nulls":
        assert gold["null_every"] == strref.NULL_EVERY
        cust["strings_valid"] = {"c_nation_name": strref.nation_valid(cust["keys"][0])}
    if engine == "generic":
        for j in wl["joins"]:
            j["perfect"] = None  # hash tables: the generic pool
    joins = capi.build_joins(gpu_ctx, wl, auto=engine == "flat")
    paths = np.asarray(common.load_golden("ssb_skew_sample")["cases"]["q4.1/3"]["paths"], dtype=np.int32)
    pipe = capi.Pipeline(gpu_ctx, cols, n, joins, paths)
    assert pipe.launch_info(True)["flat"] == int(engine == "flat")
    out = capi.Output(pipe, 1024, 16384)
    mpx = capi.DeviceMultiplexer(pipe, "adaptive_reinit")
    capi.run_resident([mpx], [(0, (n + 1023) // 1024)], out=out, reset=True, finish=True)
    mpx.finish()
    gcols = [(3, 0), (0, capi.string_payload_index(cust, "c_nation_name"))]
    specs = [("sum", -1, names.index("lo_revenue")), ("sum", -1, names.index("lo_supplycost")), ("count_star", -1, 0)]
    got = out.aggregate_hashed_str(gcols, specs, 1024)
    assert {k: v[0] - v[1] for k, v in got.items()} == want
    assert sum(v[2] for v in got.values()) == out.stats()[0]
    if run == "rows_nulls":
        assert any(k[1] is None for k in got)
    mpx.close()
    out.close()
    pipe.close()
    for h, _ in joins:
        h.close()
