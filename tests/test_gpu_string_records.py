"""String records, the one format in which strings leave the device (csrc/polr_strrec_plan.h, polr_fetch_str_records of
polr_strheap.hip): ONE set of strings through all three producers -- the whole dictionary (first-appearance and sorted
codes), a code list that is out of order and has duplicates, and polr_out_aggregate_hashed_str over two VARCHAR group
columns with an integer column between them -- and back byte for byte.  Each producer three ways through the C ABI into
canary-filled buffers: the arena exactly *str_used bytes (the last record ends on its last byte), one byte short
(POLR_E_OVERFLOW, *str_used exact, nothing touched), and with slack (the bytes beyond *str_used untouched).  Expected
bytes come from Python over the inputs alone.  Tiny shapes: 16 build rows, 200 probe rows."""
import contextlib
import ctypes as C
import gc

import numpy as np
import pytest

from polr_amd import capi
from test_gpu_sink_matrix import MAX_WAVE_CHUNKS, string_blocks

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 11, 12, 13, 16, 63, 64, 65, 255, 4097]  # inline / heap boundary at 12, 64-byte edges, beyond a page
WORDS = [bytes((31 * n + 7 * j + 1) % 256 for j in range(n)) for n in LENGTHS]
CANARY, CANARY64 = 0xEE, 0xABABABABABABABAB
NB, N = 16, 200
# build rows: every word once, WORDS[4] on three more rows, one NULL row (its cell holds garbage)
S1 = WORDS + [WORDS[4]] * 3 + [b"never read"] + [WORDS[9]]
S1_VALID = np.array([1] * 14 + [0, 1], np.uint8)
# the second VARCHAR column: the same words in another order, NULL on another row
S2 = [WORDS[(3 * i + 5) % len(WORDS)] for i in range(NB)]
S2_VALID = np.array([1] * 6 + [0] + [1] * 9, np.uint8)
G = (np.arange(NB) % 3 - 1).astype(np.int32)  # the integer group column between them: -1, 0, 1
G_VALID = np.array([1] * 11 + [0] + [1] * 4, np.uint8)
assert len(S1) == len(S2) == NB and max(LENGTHS) > 4096


def record(w):
    return len(w).to_bytes(4, "little") + w


def first_appearance(strs, valid):
    seen = []
    for s, ok in zip(strs, valid):
        if ok and s not in seen:
            seen.append(s)
    return seen


@contextlib.contextmanager
def bank(ctx):
    """the build side (s1 VARCHAR, g int32, s2 VARCHAR) keyed 0 .. NB - 1, long strings on an uploaded heap of two blocks;
    every device byte it takes is given back when the block ends"""
    gc.collect()
    live0 = capi.device_bytes_live()
    cells1, heap1 = string_blocks(S1, S1_VALID, 2, 11)
    cells2, heap2 = string_blocks(S2, S2_VALID, 2, 12)
    ht = capi.HashTable.from_columns(ctx, [np.arange(NB, dtype=np.int32)], [cells1, G, cells2],
                                     payload_valid=[S1_VALID, G_VALID, S2_VALID])
    ht.set_payload_heaps(0, heap1)
    ht.set_payload_heaps(2, heap2)
    yield ht
    ht.close()
    gc.collect()
    assert capi.device_bytes_live() == live0


def three_ways(call, used, check_ok):
    """call(str_cap) -> (rc, str_used, arena, the other output buffers); check_ok(arena bytes up to used, others)"""
    rc, got, arena, others = call(used)  # exactly: the last record ends on the arena's last byte
    assert (rc, got) == (capi.OK, used) and len(arena) == used
    check_ok(arena.tobytes(), others)
    rc, got, arena, others = call(used - 1)  # one byte short: nothing is touched
    assert (rc, got) == (capi.E_OVERFLOW, used)
    assert (arena == CANARY).all()
    for o in others:
        assert (o == CANARY64).all()
    rc, got, arena, others = call(used + 37)  # slack: the bytes beyond used are untouched
    assert (rc, got) == (capi.OK, used)
    assert (arena[used:] == CANARY).all()
    check_ok(arena[:used].tobytes(), others)


def canary_arena(cap):
    """an arena of exactly cap bytes inside a larger canary buffer: the guard bytes behind it stay as they are"""
    whole = np.full(cap + 64, CANARY, np.uint8)
    return whole, whole[:cap]


@pytest.mark.parametrize("sorted_", [False, True], ids=["first-appearance", "sorted"])
def test_whole_dictionary(gpu_ctx, sorted_):
    with bank(gpu_ctx) as ht:
        words = first_appearance(S1, S1_VALID)
        assert sorted(words) == sorted(WORDS)
        if sorted_:
            words = sorted(words)
        code_col, n_codes, has_null = ht.encode_dictionary(0, sorted=sorted_)
        assert (code_col, n_codes, has_null) == (3, len(WORDS), 1)
        want = b"".join(record(w) for w in words)  # code after code
        want_offs = np.cumsum([0] + [4 + len(w) for w in words[:-1]]).astype(np.uint64)

        def call(cap):
            whole, arena = canary_arena(cap)
            offs = np.full(n_codes + 2, CANARY64, np.uint64)
            used = C.c_uint64()
            rc = gpu_ctx.L.polr_ht_fetch_dictionary(ht.h, code_col, None, offs.ctypes.data, n_codes, arena.ctypes.data, cap, C.byref(used))
            assert (whole[cap:] == CANARY).all() and (offs[n_codes:] == CANARY64).all()
            return rc, used.value, arena, [offs[:n_codes]]

        def check_ok(raw, others):
            assert raw == want and np.array_equal(others[0], want_offs)

        three_ways(call, len(want), check_ok)
        assert ht.dictionary(code_col, str_cap=1) == words  # (the binding's decoder and its one retry)


@pytest.mark.parametrize("sorted_", [False, True], ids=["first-appearance", "sorted"])
def test_code_list_out_of_order_with_duplicates(gpu_ctx, sorted_):
    with bank(gpu_ctx) as ht:
        words = first_appearance(S1, S1_VALID)
        if sorted_:
            words = sorted(words)
        code_col, n_codes, _ = ht.encode_dictionary(0, sorted=sorted_)
        codes = np.array([10, 0, 10, 4, 3, 4, 9, 0, 1, 2, 5, 6, 7, 8, 10], np.uint32)  # every code, three of them twice or more
        assert set(codes.tolist()) == set(range(n_codes))
        listed = [words[c] for c in codes.tolist()]
        want = b"".join(record(w) for w in listed)  # list order, a record per duplicate
        want_offs = np.cumsum([0] + [4 + len(w) for w in listed[:-1]]).astype(np.uint64)
        n = len(codes)

        def call(cap):
            whole, arena = canary_arena(cap)
            offs = np.full(n + 2, CANARY64, np.uint64)
            used = C.c_uint64()
            rc = gpu_ctx.L.polr_ht_fetch_dictionary_codes(ht.h, code_col, None, codes.ctypes.data, n, offs.ctypes.data,
                                                          arena.ctypes.data, cap, C.byref(used))
            assert (whole[cap:] == CANARY).all() and (offs[n:] == CANARY64).all()
            return rc, used.value, arena, [offs[:n]]

        def check_ok(raw, others):
            assert raw == want and np.array_equal(others[0], want_offs)

        three_ways(call, len(want), check_ok)
        assert ht.dictionary_strings(code_col, codes, str_cap=1) == listed


def test_hashed_groups_two_varchar_columns_around_an_integer(gpu_ctx):
    """GROUP BY s1, g, s2 over a join that keeps every build row: the records go group-major, then column; the integer
    column and a NULL value take none (key word: the integer, and 0)"""
    with bank(gpu_ctx) as ht:
        ht.finalize_hash()
        pk = (np.arange(N) % NB).astype(np.int32)
        pipe = capi.Pipeline(gpu_ctx, [pk], N, [(ht, [(-1, 0)])], [[0]])
        out = capi.Output(pipe, 64, N // 64 + 1 + MAX_WAVE_CHUNKS)
        pipe.probe_rounds([(0, N, 0, 1)], out=out)
        assert len(out.fetch_ids()) == N
        groups = {}
        for r in pk.tolist():
            key = (S1[r] if S1_VALID[r] else None, int(G[r]) if G_VALID[r] else None, S2[r] if S2_VALID[r] else None)
            groups[key] = groups.get(key, 0) + 1
        n_groups = len(groups)
        assert any(k[0] is None for k in groups) and any(k[1] is None for k in groups) and any(k[2] is None for k in groups)
        used_want = sum(4 + len(s) for k in groups for s in (k[0], k[2]) if s is not None)
        cols, specs = capi._group_keys([(0, 0), (0, 1), (0, 2)])[0], capi._agg_specs([("count_star", -1, 0)])
        max_groups = 32

        def call(cap):
            whole, arena = canary_arena(cap)
            keys = np.full((max_groups, 3), CANARY64, np.uint64)
            nulls = np.full(2 * max_groups, CANARY64, np.uint64)  # (uint32 words under one canary pattern)
            res = np.full(max_groups * C.sizeof(capi.AggValue) // 8, CANARY64, np.uint64)
            n, used = C.c_uint64(), C.c_uint64()
            rc = gpu_ctx.L.polr_out_aggregate_hashed_str(out.h, None, cols, 3, specs, 1, max_groups, keys.ctypes.data, nulls.ctypes.data,
                                                         res.ctypes.data, C.byref(n), arena.ctypes.data, cap, C.byref(used))
            assert (whole[cap:] == CANARY).all() and n.value == n_groups
            return rc, used.value, arena, [keys, nulls, res]

        def check_ok(raw, others):
            keys = others[0].view(np.int64)
            nulls = others[1].view(np.uint32)
            res = (capi.AggValue * max_groups).from_buffer(others[2])
            at, got = 0, {}
            for g in range(n_groups):
                key = []
                for c in range(3):
                    if (nulls[g] >> c) & 1:
                        assert c == 1 or keys[g, c] == 0  # (a NULL VARCHAR value: no record, key word 0)
                        key.append(None)
                    elif c == 1:
                        key.append(int(keys[g, c]))
                    else:
                        assert keys[g, c] == at  # records interleave: group-major, then column, nothing between them
                        w = capi._record(raw, at)
                        at += 4 + len(w)
                        key.append(w)
                got[tuple(key)] = capi._agg_int(res[g])
            assert at == len(raw) == used_want and got == groups
            assert (others[0][n_groups:] == CANARY64).all()

        three_ways(call, used_want, check_ok)
        # (the binding's decoder and its one retry)
        assert out.aggregate_hashed_str([(0, 0), (0, 1), (0, 2)], [("count_star", -1, 0)], max_groups, str_cap=1) == {
            k: [v] for k, v in groups.items()}
        out.close()
        pipe.close()
