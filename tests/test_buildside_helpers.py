"""tests/buildside.py against the oracle, without a GPU: row_blob is the byte image orc.HashTable serialises (outside the 8
trailing bytes of a row, where the oracle keeps chain pointers), perfect_arrays what make_perfect leaves."""
import numpy as np
import pytest

import buildside
from common import orc
from joinref import DTYPES, _perfect_ranges


def ten_columns(seed, n):
    """two keys (int16, uint8: the second NULL = NULL) and eight payload columns of widths 1, 2, 4, 8, signed and unsigned:
    10 columns -> 2 validity bytes, a 43-byte row, nothing aligned.  NULLs in both keys and in columns 7, 8 and 9 (the last
    two have their bits in the second validity byte) -> (keys, key_valid, payload, payload_valid, null_equal)"""
    rng = np.random.default_rng(seed)
    keys = [rng.integers(-40, 40, n).astype(np.int16), rng.integers(0, 12, n).astype(np.uint8)]
    key_valid = [(rng.random(n) > 0.04).astype(np.uint8), (rng.random(n) > 0.1).astype(np.uint8)]
    payload = []
    for dt in DTYPES:
        info = np.iinfo(dt)
        payload.append(rng.integers(info.min, info.max, n, dtype=dt, endpoint=True))
    payload_valid = [None] * 5 + [(rng.random(n) > f).astype(np.uint8) for f in (0.1, 0.3, 0.5)]
    return keys, key_valid, payload, payload_valid, [False, True]


def same_outside_trailer(blob, oblob, row_width):
    a, b = blob.reshape(-1, row_width), np.asarray(oblob).reshape(-1, row_width)
    return a.shape == b.shape and np.array_equal(a[:, :-buildside.TRAILER], b[:, :-buildside.TRAILER])


def test_row_blob_ten_unaligned_columns():
    keys, kv, pay, pv, ne = ten_columns(1, 3000)
    blob, row_width, offs, kept = buildside.row_blob(keys, kv, pay, pv, ne)
    oht = orc.HashTable(keys, pay, key_valid=kv, payload_valid=pv, null_equal=ne)
    assert row_width == oht.row_width == 43 and offs[0] == 2
    assert offs == [oht.col_offset(i) for i in range(10)]
    assert len(kept) == oht.count and 0 < len(kept) < 3000
    assert np.array_equal(kept, oht.orig_rows())
    assert same_outside_trailer(blob, oht.rows_blob(), row_width)
    rows = blob.reshape(-1, row_width)
    assert (rows[:, -buildside.TRAILER:] != 0).all()
    assert (rows[:, 1] != 0xFF).any() and (rows[:, 0] & 2 == 0).any()  # second validity byte in use; NULL keys kept
    assert (rows[:, 0] & 1 == 1).all()  # (the first key is not NULL = NULL: its NULL rows are gone)


@pytest.mark.parametrize("dt", DTYPES, ids=[np.dtype(d).name for d in DTYPES])
def test_row_blob_single_key(dt):
    rng = np.random.default_rng(2)
    info = np.iinfo(dt)
    for n in (0, 1, 257):
        keys = [rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)]
        kv = [(rng.random(n) > 0.2).astype(np.uint8)]
        pay = [rng.integers(-100, 100, n).astype(np.int16), np.frombuffer(rng.bytes(16 * n), dtype="V16").copy()]
        pv = [(rng.random(n) > 0.2).astype(np.uint8), None]
        blob, row_width, offs, kept = buildside.row_blob(keys, kv, pay, pv)
        oht = orc.HashTable(keys, pay, key_valid=kv, payload_valid=pv)
        assert row_width == oht.row_width and offs == [oht.col_offset(i) for i in range(3)]
        assert np.array_equal(kept, oht.orig_rows())
        assert same_outside_trailer(blob, oht.rows_blob(), row_width)


PERFECT_CASES = [(dt, name) for dt in DTYPES for name in _perfect_ranges(dt)]


@pytest.mark.parametrize("dt,name", PERFECT_CASES, ids=["%s-%s" % (np.dtype(d).name, k) for d, k in PERFECT_CASES])
def test_perfect_arrays(dt, name):
    """bitmap and slot -> build row against make_perfect + pht_bitmap() + pht_orig_rows(); the cells against the build
    rows they came from"""
    rng = np.random.default_rng(3)
    lo, hi = _perfect_ranges(dt)[name]
    ulo = lo & buildside.U64 if dt == np.uint64 else lo
    size = ((hi - lo) & buildside.U64) + 1
    picks = rng.permutation(size)[: min(size, 2000) * 3 // 4]
    keys = np.array([ulo + int(x) for x in picks], dtype=np.uint64 if dt == np.uint64 else np.int64).astype(dt)
    n = len(keys)
    kv = (rng.random(n) > 0.05).astype(np.uint8)
    pay = [rng.integers(-120, 120, n).astype(np.int8), rng.integers(0, 2**63, n).astype(np.uint64)]
    pv = [(rng.random(n) > 0.2).astype(np.uint8), None]
    bitmap, cells, cell_valid, id_to_row = buildside.perfect_arrays(keys, kv, pay, pv, lo, hi)
    oht = orc.HashTable([keys], pay, key_valid=[kv], payload_valid=pv)
    assert oht.make_perfect(lo, hi)
    assert bitmap.dtype == np.uint8 and np.array_equal(bitmap, oht.pht_bitmap())
    orows = oht.pht_orig_rows()
    assert np.array_equal(np.where(id_to_row < 0, 0xFFFFFFFF, id_to_row), orows.astype(np.int64))
    assert bitmap.sum() == kv.sum() and np.array_equal(bitmap == 1, id_to_row >= 0)
    ids = np.nonzero(bitmap)[0]
    for c in range(2):
        ok = np.ones(n, bool) if pv[c] is None else pv[c].astype(bool)
        assert np.array_equal(cell_valid[c][ids], ok[id_to_row[ids]])
        assert np.array_equal(cells[c][ids], np.where(ok, pay[c], 0)[id_to_row[ids]])
        assert not cells[c][bitmap == 0].any() and not cell_valid[c][bitmap == 0].any()


def test_perfect_arrays_leave_out_keys_outside_the_range():
    keys = np.array([-5, 0, 3, 9, 10, 11, 127], dtype=np.int8)
    bitmap, _, _, id_to_row = buildside.perfect_arrays(keys, None, [], None, 0, 10)
    assert bitmap.tolist() == [1, 0, 0, 1, 0, 0, 0, 0, 0, 1, 1]
    assert id_to_row[[0, 3, 9, 10]].tolist() == [1, 2, 3, 4]


def test_key_codes_null_equal_and_by_value():
    """NULL = NULL only in the flagged column; a NULL elsewhere takes the row out; columns compare by value across types"""
    bk = [np.array([1, 1, 2, 2], np.int64), np.array([7, 0, 7, 0], np.uint8)]
    bv = [None, np.array([1, 0, 1, 0], np.uint8)]
    pk = [np.array([1, 1, 2, 3, 1], np.int32), np.array([7, 9, 7, 7, 0], np.uint8)]
    pv = [np.array([1, 1, 0, 1, 1], np.uint8), np.array([1, 0, 1, 1, 1], np.uint8)]
    bc, bok, pc, pok = buildside.key_codes(bk, bv, pk, pv, null_equal=[False, True])
    assert bok.all() and pok.tolist() == [True, True, False, True, True]
    match = [[int(b) for b in np.nonzero(bok & (bc == c))[0]] if ok else [] for c, ok in zip(pc, pok)]
    assert match == [[0], [1], [], [], []]
