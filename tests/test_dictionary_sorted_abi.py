"""The sorted-dictionary entry points of the C ABI (polr_ht_encode_dictionary_ex / polr_ht_fetch_dictionary_codes) on a
machine without a GPU: declared in the header with their two flags, exported by the library, declared by the binding; a NULL
handle is refused before anything touches a device.  What they compute is checked on the GPU
(tests/test_gpu_dictionary_sorted.py)."""
import ctypes as C
import inspect
import os
import re

import numpy as np

import common
from polr_amd import capi

NAMES = ["polr_ht_encode_dictionary_ex", "polr_ht_fetch_dictionary_codes"]
FLAGS = {"POLR_DICT_SORTED": 1, "POLR_DICT_NULL_INVALID": 2}


def _header():
    text = open(os.path.join(common.ROOT, "include", "polr_hip.h")).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_library_and_binding_have_both_entry_points_and_both_flags():
    _text, code = _header()
    lib = capi.load()
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, code), "include/polr_hip.h does not declare %s" % n
        assert hasattr(lib, n), "libpolr_hip.so does not export %s" % n
        assert n in capi.EXPORTS
        assert getattr(lib, n).argtypes is not None
    for name, value in FLAGS.items():
        m = re.search(r"#define\s+%s\s+(\d+)u\b" % name, code)
        assert m and int(m.group(1)) == value, name
    assert (capi.DICT_SORTED, capi.DICT_NULL_INVALID) == (1, 2)
    assert lib.polr_abi_version() == 1  # (additive: the ABI version stays)
    assert hasattr(capi.HashTable, "dictionary_strings")
    params = inspect.signature(capi.HashTable.encode_dictionary).parameters
    assert params["sorted"].default is False and params["null_invalid"].default is False  # (the defaults keep the old call)


def test_the_header_no_longer_lists_sorted_codes_as_missing():
    text, _code = _header()
    missing = [m for m in re.findall(r"Not provided:[^*]*?\*/", text, flags=re.S) if "probe-side columns" in m]
    assert len(missing) == 1
    assert "dictionaries of probe-side columns" in missing[0] and "sorted" not in missing[0]


def test_null_handles_and_null_results_are_refused_without_a_device():
    lib = capi.load()
    col, n, null, used = C.c_uint32(7), C.c_uint32(7), C.c_uint32(7), C.c_uint64(7)
    for flags in (0, 1, 2, 3, 4):
        assert lib.polr_ht_encode_dictionary_ex(None, 0, flags, None, C.byref(col), C.byref(n), C.byref(null)) == capi.E_INVALID
    assert (col.value, n.value, null.value) == (7, 7, 7)
    codes = np.zeros(1, np.uint32)
    assert lib.polr_ht_fetch_dictionary_codes(None, 0, None, codes.ctypes.data, 1, None, None, 0, C.byref(used)) == capi.E_INVALID
    assert used.value == 7


class StubTable:
    """stands in for capi.HashTable: records what build_joins calls, in order"""

    def __init__(self):
        self.calls = []

    def set_payload_heap(self, col, heap):
        pass

    def encode_dictionary(self, col, **kw):
        self.calls.append((col, kw))
        return 10 + col, 3, 1

    def finalize_hash(self):
        pass


def test_build_joins_passes_dictionary_flags_per_column(monkeypatch):
    """j["dictionary_flags"] = {name: flags}: a named column is encoded with its flags, any other as before"""
    made = []

    def from_columns(ctx, keys, payload, key_valid=None, payload_valid=None):
        made.append(StubTable())
        return made[-1]
    monkeypatch.setattr(capi.HashTable, "from_columns", staticmethod(from_columns))
    j = {"keys": [np.arange(4, dtype=np.int32)], "payload": {"a": np.arange(4, dtype=np.int32)},
         "strings": {"s": [b"x", b"y" * 20, b"x", b"z"], "t": [b"p", b"q", b"p", b"q"]}, "key_src": [(-1, 0)],
         "dictionary": ["s", "t"], "dictionary_flags": {"t": capi.DICT_SORTED | capi.DICT_NULL_INVALID}}
    capi.build_joins(None, {"joins": [j]})
    assert made[-1].calls == [(1, {}), (2, {"flags": 3})]
    assert capi.dictionary_payload_index(j, "t") == (12, (3, 1))
