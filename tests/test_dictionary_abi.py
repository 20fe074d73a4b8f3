"""The dictionary entry points of the C ABI (polr_ht_encode_dictionary / polr_ht_fetch_dictionary) on a machine without a
GPU: declared in the header, exported by the library, declared by the binding; a NULL handle is refused before anything
touches a device.  What they compute is checked on the GPU (tests/test_gpu_dictionary.py)."""
import ctypes as C
import os
import re

import common
from polr_amd import capi

NAMES = ["polr_ht_encode_dictionary", "polr_ht_fetch_dictionary"]


def test_header_library_and_binding_have_both_entry_points():
    text = open(os.path.join(common.ROOT, "include", "polr_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = capi.load()
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, code), "include/polr_hip.h does not declare %s" % n
        assert hasattr(lib, n), "libpolr_hip.so does not export %s" % n
        assert n in capi.EXPORTS
        assert getattr(lib, n).argtypes is not None
    assert lib.polr_abi_version() == 1  # (additive: the ABI version stays)
    assert hasattr(capi.HashTable, "encode_dictionary") and hasattr(capi.HashTable, "dictionary")


def test_null_handles_and_null_results_are_refused_without_a_device():
    lib = capi.load()
    col, n, null, used = C.c_uint32(7), C.c_uint32(7), C.c_uint32(7), C.c_uint64(7)
    assert lib.polr_ht_encode_dictionary(None, 0, None, C.byref(col), C.byref(n), C.byref(null)) == capi.E_INVALID
    assert (col.value, n.value, null.value) == (7, 7, 7)
    assert lib.polr_ht_fetch_dictionary(None, 0, None, None, 0, None, 0, C.byref(used)) == capi.E_INVALID
    assert used.value == 7


class StubTable:
    """stands in for capi.HashTable: records what build_joins calls, in order"""

    def __init__(self):
        self.calls = []

    def set_payload_heap(self, col, heap):
        self.calls.append(("heap", col))

    def set_key_flags(self, c, f):
        self.calls.append(("flags", c))

    def encode_dictionary(self, col):
        self.calls.append(("encode", col))
        return 10 + col, 3, 1

    def finalize_hash(self):
        self.calls.append(("finalize",))


def _join(**extra):
    import numpy as np
    return dict({"keys": [np.arange(4, dtype=np.int32)], "payload": {"a": np.arange(4, dtype=np.int32), "b": np.arange(4, dtype=np.int32)},
                 "strings": {"s": [b"x", b"y" * 20, b"x", b"z"], "t": [b"p", b"q", b"p", b"q"]}, "key_src": [(-1, 0)]}, **extra)


def test_build_joins_encodes_only_the_columns_named_under_dictionary(monkeypatch):
    """without the key build_joins never reaches encode_dictionary; with it, exactly the named columns are encoded, after their
    heap is set and before the table is finalized, and dictionary_payload_index returns what the call returned"""
    made = []

    def from_columns(ctx, keys, payload, key_valid=None, payload_valid=None):
        assert len(payload) == 4  # (two fixed-width columns, then the two VARCHAR ones)
        made.append(StubTable())
        return made[-1]
    monkeypatch.setattr(capi.HashTable, "from_columns", staticmethod(from_columns))
    plain = _join()
    capi.build_joins(None, {"joins": [plain]})
    assert made[-1].calls == [("heap", 2), ("heap", 3), ("finalize",)]
    assert "dictionary_cols" not in plain
    both = _join(dictionary=["t", "s"])
    capi.build_joins(None, {"joins": [both]})
    assert made[-1].calls == [("heap", 2), ("heap", 3), ("encode", 3), ("encode", 2), ("finalize",)]
    assert capi.dictionary_payload_index(both, "t") == (13, (3, 1)) and capi.dictionary_payload_index(both, "s") == (12, (3, 1))
    one = _join(dictionary=["s"])
    capi.build_joins(None, {"joins": [one]})
    assert made[-1].calls == [("heap", 2), ("heap", 3), ("encode", 2), ("finalize",)]
    assert list(one["dictionary_cols"]) == ["s"]
