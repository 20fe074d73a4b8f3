"""polr_pipeline_scan_filter_expr in header, library and binding, the part that needs no GPU: the declaration, the export,
the refusal of a NULL pipeline, the limits, and the binding's struct layouts against sizeof / offsetof as a C program
compiled against the header prints them."""
import ctypes as C
import os
import re
import subprocess

import common
from polr_amd import capi

NAME = "polr_pipeline_scan_filter_expr"
HEADER = os.path.join(common.ROOT, "include", "polr_hip.h")


def test_header_library_and_binding_declare_the_entry_point():
    header = open(HEADER).read()
    lib = capi.load()
    assert re.search(r"\bint\s+%s\s*\(" % NAME, header)
    assert NAME in capi.EXPORTS and hasattr(lib, NAME)
    for macro, value in (("NODES", capi.MAX_FILTER_NODES), ("DEPTH", capi.MAX_FILTER_DEPTH), ("VALUES", capi.MAX_FILTER_VALUES),
                         ("BYTES", capi.MAX_FILTER_BYTES)):
        assert re.search(r"#define\s+POLR_MAX_FILTER_%s\s+%d\b" % (macro, value), header), macro
    assert (capi.MAX_FILTER_NODES, capi.MAX_FILTER_DEPTH, capi.MAX_FILTER_VALUES, capi.MAX_FILTER_BYTES) == (64, 32, 64, 16384)
    enum = re.search(r"enum \{ (POLR_FX_CMP.*?) \};", header).group(1)
    assert {k.strip()[len("POLR_FX_"):].lower(): int(v) for k, v in (kv.split("=") for kv in enum.split(","))} == capi.FX
    for struct, cls in (("polr_filter_value", capi.FilterValue), ("polr_filter_node", capi.FilterNode)):
        fields = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
        fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
        assert re.findall(r"\b(\w+);", fields) == [f[0] for f in cls._fields_]


def test_null_pipeline_is_invalid_without_a_gpu():
    lib = capi.load()
    ns, nc = C.c_uint64(), C.c_uint64()
    assert lib.polr_pipeline_scan_filter_expr(None, None, None, 0, None, 0, 0, 1024, C.byref(ns), C.byref(nc)) == capi.E_INVALID


def test_struct_layouts_equal_the_headers(tmp_path):
    src, exe = str(tmp_path / "sizes.c"), str(tmp_path / "sizes")
    open(src, "w").write(
        '#include <stdio.h>\n#include <stddef.h>\n#include "polr_hip.h"\n'
        'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(polr_filter_value), sizeof(polr_filter_node), '
        'offsetof(polr_filter_value, str), offsetof(polr_filter_value, str_len), offsetof(polr_filter_node, op), '
        'offsetof(polr_filter_node, first_value), offsetof(polr_filter_node, n_values)); return 0; }\n')
    build = subprocess.run(["gcc", "-std=c99", "-Wall", "-I", os.path.dirname(HEADER), src, "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    V, N = capi.FilterValue, capi.FilterNode
    assert got == [C.sizeof(V), C.sizeof(N), V.str.offset, V.str_len.offset, N.op.offset, N.first_value.offset, N.n_values.offset]
    assert got[:2] == [24, 24]


def test_flatten_filter_expr_is_postfix():
    nodes, values = capi.flatten_filter_expr(("or", ("like", 1, b"%(USA)%"), ("not", ("in", 1, [b"a", "b"])), ("cmp", 2, "is null")))
    assert nodes == [("like", 1, 0, 0, 1), ("in", 1, 0, 1, 2), ("not", 0, 0, 0, 0), ("or", 0, 0, 0, 0), ("cmp", 2, 6, 0, 0),
                     ("or", 0, 0, 0, 0)]
    assert values == [(0, b"%(USA)%", 7), (0, b"a", 1), (0, b"b", 1)]
    assert capi.flatten_filter_expr(("cmp", 0, "<", -5)) == ([("cmp", 0, 2, 0, 1)], [(-5, None, 0)])
    assert capi.flatten_filter_expr(None) == ([], [])
