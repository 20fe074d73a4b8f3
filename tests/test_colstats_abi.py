"""polr_ht_column_stats, polr_pipeline_column_stats, polr_ht_finalize_auto_stats and polr_col_stats_plan_info in header,
library and binding, the part that needs no GPU: the declarations, the exports, the struct's fields and layout, the limits,
the refusal of NULL handles and NULL results, polr_col_stats_plan_info against the stand-alone plan program -- and the numpy
reference the GPU tests compare with (tests/colstats.py) against hand-written cases."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import colstats
import common
import test_colstats_plan as plan
from polr_amd import capi

NAMES = ["polr_ht_column_stats", "polr_pipeline_column_stats", "polr_ht_finalize_auto_stats", "polr_col_stats_plan_info"]
HEADER = os.path.join(common.ROOT, "include", "polr_hip.h")


def test_header_library_and_binding_declare_the_entry_points():
    header = open(HEADER).read()
    lib = capi.load()
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, header), n
        assert n in capi.EXPORTS and hasattr(lib, n), n
    assert re.search(r"#define\s+POLR_MAX_STATS_COLS\s+16\b", header) and capi.MAX_STATS_COLS == 16
    assert re.search(r"#define\s+POLR_STATS_SELECTED\s+1u\b", header) and capi.STATS_SELECTED == 1
    assert re.search(r"#define\s+POLR_ABI_VERSION\s+1\b", header) and lib.polr_abi_version() == 1
    for struct, cls in (("polr_col_stats", capi.ColStats), ("polr_col_stats_plan", capi.ColStatsPlan)):
        fields = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
        fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
        assert re.findall(r"\b(\w+)\s*[,;]", fields) == [f[0] for f in cls._fields_]
    assert [f[0] for f in capi.ColStats._fields_] == ["min_value", "max_value", "n_rows", "n_valid", "n_long", "long_bytes",
                                                      "width", "flags"]
    # statistics of a finalized table are listed as not provided
    doc = header[header.index("Column statistics on the device"):header.index("#define POLR_MAX_STATS_COLS")]
    assert "Not provided: statistics of a finalized table" in doc


def test_struct_layouts_equal_the_headers(tmp_path):
    src, exe = str(tmp_path / "sizes.c"), str(tmp_path / "sizes")
    open(src, "w").write(
        '#include <stdio.h>\n#include <stddef.h>\n#include "polr_hip.h"\n'
        'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(polr_col_stats), offsetof(polr_col_stats, n_rows), '
        'offsetof(polr_col_stats, long_bytes), offsetof(polr_col_stats, width), offsetof(polr_col_stats, flags), '
        'sizeof(polr_col_stats_plan), offsetof(polr_col_stats_plan, n_workgroups), offsetof(polr_col_stats_plan, stride_rows)); '
        'return 0; }\n')
    build = subprocess.run(["gcc", "-std=c99", "-Wall", "-I", os.path.dirname(HEADER), src, "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    S, P = capi.ColStats, capi.ColStatsPlan
    assert got == [C.sizeof(S), S.n_rows.offset, S.long_bytes.offset, S.width.offset, S.flags.offset, C.sizeof(P),
                   P.n_workgroups.offset, P.stride_rows.offset]
    assert got[0] == 56 and got[5] == 32


def test_null_handles_and_null_results_are_refused_without_a_device():
    lib = capi.load()
    cols, st, kind = (C.c_uint32 * 1)(0), (capi.ColStats * 1)(), C.c_uint32(7)
    st[0].n_rows = 99
    assert lib.polr_ht_column_stats(None, None, cols, 1, st) == capi.E_INVALID
    assert lib.polr_pipeline_column_stats(None, None, cols, 1, 0, st) == capi.E_INVALID
    assert lib.polr_ht_finalize_auto_stats(None, None, C.byref(kind), st) == capi.E_INVALID
    assert lib.polr_ht_finalize_auto_stats(None, None, None, None) == capi.E_INVALID
    assert lib.polr_col_stats_plan_info(1000, 4, None) == capi.E_INVALID
    info = capi.ColStatsPlan()
    for width in (0, 3, 5, 32):
        assert lib.polr_col_stats_plan_info(1000, width, C.byref(info)) == capi.E_INVALID
    assert st[0].n_rows == 99 and kind.value == 7  # untouched


def test_plan_info_agrees_with_the_stand_alone_program(tmp_path):
    exe, path = plan.build(tmp_path, None), str(tmp_path / "requests.txt")
    infos = [(n, w) for w in plan.WIDTHS for t in [plan.tile_rows(w)]
             for n in (0, 1, 63, 64, 65, t - 1, t, t + 1, plan.CAP * t - 1, plan.CAP * t, plan.CAP * t + 1, 30_000_000, 2 ** 33)]
    plan.write_requests(path, {}, {}, infos)
    _, _, info = plan.parse(plan.run(exe, path))
    assert len(info) == len(set(infos))
    for (n, w), want in info.items():
        got = capi.col_stats_plan_info(n, w)
        assert [got[f[0]] for f in capi.ColStatsPlan._fields_] == want, (n, w)
    # known answers: 30 M 4-byte cells are 7325 tiles of 4096 rows on 2048 workgroups
    assert capi.col_stats_plan_info(30_000_000, 4) == {"cells_per_load": 4, "loads_in_flight": 4, "tile_rows": 4096,
                                                       "n_workgroups": 2048, "stride_rows": 2048 * 4096,
                                                       "scratch_bytes": 2049 * 40}
    assert capi.col_stats_plan_info(0, 8)["n_workgroups"] == 0 and capi.col_stats_plan_info(0, 8)["scratch_bytes"] == 0


def test_the_numpy_reference_against_hand_written_cases():
    R = colstats.reference
    base = {"n_long": 0, "long_bytes": 0}
    # signed widths: sign-extended, NULL rows apart whatever their cells hold
    assert R(np.array([3, -1, 127, -128], dtype=np.int8), [1, 1, 0, 0]) == dict(
        base, min_value=-1, max_value=3, n_rows=4, n_valid=2, width=1, flags=1)
    assert R(np.array([-1, 5], dtype=np.int16)) == dict(base, min_value=-1, max_value=5, n_rows=2, n_valid=2, width=2, flags=1)
    assert R(np.array([-2 ** 31, 2 ** 31 - 1], dtype=np.int32)) == dict(
        base, min_value=-2 ** 31, max_value=2 ** 31 - 1, n_rows=2, n_valid=2, width=4, flags=1)
    assert R(np.array([-2 ** 63, 2 ** 63 - 1, 0], dtype=np.int64)) == dict(
        base, min_value=-2 ** 63, max_value=2 ** 63 - 1, n_rows=3, n_valid=3, width=8, flags=1)
    # unsigned widths: zero-extended -- 0x80000000 is a large value, 0xFF is 255
    assert R(np.array([0x80000000, 7], dtype=np.uint32)) == dict(
        base, min_value=7, max_value=0x80000000, n_rows=2, n_valid=2, width=4, flags=0)
    assert R(np.array([255, 1], dtype=np.uint8)) == dict(base, min_value=1, max_value=255, n_rows=2, n_valid=2, width=1, flags=0)
    assert R(np.array([65535, 65534], dtype=np.uint16), [1, 0]) == dict(
        base, min_value=65535, max_value=65535, n_rows=2, n_valid=1, width=2, flags=0)
    # unsigned 8 bytes: compared as unsigned, returned as the bit pattern
    assert R(np.array([2 ** 63 + 5, 9], dtype=np.uint64)) == dict(
        base, min_value=9, max_value=-2 ** 63 + 5, n_rows=2, n_valid=2, width=8, flags=0)
    # no non-NULL row, no row at all: both 0
    assert R(np.array([5, 6], dtype=np.int32), [0, 0]) == dict(base, min_value=0, max_value=0, n_rows=2, n_valid=0, width=4, flags=1)
    assert R(np.zeros(0, dtype=np.uint64)) == dict(base, min_value=0, max_value=0, n_rows=0, n_valid=0, width=8, flags=0)
    # through a selection: the rows named, repeats and all
    assert R(np.array([10, 20, 30, 40], dtype=np.int32), [1, 1, 0, 1], rows=[2, 1, 1]) == dict(
        base, min_value=20, max_value=20, n_rows=3, n_valid=2, width=4, flags=1)
    assert R(np.array([10, 20], dtype=np.int32), rows=[]) == dict(base, min_value=0, max_value=0, n_rows=0, n_valid=0, width=4, flags=1)
    # VARCHAR: lengths; long strings are those beyond 12 bytes
    cells, _heap = capi.string_cells([b"", b"x" * 12, b"y" * 13, b"z" * 4096, b"w" * 20])
    assert list(colstats.lengths(cells)) == [0, 12, 13, 4096, 20]
    assert R(cells, [1, 1, 1, 1, 0]) == {"min_value": 0, "max_value": 4096, "n_rows": 5, "n_valid": 4, "n_long": 2,
                                         "long_bytes": 13 + 4096, "width": 16, "flags": 0}
    assert colstats.as_i64(2 ** 64 - 1) == -1 and colstats.as_i64(-5) == -5 and colstats.as_i64(2 ** 63) == -2 ** 63
