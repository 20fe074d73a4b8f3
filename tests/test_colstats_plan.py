"""The host-side plan of polr_ht_column_stats / polr_pipeline_column_stats / polr_ht_finalize_auto_stats
(duckdb-polr_amd/csrc/polr_colstats_plan.h), the part that needs no GPU: the header alone behind a stand-alone host program
(tests/colstats/colstats_plan_main.cpp).  Every refusal with its code and whole message, in the documented order (a request
that earns several is refused for the first); 16 columns and 17; the column numbering at n_keys - 1 and n_keys; the launch
shape and the scratch at 0, 1, one tile +- 1 and grid cap x tile +- 1 rows for every width, with aligned and unaligned bases
and through a selection; and the decision table of polr_ht_finalize_auto_stats.  Built plain and with the address +
undefined-behaviour sanitizers, and run directly."""
import os
import subprocess

import pytest

import common

SRC = os.path.join(common.ROOT, "tests", "colstats", "colstats_plan_main.cpp")
OK, INVALID, UNSUPPORTED = 0, -2, -3
BLOCK, LOADS, CAP, WORDS = 256, 4, 2048, 5  # lanes, loads in flight per lane, workgroups of a launch, 8-byte words of a record
WIDTHS = (1, 2, 4, 8, 16)
AUTO, HASH = 0, 1
HT, PIPE = "polr_ht_column_stats: ", "polr_pipeline_column_stats: "
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1


def tile_rows(width, selected=False):
    return BLOCK * LOADS * (1 if selected else 16 // width)


def req(table=True, handle=1, has_cols=1, stats=1, finalized=0, n_keys=1, flags=0, selected=0, rows=1000,
        columns=((4, 1, 0),), cols=(0,), n_cols=None, code=OK, message=None):
    return dict(state=(int(table), handle, has_cols, stats, finalized), n_keys=n_keys, flags=(flags, selected), rows=rows,
                columns=list(columns), cols=list(cols), n_cols=n_cols, code=code, message=message)


def cases():
    c = {}
    five = [(4, 1, 0), (8, 1, 0), (2, 0, 0), (1, 1, 0), (16, 0, 0)]
    c["one_column"] = req()
    # the refusals of the contract, each alone ...
    c["null_table"] = req(handle=0, code=INVALID, message=HT + "the table is NULL")
    c["null_pipeline"] = req(table=False, handle=0, code=INVALID, message=PIPE + "the pipeline is NULL")
    c["null_cols"] = req(has_cols=0, n_cols=1, code=INVALID, message=HT + "cols is NULL")
    c["null_stats"] = req(stats=0, code=INVALID, message=HT + "stats is NULL")
    c["no_cols"] = req(cols=(), code=INVALID, message=HT + "no columns (n_cols is 0)")
    c["cols_16"] = req(columns=five, n_keys=2, cols=[i % 5 for i in range(16)])
    c["cols_17"] = req(columns=five, n_keys=2, cols=[i % 5 for i in range(17)], code=UNSUPPORTED,
                       message=HT + "17 columns (at most 16 in one call)")
    c["finalized"] = req(finalized=1, code=INVALID,
                         message=HT + "the table is finalized (statistics are taken before polr_ht_finalize_*)")
    c["pipeline_finalized_means_nothing"] = req(table=False, finalized=1)
    c["flag_bits"] = req(table=False, flags=2, code=INVALID, message=PIPE + "flags 0x2 (0 or POLR_STATS_SELECTED)")
    c["flag_bits_beside_selected"] = req(table=False, flags=5, code=INVALID, message=PIPE + "flags 0x5 (0 or POLR_STATS_SELECTED)")
    c["col_beyond"] = req(columns=five, n_keys=2, cols=(4, 5, 9), code=INVALID,
                          message=HT + "cols[1]: column 5 out of range (5 columns)")
    c["col_beyond_pipeline"] = req(table=False, cols=(1,), code=INVALID,
                                   message=PIPE + "cols[0]: column 1 out of range (1 columns)")
    # ... and in their order: the earlier one wins
    c["order_null_first"] = req(handle=0, has_cols=0, stats=0, finalized=1, cols=(), code=INVALID, message=HT + "the table is NULL")
    c["order_cols_before_stats"] = req(has_cols=0, stats=0, n_cols=0, code=INVALID, message=HT + "cols is NULL")
    c["order_stats_before_count"] = req(stats=0, cols=(), finalized=1, code=INVALID, message=HT + "stats is NULL")
    c["order_count_before_finalized"] = req(cols=(), finalized=1, code=INVALID, message=HT + "no columns (n_cols is 0)")
    c["order_limit_before_finalized"] = req(finalized=1, cols=[9] * 17, code=UNSUPPORTED,
                                            message=HT + "17 columns (at most 16 in one call)")
    c["order_finalized_before_col"] = req(finalized=1, cols=(9,), code=INVALID, message=c["finalized"]["message"])
    c["order_flags_before_col"] = req(table=False, flags=2, cols=(9,), code=INVALID, message=c["flag_bits"]["message"])
    c["order_first_col_first"] = req(columns=five, cols=(0, 7, 6), code=INVALID,
                                     message=HT + "cols[1]: column 7 out of range (5 columns)")
    # the numbering: keys first, then payload
    c["numbering"] = req(columns=five, n_keys=2, cols=(1, 2, 0, 4, 1))
    c["numbering_pipeline"] = req(table=False, columns=five, cols=(3, 0))
    # the launch shape and the scratch, for every width: 0, 1, one tile +- 1, the first stride +- 1
    for w in WIDTHS:
        t = tile_rows(w)
        for n in (0, 1, 63, 64, 65, 16 // w if w < 16 else 1, t - 1, t, t + 1, t + 16 // w if w < 16 else t + 1,
                  CAP * t - 1, CAP * t, CAP * t + 1, CAP * t + t):
            c["shape_w%d_n%d" % (w, n)] = req(rows=n, columns=[(w, 0, 0)])
        # a base that is only as aligned as its cells: the rows up to the next 16-byte boundary are read one by one
        for off in (1, 3, 7):
            for n in (0, 1, 5, 40, t + 3):
                c["shape_w%d_off%d_n%d" % (w, off, n)] = req(rows=n, columns=[(w, 0, 4096 + off * w)])
        # through a selection list: one row per load, whatever the width and the base
        for n in (0, 1, 1023, 1024, 1025):
            c["selected_w%d_n%d" % (w, n)] = req(table=False, flags=1, selected=1, rows=n, columns=[(w, 0, 4096 + w)])
    # several columns share the workgroups of one launch
    c["five_columns"] = req(rows=30_000_000, columns=five, n_keys=1, cols=(0, 1, 2, 3, 4))
    c["sixteen_columns"] = req(rows=30_000_000, columns=five, n_keys=1, cols=[i % 5 for i in range(16)])
    return c


def write_requests(path, reqs, finals, infos):
    with open(path, "w") as f:
        for name, r in reqs.items():
            f.write("request %s\nstate %d %d %d %d %d\ntable %d\nflags %d %d\nrows %d\n" %
                    ((name,) + tuple(r["state"]) + (r["n_keys"],) + tuple(r["flags"]) + (r["rows"],)))
            for col in r["columns"]:
                f.write("column %d %d %d\n" % col)
            f.write("cols %s\n" % " ".join(str(x) for x in r["cols"]))
            if r["n_cols"] is not None:
                f.write("ncols %d\n" % r["n_cols"])
            f.write("end\n")
        for name, a in finals.items():
            f.write("finalize %s %d %d %d %d %d %d %d %d %d\n" % ((name,) + tuple(a[:9])))
        for n, w in infos:
            f.write("info %d %d\n" % (n, w))


def parse(stdout):
    out, fin, info, cur = {}, {}, {}, None
    for line in stdout.splitlines():
        if line.startswith("  "):
            key, *rest = line.split()
            cur.setdefault(key, []).append([int(x) for x in rest])
        elif line.startswith("finalize "):
            _, name, *rest = line.split()
            fin[name] = [int(x) for x in rest]
        elif line.startswith("info "):
            v = [int(x) for x in line.split()[1:]]
            info[(v[0], v[1])] = v[2:]
        elif line not in ("ok",) and not line.endswith(" requests"):
            name, code, *msg = line.split(" ", 2)
            cur = out[name] = {"code": int(code), "message": " ".join(msg)}
    return out, fin, info


def want_shape(n, width, addr, selected, cap):
    """[cells_per_load, tile_rows, head_rows, n_loads, tail_rows, n_tiles, grid, stride_rows]"""
    v = 1 if selected else 16 // width
    head = 0
    if v > 1 and addr % 16:
        head = (16 - addr % 16 + width - 1) // width
    head = min(head, n)
    n_loads = (n - head) // v
    tail = n - head - n_loads * v
    n_tiles = (n_loads + BLOCK * LOADS - 1) // (BLOCK * LOADS)
    grid = min(n_tiles or (1 if n else 0), cap)
    return [v, BLOCK * LOADS * v, head, n_loads, tail, n_tiles, grid, grid * BLOCK * LOADS * v]


def check_plan(got, r):
    table, n_keys = r["state"][0], r["n_keys"]
    cap = CAP // len(r["cols"])
    rows, grids = [], []
    for i, col in enumerate(r["cols"]):
        width, _flags, addr = r["columns"][col]
        s = want_shape(r["rows"], width, addr, r["flags"][1], cap)
        is_key = int(bool(table) and col < n_keys)
        idx = col if not table or is_key else col - n_keys
        rows.append([i, col, is_key, idx] + s)
        grids.append(s[6])
        # every row is read exactly once: the head, the whole loads, the tail
        assert s[2] + s[3] * s[0] + s[4] == r["rows"] and s[2] < 16 and s[4] < s[0]
    assert got["col"] == rows
    grid = max(grids)
    if grid == 0:
        assert got["launch"] == [[0, 0, 0, 8 * WORDS, 0]]  # no rows: nothing launched, no scratch
    else:
        result_off = len(r["cols"]) * grid * 8 * WORDS
        assert got["launch"] == [[grid, 0, result_off, 8 * WORDS, result_off + len(r["cols"]) * 8 * WORDS]]
        assert grid * len(r["cols"]) <= CAP


def finalize_cases():
    """name -> (n_keys, flags0, flags1, n_rows_in, wants_stats, n_valid, min, max, signed,   needs_pass, decision, tries_perfect)"""
    f = {}
    f["dense"] = (1, 0, 0, 1000, 0, 1000, 0, 999, 1, 1, AUTO, 1)
    f["dense_with_nulls"] = (1, 0, 0, 1000, 0, 900, -50, 7000, 1, 1, AUTO, 1)  # range / 8 <= rows as uploaded
    f["small_range_few_rows"] = (1, 0, 0, 10, 1, 10, 0, 999_999, 1, 1, AUTO, 1)
    f["small_range_at_the_bound"] = (1, 0, 0, 10, 0, 10, 5, 1_000_005, 1, 1, AUTO, 1)
    f["sparse"] = (1, 0, 0, 10, 0, 10, 0, 1_000_001, 1, 1, AUTO, 0)  # finalize_auto goes straight to a hash table
    f["sparse_wide"] = (1, 0, 0, 1000, 0, 1000, I64_MIN, I64_MAX, 1, 1, AUTO, 0)
    f["all_null"] = (1, 0, 0, 1000, 0, 0, 0, 0, 1, 1, HASH, 0)
    f["all_null_wants_stats"] = (1, 0, 0, 1000, 1, 0, 0, 0, 1, 1, HASH, 0)
    f["no_rows"] = (1, 0, 0, 0, 0, 0, 0, 0, 1, 1, HASH, 0)
    f["two_keys"] = (2, 0, 0, 1000, 0, 1000, 0, 999, 1, 0, HASH, 0)  # no pass at all
    f["two_keys_wants_stats"] = (2, 0, 0, 1000, 1, 1000, 0, 999, 1, 1, HASH, 0)  # the pass, for the caller alone
    f["by_value_key"] = (1, 1, 0, 1000, 0, 1000, 0, 999, 1, 0, HASH, 0)
    f["null_equal_key_wants_stats"] = (1, 2, 0, 1000, 1, 1000, 0, 999, 1, 1, HASH, 0)
    f["flag_on_second_key"] = (2, 0, 1, 1000, 0, 1000, 0, 999, 1, 0, HASH, 0)
    # an unsigned 8-byte range across 2^63: ordered as unsigned (min 2^63 - 3, max 2^63 + 5, as bit patterns) ...
    f["unsigned_across_2_63"] = (1, 0, 0, 9, 0, 9, 2 ** 63 - 3, colstats_i64(2 ** 63 + 5), 0, 1, AUTO, 1)
    # ... the same two bit patterns read as signed are out of order: no perfect table
    f["signed_reading_of_it"] = (1, 0, 0, 9, 0, 9, 2 ** 63 - 3, colstats_i64(2 ** 63 + 5), 1, 1, AUTO, 0)
    return f


def colstats_i64(x):
    return x - 2 ** 64 if x >= 2 ** 63 else x


def build(tmp_path, sanitize):
    exe = str(tmp_path / "colstats_plan")
    flags = ["-fsanitize=" + sanitize, "-fno-sanitize-recover=all"] if sanitize else []
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall"] + flags + [SRC, "-o", exe], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-4000:]
    return exe


def run(exe, path):
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    return r.stdout


@pytest.mark.parametrize("sanitize", [None, "address,undefined"], ids=["plain", "asan-ubsan"])
def test_refusals_numbering_shape_and_the_finalize_table(tmp_path, sanitize):
    exe, path = build(tmp_path, sanitize), str(tmp_path / "requests.txt")
    reqs, finals = cases(), finalize_cases()
    infos = [(n, w) for w in WIDTHS for n in (0, 1, tile_rows(w), CAP * tile_rows(w) + 1)]
    write_requests(path, reqs, finals, infos)
    stdout = run(exe, path)
    assert stdout.strip().splitlines()[-2:] == ["%d requests" % (len(reqs) + len(finals) + len(infos)), "ok"]
    got, fin, info = parse(stdout)
    for name, r in reqs.items():
        assert got[name]["code"] == r["code"], (name, got[name])
        if r["code"] == OK:
            assert got[name]["message"] == "", (name, got[name])
            check_plan(got[name], r)
        else:
            assert got[name]["message"] == r["message"], (name, got[name])  # the whole message
    # known answers beside the restated rules.  The numbering: column 1 is the last key, column 2 the first payload column
    assert [c[1:4] for c in got["numbering"]["col"]] == [[1, 1, 1], [2, 0, 0], [0, 1, 0], [4, 0, 2], [1, 1, 1]]
    assert [c[1:4] for c in got["numbering_pipeline"]["col"]] == [[3, 0, 3], [0, 0, 0]]
    # cells per load and rows per tile: 16, 8, 4, 2, 1 cells; 1024 loads
    assert [got["shape_w%d_n1" % w]["col"][0][4:6] for w in WIDTHS] == [[16, 16384], [8, 8192], [4, 4096], [2, 2048], [1, 1024]]
    # one row: no whole load but for a string cell, one workgroup all the same
    assert got["shape_w4_n1"]["col"][0][6:] == [0, 0, 1, 0, 1, 4096] and got["shape_w16_n1"]["col"][0][6:] == [0, 1, 0, 1, 1, 1024]
    assert got["shape_w4_n0"]["launch"] == [[0, 0, 0, 40, 0]]
    # a tile and one row more: the row is the tail; a tile and one load more: a second tile
    assert got["shape_w4_n4096"]["col"][0][6:11] == [0, 1024, 0, 1, 1] and got["shape_w4_n4097"]["col"][0][6:11] == [0, 1024, 1, 1, 1]
    assert got["shape_w4_n4100"]["col"][0][6:11] == [0, 1025, 0, 2, 2]
    # the grid cap: 2048 workgroups, the next tile is some workgroup's second
    assert got["shape_w8_n%d" % (CAP * 2048)]["col"][0][9:] == [2048, 2048, CAP * 2048]
    assert got["shape_w8_n%d" % (CAP * 2048 + 2048)]["col"][0][9:] == [2049, 2048, CAP * 2048]
    assert got["shape_w8_n%d" % (CAP * 2048)]["launch"] == [[2048, 0, 2048 * 40, 40, 2049 * 40]]
    # 4-byte cells that start 3 cells behind a 16-byte boundary: one row of head; 1-byte cells 7 behind: nine
    assert got["shape_w4_off3_n40"]["col"][0][6:9] == [1, 9, 3] and got["shape_w1_off7_n40"]["col"][0][6:9] == [9, 1, 15]
    assert got["shape_w1_off7_n5"]["col"][0][6:9] == [5, 0, 0] and got["shape_w16_off1_n5"]["col"][0][6:9] == [0, 5, 0]
    # through a selection: a tile is 1024 rows whatever the width, no head, no tail
    assert all(got["selected_w%d_n1025" % w]["col"][0][4:] == [1, 1024, 0, 1025, 0, 2, 2, 2048] for w in WIDTHS)
    # five columns share 2048 workgroups: 409 each; the narrowest column has the fewest tiles
    assert got["five_columns"]["launch"][0][0] == 409 and got["sixteen_columns"]["launch"][0][0] == 128
    assert [c[9] for c in got["five_columns"]["col"]] == [7325, 14649, 3663, 1832, 29297]
    for name, a in finals.items():
        assert fin[name] == list(a[9:]), (name, fin[name])
    for (n, w), v in info.items():
        s = want_shape(n, w, 0, False, CAP)
        assert v == [s[0], LOADS, s[1], s[6], s[7], (s[6] + 1) * 8 * WORDS if s[6] else 0]


def test_the_rule_of_the_perfect_table_stands_once():
    """whether a perfect table is tried is polr_build_auto_tries_perfect (polr_build_plan.h); the statistics plan calls it and
    restates neither the density factor nor the small-range bound"""
    csrc = os.path.join(common.ROOT, "duckdb-polr_amd", "csrc")
    plan = open(os.path.join(csrc, "polr_colstats_plan.h")).read()
    build = open(os.path.join(csrc, "polr_build_plan.h")).read()
    assert build.count("static inline bool polr_build_auto_tries_perfect(") == 1
    assert plan.count("polr_build_auto_tries_perfect(") == 1
    assert "POLR_DENSE_FACTOR" not in plan and "POLR_BUILD_SMALL_RANGE" not in plan
