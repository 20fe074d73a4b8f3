"""The host-side plan of polr_pipeline_from_output (duckdb-polr_amd/csrc/polr_pipesrc_plan.h), the part that needs no GPU:
the header alone behind a stand-alone host program (tests/pipesrc/pipesrc_plan_main.cpp).  Every refusal of the contract
returns its code and a message; requests that break several rules at once show the ORDER the header states; each limit is
tried at the limit and one beyond (66 and 67 columns, 2^32 - 17 and 2^32 - 16 rows, 8 and 9 joins, 32 and 33 join orders);
duplicate references are kept apart; a plan with all nine slots in use is checked line by line: the probe columns of the
new pipeline, the columns ordered by slot, the VARCHAR columns with their guards, the places of the columns in the one
allocation; and an output of zero rows.  Built plain and with the address + undefined-behaviour sanitizers, and run
directly."""
import os
import subprocess

import pytest

import common

SRC = os.path.join(common.ROOT, "tests", "pipesrc", "pipesrc_plan_main.cpp")
OK, INVALID, UNSUPPORTED = 0, -2, -3
MAX_ROWS = 0xFFFFFFF0
MAX_COLS = 66
PERFECT, S8 = 1, 2


def col(slot, width, signed=0, has_valid=0, owned=1, rebased=0, resolved=1):
    return (resolved, slot, width, signed, has_valid, owned, rebased)


def join(kind=PERFECT, key_width=4, src_join=-1, src_col=0, payload_width=0):
    return (kind, key_width, src_join, src_col, payload_width)


K4 = col(0, 4, 1)
ALL = (1, 1, 1, 1, 1, 0)  # has_out, has_result, has_cols, has_joins, has_paths, fused
ONE = dict(joins=[join()], paths=[[0]])


def nine_slots():
    """columns from every slot in a scrambled order, slot 3 three times, three VARCHAR columns (one needing the guard),
    every width; column 0 is the 4-byte key the join reads"""
    return [K4, col(8, 8, 1), col(5, 4), col(3, 1, 1), col(7, 16, owned=1, rebased=0), col(1, 8), col(3, 2), col(0, 2),
            col(6, 4, 1), col(2, 16, owned=1, rebased=1), col(4, 8, 1), col(3, 1, 1), col(8, 8, 1), col(2, 16, owned=0),
            col(7, 1), col(2, 4)]


def req(cols, flags=ALL, rows=(1000, 16), joins=None, paths=None, code=OK, count=None, k=None, npaths=None):
    return dict(cols=cols, flags=flags, rows=rows, joins=ONE["joins"] if joins is None else joins,
                paths=ONE["paths"] if paths is None else paths, code=code, count=count, k=k, npaths=npaths)


def star(k):
    return [join(src_col=0) for _ in range(k)], [list(range(k))]


def cases():
    c = {}
    c["one_col"] = req([K4])
    # 1. NULL pointers, in their order -- each with later violations in the same request
    c["null_out"] = req([K4], flags=(0, 0, 0, 0, 0, 1), code=INVALID)
    c["null_result"] = req([K4], flags=(1, 0, 0, 1, 1, 1), code=INVALID)
    c["null_cols"] = req([], flags=(1, 1, 0, 0, 1, 0), count=3, code=INVALID)
    c["null_joins"] = req([K4], flags=(1, 1, 1, 0, 0, 0), code=INVALID)
    c["null_paths"] = req([], flags=(1, 1, 1, 1, 0, 1), code=INVALID)
    # 2. no columns -- before the fused sink (4) and nine joins (7)
    c["no_cols"] = req([], flags=(1, 1, 1, 1, 1, 1), joins=star(9)[0], paths=star(9)[1], code=INVALID)
    # 3. the column limit -- before the fused sink and an unresolved reference
    c["cols_66"] = req([K4] + [col(i % 9, 4) for i in range(MAX_COLS - 1)])
    c["cols_67"] = req([K4] + [col(i % 9, 4) for i in range(MAX_COLS)], code=UNSUPPORTED)
    c["cols_67_fused"] = req([col(0, 0, resolved=0)] * (MAX_COLS + 1), flags=(1, 1, 1, 1, 1, 1), code=UNSUPPORTED)
    # 4. fused -- before a reference out of range
    c["fused"] = req([col(0, 0, resolved=0)], flags=(1, 1, 1, 1, 1, 1), code=INVALID)
    # 5. references, the first bad one -- before the row bound and nine joins
    c["reference_refused"] = req([K4, col(1, 4), col(0, 0, resolved=0), col(0, 0, resolved=0)], rows=(MAX_ROWS, 1 << 20),
                                 joins=star(9)[0], paths=star(9)[1], code=INVALID)
    c["cell_3_bytes"] = req([K4, col(0, 3)], code=UNSUPPORTED)
    # 6. rows -- before the plan of the joins
    c["rows_at_the_bound"] = req([K4], rows=(MAX_ROWS, 1 << 20), joins=star(9)[0], paths=star(9)[1], code=UNSUPPORTED)
    c["rows_below_the_bound"] = req([K4, col(1, 16)], rows=(MAX_ROWS - 1, 1 << 20))
    # 7. polr_pipeline_create's refusals pass through
    j8, p8 = star(8)
    c["joins_8"] = req([K4], joins=j8, paths=p8)
    j9, p9 = star(9)
    c["joins_9"] = req([K4], joins=j9, paths=p9, code=UNSUPPORTED)
    c["joins_0"] = req([K4], joins=[], paths=[], k=0, npaths=1, code=UNSUPPORTED)
    c["paths_32"] = req([K4], joins=star(2)[0], paths=[[0, 1], [1, 0]] * 16)
    c["paths_33"] = req([K4], joins=star(2)[0], paths=[[0, 1], [1, 0]] * 16 + [[0, 1]], code=UNSUPPORTED)
    c["paths_0"] = req([K4], joins=star(2)[0], paths=[], code=UNSUPPORTED)
    c["not_finalized"] = req([K4], joins=[join(kind=0)], code=INVALID)
    c["not_a_permutation"] = req([K4], joins=star(2)[0], paths=[[0, 0]], code=INVALID)
    c["key_column_out_of_range"] = req([K4, col(1, 4)], joins=[join(src_col=2)], code=INVALID)
    c["key_width_differs"] = req([col(0, 8, 1)], joins=[join(key_width=4)], code=INVALID)
    c["varchar_key"] = req([col(0, 16)], joins=[join(key_width=16)], code=UNSUPPORTED)
    c["dependent_before_provider"] = req([K4], joins=[join(payload_width=4), join(src_join=0, src_col=0)], paths=[[1, 0]],
                                         code=INVALID)
    # a key that was a build column of an earlier join BEFORE the cut is a plain probe column after it: flat
    c["carried_key_is_flat"] = req([K4, col(3, 4, 1)], joins=[join(src_col=0), join(src_col=1)], paths=[[0, 1], [1, 0]])
    c["dependent_is_generic"] = req([K4], joins=[join(payload_width=4), join(src_join=0, src_col=0)], paths=[[0, 1]])
    c["no_rows"] = req([K4, col(1, 16), col(1, 8)], rows=(0, 0))
    c["duplicates"] = req([col(2, 4, 1), col(2, 4, 1), col(2, 4, 1), col(1, 16), col(2, 4, 1), col(1, 16)], rows=(100, 2))
    c["nine_slots"] = req(nine_slots(), rows=(12345, 200))
    return c


def write_requests(path, reqs):
    with open(path, "w") as f:
        for name, r in reqs.items():
            f.write("request %s\nflags %d %d %d %d %d %d\nrows %d %d\n" % ((name,) + tuple(r["flags"]) + tuple(r["rows"])))
            for x in r["cols"]:
                f.write("col %d %d %d %d %d %d %d\n" % x)
            if r["count"] is not None:
                f.write("count %d\n" % r["count"])
            for j in r["joins"]:
                f.write("join %d %d %d %d %d\n" % j)
            if r["k"] is not None:
                f.write("k %d\n" % r["k"])
            for p in r["paths"]:
                f.write("path %s\n" % " ".join(str(x) for x in p))
            if r["npaths"] is not None:
                f.write("npaths %d\n" % r["npaths"])
            f.write("end\n")


def parse(stdout):
    out, cur = {}, None
    for line in stdout.splitlines():
        if line.startswith("  "):
            key, *rest = line.split()
            cur.setdefault(key, []).append([int(x) for x in rest])
        elif line not in ("ok",) and not line.endswith(" requests"):
            name, code, *msg = line.split(" ", 2)
            cur = out[name] = {"code": int(code), "message": " ".join(msg)}
    return out


def alloc(n):
    return n if n else 16  # (DevBuf::alloc: an empty buffer is 16 bytes)


def up(n):
    return (n + 255) // 256 * 256


def check_plan(got, r):
    """the plan of an accepted request against the request itself"""
    n, nc = r["rows"]
    cols = r["cols"]
    # the probe side of the new pipeline: a column per reference with the width and signedness of its source, a row per output row
    assert got["probe"] == [[c[2], c[3]] for c in cols]
    assert got["pipe"][0][0] == n and got["pipe"][0][3] == 1 + len(r["joins"])
    fixed, strings = got.get("fixed", []), got.get("string", [])
    want_fixed = [i for i, c in enumerate(cols) if c[2] != 16]
    want_str = [i for i, c in enumerate(cols) if c[2] == 16]
    # every fixed-width column once, by slot, the request's order inside a slot; slot and width are the column's
    assert [f[0] for f in fixed] == sorted(want_fixed, key=lambda i: (cols[i][1], i))
    assert all((f[1], f[2]) == (cols[f[0]][1], cols[f[0]][2]) for f in fixed)
    # the slot groups: consecutive runs of fixed[] that cover it, one per distinct slot
    n_slots, *first = got["slots"][0]
    assert n_slots == len({cols[i][1] for i in want_fixed}) and len(first) == n_slots + 1
    assert first[0] == 0 and first[-1] == len(fixed) and first == sorted(set(first))
    for g in range(n_slots):
        assert len({f[1] for f in fixed[first[g]:first[g + 1]]}) == 1
    # the VARCHAR columns in the request's order; the guard: uploaded by the library and never rebased
    assert [s[0] for s in strings] == want_str
    assert [s[1:] for s in strings] == [[cols[i][1], int(cols[i][5] and not cols[i][6])] for i in want_str]
    # one allocation: cells, then validity, column after column, every array at a multiple of 256 bytes, none overlapping;
    # the descriptors of the fixed-width columns behind the columns
    at, want_place = 0, []
    for c in cols:
        want_place.append([at, at + up(n * c[2])])
        at += up(n * c[2]) + up(n)
    table, desc_off, desc_size = got["bytes"][0]
    assert got["place"] == want_place and desc_off == at and desc_size == 40  # (four pointers and two words)
    assert table == alloc(at + len(want_fixed) * desc_size)
    assert got["scratch"] == [[len(want_str) * n, len(want_str) * 2 * nc, len(want_str) * 2]]


@pytest.mark.parametrize("sanitize", [None, "address,undefined"], ids=["plain", "asan-ubsan"])
def test_refusals_in_order_limits_and_the_plan(tmp_path, sanitize):
    exe, path = str(tmp_path / "pipesrc_plan"), str(tmp_path / "requests.txt")
    reqs = cases()
    write_requests(path, reqs)
    flags = ["-fsanitize=" + sanitize, "-fno-sanitize-recover=all"] if sanitize else []
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall"] + flags + [SRC, "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert run.stdout.strip().splitlines()[-2:] == ["%d requests" % len(reqs), "ok"]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-4000:]
    got = parse(run.stdout)
    for name, r in reqs.items():
        assert got[name]["code"] == r["code"], (name, got[name])
        assert (got[name]["message"] != "") == (r["code"] != OK), (name, got[name])
        if r["code"] == OK:
            check_plan(got[name], r)
    # the messages say what was wrong -- and, where a request breaks several rules, which rule came first
    msg = {n: g["message"] for n, g in got.items()}
    assert msg["null_out"].endswith("the output is NULL") and msg["null_result"].endswith(": out is NULL")
    assert msg["null_cols"].endswith("cols is NULL") and msg["null_joins"].endswith("joins is NULL")
    assert msg["null_paths"].endswith("paths is NULL")
    assert "no columns" in msg["no_cols"]
    assert "67 columns" in msg["cols_67"] and "67 columns" in msg["cols_67_fused"]
    assert "fused GROUP BY sink" in msg["fused"]
    assert msg["reference_refused"].startswith("column 2:")
    assert "cells of 3 bytes" in msg["cell_3_bytes"]
    assert "%d rows" % MAX_ROWS in msg["rows_at_the_bound"]
    # ... and polr_pipeline_create's own words pass through
    assert "9 multiplexed joins not supported (1..8)" in msg["joins_9"] and "0 multiplexed joins" in msg["joins_0"]
    assert "33 join orders not supported" in msg["paths_33"] and "0 join orders" in msg["paths_0"]
    assert "not finalized" in msg["not_finalized"] and "not a permutation" in msg["not_a_permutation"]
    assert "probe column 2 out of range" in msg["key_column_out_of_range"]
    assert "probe key is 8 bytes, build key 4 bytes" in msg["key_width_differs"]
    assert "probe key of 16 bytes" in msg["varchar_key"]
    assert "probes join 1 before join 0" in msg["dependent_before_provider"]
    # the flat kernel: a carried key is a probe column; a key read through a build column of this pipeline is not
    assert got["carried_key_is_flat"]["pipe"][0][1:3] == [1, 1]
    assert got["dependent_is_generic"]["pipe"][0][1:3] == [0, 2]
    # all nine slots in use: nine row ids per output row, 13 fixed-width columns in slot order, three VARCHAR columns
    nine = got["nine_slots"]
    assert nine["slots"] == [[9, 0, 2, 3, 4, 7, 8, 9, 10, 11, 13]] and len(nine["fixed"]) == 13 and len(nine["string"]) == 3
    assert [f[1] for f in nine["fixed"]] == [0, 0, 1, 2, 3, 3, 3, 4, 5, 6, 7, 8, 8]
    assert [f[0] for f in nine["fixed"]] == [0, 7, 5, 15, 3, 6, 11, 10, 2, 8, 14, 1, 12]
    assert nine["string"] == [[4, 7, 1], [9, 2, 0], [13, 2, 0]]
    # duplicates are columns of their own: four copies of (2, 4-byte), two of the VARCHAR column
    dup = got["duplicates"]
    assert [f[0] for f in dup["fixed"]] == [0, 1, 2, 4] and dup["slots"] == [[1, 0, 4]] and [s[0] for s in dup["string"]] == [3, 5]
    # an empty output: nothing but the two descriptors, no scratch rows, a pipeline of zero probe rows
    assert got["no_rows"]["bytes"] == [[2 * 40, 0, 40]] and got["no_rows"]["scratch"] == [[0, 0, 2]]
    assert got["no_rows"]["pipe"][0][0] == 0
