"""The host-side plan of polr_pipeline_scan_filter_expr (duckdb-polr_amd/csrc/polr_filter_plan.h), the part that needs no
GPU: the header alone behind a stand-alone host program (tests/filterplan/filter_plan_main.cpp).  Every refusal of the
contract returns its code, the four limits are tried at the limit and one beyond, and a well-formed program of 64 nodes that
reaches stack depth 32 is accepted and its lowered form checked.  Built plain and with the address + undefined-behaviour
sanitizers, and run directly."""
import os
import subprocess

import pytest

import common

SRC = os.path.join(common.ROOT, "tests", "filterplan", "filter_plan_main.cpp")
OK, INVALID, UNSUPPORTED = 0, -2, -3
CMP, IN, LIKE, NOT, AND, OR = range(6)
EQ, NE, LT, GT, LE, GE, IS_NULL, IS_NOT_NULL = range(8)
I, S, U = 0, 1, 2  # the columns below: signed 4-byte, VARCHAR, unsigned 4-byte; 3..10: signed 8-byte
COLS = [(4, 1), (16, 0), (4, 0)] + [(8, 1)] * 8


def s(b):
    return (0, len(b), b)


def k(c):
    return (c, 0, None)


LEAF = (CMP, I, EQ, 0, 1)


def deep(n_leaves):
    """n_leaves comparisons pushed, then AND-ed down to one"""
    return [LEAF] * n_leaves + [(AND, 0, 0, 0, 0)] * (n_leaves - 1)


def big_program():
    """64 nodes, depth 32: 32 leaves over three columns -- comparisons, IN lists, LIKE patterns, IS NULL -- folded by
    alternating AND / OR, one NOT on top"""
    nodes, values = [], []
    patterns = [b"%(USA)%", b"abc%", b"%x_z", b"a%b%c", b"plain", b"%", b"", b"%%a%%"]
    for i in range(32):
        col = (I, S, U)[i % 3]
        if i % 8 == 7:
            nodes.append((CMP, col, IS_NULL if i % 16 == 7 else IS_NOT_NULL, 0, 0))
        elif col == S and i % 2 == 0:
            nodes.append((LIKE, S, 0, len(values), 1))
            values.append(s(patterns[(i // 2) % len(patterns)]))
        elif i % 5 == 0:
            nodes.append((IN, col, 0, len(values), 3))
            values += [s(b"m%d" % j) if col == S else k(i + j) for j in range(3)]
        else:
            nodes.append((CMP, col, i % 6, len(values), 1))
            values.append(s(b"a constant of more than twelve bytes") if col == S else k(i))
    nodes += [((AND, OR)[i % 2], 0, 0, 0, 0) for i in range(31)] + [(NOT, 0, 0, 0, 0)]
    return nodes, values


def cases():
    """name -> (nodes, values, counts or None, expected code)"""
    c = {}
    c["empty"] = ([], [], None, OK)
    c["one_leaf"] = ([LEAF], [k(5)], None, OK)
    c["not_on_empty_stack"] = ([(NOT, 0, 0, 0, 0)], [], None, INVALID)
    c["and_with_one_operand"] = ([LEAF, (AND, 0, 0, 0, 0)], [k(5)], None, INVALID)
    c["or_with_one_operand"] = ([LEAF, (OR, 0, 0, 0, 0)], [k(5)], None, INVALID)
    c["two_values_left"] = ([LEAF, LEAF], [k(5)], None, INVALID)
    c["unknown_kind"] = ([(6, I, EQ, 0, 1)], [k(5)], None, INVALID)
    c["unknown_op"] = ([(CMP, I, 8, 0, 1)], [k(5)], None, INVALID)
    c["value_range_begins_outside"] = ([(CMP, I, EQ, 1, 1)], [k(5)], None, INVALID)
    c["value_range_ends_outside"] = ([(IN, I, 0, 0, 2)], [k(5)], None, INVALID)
    c["value_range_wraps"] = ([(IN, I, 0, 1, 0xFFFFFFFF)], [k(5), k(6)], None, INVALID)
    c["col_out_of_range"] = ([(CMP, len(COLS), EQ, 0, 1)], [k(5)], None, INVALID)
    c["bytes_against_integer"] = ([(CMP, I, EQ, 0, 1)], [s(b"x")], None, INVALID)
    c["bytes_member_against_integer"] = ([(IN, I, 0, 0, 2)], [k(1), s(b"x")], None, INVALID)
    c["length_without_bytes"] = ([(CMP, S, EQ, 0, 1)], [(0, 5, None)], None, INVALID)
    c["like_on_integer"] = ([(LIKE, I, 0, 0, 1)], [k(5)], None, INVALID)
    c["like_two_patterns"] = ([(LIKE, S, 0, 0, 2)], [s(b"a"), s(b"b")], None, INVALID)
    c["in_without_members"] = ([(IN, S, 0, 0, 0)], [s(b"a")], None, INVALID)
    c["cmp_two_values"] = ([(CMP, I, EQ, 0, 2)], [k(1), k(2)], None, INVALID)
    c["cmp_no_value"] = ([(CMP, I, EQ, 0, 0)], [k(1)], None, INVALID)
    c["is_null_with_a_value"] = ([(CMP, I, IS_NULL, 0, 1)], [k(1)], None, INVALID)
    c["negative_against_unsigned"] = ([(CMP, U, LT, 0, 1)], [k(-1)], None, INVALID)
    c["negative_member_against_unsigned"] = ([(IN, U, 0, 0, 2)], [k(1), k(-1)], None, INVALID)
    c["negative_against_signed"] = ([(CMP, I, LT, 0, 1)], [k(-1)], None, OK)
    c["nodes_without_array"] = ([], [], (1, 0), INVALID)
    c["empty_string_is_not_null"] = ([(CMP, S, EQ, 0, 1)], [(0, 0, None)], None, OK)
    c["is_null_on_varchar"] = ([(CMP, S, IS_NULL, 0, 0)], [], None, OK)
    # the limits, at the limit and one beyond
    c["nodes_64"] = (deep(32) + [(NOT, 0, 0, 0, 0)], [k(5)], None, OK)
    c["nodes_65"] = (deep(32) + [(NOT, 0, 0, 0, 0)] * 2, [k(5)], None, UNSUPPORTED)
    c["depth_32"] = (deep(32), [k(5)], None, OK)
    c["depth_33"] = (deep(33), [k(5)], None, UNSUPPORTED)
    c["values_64"] = ([(IN, I, 0, 0, 64)], [k(i) for i in range(64)], None, OK)
    c["values_65"] = ([(IN, I, 0, 0, 64)], [k(i) for i in range(65)], None, UNSUPPORTED)
    c["string_4096"] = ([(CMP, S, EQ, 0, 1)], [s(b"y" * 4096)], None, OK)
    c["string_4097"] = ([(CMP, S, EQ, 0, 1)], [s(b"y" * 4097)], None, UNSUPPORTED)
    c["bytes_16384"] = ([(IN, S, 0, 0, 4)], [s(b"y" * 4096)] * 4, None, OK)
    c["bytes_16385"] = ([(IN, S, 0, 0, 5)], [s(b"y" * 4096)] * 4 + [s(b"z")], None, UNSUPPORTED)
    eight = [(CMP, 3 + i, EQ, 0, 1) for i in range(8)]
    c["columns_8"] = (eight + [(AND, 0, 0, 0, 0)] * 7, [k(5)], None, OK)
    c["columns_9"] = (eight + [LEAF] + [(AND, 0, 0, 0, 0)] * 8, [k(5)], None, UNSUPPORTED)
    c["nul_in_pattern"] = ([(LIKE, S, 0, 0, 1)], [s(b"a\0%")], None, UNSUPPORTED)
    c["nul_in_constant"] = ([(CMP, S, EQ, 0, 1)], [s(b"a\0b")], None, OK)
    c["big"] = big_program() + (None, OK)
    return c


def write_programs(path, progs):
    with open(path, "w") as f:
        for w, sg in COLS:
            f.write("col %d %d\n" % (w, sg))
        for name, (nodes, values, counts, _) in progs.items():
            f.write("program %s\n" % name)
            for n in nodes:
                f.write("node %d %d %d %d %d\n" % n)
            for const, length, b in values:
                f.write("value %d %d %s\n" % (const, length, "-" if b is None else "x" + b.hex()))
            if counts:
                f.write("counts %d %d\n" % counts)
            f.write("end\n")


def parse(stdout):
    out, cur = {}, None
    for line in stdout.splitlines():
        if line.startswith("  "):
            key, *rest = line.split()
            cur.setdefault(key, []).append(rest)
        elif line not in ("ok",) and not line.endswith(" programs"):
            name, code, *msg = line.split(" ", 2)
            cur = out[name] = {"code": int(code), "message": " ".join(msg)}
    return out


def segments(pattern):
    """what polr_like.h expects of a pattern: [(offset, length)], flags (1 front, 2 back), the lengths together"""
    pieces, at = [], 0
    for piece in pattern.split(b"%"):
        pieces.append((at, len(piece)))
        at += len(piece) + 1
    segs, flags = [], 0
    for i, (off, n) in enumerate(pieces):
        first, last = i == 0, i == len(pieces) - 1
        if n or (first and last):
            segs.append((off, n))
            flags |= (1 if first else 0) | (2 if last else 0)
    return segs, flags, sum(n for _, n in segs)


@pytest.mark.parametrize("sanitize", [None, "address,undefined"], ids=["plain", "asan-ubsan"])
def test_refusals_limits_and_the_lowered_form(tmp_path, sanitize):
    exe, path = str(tmp_path / "filter_plan"), str(tmp_path / "programs.txt")
    progs = cases()
    write_programs(path, progs)
    flags = ["-fsanitize=" + sanitize, "-fno-sanitize-recover=all"] if sanitize else []
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall"] + flags + [SRC, "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert run.stdout.strip().splitlines()[-2:] == ["%d programs" % len(progs), "ok"]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-4000:]
    got = parse(run.stdout)
    for name, (_, _, _, code) in progs.items():
        assert got[name]["code"] == code, (name, got[name])
        assert (got[name]["message"] != "") == (code != OK), (name, got[name])
    # the lowered form of the 64-node, depth-32 program
    nodes, values = big_program()
    assert len(nodes) == 64
    depth = top = 0
    for n in nodes:
        depth += 1 if n[0] <= LIKE else 0 if n[0] == NOT else -1
        top = max(top, depth)
    assert (depth, top) == (1, 32)
    low = got["big"]
    words = [int(w, 16) for w in low["nodes"][0]]
    cols = [[int(x) for x in c] for c in low["col"]]
    leaves = [tuple(int(x) for x in lf) for lf in low["leaf"]]
    assert len(words) == 64 and len(leaves) == 32 and sorted(c[0] for c in cols) == [I, S, U]
    # the columns' leaves: consecutive runs that cover all leaves; needs_cell unless every leaf is a NULL test
    assert [c[1] for c in cols] == [sum(c[2] for c in cols[:g]) for g in range(len(cols))] and sum(c[2] for c in cols) == 32
    seen = []
    for n, w in zip(nodes, words):
        assert w & 0xFF == n[0]
        if n[0] > LIKE:
            assert w == n[0]
            continue
        leaf, slot, never_null = (w >> 8) & 0xFF, (w >> 16) & 0xFF, (w >> 24) & 1
        assert cols[slot][0] == n[1] and cols[slot][1] <= leaf < cols[slot][1] + cols[slot][2]
        assert leaves[leaf] == (n[0], n[2] if n[0] == CMP else EQ, n[3], n[4])
        assert never_null == (n[0] == CMP and n[2] >= IS_NULL)
        seen.append((slot, leaf))
    assert len(set(leaf for _, leaf in seen)) == 32
    for slot in range(len(cols)):  # program order inside a column
        mine = [leaf for sl, leaf in seen if sl == slot]
        assert mine == sorted(mine)
        assert cols[slot][3] == 1
    # the values index for index, their bytes one after the other, every pattern cut at its '%'
    lowered, segs = low["value"], [tuple(int(x) for x in sg) for sg in low.get("seg", [])]
    assert len(lowered) == len(values)
    at = 0
    patterns = {n[3] for n in nodes if n[0] == LIKE}
    for v, ((const, length, b), lv) in enumerate(zip(values, lowered)):
        assert (int(lv[0]), int(lv[1]), int(lv[2])) == (const, length, at), v
        first_seg, n_segs, flags, min_len = (int(x) for x in lv[4:8])
        if v in patterns:
            want, want_flags, want_min = segments(b)
            assert segs[first_seg:first_seg + n_segs] == [(at + off, n) for off, n in want], b
            assert (flags, min_len) == (want_flags, want_min), b
        else:
            assert (n_segs, flags, min_len) == (0, 0, 0)
        at += length
    assert int(low["bytes"][0][0]) == at
