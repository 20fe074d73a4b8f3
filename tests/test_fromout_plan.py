"""The host-side plan of polr_ht_from_output (duckdb-polr_amd/csrc/polr_fromout_plan.h), the part that needs no GPU: the
header alone behind a stand-alone host program (tests/fromout/fromout_plan_main.cpp).  Every refusal of the contract
returns its code and a message, the two limits are tried at the limit and one beyond (4 and 5 keys, 62 and 63 payload
columns), duplicate references are kept apart, and a plan with all nine slots in use is checked line by line: the columns
ordered by slot, the VARCHAR columns with their guards, the places of the columns in the table's one allocation.  Built plain
and with the address +
undefined-behaviour sanitizers, and run directly."""
import os
import subprocess

import pytest

import common

SRC = os.path.join(common.ROOT, "tests", "fromout", "fromout_plan_main.cpp")
OK, INVALID, UNSUPPORTED = 0, -2, -3
MAX_ROWS = 0xFFFFFFF0


def col(slot, width, signed=0, has_valid=0, owned=1, rebased=0, resolved=1):
    return (resolved, slot, width, signed, has_valid, owned, rebased)


K4 = col(0, 4, 1)
ALL = (1, 1, 1, 1, 0)  # has_out, has_result, has_keys, has_payload, fused


def nine_slots():
    """keys from slots 8 and 0, payload from every slot in a scrambled order, slot 3 three times (once the key's column
    again), two VARCHAR columns (one needing the guard), every width"""
    keys = [col(8, 8, 1), col(0, 2)]
    payload = [col(5, 4), col(3, 1, 1), col(7, 16, owned=1, rebased=0), col(1, 8), col(3, 2), col(0, 2), col(6, 4, 1),
               col(2, 16, owned=1, rebased=1), col(4, 8, 1), col(3, 1, 1), col(8, 8, 1), col(2, 16, owned=0), col(7, 1), col(2, 4)]
    return keys, payload


def cases():
    """name -> (flags, (n_rows, n_chunks), keys, payload, counts or None, expected code)"""
    c = {}
    c["one_key"] = (ALL, (1000, 16), [K4], [], None, OK)
    c["no_payload_array_no_payload"] = ((1, 1, 1, 0, 0), (1000, 16), [K4], [], None, OK)
    c["null_out"] = ((0, 1, 1, 1, 0), (0, 0), [K4], [], None, INVALID)
    c["null_result"] = ((1, 0, 1, 1, 0), (0, 0), [K4], [], None, INVALID)
    c["null_keys"] = ((1, 1, 0, 1, 0), (0, 0), [], [], (1, 0), INVALID)
    c["null_payload_with_count"] = ((1, 1, 1, 0, 0), (0, 0), [K4], [], (1, 2), INVALID)
    c["fused"] = ((1, 1, 1, 1, 1), (0, 0), [K4], [], None, INVALID)
    c["key_reference_refused"] = (ALL, (10, 1), [col(0, 0, resolved=0)], [], None, INVALID)
    c["payload_reference_refused"] = (ALL, (10, 1), [K4], [col(1, 4), col(0, 0, resolved=0)], None, INVALID)
    c["keys_0"] = (ALL, (10, 1), [], [col(0, 4)], None, UNSUPPORTED)
    c["keys_4"] = (ALL, (10, 1), [K4] * 4, [], None, OK)
    c["keys_5"] = (ALL, (10, 1), [K4] * 5, [], None, UNSUPPORTED)
    c["key_16_bytes"] = (ALL, (10, 1), [col(0, 16)], [], None, UNSUPPORTED)
    c["second_key_16_bytes"] = (ALL, (10, 1), [K4, col(1, 16)], [], None, UNSUPPORTED)
    c["key_3_bytes"] = (ALL, (10, 1), [col(0, 3)], [], None, UNSUPPORTED)
    c["payload_3_bytes"] = (ALL, (10, 1), [K4], [col(0, 3)], None, UNSUPPORTED)
    c["payload_62"] = (ALL, (10, 1), [K4], [col(i % 9, 4) for i in range(62)], None, OK)
    c["payload_63"] = (ALL, (10, 1), [K4], [col(i % 9, 4) for i in range(63)], None, UNSUPPORTED)
    c["rows_at_the_bound"] = (ALL, (MAX_ROWS, 1 << 20), [K4], [], None, UNSUPPORTED)
    c["rows_below_the_bound"] = (ALL, (MAX_ROWS - 1, 1 << 20), [K4], [col(1, 16)], None, OK)
    c["no_rows"] = (ALL, (0, 0), [K4], [col(1, 16), col(1, 8)], None, OK)
    c["duplicates"] = (ALL, (100, 2), [col(2, 4, 1), col(2, 4, 1)], [col(2, 4, 1), col(1, 16), col(2, 4, 1), col(1, 16)], None, OK)
    c["nine_slots"] = (ALL, (12345, 200)) + nine_slots() + (None, OK)
    return c


def write_requests(path, reqs):
    with open(path, "w") as f:
        for name, (flags, rows, keys, payload, counts, _) in reqs.items():
            f.write("request %s\nflags %d %d %d %d %d\nrows %d %d\n" % ((name,) + tuple(flags) + tuple(rows)))
            for k in keys:
                f.write("key %d %d %d %d %d %d %d\n" % k)
            for p in payload:
                f.write("payload %d %d %d %d %d %d %d\n" % p)
            if counts:
                f.write("counts %d %d\n" % counts)
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


def check_plan(got, rows, keys, payload):
    """the plan of an accepted request against the request itself"""
    n, nc = rows
    cols = keys + payload
    fixed, strings = got.get("fixed", []), got.get("string", [])
    want_fixed = [i for i, c in enumerate(cols) if c[2] != 16]
    want_str = [i for i, c in enumerate(cols) if c[2] == 16]
    # every fixed-width column once, by slot, the request's order inside a slot; slot and width are the column's
    assert sorted(f[0] for f in fixed) == want_fixed
    assert [f[0] for f in fixed] == sorted(want_fixed, key=lambda i: (cols[i][1], i))
    assert all((f[1], f[2]) == (cols[f[0]][1], cols[f[0]][2]) for f in fixed)
    # the slot groups: consecutive runs of fixed[] that cover it, one per distinct slot
    n_slots, *first = got["slots"][0]
    assert n_slots == len({cols[i][1] for i in want_fixed}) and len(first) == n_slots + 1
    assert first[0] == 0 and first[-1] == len(fixed) and first == sorted(set(first)) if fixed else first == [0]
    for g in range(n_slots):
        assert len({f[1] for f in fixed[first[g]:first[g + 1]]}) == 1
    # the VARCHAR columns in the request's order; the guard: uploaded by the library and never rebased
    assert [s[0] for s in strings] == want_str and all(s[0] >= len(keys) for s in strings)
    assert [s[1:] for s in strings] == [[cols[i][1], int(cols[i][5] and not cols[i][6])] for i in want_str]
    # one allocation: cells, then validity, column after column, every array at a multiple of 256 bytes, none overlapping
    at, want_place = 0, []
    for c in cols:
        want_place.append([at, at + up(n * c[2])])
        at += up(n * c[2]) + up(n)
    table, desc_off, desc_size = got["bytes"][0]
    assert got["place"] == want_place and desc_off == at and desc_size == 40  # (four pointers and two words)
    assert table == alloc(at + len(want_fixed) * desc_size)  # the descriptors of the fixed-width columns behind the columns
    assert got["scratch"] == [[len(want_str) * n, len(want_str) * 2 * nc, len(want_str) * 2]]


@pytest.mark.parametrize("sanitize", [None, "address,undefined"], ids=["plain", "asan-ubsan"])
def test_refusals_limits_and_the_plan(tmp_path, sanitize):
    exe, path = str(tmp_path / "fromout_plan"), str(tmp_path / "requests.txt")
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
    for name, (_, rows, keys, payload, _, code) in reqs.items():
        assert got[name]["code"] == code, (name, got[name])
        assert (got[name]["message"] != "") == (code != OK), (name, got[name])
        if code == OK:
            check_plan(got[name], rows, keys, payload)
    # the messages say what was wrong
    assert "fused GROUP BY sink" in got["fused"]["message"]
    assert "5 equality keys" in got["keys_5"]["message"] and "0 equality keys" in got["keys_0"]["message"]
    assert "63 payload columns" in got["payload_63"]["message"]
    assert "VARCHAR join keys" in got["key_16_bytes"]["message"] and got["second_key_16_bytes"]["message"].startswith("key 1:")
    assert "%d rows" % MAX_ROWS in got["rows_at_the_bound"]["message"]
    assert got["payload_reference_refused"]["message"].startswith("payload column 1:")
    # all nine slots in use: nine row ids per output row, 2 + 11 fixed-width columns in slot order, three VARCHAR columns
    nine = got["nine_slots"]
    assert nine["slots"] == [[9, 0, 2, 3, 4, 7, 8, 9, 10, 11, 13]] and len(nine["fixed"]) == 13 and len(nine["string"]) == 3
    assert [f[1] for f in nine["fixed"]] == [0, 0, 1, 2, 3, 3, 3, 4, 5, 6, 7, 8, 8]
    assert [f[0] for f in nine["fixed"]] == [1, 7, 5, 15, 3, 6, 11, 10, 2, 8, 14, 0, 12]
    assert nine["string"] == [[4, 7, 1], [9, 2, 0], [13, 2, 0]]
    # duplicates are columns of their own: four copies of (2, 4-byte), two of the VARCHAR column
    dup = got["duplicates"]
    assert [f[0] for f in dup["fixed"]] == [0, 1, 2, 4] and dup["slots"] == [[1, 0, 4]] and [s[0] for s in dup["string"]] == [3, 5]
    # an empty output: nothing but the two descriptors, no scratch rows
    assert got["no_rows"]["bytes"] == [[2 * 40, 0, 40]] and got["no_rows"]["scratch"] == [[0, 0, 2]]
