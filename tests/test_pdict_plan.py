"""The host-side rules of the dictionary of a VARCHAR probe column (duckdb-polr_amd/csrc/polr_pdict_plan.h), the part that
needs no GPU: the header alone behind a stand-alone host program (tests/pdictplan/pdict_plan_main.cpp).  Known answers for
every refusal of an encode request alone and, for each adjacent pair in their order, for a request that violates both; the
rules over the device's answer and their order; what POLR_DICT_SELECTED means with and without a selection in force; the
scratch layout of both modes at 0, 1, 1023, 1024 and 1025 rows with 0, 1 and n rows selected, and which arrays follow the
table's rows and which the selected count; the build side's layout, unchanged; the fetch rules.  Built plain and with the
address + undefined-behaviour sanitizers, and run directly."""
import os
import subprocess

import pytest

import common

SRC = os.path.join(common.ROOT, "tests", "pdictplan", "pdict_plan_main.cpp")
OK, INVALID, UNSUPPORTED, HIP = 0, -2, -3, -4
BLOCK_ROWS = 256 * 4  # POLR_DICT_BLOCK * POLR_DICT_ITEMS
SORTED, NULL_INVALID, SELECTED = 1, 2, 4

GOOD = dict(flags=0, probe_col=1, n_probe_cols=3, width=16, encoded=0, encoded_as=0, is_code_col=0, n_rows=1000, has_selection=0,
            n_selected=1000)
# the encode refusals in their order: (name, the fields that violate the rule, the code, the message)
ENCODE_RULES = [
    ("flags", dict(flags=8), INVALID, "dictionary flags 0x8: only POLR_DICT_SORTED, POLR_DICT_NULL_INVALID and POLR_DICT_SELECTED are "
                                      "defined"),
    ("no_column", dict(probe_col=3), INVALID, "probe column 3 of 3"),
    ("width", dict(width=4), INVALID, "a dictionary is made of a column of 16-byte string cells (this one: 4 bytes)"),
    ("encoded", dict(encoded=1, encoded_as=2), INVALID, "probe column 1 is encoded already (code column 2)"),
    ("code_col", dict(is_code_col=1), INVALID, "probe column 1 is a code column: codes are not encoded again"),
    ("slots", dict(n_rows=2**30 + 1), UNSUPPORTED, "a dictionary over 1073741825 probe rows exceeds the 32-bit slot space"),
]


def encode_line(**changed):
    f = dict(GOOD, **changed)
    return "encode %d %d %d %d %d %d %d %d %d %d" % (f["flags"], f["probe_col"], f["n_probe_cols"], f["width"], f["encoded"],
                                                     f["encoded_as"], f["is_code_col"], f["n_rows"], f["has_selection"], f["n_selected"])


def r16(x):
    return (x + 15) & ~15


def capacity_of(n):
    """the build side's capacity rule: a power of two >= 2 n, at least 1024"""
    c = 1024
    while c < 2 * n:
        c *= 2
    return c


def scratch_layout(capacity, n_rows, n_insert):
    """rep, hash, state, first_row, code, slot_of_row, row_of_code, block_sums, scalars, n_long, total, n_blocks.  The
    table's arrays: 16, 8, 4, 4, 4 bytes a slot; PER TABLE ROW: slot_of_row (a word) and block_sums (a word per 1024 rows);
    PER INSERTED POSITION: row_of_code (a word); 64 bytes of scalars"""
    n_blocks = max(1, -(-n_rows // BLOCK_ROWS))
    sizes = [16 * capacity, 8 * capacity, 4 * capacity, 4 * capacity, 4 * capacity, r16(4 * n_rows), r16(4 * n_insert),
             r16(4 * n_blocks), 64]
    offs = [sum(sizes[:i]) for i in range(len(sizes))]
    return offs + [offs[-1] + 32, sum(sizes), n_blocks]


def requests():
    """name -> (request line, check of the answer's words)"""
    r = {}

    def code(want, *parts):
        return lambda a: int(a[0]) == want and all(p in " ".join(a[1:]) for p in parts) and (want != OK or len(a) == 1)

    def encode(want, *parts, capacity=0, sorted_=0, null_invalid=0, selected=0, own_valid=0, n_insert=0):
        def check(a):
            if want == OK:
                return [int(x) for x in a] == [OK, capacity, sorted_, null_invalid, selected, own_valid, n_insert]
            return int(a[0]) == want and int(a[1]) == 0 and " ".join(a[7:]) == parts[0]
        return check

    # the encode request: the flags, and what SELECTED means
    r["encode_good"] = (encode_line(), encode(OK, capacity=2048, n_insert=1000))
    r["encode_sorted"] = (encode_line(flags=SORTED), encode(OK, capacity=2048, sorted_=1, n_insert=1000))
    r["encode_null_invalid"] = (encode_line(flags=NULL_INVALID), encode(OK, capacity=2048, null_invalid=1, n_insert=1000))
    r["encode_no_rows"] = (encode_line(n_rows=0, n_selected=0), encode(OK, capacity=1024))
    r["encode_2^30_rows"] = (encode_line(n_rows=2**30), encode(OK, capacity=2**31, n_insert=2**30))
    # (without the flag a selection in force plays no part; with the flag and no selection: all rows)
    r["encode_selection_ignored"] = (encode_line(has_selection=1, n_selected=10), encode(OK, capacity=2048, n_insert=1000))
    r["encode_selected_no_selection"] = (encode_line(flags=SELECTED | NULL_INVALID, n_selected=10),
                                         encode(OK, capacity=2048, null_invalid=1, n_insert=1000))
    r["encode_selected"] = (encode_line(flags=SELECTED, has_selection=1, n_selected=10), encode(OK, capacity=1024, selected=1, n_insert=10))
    r["encode_selected_all_flags"] = (encode_line(flags=7, has_selection=1, n_selected=600),
                                      encode(OK, capacity=2048, sorted_=1, null_invalid=1, selected=1, own_valid=1, n_insert=600))
    r["encode_selected_none"] = (encode_line(flags=SELECTED, has_selection=1, n_selected=0), encode(OK, capacity=1024, selected=1))
    # (the slot space follows the selected count: a table too large to encode whole is encoded through a selection)
    r["encode_selected_of_huge"] = (encode_line(flags=SELECTED, n_rows=2**31, has_selection=1, n_selected=2**20),
                                    encode(OK, capacity=2**21, selected=1, n_insert=2**20))
    r["encode_selected_slots"] = (encode_line(flags=SELECTED, n_rows=10, has_selection=1, n_selected=2**30 + 1),
                                  encode(UNSUPPORTED, "a dictionary over 1073741825 selected rows exceeds the 32-bit slot space"))
    for name, fields, want, text in ENCODE_RULES:
        r["encode_" + name] = (encode_line(**fields), encode(want, text))
    for (n1, f1, want, text), (n2, f2, _, _text2) in zip(ENCODE_RULES, ENCODE_RULES[1:]):
        r["encode_%s_before_%s" % (n1, n2)] = (encode_line(**dict(f2, **f1)), encode(want, text))

    # what the device's answer means: the build side's rules and order, the heap guard in the pipeline's words
    r["outcome_ok"] = ("outcome 0 0 0 2", code(OK))
    r["outcome_hip"] = ("outcome 1 0 0 2", lambda a: int(a[0]) == HIP and " ".join(a[1:]) == "dictionary encoding failed: out of memory")
    r["outcome_heap_never_came"] = ("outcome 0 3 0 2", lambda a: int(a[0]) == INVALID and " ".join(a[1:]) == (
        "probe column 2: 3 rows hold strings longer than 12 bytes, but the column's heap was never put on the device "
        "(polr_pipeline_set_probe_heaps)"))
    r["outcome_full"] = ("outcome 0 0 1 2", lambda a: int(a[0]) == HIP and " ".join(a[1:]) == "dictionary encoding failed: the string table filled up")
    r["outcome_hip_first"] = ("outcome 1 3 1 2", code(HIP, "out of memory"))
    r["outcome_heap_before_full"] = ("outcome 0 3 1 2", code(INVALID, "3 rows"))

    # the scratch layout of both modes
    def layout(n_rows, n_insert):
        capacity = capacity_of(n_insert)
        want = scratch_layout(capacity, n_rows, n_insert)
        return ("layout %d %d %d" % (capacity, n_rows, n_insert), lambda a: [int(x) for x in a] == want)

    for n in (0, 1, 1023, 1024, 1025):
        r["layout_all_%d" % n] = layout(n, n)
        # (every row inserted: the build side's layout, field for field)
        r["layout_all_%d_is_build" % n] = ("layout %d %d %d" % (capacity_of(n), n, n), None)
        r["layout_build_%d" % n] = ("build_layout %d %d" % (capacity_of(n), n), "same as previous")
        for s in sorted({0, 1, n}):
            r["layout_%d_selected_%d" % (n, s)] = layout(n, s)
    r["layout_literal"] = ("layout 1024 1025 1", lambda a: [int(x) for x in a] == [0, 16384, 24576, 28672, 32768, 36864, 40976, 40992,
                                                                                   41008, 41040, 41072, 2])
    # (1/16 of 2^24 rows selected: the table follows the selection, 4 bytes a table row remain)
    sel = scratch_layout(capacity_of(2**20), 2**24, 2**20)
    r["layout_16th"] = ("layout %d %d %d" % (capacity_of(2**20), 2**24, 2**20),
                        lambda a: [int(x) for x in a] == sel and int(a[10]) == 36 * 2**21 + 4 * 2**24 + 4 * 2**20 + 4 * 2**14 + 64)
    # a selection that lists rows twice is longer than the table: row_of_code follows the positions
    r["layout_duplicates"] = layout(10, 25)
    # the build side's layout is what it was (the known answers of tests/test_dict_plan.py)
    r["build_layout_0"] = ("build_layout 1024 0", lambda a: [int(x) for x in a] == [0, 16384, 24576, 28672, 32768, 36864, 36864, 36864,
                                                                                    36880, 36912, 36944, 1])
    r["build_layout_1"] = ("build_layout 1024 1", lambda a: [int(x) for x in a][5:] == [36864, 36880, 36896, 36912, 36944, 36976, 1])
    r["build_layout_edge"] = ("build_layout %d %d" % (2**31, 2**30), lambda a: int(a[10]) == 36 * 2**31 + 2 * 2**32 + 2**22 + 64)

    # the fetch requests: the build side's rules, the first in the pipeline's words
    not_held = "probe column 7 is not a code column whose dictionary this pipeline holds"
    r["fetch_whole"] = ("fetch 1 7 5 0 0", code(OK))
    r["fetch_whole_not_held"] = ("fetch 0 7 0 0 0", lambda a: int(a[0]) == INVALID and " ".join(a[1:]) == not_held)
    r["fetch_list"] = ("fetch 1 7 5 1 5 4 0 4 2 4", code(OK))
    r["fetch_list_empty"] = ("fetch 1 7 5 1 0", code(OK))
    r["fetch_list_not_held"] = ("fetch 0 7 0 1 2 0 0", code(INVALID, not_held))
    r["fetch_list_bad_code"] = ("fetch 1 7 5 1 4 0 5 9 2", code(INVALID, "code 5 at position 1 of the list: the dictionary has 5 strings "
                                                                          "(the NULL code is none)"))
    r["fetch_list_2^30+1"] = ("fetch 1 7 0 1 %d 0" % (2**30 + 1), code(UNSUPPORTED, "a list of 1073741825 codes: at most 2^30 strings are "
                                                                                    "fetched by one call"))
    r["fetch_list_not_held_before_count"] = ("fetch 0 7 0 1 %d 0" % (2**30 + 1), code(INVALID, not_held))
    return r


@pytest.mark.parametrize("sanitize", [None, "address,undefined"], ids=["plain", "asan-ubsan"])
def test_known_answers(tmp_path, sanitize):
    exe, path = str(tmp_path / "pdict_plan"), str(tmp_path / "requests.txt")
    reqs = requests()
    with open(path, "w") as f:
        for line, _ in reqs.values():
            f.write(line + "\n")
    flags = ["-fsanitize=" + sanitize, "-fno-sanitize-recover=all"] if sanitize else []
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall"] + flags + [SRC, "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    assert "warning" not in build.stderr, build.stderr[-4000:]
    run = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert lines[-2:] == ["%d requests" % len(reqs), "ok"] and len(lines) == len(reqs) + 2
    previous = None
    for (name, (line, check)), answer in zip(reqs.items(), lines):
        if check == "same as previous":
            assert answer == previous, (name, line, answer, previous)
        elif check is not None:
            assert check(answer.split()), (name, line, answer)
        previous = answer
