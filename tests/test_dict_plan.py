"""The host-side rules of the dictionary of a VARCHAR build column and of the string records by which strings leave the
device (duckdb-polr_amd/csrc/polr_dict_plan.h, polr_strrec_plan.h), the part that needs no GPU: the headers alone behind a
stand-alone host program (tests/dictplan/dict_plan_main.cpp).  Known answers for every refusal of an encode request alone
and, for each adjacent pair in their order, for a request that violates both; the rules over the device's answer and their
order; the scratch layout and the sort's; what a code column adds to the table's device bytes; the refusals of the two fetch
calls; the layout of the records and the capacity rule.  Built plain and with the address + undefined-behaviour sanitizers,
and run directly."""
import os
import subprocess

import pytest

import common

SRC = os.path.join(common.ROOT, "tests", "dictplan", "dict_plan_main.cpp")
OK, INVALID, UNSUPPORTED, HIP = 0, -2, -3, -4
BLOCK_ROWS = 256 * 4  # POLR_DICT_BLOCK * POLR_DICT_ITEMS
TILE = 1024           # POLR_DICT_SORT_TILE

# the encode refusals in their order: (the fields that violate the rule, the code, words of the message)
GOOD = dict(flags=0, finalized=0, payload_col=1, n_payload=3, width=16, encoded=0, encoded_as=0, n_rows=1000)
ENCODE_RULES = [
    ("flags", dict(flags=4), INVALID, "dictionary flags 0x4: only POLR_DICT_SORTED and POLR_DICT_NULL_INVALID are defined"),
    ("finalized", dict(finalized=1), INVALID, "a payload column is dictionary-encoded before the table is finalized"),
    ("no_column", dict(payload_col=3), INVALID, "payload column 3 of 3"),
    ("width", dict(width=8), INVALID, "a dictionary is made of a column of 16-byte string cells (this one: 8 bytes)"),
    ("encoded", dict(encoded=1, encoded_as=2), INVALID, "is encoded already (code column 2)"),
    ("max_payload", dict(n_payload=62), UNSUPPORTED, "the table has 62 payload columns already: a code column would be the 63rd, "
                                                     "more than polr_ht_export carries"),
    ("slots", dict(n_rows=2**30 + 1), UNSUPPORTED, "a dictionary over 1073741825 build rows exceeds the 32-bit slot space"),
]


def encode_line(**changed):
    f = dict(GOOD, **changed)
    return "encode %d %d %d %d %d %d %d %d" % (f["flags"], f["finalized"], f["payload_col"], f["n_payload"], f["width"], f["encoded"],
                                               f["encoded_as"], f["n_rows"])


def r16(x):
    return (x + 15) & ~15


def scratch_layout(capacity, n):
    """rep, hash, state, first_row, code, slot_of_row, row_of_code, block_sums, scalars, n_long, total, n_blocks: the table's
    arrays (16, 8, 4, 4, 4 bytes a slot), two 4-byte words a row, a word per 1024 rows, 64 bytes of scalars"""
    n_blocks = max(1, -(-n // BLOCK_ROWS))
    sizes = [16 * capacity, 8 * capacity, 4 * capacity, 4 * capacity, 4 * capacity, r16(4 * n), r16(4 * n), r16(4 * n_blocks), 64]
    offs = [sum(sizes[:i]) for i in range(len(sizes))]
    return offs + [offs[-1] + 32, sum(sizes), n_blocks], sizes


def requests():
    """name -> (request line, check of the answer's words)"""
    r = {}

    def code(want, *parts):
        return lambda a: int(a[0]) == want and all(p in " ".join(a[1:]) for p in parts) and (want != OK or len(a) == 1)

    def encode(want, *parts, capacity=0, sorted_=0, null_invalid=0):
        def check(a):
            text = " ".join(a[4:])
            if want == OK:
                return [int(x) for x in a] == [OK, capacity, sorted_, null_invalid]
            return int(a[0]) == want and int(a[1]) == 0 and all(p in text for p in parts)
        return check

    # the encode request
    r["encode_good"] = (encode_line(), encode(OK, capacity=2048))
    r["encode_sorted"] = (encode_line(flags=1), encode(OK, capacity=2048, sorted_=1))
    r["encode_null_invalid"] = (encode_line(flags=2), encode(OK, capacity=2048, null_invalid=1))
    r["encode_both_flags"] = (encode_line(flags=3), encode(OK, capacity=2048, sorted_=1, null_invalid=1))
    r["encode_no_rows"] = (encode_line(n_rows=0), encode(OK, capacity=1024))
    r["encode_61_columns"] = (encode_line(n_payload=61), encode(OK, capacity=2048))
    r["encode_2^30_rows"] = (encode_line(n_rows=2**30), encode(OK, capacity=2**31))
    for name, fields, want, text in ENCODE_RULES:
        r["encode_" + name] = (encode_line(**fields), encode(want, text))
    for (n1, f1, want, text), (n2, f2, _, text2) in zip(ENCODE_RULES, ENCODE_RULES[1:]):
        # (a column out of range has no width of its own: the request says 8)
        both = dict(f1, **f2)
        r["encode_%s_before_%s" % (n1, n2)] = (encode_line(**both), lambda a, want=want, text=text, text2=text2: (
            int(a[0]) == want and text in " ".join(a[4:]) and text2 not in " ".join(a[4:])))

    # what the device's answer means
    r["outcome_ok"] = ("outcome 0 0 0 2", code(OK))
    r["outcome_hip"] = ("outcome 1 0 0 2", lambda a: int(a[0]) == HIP and " ".join(a[1:]) == "dictionary encoding failed: out of memory")
    r["outcome_heap_never_came"] = ("outcome 0 3 0 2", code(INVALID, "payload column 2: 3 build rows hold strings longer than 12 bytes, "
                                                                       "but the column's heap was never put on the device "
                                                                       "(polr_ht_set_payload_heaps)"))
    r["outcome_full"] = ("outcome 0 0 1 2", lambda a: int(a[0]) == HIP and " ".join(a[1:]) == "dictionary encoding failed: the string table filled up")
    r["outcome_hip_first"] = ("outcome 1 3 1 2", code(HIP, "out of memory"))
    r["outcome_heap_before_full"] = ("outcome 0 3 1 2", code(INVALID, "3 build rows"))

    # the scratch layout
    def layout(capacity, n):
        want, sizes = scratch_layout(capacity, n)

        def check(a):
            got = [int(x) for x in a]
            offs = got[:9]
            return (got == want and offs[0] == 0 and all(o % 16 == 0 for o in offs)
                    and all(offs[i] + sizes[i] == offs[i + 1] for i in range(8)) and got[10] == offs[8] + 64 == sum(sizes))
        return ("layout %d %d" % (capacity, n), check)

    r["layout_0"] = layout(1024, 0)
    r["layout_0_literal"] = ("layout 1024 0", lambda a: [int(x) for x in a] == [0, 16384, 24576, 28672, 32768, 36864, 36864, 36864, 36880,
                                                                               36912, 36944, 1])
    r["layout_1"] = layout(1024, 1)
    r["layout_1_literal"] = ("layout 1024 1", lambda a: [int(x) for x in a][5:] == [36864, 36880, 36896, 36912, 36944, 36976, 1])
    r["layout_block"] = layout(2048, BLOCK_ROWS)
    r["layout_block_blocks"] = ("layout 2048 %d" % BLOCK_ROWS, lambda a: int(a[-1]) == 1)
    r["layout_block+1"] = layout(4096, BLOCK_ROWS + 1)
    r["layout_block+1_blocks"] = ("layout 4096 %d" % (BLOCK_ROWS + 1), lambda a: int(a[-1]) == 2)
    r["layout_5_blocks"] = layout(16384, 4 * BLOCK_ROWS + 3)  # (5 block sums: 20 bytes, rounded to 32)
    r["layout_32bit_edge"] = layout(2**31, 2**30)
    r["layout_32bit_edge_total"] = ("layout %d %d" % (2**31, 2**30), lambda a: int(a[10]) == 36 * 2**31 + 2 * 2**32 + 2**22 + 64)

    # the sort's scratch: ping, pong, rep_old, rank, total, tiles, merge passes
    def sort(nc, tiles, passes):
        want = [0, 16 * nc, 32 * nc, 48 * nc, 52 * nc, tiles, passes]
        return ("sort %d" % nc, lambda a: [int(x) for x in a] == want)

    r["sort_2"] = sort(2, 1, 0)
    r["sort_tile"] = sort(TILE, 1, 0)
    r["sort_tile+1"] = sort(TILE + 1, 2, 1)
    r["sort_2_tiles"] = sort(2 * TILE, 2, 1)
    r["sort_2_tiles+1"] = sort(2 * TILE + 1, 3, 2)
    r["sort_4_tiles"] = sort(4 * TILE, 4, 2)
    r["sort_2^31"] = sort(2**31, 2**21, 21)

    # device bytes: the code column as export reports it, the validity copy, 16 bytes a code
    one = lambda want: (lambda a: [int(x) for x in a] == [want])
    r["bytes_no_rows"] = ("bytes 0 0 0", one(16))
    r["bytes_no_rows_valid"] = ("bytes 0 1 0", one(32))
    r["bytes_1000"] = ("bytes 1000 0 5", one(4000 + 80))
    r["bytes_1000_valid"] = ("bytes 1000 1 5", one(4000 + 1000 + 80))

    # the fetch requests
    not_held = "payload column 7 is not a code column whose dictionary this table holds"
    r["fetch_whole"] = ("fetch 1 7 5 0 0", code(OK))
    r["fetch_whole_not_held"] = ("fetch 0 7 0 0 0", code(INVALID, not_held))
    r["fetch_list"] = ("fetch 1 7 5 1 5 4 0 4 2 4", code(OK))
    r["fetch_list_empty"] = ("fetch 1 7 5 1 0", code(OK))
    r["fetch_list_not_held"] = ("fetch 0 7 0 1 2 0 0", code(INVALID, not_held))
    r["fetch_list_bad_code"] = ("fetch 1 7 5 1 4 0 5 9 2", code(INVALID, "code 5 at position 1 of the list: the dictionary has 5 strings "
                                                                          "(the NULL code is none)"))
    r["fetch_list_null_code_last"] = ("fetch 1 7 5 1 3 0 4 5", code(INVALID, "code 5 at position 2"))
    # (2^30 codes pass the count rule and reach the first code; one more does not get that far)
    r["fetch_list_2^30"] = ("fetch 1 7 0 1 %d 0" % 2**30, code(INVALID, "code 0 at position 0 of the list: the dictionary has 0 strings"))
    r["fetch_list_2^30+1"] = ("fetch 1 7 0 1 %d 0" % (2**30 + 1), code(UNSUPPORTED, "a list of 1073741825 codes: at most 2^30 strings are "
                                                                                    "fetched by one call"))
    r["fetch_list_not_held_before_count"] = ("fetch 0 7 0 1 %d 0" % (2**30 + 1), code(INVALID, not_held))

    # the records: used, fits, offsets
    def records(line, used, fits, *offs):
        want = [str(used), str(fits)] + [str(o) for o in offs]
        return ("records " + line, lambda a: a == want)

    big = 2**32 - 1
    r["records_mixed"] = records("8 %d 8  0 - 1 12 - 13 %d 0" % (2**33, big), 2**32 + 49, 1, 0, "-", 4, 9, "-", 25, 42, 2**32 + 45)
    r["records_none"] = records("0 0 0", 0, 1)
    r["records_all_skipped"] = records("2 0 2  - -", 0, 1, "-", "-")
    r["records_one_empty_string"] = records("1 4 1  0", 4, 1, 0)
    r["records_used_is_cap"] = records("3 38 3  1 12 13", 38, 1, 0, 5, 21)
    r["records_used_is_cap+1"] = records("3 37 3  1 12 13", 38, 0, 0, 5, 21)
    r["records_offsets_n-1"] = records("2 38 3  1 12 13", 38, 0, 0, 5, 21)
    r["records_offsets_more"] = records("9 38 3  1 12 13", 38, 1, 0, 5, 21)
    r["records_group_major"] = records("6 100 6  3 - 5  - - 0", 20, 1, 0, "-", 7, "-", "-", 16)  # (two groups x VARCHAR, int, VARCHAR)
    return r


@pytest.mark.parametrize("sanitize", [None, "address,undefined"], ids=["plain", "asan-ubsan"])
def test_known_answers(tmp_path, sanitize):
    exe, path = str(tmp_path / "dict_plan"), str(tmp_path / "requests.txt")
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
    for (name, (line, check)), answer in zip(reqs.items(), lines):
        assert check(answer.split()), (name, line, answer)
