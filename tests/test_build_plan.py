"""The host-side rules of a build side (duckdb-polr_amd/csrc/polr_build_plan.h), the part that needs no GPU: the header
alone behind a stand-alone host program (tests/buildplan/build_plan_main.cpp).  Known answers for the limits and upload
shapes, the range of a perfect table (the signed difference that used to overflow among them), the choice of
polr_ht_finalize_auto, the hash capacity and kind, the packed form of composite keys, the buffers of a finalized table as
the sending and the receiving side of a broadcast list them, and the check of a received metadata blob.  Built plain and
with the address + undefined-behaviour sanitizers, and run directly."""
import os
import subprocess

import pytest

import common

SRC = os.path.join(common.ROOT, "tests", "buildplan", "build_plan_main.cpp")
OK, INVALID, UNSUPPORTED = 0, -2, -3
PERFECT, S8, S16 = 1, 2, 3
TABLE, ROWIDS, DATA, VALID = 0, 1, 2, 3
MAX_ROWS = 0xFFFFFFF0
I64_MIN, I64_MAX = -2**63, 2**63 - 1
MAGIC = 0x504F4C52


def s64(u):
    """an unsigned key's bit pattern as the signed 64-bit value the ABI carries"""
    return u - 2**64 if u >= 2**63 else u


def good_meta(kind):
    """kind, n_keys, n_payload, capacity, range, n_rows_in, magic, key_width0, payload_width0"""
    return {PERFECT: [PERFECT, 1, 2, 3001, 3000, 2000, MAGIC, 4, 16],
            S8: [S8, 1, 1, 1024, 0, 100, MAGIC, 4, 2],
            S16: [S16, 3, 62, 2**31, 0, MAX_ROWS - 1, MAGIC, 8, 1]}[kind]


def mutated(kind, field, value):
    m = good_meta(kind)
    m[field] = value
    return m


def requests():
    """name -> (request line, check of the answer's words)"""
    r = {}

    def code(want, *parts):
        return lambda a: int(a[0]) == want and all(p in " ".join(a[1:]) for p in parts) and (want != OK or len(a) == 1)

    # limits and upload shapes
    r["rows_below"] = ("rows %d" % (MAX_ROWS - 1), code(OK))
    r["rows_at"] = ("rows %d" % MAX_ROWS, code(UNSUPPORTED, "%d rows" % MAX_ROWS, "32-bit row-id space"))
    for w in (1, 2, 4, 8, 16):
        r["colwidth_%d" % w] = ("colwidth %d" % w, code(OK))
    for w in (0, 3, 12, 32):
        r["colwidth_%d" % w] = ("colwidth %d" % w, code(UNSUPPORTED, "column width %d not supported (1,2,4,8,16)" % w))
    r["keys_0"] = ("keys 0", code(UNSUPPORTED, "0 equality keys per join not supported (1..4)"))
    r["keys_4"] = ("keys 4 1 2 4 8", code(OK))
    r["keys_5"] = ("keys 5 4 4 4 4 4", code(UNSUPPORTED, "5 equality keys"))
    r["key_16"] = ("keys 2 4 16", code(UNSUPPORTED, "VARCHAR join keys are outside this path"))
    r["key_3"] = ("keys 1 3", code(UNSUPPORTED, "join key of 3 bytes"))
    r["layout_fits"] = ("layout 16 2 1 4 8 8", code(OK))  # the second column ends exactly at the row width
    r["layout_one_beyond"] = ("layout 16 2 1 4 9 8", code(INVALID, "column 1 (offset 9, width 8) does not fit row width 16"))
    r["layout_width_3"] = ("layout 16 2 1 4 5 3", code(INVALID, "column 1 (offset 5, width 3)"))
    r["layout_validity_fits"] = ("layout 1 7" + " 0 1" * 7, code(OK))  # 7 columns + the row: 8 bits, one byte
    r["layout_validity_beyond"] = ("layout 1 8" + " 0 1" * 8, code(INVALID, "validity bytes exceed row width"))

    # the perfect range
    def perfect(want, rng=None, size=None, words=None):
        if want != OK:
            return lambda a: int(a[0]) == want and "perfect hash range" in " ".join(a[4:])
        return lambda a: [int(x) for x in a] == [OK, rng, size, words]

    r["perfect_2^31-1"] = ("perfect 0 %d 1" % (2**31 - 1), perfect(OK, 2**31 - 1, 2**31, 2**26))
    r["perfect_2^31"] = ("perfect 0 %d 1" % 2**31, perfect(INVALID))
    r["perfect_signed_full"] = ("perfect %d %d 1" % (I64_MIN, I64_MAX), perfect(INVALID))  # (overflowed as int64_t)
    r["perfect_signed_unordered"] = ("perfect %d %d 1" % (I64_MAX, I64_MIN), perfect(INVALID))  # (wraps to a range of 1)
    r["perfect_signed_negative"] = ("perfect -1000 1999 1", perfect(OK, 2999, 3000, 94))
    r["perfect_unsigned_top_bit"] = ("perfect %d %d 0" % (s64(2**63 - 10), s64(2**63 + 21)), perfect(OK, 31, 32, 1))
    r["perfect_unsigned_top_bit_unordered"] = ("perfect %d %d 0" % (s64(2**63 + 21), s64(2**63 - 10)), perfect(INVALID))
    r["perfect_same_bits_signed"] = ("perfect %d %d 1" % (s64(2**63 - 10), s64(2**63 + 21)), perfect(INVALID))
    r["perfect_size_1"] = ("perfect 7 7 1", perfect(OK, 0, 1, 1))
    r["perfect_size_32"] = ("perfect 7 38 1", perfect(OK, 31, 32, 1))
    r["perfect_size_33"] = ("perfect 7 39 1", perfect(OK, 32, 33, 2))
    shape = lambda a: int(a[0]) == INVALID and " ".join(a[4:]) == "perfect table shape invalid"
    r["pht_ok"] = ("pht 8 -5 58 1", perfect(OK, 63, 64, 2))
    r["pht_2^31"] = ("pht 4 0 %d 1" % 2**31, shape)
    r["pht_signed_unordered"] = ("pht 8 %d %d 1" % (I64_MAX, I64_MIN), shape)
    r["pht_width_3"] = ("pht 3 0 63 1", shape)
    r["pht_width_16"] = ("pht 16 0 63 1", shape)

    # polr_ht_finalize_auto
    yes, no = (lambda a: a == ["1"]), (lambda a: a == ["0"])
    n = 1000
    r["auto_dense_limit"] = ("auto %d 0 %d 1 1 0" % (n, 8 * n + 7), yes)
    r["auto_small_range_sparse"] = ("auto %d 0 %d 1 1 0" % (n, 8 * n + 8), yes)  # (not dense, but within 1 M values)
    r["auto_sparse"] = ("auto 1000 0 %d 1 1 0" % 1000001, no)  # range/8 = 125000 > 1000 rows, range > 1 M
    r["auto_dense_beyond_1M"] = ("auto 125001 0 %d 1 1 0" % (8 * 125001 + 7), yes)
    r["auto_sparse_beyond_1M"] = ("auto 125001 0 %d 1 1 0" % (8 * 125001 + 8), no)
    r["auto_1M_one_row"] = ("auto 1 0 1000000 1 1 0", yes)
    r["auto_1M+1_one_row"] = ("auto 1 0 1000001 1 1 0", no)
    r["auto_no_rows"] = ("auto 0 0 10 1 1 0", no)
    r["auto_two_keys"] = ("auto 1000 0 10 1 2 0 0", no)
    r["auto_by_value"] = ("auto 1000 0 10 1 1 1", no)
    r["auto_null_equal"] = ("auto 1000 0 10 1 1 2", no)
    r["auto_unordered"] = ("auto 1000 10 0 1 1 0", no)
    r["auto_unsigned_top_bit"] = ("auto 1000 %d %d 0 1 0" % (s64(2**63 - 10), s64(2**63 + 21)), yes)
    r["auto_2^31"] = ("auto %d 0 %d 1 1 0" % (2**31, 2**31), no)

    # the hash capacity
    def capacity(want, cap):
        return lambda a: [int(a[0]), int(a[1])] == [want, cap] and (want == OK) == (len(a) == 2)

    r["capacity_0"] = ("capacity 0", capacity(OK, 1024))
    r["capacity_512"] = ("capacity 512", capacity(OK, 1024))
    r["capacity_513"] = ("capacity 513", capacity(OK, 2048))
    r["capacity_2^30"] = ("capacity %d" % 2**30, capacity(OK, 2**31))
    r["capacity_2^30+1"] = ("capacity %d" % (2**30 + 1), capacity(UNSUPPORTED, 2**32))
    r["capacity_rows_bound"] = ("capacity %d" % (MAX_ROWS - 1), capacity(UNSUPPORTED, 2**33))
    r["capacity_2^64-1"] = ("capacity %d" % (2**64 - 1), capacity(UNSUPPORTED, 2**63))  # (no endless loop, no overflow)

    # needs_key_pack
    r["pack_one_key"] = ("needs_pack 1 8 0", no)
    r["pack_two_narrow"] = ("needs_pack 2 4 0 2 0", no)
    r["pack_second_8"] = ("needs_pack 2 4 0 8 0", yes)
    r["pack_first_8"] = ("needs_pack 2 8 0 4 0", yes)
    r["pack_one_by_value"] = ("needs_pack 1 4 1", yes)
    r["pack_second_null_equal"] = ("needs_pack 2 4 0 4 2", yes)
    r["pack_three"] = ("needs_pack 3 1 0 1 0 1 0", yes)

    # the kind
    def kind(want, k=0, run=None):
        return lambda a: int(a[0]) == want and (int(a[1]), int(a[2])) == (k, run) and ("2^25" in " ".join(a[3:])) == (want != OK)

    r["kind_unique32"] = ("kind 1 0 1 4 0", kind(OK, S8, 1))
    r["kind_empty"] = ("kind 0 0 1 4 0", kind(OK, S8, 0))
    r["kind_run_2"] = ("kind 2 0 1 4 0", kind(OK, S16, 2))
    r["kind_sentinels_2"] = ("kind 1 2 1 4 0", kind(OK, S16, 2))
    r["kind_8_bytes"] = ("kind 1 0 1 8 0", kind(OK, S16, 1))
    r["kind_2_bytes"] = ("kind 1 0 1 2 0", kind(OK, S16, 1))
    r["kind_two_keys"] = ("kind 1 0 2 4 0", kind(OK, S16, 1))
    r["kind_packed"] = ("kind 1 0 1 4 1", kind(OK, S16, 1))
    r["kind_run_2^25-1"] = ("kind %d 0 1 4 0" % (2**25 - 1), kind(OK, S16, 2**25 - 1))
    r["kind_run_2^25"] = ("kind %d 0 1 4 0" % 2**25, kind(UNSUPPORTED, 0, 2**25))
    r["kind_sentinels_2^25"] = ("kind 3 %d 1 4 0" % 2**25, kind(UNSUPPORTED, 0, 2**25))

    # the key-pack layout: -> packed, null_eq, then per column shift, sx, min, range
    def pack(null_eq, *cols):
        want = [OK, 1, null_eq] + [x for c in cols for x in c]
        return lambda a: [int(x) for x in a] == want

    too_wide = lambda a: int(a[0]) == UNSUPPORTED and "64 bits" in " ".join(a[1:])
    r["layout3"] = ("pack 3 0  5 5 1  -100 155 1  0 65536 0", pack(0, (0, 1, 5, 0), (0, 1, -100, 255), (8, 0, 0, 65536)))
    r["layout3_bits"] = ("pack 4 0  5 5 1  -100 155 1  0 65536 0  0 1 0",
                         pack(0, (0, 1, 5, 0), (0, 1, -100, 255), (8, 0, 0, 65536), (25, 0, 0, 1)))  # 0 + 8 + 17 = 25 bits
    r["null_eq_255"] = ("pack 2 1  0 255 0  0 1 0", pack(1, (0, 0, 0, 255), (9, 0, 0, 1)))  # 256 codes: 9 bits
    r["empty_column"] = ("pack 2 0  %d %d 1  3 4 0" % (I64_MAX, I64_MIN), pack(0, (0, 1, 0, 0), (0, 0, 3, 1)))
    r["null_eq_empty"] = ("pack 2 1  %d %d 1  3 4 0" % (I64_MAX, I64_MIN), pack(1, (0, 1, 0, 0), (1, 0, 3, 1)))
    r["bits_64"] = ("pack 2 0  0 %d 0  %d %d 1" % (2**32 - 1, -2**31, 2**31 - 1),
                    pack(0, (0, 0, 0, 2**32 - 1), (32, 1, -2**31, 2**32 - 1)))
    r["bits_65"] = ("pack 2 0  0 %d 0  %d %d 1" % (2**32, -2**31, 2**31 - 1), too_wide)
    r["full_range_alone"] = ("pack 1 0  %d %d 1" % (I64_MIN, I64_MAX), pack(0, (0, 1, I64_MIN, 2**64 - 1)))
    r["full_range_null_eq"] = ("pack 1 1  %d %d 1" % (I64_MIN, I64_MAX), too_wide)
    r["null_eq_63_bits_plus_code"] = ("pack 1 1  0 %d 1" % I64_MAX, pack(1, (0, 1, 0, 2**63 - 1)))  # 2^63 codes: 64 bits

    # the buffers: the list export reports, then the list alloc_like allocates
    def buffers(*want):
        flat = [len(want)] + [x for b in want for x in b]
        return lambda a: [int(x) for x in a] == flat

    r["buffers_perfect"] = ("buffers 1 3000 2000 2  4 1  16 1",
                            buffers((TABLE, 0, 94 * 4), (DATA, 0, 12000), (VALID, 0, 3000), (DATA, 1, 48000), (VALID, 1, 3000)))
    r["buffers_s8"] = ("buffers 2 2048 1000 2  2 0  8 1", buffers((TABLE, 0, 2048 * 8), (DATA, 0, 2000), (DATA, 1, 8000), (VALID, 1, 1000)))
    r["buffers_s16_valid"] = ("buffers 3 1024 300 2  1 1  16 1", buffers((TABLE, 0, 1024 * 16), (ROWIDS, 0, 1200), (DATA, 0, 300), (VALID, 0, 300),
                                                                        (DATA, 1, 4800), (VALID, 1, 300)))
    r["buffers_s16_no_valid"] = ("buffers 3 1024 300 2  1 0  16 0", buffers((TABLE, 0, 1024 * 16), (ROWIDS, 0, 1200), (DATA, 0, 300), (DATA, 1, 4800)))
    r["buffers_no_rows"] = ("buffers 3 1024 0 2  4 1  8 0", buffers((TABLE, 0, 1024 * 16), (ROWIDS, 0, 16), (DATA, 0, 16), (VALID, 0, 16), (DATA, 1, 16)))
    r["buffers_one_row"] = ("buffers 3 1024 1 3  1 1  16 1  2 0", buffers((TABLE, 0, 1024 * 16), (ROWIDS, 0, 4), (DATA, 0, 1), (VALID, 0, 1),
                                                                       (DATA, 1, 16), (VALID, 1, 1), (DATA, 2, 2)))
    r["buffers_s8_no_payload"] = ("buffers 2 1024 1 0", buffers((TABLE, 0, 1024 * 8)))
    r["buffers_perfect_one_slot"] = ("buffers 1 1 1 1  8 1", buffers((TABLE, 0, 4), (DATA, 0, 8), (VALID, 0, 1)))

    # the metadata check: a good blob of each kind, then one mutation per rule
    K, NK, NP, CAP, RNG, ROWS, MAG, KW, PW = range(9)

    def meta(fields, want, *parts):
        return ("meta " + " ".join(str(x) for x in fields), code(want, *parts))

    for k, name in ((PERFECT, "perfect"), (S8, "s8"), (S16, "s16")):
        r["meta_good_" + name] = meta(good_meta(k), OK)
    r["meta_magic"] = meta(mutated(S8, MAG, MAGIC + 1), INVALID, "bad table metadata")
    r["meta_kind_0"] = meta(mutated(S8, K, 0), INVALID, "bad table kind")
    r["meta_kind_7"] = meta(mutated(S8, K, 7), INVALID, "bad table kind")
    r["meta_keys_0"] = meta(mutated(S8, NK, 0), INVALID, "bad table metadata")
    r["meta_keys_5"] = meta(mutated(S8, NK, 5), INVALID, "bad table metadata")
    r["meta_payload_63"] = meta(mutated(S8, NP, 63), INVALID, "bad table metadata")
    r["meta_key_width_3"] = meta(mutated(S8, KW, 3), INVALID, "key 0 of 3 bytes")
    r["meta_key_width_16"] = meta(mutated(S16, KW, 16), INVALID, "key 0 of 16 bytes")
    r["meta_payload_width_3"] = meta(mutated(S8, PW, 3), INVALID, "payload column 0 of 3 bytes")
    r["meta_payload_width_32"] = meta(mutated(S16, PW, 32), INVALID, "payload column 0 of 32 bytes")
    r["meta_capacity_1000"] = meta(mutated(S8, CAP, 1000), INVALID, "hash table of 1000 slots")
    r["meta_capacity_512"] = meta(mutated(S8, CAP, 512), INVALID, "hash table of 512 slots")
    r["meta_capacity_2^32"] = meta(mutated(S16, CAP, 2**32), INVALID, "hash table of")
    r["meta_capacity_0"] = meta(mutated(S16, CAP, 0), INVALID, "hash table of 0 slots")
    r["meta_perfect_capacity"] = meta(mutated(PERFECT, CAP, 3000), INVALID, "perfect table of 3000 slots over a range of 3000")
    good = good_meta(PERFECT)
    r["meta_perfect_range_2^31-1"] = meta(good[:CAP] + [2**31, 2**31 - 1] + good[ROWS:], OK)
    r["meta_perfect_range_2^31"] = meta(good[:CAP] + [2**31 + 1, 2**31] + good[ROWS:], INVALID, "perfect table of")
    r["meta_perfect_range_wraps"] = meta(good[:CAP] + [0, 2**64 - 1] + good[ROWS:], INVALID, "perfect table of")  # (range + 1 = 0)
    r["meta_rows_at_bound"] = meta(mutated(S16, ROWS, MAX_ROWS), INVALID, "%d build rows" % MAX_ROWS)
    return r


@pytest.mark.parametrize("sanitize", [None, "address,undefined"], ids=["plain", "asan-ubsan"])
def test_known_answers(tmp_path, sanitize):
    exe, path = str(tmp_path / "build_plan"), str(tmp_path / "requests.txt")
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
    n_lines = sum(2 if line.startswith("buffers") else 1 for line, _ in reqs.values())
    assert lines[-2:] == ["%d requests" % len(reqs), "ok"] and len(lines) == n_lines + 2
    at = 0
    for name, (line, check) in reqs.items():
        answer = lines[at].split()
        at += 1
        if line.startswith("buffers"):
            # the list the receiving side allocates is the list the sending side reported, element for element
            assert lines[at].split() == answer, (name, answer, lines[at])
            at += 1
        assert check(answer), (name, line, " ".join(answer))
