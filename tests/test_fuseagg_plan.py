"""The host-side plan of polr_out_fuse_aggregate / polr_out_fused_aggregate_result (duckdb-polr_amd/csrc/polr_fuseagg_plan.h),
the part that needs no GPU: the header alone behind a stand-alone host program (tests/fuseagg/fuseagg_plan_main.cpp).  Every
refusal with its code and whole message, in the documented order (a request that earns several is refused for the first);
1, 8 and 9 aggregates; the cell layout and the reset words for 1 and 8 aggregates; and the decode of fabricated cell tables
-- sums that leave 64 bits, mixed signs, the bounds of the eight column types, no rows, and the 2^32 bound of the SUM
cells.  Built plain and with the address + undefined-behaviour sanitizers, and run directly."""
import os
import subprocess

import pytest

import common

SRC = os.path.join(common.ROOT, "tests", "fuseagg", "fuseagg_plan_main.cpp")
OK, INVALID, UNSUPPORTED, RANGE = 0, -2, -3, -7
COUNT_STAR, COUNT, SUM, MIN, MAX = range(5)
ADD, KMIN, KMAX = 0, 1, 2
TABLES = 256
M64 = (1 << 64) - 1
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1
SIGNED = 1  # POLR_COL_SIGNED
COL_RULE = "only integer columns of up to 8 bytes (signed if 8)"  # the wording of polr_out_aggregate


def agg(fn, src_join=-1, src_col=0, in_range=1, width=4, flags=SIGNED):
    return (fn, src_join, src_col, in_range, width, flags)


def plan(aggs=(agg(SUM),), has_out=1, has_specs=1, n_aggs=None, already=0, code=OK, message=""):
    return dict(aggs=list(aggs), head=(has_out, has_specs, len(aggs) if n_aggs is None else n_aggs, already), code=code,
                message=message)


def plan_cases():
    c = {}
    eight = [agg(COUNT_STAR), agg(COUNT, 0, 1, width=1), agg(SUM, 1, 0, width=8), agg(MIN, -1, 2, width=2, flags=0),
             agg(MAX, 2, 0, width=4, flags=0), agg(SUM, -1, 0, width=1, flags=0), agg(MIN, 0, 0, width=8), agg(MAX, 0, 0, width=8)]
    c["one"] = plan()
    c["eight"] = plan(eight)
    # the refusals of the contract, each alone ...
    c["null_out"] = plan(has_out=0, code=INVALID, message="polr_out_fuse_aggregate: the output is NULL")
    c["nine"] = plan([], n_aggs=9, code=UNSUPPORTED, message="at most 8 aggregates per call")  # (no aggregate is looked at)
    c["already"] = plan(already=1, code=INVALID, message="the output object already has a fused sink")
    c["unknown_fn"] = plan([agg(SUM), agg(5)], code=INVALID, message="aggregate 1: unknown function 5")
    c["probe_col_beyond"] = plan([agg(MIN, -1, 7, in_range=0)], code=INVALID, message="aggregate 0: probe column 7 out of range")
    c["build_col_beyond"] = plan([agg(COUNT_STAR), agg(MAX, 2, 9, in_range=0)], code=INVALID,
                                 message="aggregate 1: build column (2,9) out of range")
    c["varchar"] = plan([agg(MIN, 0, 0, width=16, flags=0)], code=UNSUPPORTED, message="aggregate 0: " + COL_RULE)
    c["unsigned_8"] = plan([agg(SUM), agg(SUM, 0, 0, width=8, flags=0)], code=UNSUPPORTED, message="aggregate 1: " + COL_RULE)
    c["signed_8"] = plan([agg(SUM, 0, 0, width=8)])
    c["count_star_ignores_its_column"] = plan([agg(COUNT_STAR, 5, 99, in_range=0, width=16, flags=0)])
    # ... un-fusing is never refused but for a NULL output
    c["unfuse_null_specs"] = plan(has_specs=0, already=1)
    c["unfuse_no_aggs"] = plan([], already=1)
    c["unfuse_nothing_attached"] = plan([], has_specs=0)
    # ... and in their order: the earlier one wins
    c["order_null_first"] = plan([], has_out=0, has_specs=0, n_aggs=9, already=1, code=INVALID, message=c["null_out"]["message"])
    c["order_unfuse_before_count"] = plan([], has_specs=0, n_aggs=9, already=1)
    c["order_count_before_already"] = plan([], n_aggs=9, already=1, code=UNSUPPORTED, message=c["nine"]["message"])
    c["order_already_before_aggregates"] = plan([agg(9)], already=1, code=INVALID, message=c["already"]["message"])
    c["order_first_aggregate_first"] = plan([agg(SUM), agg(MIN, 0, 0, width=16), agg(7)], code=UNSUPPORTED,
                                            message="aggregate 1: " + COL_RULE)
    c["order_function_before_column"] = plan([agg(6, -1, 3, in_range=0, width=16)], code=INVALID,
                                             message="aggregate 0: unknown function 6")
    c["order_range_before_type"] = plan([agg(SUM, -1, 3, in_range=0, width=16)], code=INVALID,
                                        message="aggregate 0: probe column 3 out of range")
    return c


def u64(x):
    return x & M64


def cells_of(rows, per_agg):
    """per_agg: (fn, [values that took part]) -> the combined table a run over them leaves, restated in Python ints"""
    w = [rows]
    for fn, vals in per_agg:
        a = b = 0
        if fn == SUM:
            a, b = u64(sum(v & 0xFFFFFFFF for v in vals)), u64(sum(v >> 32 for v in vals))
        elif fn == MIN:
            a = min((u64(v) ^ (1 << 63) for v in vals), default=M64)
        elif fn == MAX:
            a = max((u64(v) ^ (1 << 63) for v in vals), default=0)
        w += [a, b, len(vals)]
    return w


def want_values(rows, per_agg):
    out = []
    for fn, vals in per_agg:
        if fn == COUNT_STAR:
            out.append((rows, rows, 0))
        elif fn == COUNT:
            out.append((len(vals), len(vals), 0))
        elif not vals:
            out.append((0, 0, 1))
        else:
            out.append(({SUM: sum, MIN: min, MAX: max}[fn](vals), len(vals), 0))
    return out


def decode_cases():
    d = {}
    d["five_int64_max"] = (5, [(SUM, [I64_MAX] * 5)])      # 5 x (2^63 - 1): leaves 64 bits
    d["five_int64_min"] = (5, [(SUM, [I64_MIN] * 5)])
    d["mixed_signs"] = (6, [(SUM, [I64_MAX, I64_MIN, -1, 1, -(2 ** 32), 2 ** 32 + 5]), (COUNT, [1, 2, 3]), (COUNT_STAR, [])])
    d["uint32_max"] = (3, [(SUM, [2 ** 32 - 1] * 3), (MIN, [2 ** 32 - 1]), (MAX, [2 ** 32 - 1, 0])])
    # MIN / MAX at the bounds of the eight column types (1, 2, 4, 8 bytes; signed, and unsigned up to 4 -- an unsigned 8-byte
    # column is refused, its place is taken by the signed 8-byte bounds met together)
    for bits in (8, 16, 32, 64):
        lo, hi = -2 ** (bits - 1), 2 ** (bits - 1) - 1
        d["bounds_i%d" % bits] = (2, [(MIN, [lo, hi]), (MAX, [lo, hi]), (MIN, [hi]), (MAX, [lo])])
        if bits < 64:
            d["bounds_u%d" % bits] = (2, [(MIN, [0, 2 ** bits - 1]), (MAX, [0, 2 ** bits - 1]), (MIN, [2 ** bits - 1]), (MAX, [0])])
    d["no_rows"] = (0, [(SUM, []), (MIN, []), (MAX, []), (COUNT, []), (COUNT_STAR, [])])
    d["all_null_argument"] = (7, [(SUM, []), (MIN, []), (MAX, []), (COUNT, []), (COUNT_STAR, [])])
    d["eight"] = (4, [(COUNT_STAR, []), (COUNT, [5, 6]), (SUM, [-7, 9, I64_MIN]), (MIN, [3, -3]), (MAX, [3, -3]),
                      (SUM, [255] * 4), (MIN, [I64_MIN]), (MAX, [I64_MAX])])
    return d


def write_requests(path, plans, decodes, raw):
    with open(path, "w") as f:
        for name, p in plans.items():
            f.write("plan %s %d %d %d %d\n" % ((name,) + p["head"]))
            for a in p["aggs"]:
                f.write("agg %d %d %d %d %d %d\n" % a)
            f.write("end\n")
        for name, (rows, per_agg) in decodes.items():
            f.write("decode %s %d %s %s\n" % (name, len(per_agg), " ".join(str(fn) for fn, _v in per_agg),
                                             " ".join(str(x) for x in cells_of(rows, per_agg))))
        for name, (fns, words) in raw.items():
            f.write("decode %s %d %s %s\n" % (name, len(fns), " ".join(map(str, fns)), " ".join(map(str, words))))


def parse(stdout):
    plans, decodes, cur = {}, {}, None
    for line in stdout.splitlines():
        if line.startswith("  "):
            key, *rest = line.split()
            cur.setdefault(key, []).append([int(x) for x in rest])
        elif line.startswith("decode "):
            _, name, code, *msg = line.split(" ", 3)
            cur = decodes[name] = {"code": int(code), "message": msg[0] if msg else ""}
        elif line != "ok" and not line.endswith(" requests"):
            name, code, *msg = line.split(" ", 2)
            cur = plans[name] = {"code": int(code), "message": msg[0] if msg else ""}
    return plans, decodes


def build(tmp_path, sanitize):
    exe = str(tmp_path / "fuseagg_plan")
    flags = ["-fsanitize=" + sanitize, "-fno-sanitize-recover=all"] if sanitize else []
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall"] + flags + [SRC, "-o", exe], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-4000:]
    return exe


def run(exe, path):
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    return r.stdout


def check_layout(got, p):
    n = len(p["aggs"])
    words = 1 + 3 * n
    assert got["layout"] == [[TABLES, words, (TABLES + 1) * words, int(any(a[0] == SUM for a in p["aggs"]))]]
    assert got["fn"] == [[a[0] for a in p["aggs"]]]
    kinds, reset = [ADD], [0]
    for a in p["aggs"]:
        kinds += [KMIN if a[0] == MIN else (KMAX if a[0] == MAX else ADD), ADD, ADD]
        reset += [M64 if a[0] == MIN else 0, 0, 0]
    assert got["kind"] == [kinds] and got["reset"] == [reset]


@pytest.mark.parametrize("sanitize", [None, "address,undefined"], ids=["plain", "asan-ubsan"])
def test_refusals_layout_reset_words_and_decode(tmp_path, sanitize):
    exe, path = build(tmp_path, sanitize), str(tmp_path / "requests.txt")
    plans, decodes = plan_cases(), decode_cases()
    # fabricated tables at the bound of the SUM cells: 2^32 - 1 folded tuples are accepted, 2^32 are POLR_E_RANGE -- but
    # only where the sink has a SUM
    raw = {"rows_below_bound": ([SUM, MIN], [2 ** 32 - 1, 5, 0, 2 ** 32 - 1, (1 << 63) | 5, 0, 2 ** 32 - 1]),
           "rows_at_bound": ([MIN, SUM], [2 ** 32, (1 << 63) | 5, 0, 2 ** 32, 5, 0, 2 ** 32]),
           "rows_at_bound_no_sum": ([MIN, COUNT, COUNT_STAR], [2 ** 32, (1 << 63) | 5, 0, 2 ** 32, 0, 0, 7, 0, 0, 0]),
           # every lane's low part at its maximum for 2^32 - 1 rows: lo just below 2^64, hi = -(2^32 - 1): the sum is -(2^32 - 1)
           "limbs_at_their_bounds": ([SUM], [2 ** 32 - 1, (2 ** 32 - 1) * (2 ** 32 - 1), u64(-(2 ** 32 - 1)), 2 ** 32 - 1])}
    write_requests(path, plans, decodes, raw)
    stdout = run(exe, path)
    assert stdout.strip().splitlines()[-2:] == ["%d requests" % (len(plans) + len(decodes) + len(raw)), "ok"]
    got, dec = parse(stdout)
    for name, p in plans.items():
        assert got[name]["code"] == p["code"], (name, got[name])
        assert got[name]["message"] == p["message"], (name, got[name])  # the whole message
        if p["code"] == OK:
            if name.startswith("unfuse") or name == "order_unfuse_before_count":
                assert "unfuse" in got[name] and "layout" not in got[name], name
            else:
                check_layout(got[name], p)
    # known answers beside the restated rule: 1 aggregate = 4 words, 8 aggregates = 25; 257 tables are allocated
    assert got["one"]["layout"] == [[256, 4, 257 * 4, 1]] and got["eight"]["layout"] == [[256, 25, 257 * 25, 1]]
    assert got["one"]["kind"] == [[0, 0, 0, 0]] and got["one"]["reset"] == [[0, 0, 0, 0]]
    assert got["eight"]["kind"][0][10] == KMIN and got["eight"]["reset"][0][10] == M64  # (aggregate 3 is a MIN: word 1 + 3 * 3)
    assert got["eight"]["kind"][0][13] == KMAX and got["eight"]["reset"][0][13] == 0
    assert sum(got["eight"]["kind"][0]) == 2 * KMIN + 2 * KMAX and got["eight"]["reset"][0].count(M64) == 2
    for name, (rows, per_agg) in decodes.items():
        assert dec[name]["code"] == OK and dec[name]["message"] == "", (name, dec[name])
        for (lo, hi, count, is_null), (value, n, null) in zip(dec[name]["value"], want_values(rows, per_agg)):
            assert (count, is_null) == (n, null), name
            if not null:
                assert (hi << 64) + (lo & M64) == value, (name, lo, hi, value)
            else:
                assert (lo, hi) == (0, 0), name
    # known answers: 5 x INT64_MAX and 5 x INT64_MIN need 66 bits
    assert dec["five_int64_max"]["value"] == [[u64(5 * I64_MAX) - (1 << 64) if u64(5 * I64_MAX) >> 63 else u64(5 * I64_MAX), 2, 5, 0]]
    assert dec["five_int64_min"]["value"][0][1] == -3 and dec["five_int64_min"]["value"][0][0] == I64_MIN
    assert dec["no_rows"]["value"] == [[0, 0, 0, 1], [0, 0, 0, 1], [0, 0, 0, 1], [0, 0, 0, 0], [0, 0, 0, 0]]
    assert dec["all_null_argument"]["value"][4] == [7, 0, 7, 0]  # COUNT(*) counts the rows whose argument is NULL
    assert dec["bounds_i64"]["value"][:2] == [[I64_MIN, -1, 2, 0], [I64_MAX, 0, 2, 0]]
    assert dec["bounds_u32"]["value"][1] == [2 ** 32 - 1, 0, 2, 0]
    assert dec["rows_below_bound"]["code"] == OK and dec["rows_below_bound"]["value"] == [[5, 0, 2 ** 32 - 1, 0], [5, 0, 2 ** 32 - 1, 0]]
    assert dec["rows_at_bound"]["code"] == RANGE and dec["rows_at_bound"]["untouched"] == [[1]]
    assert dec["rows_at_bound"]["message"].startswith("aggregate 1: 4294967296 tuples were folded")
    assert dec["rows_at_bound_no_sum"]["code"] == OK and dec["rows_at_bound_no_sum"]["value"][2] == [2 ** 32, 0, 2 ** 32, 0]
    v = dec["limbs_at_their_bounds"]["value"][0]
    assert (v[1] << 64) + (v[0] & M64) == (2 ** 32 - 1) * (2 ** 32 - 1) - (2 ** 32 - 1) * 2 ** 32


def test_the_table_count_stands_once():
    """how many cell tables a launch spreads over is the plan's n_tables: neither the fold (polr_gen_device.h) nor the fill /
    combine kernels and entry points (polr_agg.hip) restate the constant.  (What pins the layout itself are the GPU tests.)"""
    csrc = os.path.join(common.ROOT, "duckdb-polr_amd", "csrc")
    for name in ("polr_gen_device.h", "polr_agg.hip"):
        assert "POLR_FUSEAGG_TABLES" not in open(os.path.join(csrc, name)).read(), name
