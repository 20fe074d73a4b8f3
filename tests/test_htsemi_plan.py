"""The host-side plan of polr_ht_semi_filter (duckdb-polr_amd/csrc/polr_htsemi_plan.h), the part that needs no GPU: the
header alone behind a stand-alone host program (tests/htsemi/htsemi_plan_main.cpp).  Every refusal with its code and whole
message, in the documented order (a request that earns several is refused for the first); 4 filters and 5; the order of the
device pass (smallest device_bytes first, ties by index); the column numbering at n_keys - 1 and n_keys; the key arithmetic
of the plain and the packed form; the scratch; and the layout of the table's one allocation with and without a carried row
list.  Built plain and with the address + undefined-behaviour sanitizers, and run directly."""
import os
import subprocess

import pytest

import common

SRC = os.path.join(common.ROOT, "tests", "htsemi", "htsemi_plan_main.cpp")
OK, INVALID, UNSUPPORTED = 0, -2, -3
NONE, PERFECT, S8, S16 = range(4)
BY_VALUE, NULL_EQUAL = 1, 2
ANTI = 1
KEPT = (0, 1, 12345)
DESC = 40  # sizeof(PolrHtFilterDesc)
ALL = 2 ** 64 - 1
P = "polr_ht_semi_filter: "


def col(width, signed=0, has_valid=0, owned=1, rebased=0):
    return (width, signed, has_valid, owned, rebased)


K4 = col(4, 1)
FRESH = (1, 0, 0, 0, 0)  # has_ht, finalized, filtered, has_dict, dict_col


def by(keys=((4, 0),), kind=S8, signed=0, size=1000, packed=0, null_eq=0, has=1, finalized=1, is_ht=0, same_place=1):
    """keys: (width, flags[, shift, min, range]) per key of `by`"""
    return dict(head=(has, finalized, is_ht, same_place, kind, signed, size, packed, null_eq),
                keys=[tuple(k) + (0, 0, 0)[len(k) - 2:] for k in keys])


def flt(b, cols=(0,), flags=0, n_cols=None):
    cols = list(cols)
    return (b, flags, len(cols) if n_cols is None else n_cols, cols + [0] * (4 - len(cols)))


def req(state=FRESH, rows=1000, keys=(K4,), payload=(), filters=(), n_filters=None, null_filters=False, kept=(), code=OK,
        message=None):
    return dict(state=state, rows=rows, keys=list(keys), payload=list(payload), filters=list(filters), n_filters=n_filters,
                null_filters=null_filters, kept=list(kept), code=code, message=message)


def cases():
    c = {}
    one = dict(filters=[flt(by())])
    bad = dict(filters=[flt(by(has=0), cols=(9,), flags=6)])  # earns every per-filter refusal at once
    c["keeps_every_row"] = req(kept=KEPT)
    c["one_filter"] = req(kept=KEPT, **one)
    # the refusals of the contract, each alone ...
    c["null_table"] = req(state=(0, 0, 0, 0, 0), code=INVALID, message=P + "the table is NULL", **one)
    c["finalized"] = req(state=(1, 1, 0, 0, 0), code=INVALID, **one,
                         message=P + "the table is finalized (a build side is filtered before polr_ht_finalize_*)")
    c["encoded"] = req(state=(1, 0, 0, 1, 3), code=INVALID, payload=[col(16)] * 4, **one,
                       message=P + "payload column 3 is dictionary-encoded: filter first, then encode")
    c["filters_4"] = req(filters=[flt(by())] * 4)
    c["filters_5"] = req(filters=[flt(by())] * 5, code=UNSUPPORTED, message=P + "5 filters (at most 4 in one call)")
    c["null_filters"] = req(filters=[flt(by())], null_filters=True, code=INVALID, message=P + "filters is NULL")
    c["null_by"] = req(filters=[flt(by()), flt(by(has=0))], code=INVALID, message=P + "filter 1: `by` is NULL")
    c["by_not_finalized"] = req(filters=[flt(by(finalized=0, kind=NONE))], code=INVALID,
                                message=P + "filter 0: `by` is not finalized (its index is what is probed)")
    c["by_is_ht"] = req(filters=[flt(by(is_ht=1))], code=INVALID, message=P + "filter 0: `by` is the table itself")
    c["by_elsewhere"] = req(filters=[flt(by(same_place=0))], code=INVALID,
                            message=P + "filter 0: `by` lives on another device or context")
    c["flag_bits"] = req(filters=[flt(by(), flags=2)], code=INVALID, message=P + "filter 0: flags 0x2 (0 or POLR_SEMI_ANTI)")
    c["flag_bits_beside_anti"] = req(filters=[flt(by(), flags=3)], code=INVALID,
                                     message=P + "filter 0: flags 0x3 (0 or POLR_SEMI_ANTI)")
    c["key_count"] = req(filters=[flt(by(keys=[(4, 0), (4, 0)], kind=S16), cols=(0,))], code=INVALID,
                         message=P + "filter 0: 1 columns for a 2-key table")
    c["key_count_more"] = req(filters=[flt(by(), cols=(0, 0))], code=INVALID, message=P + "filter 0: 2 columns for a 1-key table")
    c["col_beyond"] = req(payload=[col(4)], filters=[flt(by(), cols=(2,))], code=INVALID,
                          message=P + "filter 0 key 0: column 2 out of range")
    c["col_16_bytes"] = req(payload=[col(16)], filters=[flt(by(keys=[(8, 0)], kind=S16), cols=(1,))], code=UNSUPPORTED,
                            message=P + "filter 0 key 0: column 1 holds 16-byte cells (strings and wide composites are not "
                                        "verified here)")
    c["widths_differ"] = req(payload=[col(2)], filters=[flt(by(keys=[(4, 0), (4, 0)], kind=S16), cols=(0, 1))], code=INVALID,
                             message=P + "filter 0 key 1: column 1 is 2 bytes, the key of `by` 4 bytes (a CAST'ed key: "
                                         "polr_ht_set_key_flags(..., POLR_KEY_BY_VALUE) before `by` is finalized)")
    c["no_integer"] = req(payload=[col(3)], filters=[flt(by(keys=[(3, 0)], kind=S16), cols=(1,))], code=UNSUPPORTED,
                          message=P + "filter 0 key 0: column 1 of 3 bytes")
    # ... and in their order: the earlier one wins
    c["order_finalized_first"] = req(state=(1, 1, 1, 1, 0), code=INVALID, filters=bad["filters"] * 5,
                                     message=c["finalized"]["message"])
    c["order_encoded_before_limit"] = req(state=(1, 0, 1, 1, 0), code=INVALID, payload=[col(16)], filters=bad["filters"] * 5,
                                          message=P + "payload column 0 is dictionary-encoded: filter first, then encode")
    c["order_limit_before_filters"] = req(filters=bad["filters"] * 5, null_filters=True, code=UNSUPPORTED,
                                          message=c["filters_5"]["message"])
    c["order_null_by_first"] = req(code=INVALID, message=P + "filter 0: `by` is NULL", **bad)
    c["order_not_finalized"] = req(filters=[flt(by(finalized=0, is_ht=1, same_place=0), cols=(9,), flags=6)], code=INVALID,
                                   message=c["by_not_finalized"]["message"])
    c["order_is_ht"] = req(filters=[flt(by(is_ht=1, same_place=0), cols=(9,), flags=6)], code=INVALID,
                           message=c["by_is_ht"]["message"])
    c["order_elsewhere"] = req(filters=[flt(by(same_place=0), cols=(9,), flags=6)], code=INVALID,
                               message=c["by_elsewhere"]["message"])
    c["order_flags"] = req(filters=[flt(by(), cols=(9, 9), flags=6)], code=INVALID,
                           message=P + "filter 0: flags 0x6 (0 or POLR_SEMI_ANTI)")
    c["order_key_count"] = req(filters=[flt(by(), cols=(9, 9))], code=INVALID, message=c["key_count_more"]["message"])
    c["order_col_before_width"] = req(payload=[col(16)], filters=[flt(by(keys=[(4, 0), (4, 0)], kind=S16), cols=(7, 1))],
                                      code=INVALID, message=P + "filter 0 key 0: column 7 out of range")
    c["order_16_before_pairing"] = req(payload=[col(16)], filters=[flt(by(keys=[(4, 0)]), cols=(1,))], code=UNSUPPORTED,
                                       message=P + "filter 0 key 0: column 1 holds 16-byte cells (strings and wide composites "
                                                   "are not verified here)")
    c["order_first_filter_first"] = req(filters=[flt(by(), flags=2), flt(by(has=0))], code=INVALID,
                                        message=c["flag_bits"]["message"])
    # the order of the device pass: smallest device_bytes first, ties by index
    c["pass_order"] = req(filters=[flt(by(size=500)), flt(by(size=100), flags=ANTI), flt(by(size=500)), flt(by(size=7))])
    c["pass_order_ties"] = req(filters=[flt(by(size=5))] * 4)
    # the numbering and the arithmetic: a table of two keys and three payload columns
    wide = dict(keys=[K4, col(8, 1)], payload=[col(2, 0, 1), col(4, 0), col(1, 1)])
    c["numbering"] = req(filters=[flt(by(keys=[(8, 0)], kind=PERFECT, signed=1), cols=(1,)),
                                  flt(by(keys=[(2, 0)], kind=S16), cols=(2,), flags=ANTI),
                                  flt(by(keys=[(4, 0), (4, 0)], kind=S16, signed=1), cols=(3, 0))], kept=KEPT, **wide)
    c["packed"] = req(filters=[flt(by(keys=[(4, BY_VALUE, 0, -5, 100), (4, BY_VALUE | NULL_EQUAL, 7, 3, 9), (8, BY_VALUE, 11, 0, 255)],
                                      kind=S16, packed=1, null_eq=2), cols=(4, 2, 0))], **wide)
    c["by_value_wider_and_narrower"] = req(filters=[flt(by(keys=[(2, BY_VALUE, 0, 0, 65535)], kind=S16, packed=1), cols=(1,)),
                                                    flt(by(keys=[(8, BY_VALUE, 0, -9, 20)], kind=S16, packed=1), cols=(4,))], **wide)
    # the layout, with and without a carried row list: every width, as key and as payload, with and without validity
    every = dict(rows=50000, keys=[col(1), col(2, 1, 1), col(4, 1), col(8, 0, 1)],
                 payload=[col(1, 1, 1), col(2), col(4, 0, 1), col(8, 1), col(16, 0, 1), col(16)])
    c["every_width"] = req(kept=KEPT, filters=[flt(by(keys=[(4, 0)]), cols=(2,))], **every)
    c["every_width_carried"] = req(state=(1, 0, 1, 0, 0), kept=KEPT, filters=[flt(by(keys=[(4, 0)]), cols=(2,))], **every)
    c["carried_no_filters"] = req(state=(1, 0, 1, 0, 0), kept=KEPT)
    c["no_rows"] = req(rows=0, kept=[0], **one)
    c["tile_edges"] = req(rows=1024, **one)
    c["tile_edges_plus_one"] = req(rows=1025, **one)
    return c


def write_requests(path, reqs):
    with open(path, "w") as f:
        for name, r in reqs.items():
            f.write("request %s\nstate %d %d %d %d %d\nrows %d\n" % ((name,) + tuple(r["state"]) + (r["rows"],)))
            for k in r["keys"]:
                f.write("key %d %d %d %d %d\n" % k)
            for p in r["payload"]:
                f.write("payload %d %d %d %d %d\n" % p)
            for b, flags, n_cols, cols in r["filters"]:
                f.write("by %d %d %d %d %d %d %d %d %d\n" % b["head"])
                for k in b["keys"]:
                    f.write("bykey %d %d %d %d %d\n" % k)
                f.write("filter %d %d %d %d %d %d\n" % ((flags, n_cols) + tuple(cols)))
            if r["n_filters"] is not None:
                f.write("nfilters %d\n" % r["n_filters"])
            if r["null_filters"]:
                f.write("nullfilters\n")
            for k in r["kept"]:
                f.write("kept %d\n" % k)
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


def want_key(r, b, c, column):
    """the arithmetic of key c of a filter whose column is `column`: [width, sx, shift, null_eq, min, range]"""
    cols = r["keys"] + r["payload"]
    head, k = b["head"], b["keys"][c]
    if head[7]:  # packed: by's KeyPack, the signedness of the table's own column
        return [cols[column][0], cols[column][1], k[2], (head[8] >> c) & 1, k[3], k[4]]
    return [cols[column][0], int(c == 0 and head[4] == PERFECT and head[5] != 0), 32 * c, 0, 0, ALL]


def check_plan(got, r):
    cols = r["keys"] + r["payload"]
    nk = len(r["keys"])
    carried = r["state"][2]
    # the filters: keys count, SEMI / ANTI, and per key the column (numbered keys first, then payload) and the arithmetic
    assert got.get("filter", []) == [[i, len(f[0]["keys"]), f[1] & 1] for i, f in enumerate(r["filters"])]
    want = []
    for i, (b, _flags, _n, fcols) in enumerate(r["filters"]):
        for c in range(len(b["keys"])):
            x = fcols[c]
            want.append([i, c, x, int(x < nk), x if x < nk else x - nk] + want_key(r, b, c, x))
    assert got.get("fkey", []) == want
    # the order of the device pass: by device_bytes, ties by index
    sizes = [f[0]["head"][6] for f in r["filters"]]
    assert got["order"] == [sorted(range(len(sizes)), key=lambda i: (sizes[i], i))]
    # the scratch: polr_ht_filter's -- whole tiles of 1024 rows, 16 words each
    tiles = (r["rows"] + 1023) // 1024
    assert got["scratch"] == [[tiles, 16 * tiles, 0, 128 * tiles, 136 * tiles, 136 * tiles + 8, alloc(136 * tiles + 8 + 4 * tiles)]]
    # the layouts: cells, then validity if the column has an array, column after column -- the carried list as one more
    # 4-byte column --; the row list of the pass; the descriptors
    layouts = {l[0]: l[1:] for l in got.get("layout", [])}
    assert sorted(layouts) == sorted(r["kept"])
    every = cols + ([col(4)] if carried else [])
    for n in r["kept"]:
        at, places, spans = 0, [], []
        for c in every:
            d = at
            at += up(n * c[0])
            spans.append((d, d + n * c[0]))
            v = -1
            if c[2]:
                v = at
                at += up(n)
                spans.append((v, v + n))
            places.append([d, v])
        rows_off = at
        spans.append((rows_off, rows_off + 4 * n))
        at += up(4 * n)
        spans.append((at, at + DESC * len(every)))
        assert [p[2:] for p in got["place"] if p[0] == n] == places
        list_off = places[-1][0] if carried else rows_off
        assert layouts[n] == [alloc(at + DESC * len(every)), rows_off, at, list_off, len(every), DESC]
        assert all(b % 256 == 0 for b, _ in spans)
        assert all(spans[i][1] <= spans[i + 1][0] for i in range(len(spans) - 1)) and spans[-1][1] <= layouts[n][0]


@pytest.mark.parametrize("sanitize", [None, "address,undefined"], ids=["plain", "asan-ubsan"])
def test_refusals_order_numbering_and_the_layout(tmp_path, sanitize):
    exe, path = str(tmp_path / "htsemi_plan"), str(tmp_path / "requests.txt")
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
        if r["code"] == OK:
            assert got[name]["message"] == "", (name, got[name])
            check_plan(got[name], r)
        else:
            assert got[name]["message"] == r["message"], (name, got[name])  # the whole message
    # known answers beside the restated rules.  The order of the pass: 7, 100, then the two of 500 by index
    assert got["pass_order"]["order"] == [[3, 1, 0, 2]] and got["pass_order_ties"]["order"] == [[0, 1, 2, 3]]
    assert [f[2] for f in got["pass_order"]["filter"]] == [0, 1, 0, 0]
    # the numbering: column 1 is the last key, column 2 the first payload column; a signed perfect key is sign-extended, the
    # keys of a plain two-key table sit at bits 0 and 32
    assert got["numbering"]["fkey"] == [[0, 0, 1, 1, 1, 8, 1, 0, 0, 0, ALL], [1, 0, 2, 0, 0, 2, 0, 0, 0, 0, ALL],
                                        [2, 0, 3, 0, 1, 4, 0, 0, 0, 0, ALL], [2, 1, 0, 1, 0, 4, 0, 32, 0, 0, ALL]]
    # the packed form: the table's own widths and signedness, by's shifts, minima and ranges, NULL = NULL on key 1 only
    assert got["packed"]["fkey"] == [[0, 0, 4, 0, 2, 1, 1, 0, 0, -5, 100], [0, 1, 2, 0, 0, 2, 0, 7, 1, 3, 9],
                                     [0, 2, 0, 1, 0, 4, 1, 11, 0, 0, 255]]
    assert [k[5:7] for k in got["by_value_wider_and_narrower"]["fkey"]] == [[8, 1], [1, 1]]
    # a table never filtered: polr_ht_filter's layout, the list at rows_off; a table filtered before: one descriptor more,
    # the composed list where the carried column's cells land, in front of the list of the pass
    fresh = {l[0]: l[1:] for l in got["every_width"]["layout"]}
    carried = {l[0]: l[1:] for l in got["every_width_carried"]["layout"]}
    assert fresh[12345][1] == fresh[12345][3] and fresh[12345][4] == 10
    assert carried[12345][4] == 11 and carried[12345][3] == fresh[12345][1] and carried[12345][1] == fresh[12345][1] + up(4 * 12345)
    assert carried[12345][0] == fresh[12345][0] + up(4 * 12345) + DESC
    assert [p[2:] for p in got["every_width_carried"]["place"] if p[0] == 12345][:10] == \
        [p[2:] for p in got["every_width"]["place"] if p[0] == 12345]
    assert got["carried_no_filters"]["layout"][0] == [0, 2 * DESC, 0, 0, 0, 2, DESC]
    assert got["no_rows"]["scratch"] == [[0, 0, 0, 0, 0, 8, 8]] and got["no_rows"]["layout"] == [[0, DESC, 0, 0, 0, 1, DESC]]
    assert got["tile_edges"]["scratch"][0][:2] == [1, 16] and got["tile_edges_plus_one"]["scratch"][0][:2] == [2, 32]


def test_join_keys_and_semi_filters_share_the_pairing_rule():
    """the rule stands once (pipe_key_pairing, polr_pipeline_plan.h); both plans call it and neither restates it"""
    csrc = os.path.join(common.ROOT, "duckdb-polr_amd", "csrc")
    pipe = open(os.path.join(csrc, "polr_pipeline_plan.h")).read()
    semi = open(os.path.join(csrc, "polr_htsemi_plan.h")).read()
    assert pipe.count("static inline int pipe_key_pairing(") == 1
    assert pipe.count("pipe_key_pairing(") == 2 and semi.count("pipe_key_pairing(") == 1
    assert pipe.count("& POLR_KEY_BY_VALUE") == 1 and "& POLR_KEY_BY_VALUE" not in semi
