"""The host-side plan of polr_ht_filter (duckdb-polr_amd/csrc/polr_htfilter_plan.h), the part that needs no GPU: the header
alone behind a stand-alone host program (tests/htfilter/htfilter_plan_main.cpp).  Every refusal with its code and whole
message, in the documented order (a request that earns several is refused for the first); the column numbering at
n_keys - 1 and n_keys; 4 keys and 62 payload columns; the filter's limits at the limit and one beyond, through this entry;
the heap guards; the scratch; and the layout of the table's one allocation line by line -- a table with every width, kept
counts 0, 1 and 12 345, every array at a multiple of 256 bytes, none overlapping.  Built plain and with the address +
undefined-behaviour sanitizers, and run directly."""
import os
import subprocess

import pytest

import common

SRC = os.path.join(common.ROOT, "tests", "htfilter", "htfilter_plan_main.cpp")
OK, INVALID, UNSUPPORTED = 0, -2, -3
CMP, IN, LIKE, NOT, AND, OR = range(6)
EQ, NE, LT, GT, LE, GE, IS_NULL, IS_NOT_NULL = range(8)
KEPT = (0, 1, 12345)
DESC = 40  # sizeof(PolrHtFilterDesc): four pointers and two words


def col(width, signed=0, has_valid=0, owned=1, rebased=0):
    return (width, signed, has_valid, owned, rebased)


K4 = col(4, 1)
FRESH = (1, 0, 0, 0, 0)  # has_ht, finalized, filtered, has_dict, dict_col
EVERY_WIDTH = ([col(1), col(2, 1, 1), col(4, 1), col(8, 0, 1)],
               [col(1, 1, 1), col(2), col(4, 0, 1), col(8, 1), col(16, 0, 1), col(16)])


def req(state=FRESH, rows=1000, keys=(K4,), payload=(), nodes=(), values=(), counts=None, kept=(), code=OK, message=None):
    return dict(state=state, rows=rows, keys=list(keys), payload=list(payload), nodes=list(nodes), values=list(values),
                counts=counts, kept=list(kept), code=code, message=message)


def leaf(c, op=EQ, first=0):
    return (CMP, c, op, first, 1)


def cases():
    c = {}
    one = dict(nodes=[leaf(0)], values=[(5, None)])
    c["keeps_every_row"] = req(kept=KEPT)
    c["one_leaf"] = req(**one)
    # the refusals of the contract, each alone ...
    c["null_table"] = req(state=(0, 0, 0, 0, 0), code=INVALID, message="polr_ht_filter: the table is NULL", **one)
    c["finalized"] = req(state=(1, 1, 0, 0, 0), code=INVALID, **one,
                         message="polr_ht_filter: the table is finalized (a build side is filtered before polr_ht_finalize_*)")
    c["encoded"] = req(state=(1, 0, 0, 1, 3), code=INVALID, payload=[col(16)] * 4, **one,
                       message="polr_ht_filter: payload column 3 is dictionary-encoded: filter first, then encode")
    c["filtered_twice"] = req(state=(1, 0, 1, 0, 0), code=INVALID, **one,
                              message="polr_ht_filter: the table was filtered already (once per table)")
    c["col_beyond"] = req(payload=[col(4)], nodes=[leaf(2)], values=[(5, None)], code=INVALID,
                          message="filter expression: node 0: column 2 out of range")
    # ... and in their order: the earlier one wins
    c["order_finalized_first"] = req(state=(1, 1, 1, 1, 0), code=INVALID, nodes=[leaf(9)], values=[(5, None)],
                                     message=c["finalized"]["message"])
    c["order_encoded_before_filtered"] = req(state=(1, 0, 1, 1, 0), code=INVALID, payload=[col(16)], nodes=[leaf(9)], values=[(5, None)],
                                             message="polr_ht_filter: payload column 0 is dictionary-encoded: filter first, then encode")
    c["order_filtered_before_program"] = req(state=(1, 0, 1, 0, 0), code=INVALID, nodes=[leaf(9)], values=[(5, None)],
                                             message=c["filtered_twice"]["message"])
    # the numbering: col n_keys - 1 is the last key, col n_keys the first payload column
    c["numbering"] = req(keys=[K4, col(8, 1)], payload=[col(16), col(2)],
                         nodes=[leaf(1), (LIKE, 2, 0, 1, 1), (AND, 0, 0, 0, 0)], values=[(7, None), (0, b"%x%".hex())])
    c["like_on_the_last_key"] = req(keys=[K4, col(8, 1)], payload=[col(16)], nodes=[(LIKE, 1, 0, 0, 1)], values=[(0, b"a%".hex())],
                                    code=INVALID, message="filter expression: node 0: LIKE on column 1, which is 8 bytes wide")
    c["wide"] = req(keys=[K4] * 4, payload=[col(4)] * 62, nodes=[leaf(65)], values=[(1, None)], kept=[7])
    c["wide_col_66"] = req(keys=[K4] * 4, payload=[col(4)] * 62, nodes=[leaf(66)], values=[(1, None)], code=INVALID,
                           message="filter expression: node 0: column 66 out of range")
    # two more of the program's refusals
    c["stack_underflow"] = req(nodes=[leaf(0), (AND, 0, 0, 0, 0)], values=[(5, None)], code=INVALID,
                               message="filter expression: node 1: AND / OR needs two operands, the stack holds 1")
    nine = [col(4)] * 9
    chain = [leaf(1 + i, EQ, i) for i in range(9)]
    prog = [chain[0]]
    for n in chain[1:]:
        prog += [n, (OR, 0, 0, 0, 0)]
    c["columns_8"] = req(payload=nine, nodes=prog[:15], values=[(i, None) for i in range(8)])
    c["columns_9"] = req(payload=nine, nodes=prog, values=[(i, None) for i in range(9)], code=UNSUPPORTED,
                         message="filter expression: more than 8 distinct columns")
    # the limits of the scan call, through this entry: 64 nodes, depth 32, 64 values, 16 384 bytes, a NUL in a pattern
    def ors(n_leaves):  # n_leaves leaves over column 0 folded left to right: 2 n - 1 nodes
        p = [(CMP, 0, IS_NULL, 0, 0)]
        for _ in range(n_leaves - 1):
            p += [(CMP, 0, IS_NULL, 0, 0), (OR, 0, 0, 0, 0)]
        return p
    c["nodes_64"] = req(nodes=ors(32) + [(NOT, 0, 0, 0, 0)])
    c["nodes_65"] = req(nodes=ors(32) + [(NOT, 0, 0, 0, 0)] * 2, code=UNSUPPORTED,
                        message="filter expression: an expression of 65 nodes (at most 64)")
    deep = lambda d: [(CMP, 0, IS_NULL, 0, 0)] * d + [(AND, 0, 0, 0, 0)] * (d - 1)
    c["depth_32"] = req(nodes=deep(32))
    c["depth_33"] = req(nodes=deep(33)[:64], counts=(64, 0), code=UNSUPPORTED,
                        message="filter expression: node 32: the operand stack grows beyond 32")
    c["values_64"] = req(nodes=[(IN, 0, 0, 0, 64)], values=[(i, None) for i in range(64)])
    c["values_65"] = req(nodes=[(IN, 0, 0, 0, 65)], values=[(i, None) for i in range(65)], code=UNSUPPORTED,
                         message="filter expression: 65 constants (at most 64)")
    s = [col(16, 0, 1, 1, 1)]
    c["bytes_16384"] = req(payload=s, nodes=[(IN, 1, 0, 0, 4)], values=[(0, (bytes([65 + i]) * 4096).hex()) for i in range(4)])
    c["bytes_16385"] = req(payload=s, nodes=[(IN, 1, 0, 0, 5)], values=[(0, (bytes([65 + i]) * 4096).hex()) for i in range(4)] + [(0, b"x".hex())],
                           code=UNSUPPORTED, message="filter expression: 16385 bytes of string constants (at most 16384)")
    c["string_4097"] = req(payload=s, nodes=[leaf(1)], values=[(0, (b"y" * 4097).hex())], code=UNSUPPORTED,
                           message="filter expression: value 0: a string constant of 4097 bytes (at most 4096)")
    c["nul_in_pattern"] = req(payload=s, nodes=[(LIKE, 1, 0, 0, 1)], values=[(0, b"a\0b".hex())], code=UNSUPPORTED,
                              message="filter expression: node 0: a NUL byte in a LIKE pattern (the escape character of a LIKE without ESCAPE)")
    # the heap guard: VARCHAR columns some CMP / IN / LIKE leaf reads, uploaded by the library, never rebased
    strs = [col(16, 0, 1, owned=1, rebased=0), col(16, 0, 1, owned=1, rebased=1), col(16, 0, 0, owned=0, rebased=0),
            col(16, 0, 1, owned=1, rebased=0), col(16, 0, 0, owned=1, rebased=0)]
    c["guards"] = req(payload=strs, values=[(0, b"abc".hex()), (0, b"%q%".hex()), (0, "="), (0, b"r".hex())],
                      nodes=[(CMP, 5, EQ, 0, 1), (LIKE, 2, 0, 1, 1), (OR, 0, 0, 0, 0), (CMP, 3, NE, 2, 1), (OR, 0, 0, 0, 0),
                             (CMP, 4, IS_NOT_NULL, 0, 0), (AND, 0, 0, 0, 0), (IN, 1, 0, 3, 1), (OR, 0, 0, 0, 0)])
    # the layout: every width, as key and as payload, with and without validity
    c["every_width"] = req(rows=50000, keys=EVERY_WIDTH[0], payload=EVERY_WIDTH[1], kept=KEPT, **one)
    c["no_rows"] = req(rows=0, kept=[0], **one)
    c["tile_edges"] = req(rows=1024)
    c["tile_edges_plus_one"] = req(rows=1025)
    return c


def write_requests(path, reqs):
    with open(path, "w") as f:
        for name, r in reqs.items():
            f.write("request %s\nstate %d %d %d %d %d\nrows %d\n" % ((name,) + tuple(r["state"]) + (r["rows"],)))
            for k in r["keys"]:
                f.write("key %d %d %d %d %d\n" % k)
            for p in r["payload"]:
                f.write("payload %d %d %d %d %d\n" % p)
            for n in r["nodes"]:
                f.write("node %d %d %d %d %d\n" % n)
            for const, s in r["values"]:
                f.write("value %d %s\n" % (const, "-" if s is None else s))
            if r["counts"]:
                f.write("counts %d %d\n" % r["counts"])
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


def check_plan(got, r):
    cols = r["keys"] + r["payload"]
    nk = len(r["keys"])
    # the numbering: keys first, then payload
    assert got.get("number", []) == [[c, int(c < nk), c if c < nk else c - nk] for c in range(len(cols))]
    # the scratch: whole tiles of 1024 rows, 16 words each; words, first output rows and the total 8 bytes, counts 4
    tiles = (r["rows"] + 1023) // 1024
    assert got["scratch"] == [[tiles, 16 * tiles, 0, 128 * tiles, 136 * tiles, 136 * tiles + 8, alloc(136 * tiles + 8 + 4 * tiles)]]
    # the layouts: cells, then validity if the column has an array, column after column; the row list; the descriptors
    layouts = {l[0]: l[1:] for l in got.get("layout", [])}
    assert sorted(layouts) == sorted(r["kept"])
    for n in r["kept"]:
        at, want, spans = 0, [], []
        for c in cols:
            d = at
            at += up(n * c[0])
            spans.append((d, d + n * c[0]))
            v = -1
            if c[2]:
                v = at
                at += up(n)
                spans.append((v, v + n))
            want.append([d, v])
        rows_off = at
        spans.append((rows_off, rows_off + 4 * n))
        at += up(4 * n)
        spans.append((at, at + DESC * len(cols)))
        assert [p[2:] for p in got["place"] if p[0] == n] == want
        assert [p[1] for p in got["place"] if p[0] == n] == list(range(len(cols)))
        assert layouts[n] == [alloc(at + DESC * len(cols)), rows_off, at, DESC]
        # every array at a multiple of 256 bytes, none overlapping, all inside the allocation
        assert all(b % 256 == 0 for b, _ in spans)
        assert all(spans[i][1] <= spans[i + 1][0] for i in range(len(spans) - 1)) and spans[-1][1] <= layouts[n][0]


@pytest.mark.parametrize("sanitize", [None, "address,undefined"], ids=["plain", "asan-ubsan"])
def test_refusals_numbering_limits_and_the_layout(tmp_path, sanitize):
    exe, path = str(tmp_path / "htfilter_plan"), str(tmp_path / "requests.txt")
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
    # the program's columns are the table's: key 1 and payload column 0 of a table of two keys
    assert got["numbering"]["fxcol"] == [[1, 0, 1, 1], [2, 1, 1, 1]]
    assert got["wide"]["fxcol"] == [[65, 0, 1, 1]] and len(got["wide"]["number"]) == 66
    assert got["wide"]["number"][3] == [3, 1, 3] and got["wide"]["number"][4] == [4, 0, 0] and got["wide"]["number"][65] == [65, 0, 61]
    assert len(got["columns_8"]["fxcol"]) == 8
    # the guards: column 5 (CMP, never rebased) and column 1 (IN, never rebased); not column 2 (rebased), not column 3 (a
    # caller's device memory), not column 4 (only IS NOT NULL reads it: the validity, no cell)
    assert got["guards"]["guard"] == [[5, 1]]
    assert [f[0] for f in got["guards"]["fxcol"]] == [5, 2, 3, 4, 1] and [f[3] for f in got["guards"]["fxcol"]] == [1, 1, 1, 0, 1]
    assert got["one_leaf"]["guard"] == [[]]
    # an empty table: no tile, and an allocation that holds nothing but the descriptor
    assert got["no_rows"]["scratch"] == [[0, 0, 0, 0, 0, 8, 8]] and got["no_rows"]["layout"] == [[0, DESC, 0, 0, DESC]]
    assert got["tile_edges"]["scratch"][0][:2] == [1, 16] and got["tile_edges_plus_one"]["scratch"][0][:2] == [2, 32]
    # the table with every width, 12 345 rows kept: the first key's cells, then the second key's cells and validity, ...
    place = [p[2:] for p in got["every_width"]["place"] if p[0] == 12345]
    assert place[:3] == [[0, -1], [12544, 37376], [49920, -1]]
