"""Filter expressions behind the scan, the part that needs no GPU: the tests' own evaluator (tests/scanexpr.py: three-valued
logic in numpy, IN by bytes equality, LIKE through a bytes regular expression in which '_' is one byte) reproduces every
query the reference engine answered (tests/golden/scan_expr.json, made by tests/golden/make_golden_scan_expr.py).  This is
what makes scanexpr the reference of the device tests."""
import json
import os

import numpy as np
import pytest

import common
import scanexpr
import scanstr

GOLD = json.load(open(os.path.join(common.ROOT, "tests", "golden", "scan_expr.json"), encoding="utf-8"))


@pytest.fixture(scope="module")
def columns():
    s = scanstr.fixture_column(GOLD["seed"], GOLD["n_rows"])
    assert scanstr.column_digest(s) == GOLD["column_sha1"], "the seeded generator no longer makes the fixture's column"
    i = scanexpr.fixture_int(GOLD["int_seed"], GOLD["n_rows"])
    assert sum(v is None for v in s) == GOLD["n_null"] and int((i[1] == 0).sum()) == GOLD["n_int_null"]
    return {"s": s, "i": i}


def kinds(e, out):
    out.append(e[0])
    for x in e[1:]:
        if isinstance(x, list) and x and isinstance(x[0], str) and x[0] in ("and", "or", "not", "cmp", "in", "like"):
            kinds(x, out)
    return out


def test_fixture_covers_what_the_issue_asks():
    qs = GOLD["queries"]
    assert len(qs) >= 75
    likes = [q["expr"][2] for q in qs if q["expr"][0] == "like"]
    not_likes = [q["expr"][1][2] for q in qs if q["expr"][0] == "not" and q["expr"][1][0] == "like"]
    assert likes == not_likes and len(likes) >= 25
    assert {"%", "", "_", "%_", "M_nchen%", "M__nchen%", "%語%", "%ab%b"} <= set(likes)
    ins = [q["expr"] for q in qs if q["expr"][0] == "in"] + [q["expr"][1] for q in qs if q["expr"][0] == "not" and q["expr"][1][0] == "in"]
    assert sorted((e[1], len(e[2])) for e in ins) == sorted([(c, n) for c in "si" for n in (1, 3, 8)] * 2)
    assert any(q["expr"][0] == "or" and [e[0] for e in q["expr"][1:]] == ["like", "like"] for q in qs)
    assert any(q["expr"][0] == "or" and q["expr"][1] == ["cmp", "s", "is null"] for q in qs)
    assert sum(bool(q.get("kleene")) for q in qs) >= 2
    assert any({"in", "or", "not", "like", "cmp", "and"} <= set(kinds(q["expr"], [])) for q in qs)  # the 19a shape
    n = GOLD["n_rows"]
    assert all(q.get("edge") or 0 < q["count"] < n for q in qs)
    # '_' is one byte: München's ü is two
    by_where = {q["where"]: q["count"] for q in qs}
    assert by_where["s LIKE 'M_nchen%'"] == 0 < by_where["s LIKE 'M__nchen%'"]


def test_the_evaluator_reproduces_every_query(columns):
    for q in GOLD["queries"]:
        rows = scanexpr.passing(scanexpr.bind(q["expr"], {"s": "s", "i": "i"}), columns, GOLD["n_rows"])
        assert scanstr.rows_digest(rows) == {"count": q["count"], "sha1": q["sha1"]}, q["where"]


def test_null_roots_differ_from_a_two_valued_reading(columns):
    """the queries marked kleene: rows whose root is NULL do not pass, though NOT over 'NULL read as FALSE' would"""
    for q in GOLD["queries"]:
        if q.get("kleene"):
            t, null = scanexpr.evaluate(scanexpr.bind(q["expr"], {"s": "s", "i": "i"}), columns)
            assert null.sum() > 0 and not (t & null).any(), q["where"]
            assert int(t.sum()) == q["count"]


def test_three_valued_logic_tables():
    T, F, N = (True, False), (False, False), (False, True)
    col = {"a": (np.zeros(9, np.int32), np.array([1, 1, 1, 1, 1, 1, 0, 0, 0], np.uint8)),
           "b": (np.zeros(9, np.int32), np.array([1, 1, 0, 1, 1, 0, 1, 1, 0], np.uint8))}
    col["a"][0][:] = [1, 1, 1, 0, 0, 0, 9, 9, 9]
    col["b"][0][:] = [1, 0, 9, 1, 0, 9, 1, 0, 9]
    a, b = ("cmp", "a", "=", 1), ("cmp", "b", "=", 1)
    def table(e):
        t, n = scanexpr.evaluate(e, col)
        return list(zip(t.tolist(), n.tolist()))
    assert table(("and", a, b)) == [T, F, N, F, F, F, N, F, N]
    assert table(("or", a, b)) == [T, T, T, T, F, N, T, N, N]
    assert table(("not", a)) == [F, F, F, T, T, T, N, N, N]
