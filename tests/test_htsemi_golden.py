"""tests/htsemi.py -- the numpy evaluator of SEMI / ANTI filters that the device tests of polr_ht_semi_filter are checked
against -- held to the reference's own answers: every query of tests/golden/semi_build.json (k IN (SELECT ...), EXISTS,
NOT EXISTS, two-column EXISTS, several subqueries, a constant filter beside one, NOT IN over a NULL-free subquery), row set
by row set.  No GPU."""
import json
import os

import numpy as np

import common
import htsemi
import scanstr

GOLD = json.load(open(os.path.join(common.ROOT, "tests", "golden", "semi_build.json")))


def test_fixture_tables_are_the_recorded_ones():
    tables = htsemi.fixture_tables(GOLD["seed"], GOLD["n_rows"])
    assert htsemi.tables_digest(tables) == GOLD["tables_sha1"]
    for name, cnt in GOLD["n_null"].items():
        t, c = name.split(".")
        assert int((np.asarray(tables[t][c][1]) == 0).sum()) == cnt
    # what the fixture is for: NULL keys in d, repeated keys and a NULL key in a, unique NULL-free keys in b
    assert GOLD["n_null"]["d.k"] > 0 and GOLD["n_null"]["d.k2"] > 0 and GOLD["n_null"]["a.x"] == 1
    ax, av = tables["a"]["x"]
    assert len(np.unique(ax[av != 0])) < int((av != 0).sum())
    assert len(np.unique(tables["b"]["x"][0])) == len(tables["b"]["x"][0])


def test_every_query_shape_is_there():
    qs = GOLD["queries"]
    assert len(qs) >= 12
    styles = [[f["style"] for f in q["filters"]] for q in qs]
    assert ["in"] in styles and ["exists"] in styles and ["not in"] in styles
    assert any(len(f["cols"]) == 2 and not f["anti"] for q in qs for f in q["filters"])
    assert any(len(f["cols"]) == 2 and f["anti"] for q in qs for f in q["filters"])
    assert any(len(q["filters"]) == 2 and {f["anti"] for f in q["filters"]} == {True, False} for q in qs)
    assert any(q.get("const") and q["filters"][0]["style"] == "in" for q in qs)
    assert any(q.get("const") == [["k", "is not null"]] and q["filters"][0]["style"] == "not in" for q in qs)
    for q in qs:
        assert q.get("edge") or 0 < q["count"] < GOLD["n_rows"], q["where"]


def test_the_numpy_evaluator_gives_the_references_rows():
    tables = htsemi.fixture_tables(GOLD["seed"], GOLD["n_rows"])
    for q in GOLD["queries"]:
        ids = htsemi.run_query(tables, q)
        assert scanstr.rows_digest(ids) == {"count": q["count"], "sha1": q["sha1"]}, q["where"]


def test_null_rules_of_the_evaluator():
    i32 = lambda *v: np.array(v, np.int32)
    ok = lambda *v: np.array(v, np.uint8)
    # NULL never matches; a repeated key counts once; ANTI keeps the NULL rows
    m = htsemi.matches([i32(1, 2, 3, 4)], [ok(1, 1, 0, 1)], [i32(2, 2, 3, 9)], [ok(1, 1, 1, 0)])
    assert m.tolist() == [False, True, False, False]
    assert htsemi.kept(4, [([i32(1, 2, 3, 4)], [ok(1, 1, 0, 1)], [i32(2, 2, 3, 9)], [ok(1, 1, 1, 0)], True)]).tolist() == [True, False, True, True]
    # NULL = NULL: a NULL row matches iff `by` kept a NULL key
    assert htsemi.matches([i32(1, 7)], [ok(0, 1)], [i32(5, 7)], [ok(0, 1)], null_equal=[True]).tolist() == [True, True]
    assert htsemi.matches([i32(1, 7)], [ok(0, 1)], [i32(5, 7)], [ok(1, 1)], null_equal=[True]).tolist() == [False, True]
    # by value: -1 as int8 is not 255 as uint8, and is -1 as int64; bit for bit it is 255
    a = np.array([-1, 5], np.int8)
    assert htsemi.matches([a], None, [np.array([255, 5], np.uint8)], None, by_value=[True]).tolist() == [False, True]
    assert htsemi.matches([a], None, [np.array([-1], np.int64)], None, by_value=[True]).tolist() == [True, False]
    assert htsemi.matches([a], None, [np.array([255], np.uint8)], None).tolist() == [True, False]
    big = np.array([2 ** 64 - 1], np.uint64)
    assert htsemi.matches([np.array([-1], np.int64)], None, [big], None, by_value=[True]).tolist() == [False]
