"""Pushed-down VARCHAR filters, the part that needs no GPU: the tests' own reference (Python's bytes comparison over the
regenerated column of tests/scanstr.py) against what the reference engine answered (tests/golden/scan_varchar.json, made
by tests/golden/make_golden_scan_varchar.py), the LIKE rewrite of capi.like_pushdown through the same Python reference, and
the declarations of the entry point in header, library and binding."""
import json
import os
import re

import pytest

import common
import scanstr
from polr_amd import capi

GOLD = json.load(open(os.path.join(common.ROOT, "tests", "golden", "scan_varchar.json"), encoding="utf-8"))


@pytest.fixture(scope="module")
def column():
    col = scanstr.fixture_column(GOLD["seed"], GOLD["n_rows"])
    assert scanstr.column_digest(col) == GOLD["column_sha1"], "the seeded generator no longer makes the fixture's column"
    assert sum(v is None for v in col) == GOLD["n_null"]
    return col


def filters_of(q):
    """the pushed-down filters [(op, constant)] of a fixture query"""
    if q["kind"] == "cmp":
        return [(q["op"], q["constant"].encode())]
    if q["kind"] == "range":
        return [(op, c.encode()) for op, c in q["filters"]]
    return capi.like_pushdown(q["pattern"].encode() + (b"%" if q["kind"] == "prefix" else b""))


def test_fixture_covers_what_the_issue_asks():
    kinds = [q["kind"] for q in GOLD["queries"]]
    assert kinds.count("cmp") >= 40 and kinds.count("like") + kinds.count("prefix") == 6 and kinds.count("range") == 2
    assert {q["op"] for q in GOLD["queries"] if q["kind"] == "cmp"} == set(scanstr.OPS)
    assert "Filters: s>=Jap AND s<Jaq" in GOLD["explain"]  # the reference evaluated the range inside its scan


def test_python_bytes_comparison_is_the_reference_order(column):
    for q in GOLD["queries"]:
        if q["kind"] in ("cmp", "range"):
            got = scanstr.rows_digest(scanstr.passing(column, filters_of(q)))
            assert got == {"count": q["count"], "sha1": q["sha1"]}, q["where"]


def test_like_pushdown_is_the_whole_predicate_for_prefix_patterns(column):
    for q in GOLD["queries"]:
        if q["kind"] in ("like", "prefix"):
            f = filters_of(q)
            assert [op for op, _ in f] == [">=", "<", "is not null"]
            got = scanstr.rows_digest(scanstr.passing(column, f))
            assert got == {"count": q["count"], "sha1": q["sha1"]}, q["where"]


def test_like_pushdown_restates_the_filter_combiner():
    lp = capi.like_pushdown
    assert lp(b"%abc") == [] and lp(b"_bc%") == []
    assert lp(b"abc") == [("=", b"abc"), ("is not null", None)]
    assert lp(b"abc%") == [(">=", b"abc"), ("<", b"abd"), ("is not null", None)]
    assert lp(b"ab_d%x") == [(">=", b"ab"), ("<", b"ac"), ("is not null", None)]
    assert lp("Mün%") == [(">=", "Mün".encode()), ("<", "Mün".encode()[:-1] + b"o"), ("is not null", None)]
    assert lp(b"a\xfe%")[1] == ("<", b"a\xff")
    with pytest.raises(ValueError):
        lp(b"a\xff%")


def test_header_library_and_binding_declare_the_entry_point():
    header = open(os.path.join(common.ROOT, "include", "polr_hip.h")).read()
    lib = capi.load()
    name = "polr_pipeline_scan_filter_str"
    assert re.search(r"\bint\s+%s\s*\(" % name, header)
    assert name in capi.EXPORTS and hasattr(lib, name)
    assert re.search(r"#define\s+POLR_MAX_FILTER_STRING\s+4096\b", header) and capi.MAX_FILTER_STRING == 4096
    fields = re.search(r"typedef struct polr_scan_filter_str \{(.*?)\} polr_scan_filter_str;", header, re.S).group(1)
    assert re.findall(r"\b(\w+);", fields) == [f[0] for f in capi.ScanFilterStr._fields_]
