"""tests/golden/ssb_q41_varchar.json -- SSB-skew Q4.1 with c_nation a real VARCHAR column, answered by the reference
(tests/golden/make_golden_q41_varchar.py: `rows` on the sample instance, `rows_nulls` with c_nation NULL for every customer
whose c_custkey is a multiple of strref.NULL_EVERY) -- pinned against Python grouping over the ORACLE's join result for
the same instance and against the integer-coded fixture ssb_q41_groupby.json.  The device is checked against the same
fixture in tests/test_gpu_group_varchar.py."""
import os

import common
import strref
from common import GOLDEN, load_golden, orc


def _oracle_columns(gold):
    """(d_year, c_nation code, c_custkey, profit) per row of the oracle's Q4.1 join result on the fixture's instance"""
    from polr_amd import ssb_skew
    wl = ssb_skew.workload("q4.1", **gold["shape"])
    inst = wl["instance"]
    m = inst.lineorder(0, inst.n_lo, cols=["lo_revenue", "lo_supplycost"])
    pcols, pvalid, joins = common.oracle_joins(wl)
    k = len(joins)
    assert wl["joins"][0]["name"] == "customer" and wl["joins"][3]["name"] == "date"
    rows = orc.run_pipeline(pcols, joins, [list(range(k))], routing="default_path")["out_rows"]
    rev, _ = orc.materialize_column(rows, k, -1, m["lo_revenue"], None)
    sup, _ = orc.materialize_column(rows, k, -1, m["lo_supplycost"], None)
    nat, _ = orc.materialize_column(rows, k, 0, wl["joins"][0]["payload"]["c_nation"], None)
    key, _ = orc.materialize_column(rows, k, 0, wl["joins"][0]["keys"][0], None)
    yr, _ = orc.materialize_column(rows, k, 3, wl["joins"][3]["payload"]["d_year"], None)
    return yr.tolist(), nat.tolist(), key.tolist(), [int(r) - int(s) for r, s in zip(rev.tolist(), sup.tolist())]


def _fixture(gold, run):
    got = {(r[0], None if r[1] is None else r[1].encode()): r[2] for r in gold[run]}
    assert len(got) == len(gold[run])  # (no key twice)
    return got


def test_both_runs_equal_python_grouping_over_the_oracle_join():
    gold = load_golden("ssb_q41_varchar")
    assert os.path.getsize(os.path.join(GOLDEN, "ssb_q41_varchar.json")) < 50_000
    assert gold["null_every"] == strref.NULL_EVERY and gold["shape"] == load_golden("ssb_skew_sample")["shape"]
    yr, nat, key, profit = _oracle_columns(gold)
    names = strref.nation_names(nat)
    assert _fixture(gold, "rows") == strref.group_sum(zip(yr, names), profit)
    ok = strref.nation_valid(key).astype(bool).tolist()
    assert _fixture(gold, "rows_nulls") == strref.group_sum(zip(yr, [n if o else None for n, o in zip(names, ok)]), profit)


def test_rows_equal_the_integer_coded_fixture():
    """names mapped back to codes: the very rows of ssb_q41_groupby.json (same instance, same query, c_nation a code)"""
    gold, coded = load_golden("ssb_q41_varchar"), load_golden("ssb_q41_groupby")
    assert gold["shape"] == coded["shape"] and gold["sql"] == coded["sql"]
    back = sorted([r[0], strref.NATION_CODES[r[1].encode()], r[2]] for r in gold["rows"])
    assert back == sorted(coded["rows"])


def test_the_fixture_has_what_it_is_for():
    """names on both sides of the 12-byte inline limit that share a prefix; a NULL-nation group in `rows_nulls`, whose
    profits add up year by year to those of `rows`"""
    gold = load_golden("ssb_q41_varchar")
    names = {r[1].encode() for r in gold["rows"]}
    assert names == set(strref.AMERICA.values())
    assert sum(len(n) > 12 and n.startswith(b"UNITED ST") for n in names) >= 2 and sum(len(n) <= 12 for n in names) >= 2
    assert any(r[1] is None for r in gold["rows_nulls"])
    by_year = lambda rows: strref.group_sum([r[0] for r in rows], [r[2] for r in rows])  # noqa: E731
    assert by_year(gold["rows"]) == by_year(gold["rows_nulls"])
