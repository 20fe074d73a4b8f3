#!/usr/bin/env python3
"""tests/golden/make_golden_semi_build.py -- a dimension restricted by subqueries (k IN (SELECT ...), EXISTS, NOT EXISTS: the
SEMI / ANTI / MARK hash joins inside a build subtree) answered by the reference itself: the tables of htsemi.fixture_tables
(seeded: the fixture stores the seed, a digest of the tables and the answers) -- d(id, k, k2, s) with NULL keys set by
UPDATE, a(x, y) with repeated keys and one NULL key, b(x, y) NULL-free with unique keys.  For every query of QUERIES:
SELECT id FROM d WHERE ..., recorded as its spec (what tests/htsemi.py and the device evaluate), its SQL text, and count +
SHA-1 of the ascending ids (scanstr.rows_digest).  Every count must be neither 0 nor the whole table except where the query
says so ("edge").  Build container only (oracle/_ref/ref_driver).
Output: tests/golden/semi_build.json"""
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import htsemi  # noqa: E402
import scanstr  # noqa: E402
from oracle import ref_run  # noqa: E402


def f(by, cols, by_cols, style, anti=False, by_where=None):
    spec = {"by": by, "cols": cols, "by_cols": by_cols, "style": style, "anti": anti}
    if by_where:
        spec["by_where"] = by_where
    return spec


QUERIES = [
    {"filters": [f("a", ["k"], ["x"], "in")]},
    {"filters": [f("b", ["k"], ["x"], "in")]},
    {"filters": [f("a", ["k"], ["x"], "in", by_where=[["y", "<", 10]])]},
    {"filters": [f("a", ["k"], ["x"], "exists")]},
    {"filters": [f("a", ["k"], ["x"], "exists", anti=True)]},
    {"filters": [f("b", ["k2"], ["y"], "exists", anti=True, by_where=[["x", "<", 150]])]},
    {"filters": [f("a", ["k", "k2"], ["x", "y"], "exists")]},
    {"filters": [f("a", ["k", "k2"], ["x", "y"], "exists", anti=True)]},
    {"filters": [f("b", ["k"], ["x"], "in"), f("a", ["k"], ["x"], "exists", anti=True)]},
    {"filters": [f("a", ["k"], ["x"], "in"), f("b", ["k2"], ["y"], "exists", by_where=[["x", "<", 40]])]},
    {"const": [["k2", "<", 12]], "filters": [f("a", ["k"], ["x"], "in")]},
    {"const": [["k2", ">=", 5], ["id", "<", 1500]], "filters": [f("b", ["k"], ["x"], "exists", anti=True)]},
    {"const": [["k", "is not null"]], "filters": [f("b", ["k"], ["x"], "not in", anti=True)]},
    {"const": [["k", "is not null"]], "filters": [f("b", ["k"], ["x"], "not in", anti=True, by_where=[["y", ">=", 10]])]},
    {"filters": [f("a", ["k"], ["x"], "in", by_where=[["y", "<", 0]])], "edge": True},                  # an empty subquery: none
    {"filters": [f("a", ["k"], ["x"], "exists", anti=True, by_where=[["y", "<", 0]])], "edge": True},  # ... and all
]


def conds_sql(table, conds):
    return ["%s.%s %s" % (table, c[0], "IS NOT NULL" if c[1] == "is not null" else "%s %d" % (c[1], c[2])) for c in conds]


def filter_sql(s):
    by, where = s["by"], conds_sql(s["by"], s.get("by_where", []))
    if s["style"] in ("in", "not in"):
        assert len(s["cols"]) == 1 and s["anti"] == (s["style"] == "not in")
        sub = "SELECT %s.%s FROM %s%s" % (by, s["by_cols"][0], by, " WHERE " + " AND ".join(where) if where else "")
        return "d.%s %s (%s)" % (s["cols"][0], s["style"].upper(), sub)
    on = ["%s.%s = d.%s" % (by, bc, c) for c, bc in zip(s["cols"], s["by_cols"])]
    return "%sEXISTS (SELECT 1 FROM %s WHERE %s)" % ("NOT " if s["anti"] else "", by, " AND ".join(on + where))


def sql_of(q):
    return " AND ".join(conds_sql("d", q.get("const", [])) + [filter_sql(s) for s in q["filters"]])


def main():
    tables = htsemi.fixture_tables()
    n = len(tables["d"]["id"][0])
    workdir = tempfile.mkdtemp(prefix="polr_golden_")
    try:
        lines = []
        for name, t in tables.items():
            lines += ref_run.table_lines(workdir, name, {c: v[0] for c, v in t.items()})
        lines += ["sql SET threads TO 1"]
        n_null = {}
        for name, t in tables.items():
            key = "id" if name == "d" else None
            for cname, (_values, valid) in t.items():
                rows = np.nonzero(np.asarray(valid) == 0)[0].tolist()
                n_null["%s.%s" % (name, cname)] = len(rows)
                if not rows:
                    continue
                if key:
                    for at in range(0, len(rows), 200):
                        lines.append("sql UPDATE %s SET %s = NULL WHERE %s IN (%s)" % (name, cname, key, ",".join(map(str, rows[at:at + 200]))))
                else:  # (no row id column: the subquery tables name the row by its cells -- unique, asserted below)
                    for r in rows:
                        others = [c for c in t if c != cname]
                        cells = tuple(int(t[c][0][r]) for c in [cname] + others)
                        same = [i for i in range(len(valid)) if tuple(int(t[c][0][i]) for c in [cname] + others) == cells]
                        assert same == [r], (name, cname, r, same)
                        lines.append("sql UPDATE %s SET %s = NULL WHERE %s" % (
                            name, cname, " AND ".join("%s = %d" % (c, v) for c, v in zip([cname] + others, cells))))
        for key_, cnt in n_null.items():
            t_, c_ = key_.split(".")
            lines.append("query nulls_%s_%s SELECT COUNT(*) FROM %s WHERE %s IS NULL" % (t_, c_, t_, c_))
        out = []
        for i, q in enumerate(QUERIES):
            q = dict(q, where=sql_of(q))
            out.append(q)
            lines.append("query q%d SELECT d.id FROM d WHERE %s ORDER BY d.id" % (i, q["where"]))
        open(workdir + "/s.txt", "w", encoding="utf-8").write("\n".join(lines) + "\n")
        p = subprocess.run([ref_run.DRIVER, workdir + "/s.txt", workdir + "/out"], capture_output=True, text=True)
        assert p.returncode == 0, p.stdout + p.stderr
        for key_, cnt in n_null.items():
            t_, c_ = key_.split(".")
            assert int(open(workdir + "/out/nulls_%s_%s.csv" % (t_, c_)).read().split()[1]) == cnt, key_
        for i, q in enumerate(out):
            ids = [int(x) for x in open(workdir + "/out/q%d.csv" % i).read().split()[1:]]
            assert ids == sorted(ids)
            assert q.get("edge") or 0 < len(ids) < n, (q["where"], len(ids))
            q.update(scanstr.rows_digest(ids))
    finally:
        shutil.rmtree(workdir, ignore_errors=True)
    gold = {"_provenance": __doc__, "seed": htsemi.FIXTURE_SEED, "n_rows": n, "n_null": n_null,
            "tables_sha1": htsemi.tables_digest(tables), "queries": out}
    json.dump(gold, open(os.path.join(HERE, "semi_build.json"), "w"), ensure_ascii=False, indent=0)
    print(len(out), "queries; NULLs", n_null, "; counts", [q["count"] for q in out])


if __name__ == "__main__":
    main()
