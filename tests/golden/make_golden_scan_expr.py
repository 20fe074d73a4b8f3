#!/usr/bin/env python3
"""tests/golden/make_golden_scan_expr.py -- filter expressions behind the scan (OR / NOT trees, IN lists, LIKE) answered by
the reference itself: a table t(id INTEGER, s VARCHAR, i INTEGER) of scanstr.FIXTURE_ROWS rows, s from
scanstr.fixture_column and i from scanexpr.fixture_int (seeded: the fixture stores the seeds and the answers, never the
strings), the NULLs of both set by UPDATE.  For every expression of QUERIES: SELECT id FROM t WHERE ..., recorded as the
expression, its SQL text, and count + SHA-1 of the ascending ids (scanstr.rows_digest).  Every count must be neither 0 nor
the whole table except where the query says so ("edge"); the queries marked "kleene" must have rows whose root is NULL --
rows a two-valued reading (NULL as FALSE) would answer differently.  Build container only (oracle/_ref/ref_driver).
Output: tests/golden/scan_expr.json"""
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
import scanexpr  # noqa: E402
import scanstr  # noqa: E402
from oracle import ref_run  # noqa: E402

PATTERNS = ["%", "%%", "", "_", "%_", "__%", "Jap%", "Japan", "J_pan%", "J%a", "%a", "%a%", "%語%", "%日本%", "M_nchen%",
            "M__nchen%", "T_k%", "%😀", "%😀%😁%", "%ab%b", "%a_b%", "%z%z%", "char%title", "character-name%", "%-name-%",
            "%in-title%", "(voice: English version)", "%(voice%)%"]
EDGE = {("not like", "%"), ("not like", "%%"),  # none: every non-NULL row matches
        ("like", "M_nchen%")}                   # none: the ü of München is two bytes, and _ is one
S3 = ["Japan", "Tokyo", "(voice)"]
S8 = S3 + ["", "J", "日本語", "(uncredited)", "character-name-in-title"]
I3 = [1, 50, 99]
I8 = I3 + [0, 7, 13, 64, 98]


def queries():
    q = []
    for p in PATTERNS:
        q.append({"expr": ["like", "s", p], "edge": ("like", p) in EDGE})
        q.append({"expr": ["not", ["like", "s", p]], "edge": ("not like", p) in EDGE})
    for members in (S3[:1], S3, S8):
        q.append({"expr": ["in", "s", members]})
        q.append({"expr": ["not", ["in", "s", members]]})
    for members in (I3[:1], I3, I8):
        q.append({"expr": ["in", "i", members]})
        q.append({"expr": ["not", ["in", "i", members]]})
    q.append({"expr": ["or", ["like", "s", "%(voice%"], ["like", "s", "%語%"]]})
    q.append({"expr": ["or", ["like", "s", "Jap%a"], ["like", "s", "%😀"]]})
    q.append({"expr": ["or", ["cmp", "s", "is null"], ["like", "s", "Tok%"]]})
    q.append({"expr": ["or", ["cmp", "s", "is null"], ["not", ["like", "s", "%a%"]]]})
    q.append({"expr": ["not", ["and", ["cmp", "s", "=", "Japan"], ["cmp", "i", "<", 50]]], "kleene": True})
    q.append({"expr": ["not", ["or", ["like", "s", "Jap%"], ["in", "i", I8]]], "kleene": True})
    q.append({"expr": ["and", ["cmp", "s", ">=", "J"], ["or", ["cmp", "i", "<", 20], ["cmp", "i", "is null"]]]})
    q.append({"expr": ["or", ["and", ["cmp", "s", "<>", "Japan"], ["cmp", "i", ">=", 90]], ["not", ["cmp", "i", "is not null"]]],
              "kleene": True})
    # the shape of JOB 19a: an IN list, an OR of two LIKEs, a NOT LIKE and a range over two columns
    q.append({"expr": ["and", ["in", "s", ["(voice)", "(voice: English version)", "(uncredited)", "Japan", "Japanese"]],
                       ["or", ["like", "s", "%(voice%"], ["like", "s", "Jap%"]],
                       ["not", ["like", "s", "%English%"]],
                       ["cmp", "i", ">=", 20], ["cmp", "i", "<=", 80]]})
    return q


def lit(c):
    return str(c) if isinstance(c, int) else "'" + c.replace("'", "''") + "'"


def sql_of(e):
    kind = e[0]
    if kind == "not":
        if e[1][0] == "like":
            return "%s NOT LIKE %s" % (e[1][1], lit(e[1][2]))
        if e[1][0] == "in":
            return "%s NOT IN (%s)" % (e[1][1], ", ".join(lit(m) for m in e[1][2]))
        return "NOT (%s)" % sql_of(e[1])
    if kind in ("and", "or"):
        return "(" + (" %s " % kind.upper()).join(sql_of(x) for x in e[1:]) + ")"
    if kind == "cmp":
        return "%s %s" % (e[1], e[2].upper()) if len(e) == 3 else "%s %s %s" % (e[1], e[2], lit(e[3]))
    if kind == "in":
        return "%s IN (%s)" % (e[1], ", ".join(lit(m) for m in e[2]))
    return "%s LIKE %s" % (e[1], lit(e[2]))


def main():
    col = scanstr.fixture_column()
    ints, ivalid = scanexpr.fixture_int()
    n = len(col)
    s_null = [i for i, v in enumerate(col) if v is None]
    i_null = np.nonzero(ivalid == 0)[0].tolist()
    tables = {"t": {"id": np.arange(n, dtype=np.int32), "s": [v if v is not None else b"" for v in col], "i": ints}}
    qs = queries()
    workdir = tempfile.mkdtemp(prefix="polr_golden_")
    try:
        lines = []
        for name, tcols in tables.items():
            lines += ref_run.table_lines(workdir, name, tcols)
        lines += ["sql SET threads TO 1"]
        for cname, ids in (("s", s_null), ("i", i_null)):
            for at in range(0, len(ids), 200):
                lines.append("sql UPDATE t SET %s = NULL WHERE id IN (%s)" % (cname, ",".join(map(str, ids[at:at + 200]))))
        lines.append("query nulls SELECT COUNT(*) FROM t WHERE s IS NULL")
        lines.append("query inulls SELECT COUNT(*) FROM t WHERE i IS NULL")
        for i, q in enumerate(qs):
            q["where"] = sql_of(q["expr"])
            lines.append("query q%d SELECT id FROM t WHERE %s ORDER BY id" % (i, q["where"]))
        open(workdir + "/s.txt", "w", encoding="utf-8").write("\n".join(lines) + "\n")
        p = subprocess.run([ref_run.DRIVER, workdir + "/s.txt", workdir + "/out"], capture_output=True, text=True)
        assert p.returncode == 0, p.stdout + p.stderr
        n_null = int(open(workdir + "/out/nulls.csv").read().split()[1])
        n_inull = int(open(workdir + "/out/inulls.csv").read().split()[1])
        assert (n_null, n_inull) == (len(s_null), len(i_null))
        out = []
        cols = {"s": col, "i": (ints, ivalid)}
        for i, q in enumerate(qs):
            ids = [int(x) for x in open(workdir + "/out/q%d.csv" % i).read().split()[1:]]
            assert ids == sorted(ids)
            assert q.get("edge") or 0 < len(ids) < n, (q["where"], len(ids))
            if q.get("kleene"):
                _, null = scanexpr.evaluate(scanexpr.bind(q["expr"], {"s": "s", "i": "i"}), cols)
                assert null.sum() > 0, q["where"]
            out.append(dict(q, **scanstr.rows_digest(ids)))
    finally:
        shutil.rmtree(workdir, ignore_errors=True)
    gold = {"_provenance": __doc__, "seed": scanstr.FIXTURE_SEED, "int_seed": scanstr.FIXTURE_SEED + 1, "n_rows": n,
            "n_null": n_null, "n_int_null": n_inull, "column_sha1": scanstr.column_digest(col), "queries": out}
    json.dump(gold, open(os.path.join(HERE, "scan_expr.json"), "w"), ensure_ascii=False, indent=0)
    print(len(out), "queries;", n_null, "+", n_inull, "NULLs; counts", [q["count"] for q in out])


if __name__ == "__main__":
    main()
