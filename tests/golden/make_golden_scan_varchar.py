#!/usr/bin/env python3
"""tests/golden/make_golden_scan_varchar.py -- pushed-down VARCHAR comparisons answered by the reference itself: a table
t(id INTEGER, s VARCHAR) of scanstr.FIXTURE_ROWS rows whose strings come from scanstr.fixture_column (seeded: the fixture
stores the seed and the answers, never the strings), NULLs set by an UPDATE.  For every (op, constant) of COMPARISONS, every
pure-prefix pattern of PREFIXES (s LIKE 'x%' and prefix(s, 'x'): the pushed range is the whole predicate) and every range
of RANGES: SELECT id FROM t WHERE ..., recorded as count + SHA-1 of the ascending ids (scanstr.rows_digest); and one
EXPLAIN, which shows whether the filter sat in the scan.  Build container only (oracle/_ref/ref_driver).
Output: tests/golden/scan_varchar.json"""
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
import scanstr  # noqa: E402
from oracle import ref_run  # noqa: E402

CONSTANTS = ["", "J", "Jap", "Japan", "Japanese", "Tok", "tokyo", "Mün", "München", "日本", "日本語", "😀", "char",
             "character-na", "character-nam", "character-name-in-title", "(voice)", "(voice: English version)", "z", "Ünited"]
# every constant with = and <>, and with two of the four inequalities in turn: 80 comparisons
COMPARISONS = [(op, c) for i, c in enumerate(CONSTANTS)
               for op in ("=", "<>", ("<", ">=")[i % 2], (">", "<=")[(i // 2) % 2])]
PREFIXES = [("like", "Jap%"), ("like", "character%"), ("like", "日本%"), ("prefix", "Tok"), ("prefix", "(voice"), ("prefix", "😀")]
RANGES = [((">=", "Jap"), ("<", "Tokyo")), ((">", "character"), ("<=", "日本語"))]


def lit(s):
    return "'" + s.replace("'", "''") + "'"


def main():
    col = scanstr.fixture_column()
    n = len(col)
    null_ids = [i for i, v in enumerate(col) if v is None]
    tables = {"t": {"id": np.arange(n, dtype=np.int32), "s": [v if v is not None else b"" for v in col]}}
    queries = []
    for op, c in COMPARISONS:
        queries.append(({"kind": "cmp", "op": op, "constant": c}, "s %s %s" % (op, lit(c))))
    for kind, p in PREFIXES:
        queries.append(({"kind": kind, "pattern": p}, "s LIKE %s" % lit(p) if kind == "like" else "prefix(s, %s)" % lit(p)))
    for (o1, c1), (o2, c2) in RANGES:
        queries.append(({"kind": "range", "filters": [[o1, c1], [o2, c2]]}, "s %s %s AND s %s %s" % (o1, lit(c1), o2, lit(c2))))
    workdir = tempfile.mkdtemp(prefix="polr_golden_")
    try:
        lines = []
        for name, tcols in tables.items():
            lines += ref_run.table_lines(workdir, name, tcols)
        lines += ["sql SET threads TO 1"]
        for at in range(0, len(null_ids), 200):
            lines.append("sql UPDATE t SET s = NULL WHERE id IN (%s)" % ",".join(map(str, null_ids[at:at + 200])))
        lines.append("query nulls SELECT COUNT(*) FROM t WHERE s IS NULL")
        for i, (_, where) in enumerate(queries):
            lines.append("query q%d SELECT id FROM t WHERE %s ORDER BY id" % (i, where))
        lines.append("query explain EXPLAIN SELECT id FROM t WHERE s LIKE 'Jap%'")
        open(workdir + "/s.txt", "w", encoding="utf-8").write("\n".join(lines) + "\n")
        p = subprocess.run([ref_run.DRIVER, workdir + "/s.txt", workdir + "/out"], capture_output=True, text=True)
        assert p.returncode == 0, p.stdout + p.stderr
        n_null = int(open(workdir + "/out/nulls.csv").read().split()[1])
        assert n_null == len(null_ids), (n_null, len(null_ids))
        out = []
        for i, (desc, where) in enumerate(queries):
            ids = [int(x) for x in open(workdir + "/out/q%d.csv" % i).read().split()[1:]]
            assert ids == sorted(ids)
            out.append(dict(desc, where=where, **scanstr.rows_digest(ids)))
        explain = open(workdir + "/out/explain.csv", encoding="utf-8").read()
    finally:
        shutil.rmtree(workdir, ignore_errors=True)
    gold = {"_provenance": __doc__, "seed": scanstr.FIXTURE_SEED, "n_rows": n, "n_null": n_null,
            "column_sha1": scanstr.column_digest(col),
            "queries": out, "explain": explain}
    json.dump(gold, open(os.path.join(HERE, "scan_varchar.json"), "w"), ensure_ascii=False, indent=0)
    print(len(out), "queries;", n_null, "NULLs; counts", [q["count"] for q in out])
    print(explain)


if __name__ == "__main__":
    main()
