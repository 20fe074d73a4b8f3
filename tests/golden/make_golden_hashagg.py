#!/usr/bin/env python3
"""tests/golden/make_golden_hashagg.py -- the general GROUP BY answered by the REFERENCE itself: tests/joinref.HASHAGG_SQL
(SELECT g1, g2, COUNT(*), COUNT(x), SUM(x), MIN(x), MAX(x) FROM fact JOIN dim ON fk = dk GROUP BY g1, g2) over
tests/joinref.hashagg_inputs(**shape).  The group values are wide and sparse (about +-10^12): the reference plans a hash
aggregate, not a perfect-hash one; both group columns hold NULLs (loaded through the staging table of
make_golden.table_script), and SUM(x) leaves the int64 range on both sides (HUGEINT).  Build container only.
Output: tests/golden/hash_groupby.json"""
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
from joinref import HASHAGG_SQL, hashagg_inputs  # noqa: E402

SHAPE = {"seed": 2027, "n_fact": 20000, "n_dim": 600}


def main():
    fact, fact_valid, dim, dim_valid = hashagg_inputs(**SHAPE)
    workdir = tempfile.mkdtemp(prefix="polr_golden_")
    try:
        lines = []
        mg.table_script(lines, workdir, "fact", fact, fact_valid)
        mg.table_script(lines, workdir, "dim", dim, dim_valid)
        lines += ["sql SET threads TO 1", "sql PRAGMA enable_polr", "query q " + HASHAGG_SQL]
        open(os.path.join(workdir, "s.txt"), "w").write("\n".join(lines) + "\n")
        p = subprocess.run([mg.DRIVER, os.path.join(workdir, "s.txt"), os.path.join(workdir, "out")], capture_output=True,
                           text=True)
        assert p.returncode == 0, p.stdout + p.stderr
        text = open(os.path.join(workdir, "out", "q.csv")).read().strip().splitlines()[1:]
    finally:
        shutil.rmtree(workdir, ignore_errors=True)
    rows = [[None if v == "NULL" else int(v) for v in line.split(",")] for line in text]
    gold = {"_provenance": __doc__, "shape": SHAPE, "sql": HASHAGG_SQL,
            "columns": ["g1", "g2", "count_star", "count_x", "sum_x", "min_x", "max_x"], "rows": rows}
    with open(os.path.join(HERE, "hash_groupby.json"), "w") as f:
        json.dump(gold, f, separators=(",", ":"))
    print(len(rows), "groups; sums from", min(r[4] for r in rows if r[4] is not None), "to",
          max(r[4] for r in rows if r[4] is not None))


if __name__ == "__main__":
    main()
