#!/usr/bin/env python3
"""tests/golden/make_golden_q41_varchar.py -- SSB-skew Q4.1 as the reference ships it (benchmark/ssb-skew/queries/q4-1.sql:
SELECT d_year, c_nation, SUM(lo_revenue - lo_supplycost) AS profit ... GROUP BY d_year, c_nation) on the sample instance
of tests/golden/ssb_skew_sample.json with c_nation A REAL VARCHAR COLUMN (names: tests/strref.py), answered by the
reference itself with POLAR on (join_enumerator sample, max_join_orders 3, adaptive_reinit; the settings of
make_golden_q41_groupby.py).  Two runs: `rows` on the instance as it is, and `rows_nulls` after c_nation was set to NULL
for every customer whose c_custkey is a multiple of strref.NULL_EVERY, so that the reference's NULL group is in the
answer.  Build container only.  Output: tests/golden/ssb_q41_varchar.json"""
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
import make_golden_ssb_skew as g  # noqa: E402
import strref  # noqa: E402
from make_golden_q41_groupby import SQL  # noqa: E402
from oracle import ref_run  # noqa: E402
from polr_amd import ssb_skew  # noqa: E402


def parse(path):
    rows = []
    for line in open(path).read().strip().splitlines()[1:]:
        y, nation, profit = line.split(",")
        rows.append([int(y), None if nation == "NULL" else nation, int(profit)])
    return rows


def main():
    wl = ssb_skew.workload("q4.1", **g.SHAPE)
    inst = wl["instance"]
    cols = inst.lineorder(0, inst.n_lo, cols=list(ssb_skew.PROBE_COLS) + ["lo_revenue", "lo_supplycost"])
    for c in ("lo_revenue", "lo_supplycost"):  # (INTEGER columns in SSB: the difference may be negative)
        cols[c] = cols[c].astype(np.int32)
    ref = ssb_skew.reference_form(inst, "q4.1", cols)
    ref["tables"]["customer"]["c_nation"] = strref.nation_names(inst.c_nation)  # (a list of bytes: loaded as VARCHAR)
    workdir = tempfile.mkdtemp(prefix="polr_golden_")
    try:
        lines = []
        for name, tcols in ref["tables"].items():
            lines += ref_run.table_lines(workdir, name, tcols, pk=ref["pk"].get(name))
        lines += ["sql SET threads TO 1"] + ["sql " + s for s in ref["settings"]]
        lines += ["sql PRAGMA enable_polr", "sql SET join_enumerator TO 'sample'", "sql SET max_join_orders TO 3",
                  "sql SET multiplexer_routing TO 'adaptive_reinit'", "query q " + SQL,
                  "sql UPDATE customer SET c_nation = NULL WHERE c_custkey %% %d = 0" % strref.NULL_EVERY,
                  "query q_nulls " + SQL]
        open(workdir + "/s.txt", "w").write("\n".join(lines) + "\n")
        p = subprocess.run([ref_run.DRIVER, workdir + "/s.txt", workdir + "/out"], capture_output=True, text=True)
        assert p.returncode == 0, p.stdout + p.stderr
        rows, rows_nulls = parse(workdir + "/out/q.csv"), parse(workdir + "/out/q_nulls.csv")
    finally:
        shutil.rmtree(workdir, ignore_errors=True)
    gold = {"_provenance": __doc__, "shape": g.SHAPE, "sql": SQL, "null_every": strref.NULL_EVERY,
            "columns": ["d_year", "c_nation", "profit"], "rows": rows, "rows_nulls": rows_nulls}
    json.dump(gold, open(os.path.join(HERE, "ssb_q41_varchar.json"), "w"), separators=(",", ":"))
    print(len(rows), "groups;", len(rows_nulls), "with NULLs; first", rows[:3], "NULL rows",
          [r for r in rows_nulls if r[1] is None][:3])


if __name__ == "__main__":
    main()
