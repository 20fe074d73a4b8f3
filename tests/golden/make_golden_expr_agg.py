#!/usr/bin/env python3
"""Golden answers for aggregates whose ARGUMENT is a product, sum or difference of two columns (polr_out_aggregate*_expr),
produced by the REFERENCE itself (oracle/_ref, compiled from its own sources) -> tests/golden/expr_aggregates.json.

Every value is parsed from the driver's CSV text into a Python int (never through a float); for every expression the
fixture keeps typeof(expr) as the reference's binder reports it -- the tests hand that type to the device.

  flight1     SSB Q1.1 - Q1.3 as shipped (workloads.ssb_flight1): SUM / MIN / MAX / COUNT of lo_extendedprice * lo_discount,
              COUNT(*), and the rows the pushed-down probe filters keep
  q41         SSB-skew Q4.1's star join (workloads.ssb_skew_q41(sf=0.2)), lo_revenue and lo_supplycost loaded as INTEGER,
              GROUP BY d_year, c_nation: SUM / MIN / MAX / COUNT of the difference, SUM of the sum and of the product
  q41_error   the same query with the measures loaded as UINTEGER -- what the workload's arrays are --, in a driver run
              of its own: the reference refuses it (exit status and stderr are kept)
  nulls       star_skew_nulls (make_golden.py): (probe column, build payload column) pairs, COUNT / SUM / MIN / MAX of the
              product and of the difference.  The payload columns p<d> hold NULLs; the probe columns with NULLs are the
              join keys, whose NULL rows never reach the output.  A pair whose expression the reference binds to
              anything but an integer of at most 8 bytes is recorded as "unsupported"; an expression the reference
              refuses for a row out of range keeps the error text instead of values.

Run here only (the reference does not travel):  python tests/golden/make_golden_expr_agg.py
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
from polr_amd import workloads  # noqa: E402

INT_TYPES = {"TINYINT", "UTINYINT", "SMALLINT", "USMALLINT", "INTEGER", "UINTEGER", "BIGINT", "UBIGINT"}
FNS = ("sum", "min", "max", "count")


def cell(text):
    """one CSV cell -> python int, None for NULL, the text itself for anything else (a type name)"""
    text = text.strip()
    if text == "NULL" or text == "":
        return None
    try:
        return int(text)
    except ValueError:
        return text


def read_csv(path):
    return [[cell(c) for c in line.split(",")] for line in open(path).read().strip().splitlines()[1:]]


def run_driver(lines, workdir, tag="s"):
    """one driver run of its own -> (exit status, stderr, out directory)"""
    script = os.path.join(workdir, tag + ".txt")
    open(script, "w").write("\n".join(lines) + "\n")
    outdir = os.path.join(workdir, "out_" + tag)
    proc = subprocess.run([mg.DRIVER, script, outdir], capture_output=True, text=True)
    return proc.returncode, proc.stderr, outdir


def must(rc, err, what):
    if rc != 0:
        raise RuntimeError("%s: the reference driver failed (%d): %s" % (what, rc, err))


def typeof_lines(tag, left, right, ops, frm):
    """driver commands asking the binder for typeof(left OP right), OP in ops -> <tag>.csv.  typeof() evaluates its argument,
    and the argument may be out of range for the data: asked over a one-row table of the operands' types holding (1, 1)"""
    return ["sql CREATE TABLE %s_tt AS SELECT %s AS a, %s AS b FROM %s LIMIT 0" % (tag, left, right, frm),
            "sql INSERT INTO %s_tt VALUES (1, 1)" % tag,
            "query %s SELECT %s FROM %s_tt" % (tag, ", ".join("typeof(a %s b)" % op for op in ops), tag)]


def make_flight1(workdir):
    wl = workloads.ssb_flight1()
    load = []
    mg.table_script(load, workdir, "lineorder", wl["probe"]["cols"])
    mg.table_script(load, workdir, "date", wl["date_full"])
    expr = "lo_extendedprice * lo_discount"
    gold = {"expr": expr, "aggregates": list(FNS) + ["count_star"], "queries": {}}
    lines = load + ["sql SET threads TO 1", "sql PRAGMA enable_polr"]
    for name, q in wl["queries"].items():
        tag = name.replace(".", "_")
        probe_where = " AND ".join("%s %s %d" % f for f in q["filter"])
        lines += ["query %s SELECT %s, count(*) FROM lineorder JOIN date ON lo_orderdate = d_datekey WHERE %s" %
                  (tag, ", ".join("%s(%s)" % (fn, expr) for fn in FNS), q["sql_where"]),
                  "query f_%s SELECT count(*) FROM lineorder WHERE %s" % (tag, probe_where)]
    lines += typeof_lines("t", "lo_extendedprice", "lo_discount", "*", "lineorder")
    rc, err, outdir = run_driver(lines, workdir, "flight1")
    must(rc, err, "flight1")
    gold["typeof"] = read_csv(os.path.join(outdir, "t.csv"))[0][0]
    for name, q in wl["queries"].items():
        tag = name.replace(".", "_")
        gold["queries"][name] = {"sql_where": q["sql_where"], "values": read_csv(os.path.join(outdir, tag + ".csv"))[0],
                                 "filtered_rows": read_csv(os.path.join(outdir, "f_%s.csv" % tag))[0][0]}
    return gold


Q41_EXPRS = [("sum", "-"), ("min", "-"), ("max", "-"), ("count", "-"), ("sum", "+"), ("sum", "*")]


def q41_script(workdir, wl, dtype):
    """the load commands and the GROUP BY query with lo_revenue / lo_supplycost loaded as `dtype`; settings as in
    make_golden_agg.make_ssb_q41_groups"""
    cols = dict(wl["probe"]["cols"])
    for c in ("lo_revenue", "lo_supplycost"):
        cols[c] = cols[c].astype(dtype)
    lines = []
    mg.table_script(lines, workdir, wl["probe"]["name"], cols)
    for j in wl["joins"]:
        jc = {kn: kk for kn, kk in zip(j["key_names"], j["keys"])}
        jc.update(j["payload"])
        mg.table_script(lines, workdir, j["name"], jc)
    select = "d_year, c_nation, count(*), " + ", ".join("%s(lo_revenue %s lo_supplycost)" % e for e in Q41_EXPRS)
    query = mg.workload_sql(wl, select)[0] + " GROUP BY d_year, c_nation ORDER BY d_year, c_nation"
    lines += ["sql SET threads TO 1", "sql SET disabled_optimizers TO 'join_order'", "sql PRAGMA enable_polr",
              "sql SET join_enumerator TO 'dfs_min_card'", "sql SET max_join_orders TO 3"]
    return lines, query


def make_q41(workdir):
    wl = workloads.ssb_skew_q41(sf=0.2)
    lines, query = q41_script(workdir, wl, np.int32)
    lines.append("query q " + query)
    lines += typeof_lines("t", "lo_revenue", "lo_supplycost", "-+*", "lineorder")
    rc, err, outdir = run_driver(lines, workdir, "q41")
    must(rc, err, "q41")
    types = read_csv(os.path.join(outdir, "t.csv"))[0]
    gold = {"operand_type": "INTEGER", "typeof": dict(zip("-+*", types)),
            "columns": ["d_year", "c_nation", "count_star"] + ["%s(%s)" % e for e in Q41_EXPRS],
            "rows": read_csv(os.path.join(outdir, "q.csv"))}
    # the error: the same query over the measures as the workload has them, in a run of its own
    lines, query = q41_script(workdir, wl, np.uint32)
    tlines = lines + typeof_lines("t", "lo_revenue", "lo_supplycost", "-+*", "lineorder")
    rc, err, outdir = run_driver(tlines, workdir, "q41_types")
    must(rc, err, "q41 types")
    utypes = read_csv(os.path.join(outdir, "t.csv"))[0]
    rc, err, _ = run_driver(lines + ["query q " + query], workdir, "q41_error")
    error = {"operand_type": "UINTEGER", "typeof": dict(zip("-+*", utypes)), "exit_status": rc, "stderr": err.strip()}
    return gold, error


NULL_PAIRS = [("id", 1, "p1"), ("k1", 1, "p1"), ("k1", 2, "p2"), ("id", 0, "p0")]  # (probe column, join, payload column)


def make_nulls(workdir):
    wl = mg.SCENARIOS["star_skew_nulls"]()
    load = []
    mg.table_script(load, workdir, wl["probe"]["name"], wl["probe"]["cols"], wl["probe"].get("valid"))
    for j in wl["joins"]:
        cols = {kn: k for kn, k in zip(j["key_names"], j["keys"])}
        cols.update(j["payload"])
        valid = {kn: v for kn, v in zip(j["key_names"], j.get("key_valid", []))}
        valid.update(j.get("payload_valid", {}))
        mg.table_script(load, workdir, j["name"], cols, valid)
    settings = ["sql SET threads TO 1", "sql SET disabled_optimizers TO 'join_order'", "sql PRAGMA enable_polr",
                "sql SET join_enumerator TO 'each_last_once'", "sql SET max_join_orders TO 8"]
    frm = mg.workload_sql(wl, "count(*)")[0].split(" FROM ", 1)[1]
    pairs = []
    for pcol, join, bcol in NULL_PAIRS:
        left, right = "fact.%s" % pcol, "%s.%s" % (wl["joins"][join]["name"], bcol)
        rec = {"probe_col": pcol, "join": join, "build_col": bcol, "exprs": {}}
        for op in "*-":
            expr = "%s %s %s" % (left, op, right)
            # every expression in a run of its own: the reference may refuse it
            rc, err, outdir = run_driver(load + settings + typeof_lines("t", left, right, op, frm), workdir, "nt")
            must(rc, err, "typeof " + expr)
            typ = read_csv(os.path.join(outdir, "t.csv"))[0][0]
            shutil.rmtree(outdir, ignore_errors=True)
            if typ not in INT_TYPES:
                rec["exprs"][op] = {"typeof": typ, "unsupported": True}
                continue
            rc, err, outdir = run_driver(load + settings + [
                "query q SELECT count(*), %s FROM %s" % (", ".join("%s(%s)" % (fn, expr) for fn in ("count",) + FNS[:3]), frm)],
                workdir, "nq")
            if rc != 0:
                rec["exprs"][op] = {"typeof": typ, "exit_status": rc, "stderr": err.strip()}
            else:
                v = read_csv(os.path.join(outdir, "q.csv"))[0]
                rec["exprs"][op] = {"typeof": typ, "count_star": v[0], "count": v[1], "sum": v[2], "min": v[3], "max": v[4]}
            shutil.rmtree(outdir, ignore_errors=True)
        pairs.append(rec)
        print("nulls", rec)
    return pairs


def main():
    if not os.path.exists(mg.DRIVER):
        raise RuntimeError("reference driver missing: make -f oracle/ref_build.mk")
    workdir = tempfile.mkdtemp(prefix="polr_golden_")
    try:
        gold = {"flight1": make_flight1(workdir)}
        print("flight1", gold["flight1"])
        gold["q41"], gold["q41_error"] = make_q41(workdir)
        print("q41", len(gold["q41"]["rows"]), "groups", gold["q41"]["typeof"], gold["q41"]["rows"][0])
        print("q41_error", gold["q41_error"])
        gold["nulls"] = make_nulls(workdir)
    finally:
        shutil.rmtree(workdir, ignore_errors=True)
    path = os.path.join(HERE, "expr_aggregates.json")
    json.dump(gold, open(path, "w"), indent=1)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
