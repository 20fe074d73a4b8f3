"""What tests/test_job_chain.py and the whole-query GPU tests share: the four long JOB shapes they run, the instance they run
them on, the direct numpy join of ALL tables of a query (no stages, no cut; n_joins: only
the first so many joins), and one pipeline through the oracle."""
import numpy as np

from common import orc
from joinref import Join
from polr_amd import job_family

# One shape each of 10, 12, 14 and 17 tables.  The instance -- SCALE 0.002 (tables of 1000 to 72 000 rows), SEED 1337 and a
# selectivity floor of 0.8 (chain_data: the family's own selectivities, multiplied over a dozen tables of a thousand rows,
# leave no row) -- was chosen ON THE CPU, from the numpy reference alone (direct_join below), so that for each of the four
# shapes COUNT(*) >= 1 and every non-final stage emits more than CHUNK rows, i.e. its output spans at least two output
# chunks of the capacity the chain runner uses.  The reference gives, rows after stage 0 / COUNT(*):
#   20a 6908 / 5210    26c 3923 / 2534    28a 1661 / 958    29a 73033 / 2553
SHAPES = {10: "20a", 12: "26c", 14: "28a", 17: "29a"}
SCALE, SEED, SEL_FLOOR = 0.002, 1337, 0.8
CHUNK = 1024


def direct_join(plan, data, n_joins=None):
    """every join of the plan's breadth-first order applied to the probe table's (filtered) rows in numpy, keys read from the
    base tables -> {alias: base-table row (index into the rows the table's filters keep) per result row}"""
    probe = plan["probe"]
    n = data["n_probe"]
    rows = {probe: np.arange(n, dtype=np.int64) if data["sel"] is None else data["sel"].astype(np.int64)}
    src0 = {(a, c): col for (a, c, kd), col in zip(plan["stages"][0]["source"], data["source"]) if kd == "int"}
    pay = {}
    for st in plan["stages"]:
        for i, cols in zip(st["joins"], st["payload"]):
            for (c, kd), arr in zip(cols, data["joins"][i]["payload"]):
                pay[(plan["order"][i][0], c, kd)] = arr
    for i, (alias, _bcol, (sa, sc)) in enumerate(plan["order"][:n_joins]):
        col = src0[(sa, sc)] if sa == probe else pay[(sa, sc, "int")]
        key = col[rows[sa]]
        j = Join(data["joins"][i]["key"], 0)
        left, right = np.searchsorted(j.sorted, key, "left"), np.searchsorted(j.sorted, key, "right")
        cnt = (right - left).astype(np.int64)
        rep = np.repeat(np.arange(len(key)), cnt)
        within = np.arange(len(rep)) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        rows = {a: r[rep] for a, r in rows.items()}
        rows[alias] = j.order[np.repeat(left, cnt) + within]
    return rows, src0, pay


def reference(plan, data):
    """COUNT(*), the select list's MINs in the order of plan["final"], and the integer MINs of the last stage's source"""
    rows, src0, pay = direct_join(plan, data)
    probe = plan["probe"]
    mins = []
    strs0 = {(a, c): col for (a, c, kd), col in zip(plan["stages"][0]["source"], data["source"]) if kd == "str"}
    for a, c, kd in plan["final"]:
        col = strs0[(a, c)] if a == probe else pay[(a, c, kd)]
        r = np.unique(rows[a])
        mins.append(min(col[x] for x in r.tolist()) if len(r) else None)
    # the integer MINs: every key column the last stage reads from its source, over the result rows
    int_mins = []
    for a, c, kd in plan["stages"][-1]["source"]:
        if kd == "int":
            col = src0[(a, c)] if a == probe else pay[(a, c, kd)]
            int_mins.append(int(col[rows[a]].min()) if len(rows[a]) else None)
    return {"count": len(rows[probe]), "mins": mins, "int_mins": int_mins}


def stage_rows_reference(plan, data):
    """output rows of every stage: the direct join cut after each stage's last join"""
    out = []
    for st in plan["stages"]:
        out.append(len(direct_join(plan, data, st["joins"][-1] + 1)[0][plan["probe"]]))
    return out


def oracle_stage(cols, joins, sel):
    """job_family.run_chain_host's run_stage: one pipeline through the oracle, join order 0 1 2 ..."""
    k = len(joins)
    specs = [orc.JoinSpec(orc.HashTable([key], ints), [src]) for key, ints, src in joins]
    res = orc.run_pipeline(cols, specs, [list(range(k))], routing="default_path", caching=False, sel=sel)
    return res["out_rows"].astype(np.int64), res["num_intermediates"]


def instance(n_tables):
    q = job_family.shapes()[SHAPES[n_tables]]
    assert len(q["tables"]) == n_tables
    plan = job_family.chained_plan(q)
    data = job_family.chain_data(plan, job_family.Tables(scale=SCALE, seed=SEED), q, sel_floor=SEL_FLOOR)
    return q, plan, data
