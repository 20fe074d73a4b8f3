"""The chained plan of the JOB-shaped family (polr_amd.job_family.chained_plan): a query of more than eight joins as stages
of at most eight, the rows one stage emits being the source of the next.  No GPU here: the plan's structure for all 113
shapes, and four long shapes run stage by stage through the oracle (tests/jobchain.py) with the carried columns gathered in
numpy between the stages, against a direct numpy join of all tables."""
import os
import re

import numpy as np
import pytest

import common
import jobchain
from polr_amd import capi, job_family

SHAPES = job_family.shapes()
LONG = sorted(n for n, q in SHAPES.items() if len(q["tables"]) > 9)
SHORT = sorted(n for n, q in SHAPES.items() if len(q["tables"]) <= 9)


def test_the_family_has_37_long_and_76_short_shapes():
    assert len(LONG) == 37 and len(SHORT) == 76
    sizes = [len(SHAPES[n]["tables"]) for n in LONG]
    assert {s: sizes.count(s) for s in set(sizes)} == {10: 7, 11: 10, 12: 11, 14: 6, 17: 3}


@pytest.mark.parametrize("name", LONG)
def test_long_shapes_are_cut_into_stages_that_join_every_table(name):
    q = SHAPES[name]
    plan = job_family.chained_plan(q)
    order, stages = plan["order"], plan["stages"]
    assert len(stages) == (len(order) + 7) // 8 >= 2
    assert all(1 <= len(st["joins"]) <= job_family.MAX_JOINS for st in stages)
    # every table of the query exactly once: the probe table, and one join per other table, in stage order
    assert [i for st in stages for i in st["joins"]] == list(range(len(order)))
    assert sorted([plan["probe"]] + [o[0] for o in order]) == sorted(q["tables"])
    # the first stage's joins are the family's existing pipeline
    probe, first = job_family.pipeline_shape(q)
    assert probe == plan["probe"] and order[:8] == first
    placed_before = {plan["probe"]}
    for s, st in enumerate(stages):
        aliases = [order[i][0] for i in st["joins"]]
        source = st["source"]
        # the stage's source: columns of the probe table (stage 0), else exactly what the stage before carries
        assert all(a in placed_before for a, _c, _k in source) and len(set(source)) == len(source)
        if s:
            prev = stages[s - 1]
            assert len(prev["carry"]) == len(source)
            for (sj, sc), (a, c, kd) in zip(prev["carry"], source):
                if sj < 0:
                    assert prev["source"][sc] == (a, c, kd)
                else:
                    assert order[prev["joins"][sj]][0] == a and prev["payload"][sj][sc] == (c, kd)
        else:
            assert all(a == plan["probe"] for a, _c, _k in source)
        # every key a stage reads is a carried column or a column of a join of that stage
        for j, (i, (sj, sc)) in enumerate(zip(st["joins"], st["key_src"])):
            a, c = order[i][2]
            if sj < 0:
                assert source[sc] == (a, c, "int") and a in placed_before
            else:
                assert aliases[sj] == a and sj != j and st["payload"][sj][sc] == (c, "int")
        placed_before |= set(aliases)
    # the select list leaves the last stage, every column once
    assert sorted(plan["final"]) == sorted((a, c, "str") for a, c in set(plan["select"]))
    assert len(stages[-1]["carry"]) == len(plan["final"])


@pytest.mark.parametrize("name", SHORT)
def test_short_shapes_are_one_stage_equal_to_the_existing_plan(name):
    q = SHAPES[name]
    plan = job_family.chained_plan(q)
    probe, order = job_family.pipeline_shape(q)
    assert plan["probe"] == probe and plan["order"] == order and len(plan["stages"]) == 1
    st = plan["stages"][0]
    assert st["joins"] == list(range(len(order)))
    wl = job_family.workload(name, job_family.Tables(scale=0.0005), q) if len(order) >= 2 else None
    if wl is not None:
        # the same keys as the workload the benchmark runs: probe keys name the same columns, dependent keys the same join
        names = list(wl["probe"]["cols"])
        for j, (sj, sc) in zip(wl["joins"], st["key_src"]):
            wj, wc = j["key_src"][0]
            assert wj == sj
            if sj < 0:
                assert st["source"][sc][1] == names[wc]
            else:
                assert st["payload"][sj][sc][0] == list(wl["joins"][sj]["payload"])[wc]


@pytest.mark.parametrize("n_tables", sorted(jobchain.SHAPES))
def test_chain_through_the_oracle_equals_the_direct_join(n_tables):
    q, plan, data = jobchain.instance(n_tables)
    want = jobchain.reference(plan, data)
    stage_rows = jobchain.stage_rows_reference(plan, data)
    # the conditions of this check, from the numpy reference alone
    assert want["count"] >= 1 and all(r > jobchain.CHUNK for r in stage_rows[:-1]), (want["count"], stage_rows)
    got = job_family.run_chain_host(plan, data, jobchain.oracle_stage)
    assert got["count"] == want["count"] == stage_rows[-1]
    assert got["stage_rows"] == stage_rows
    assert got["mins"] == want["mins"] and all(m is not None for m in want["mins"])
    assert len(got["intermediates"]) == len(plan["stages"]) and all(x >= r for x, r in zip(got["intermediates"], stage_rows))
    assert got["int_mins"] == want["int_mins"] and len(want["int_mins"]) >= 1 and None not in want["int_mins"]


def test_abi_header_library_and_binding_agree_on_the_new_export():
    text = open(os.path.join(common.ROOT, "include", "polr_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"int polr_pipeline_from_output\((.*?)\);", text, flags=re.S)
    assert m, "the header does not declare polr_pipeline_from_output"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 9 and params[0] == "polr_out *o" and params[-1] == "polr_pipeline **out"
    lib = capi.load()
    assert hasattr(lib, "polr_pipeline_from_output") and "polr_pipeline_from_output" in capi.EXPORTS
    assert len(lib.polr_pipeline_from_output.argtypes) == 9
    assert lib.polr_pipeline_from_output(None, None, None, 0, None, 0, None, 0, None) == capi.E_INVALID
    assert callable(capi.Pipeline.from_output)
