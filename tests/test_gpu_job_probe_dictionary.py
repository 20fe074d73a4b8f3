"""The JOB shapes that the fused route left out, through probe-side dictionaries: the 9 shapes whose select list names a
VARCHAR column of the probe table (job_family.run_fused_device(..., probe_dictionary=True): the column encoded over the scan's
selection, MIN(code) folded inside the one pool launch) against the reference engine's own answers
(tests/golden/job_family.json), and chained plans with their LAST stage fused (job_family.run_chain_fused_device) against the
chain run stage by stage through the oracle."""
import pytest

import common
import jobchain
from polr_amd import capi
from polr_amd import job_family as jf
from test_gpu_job_fused import SHAPES, _paths

pytestmark = pytest.mark.gpu


def test_the_9_probe_side_shapes_against_the_reference(gpu_ctx):
    gold = common.load_golden("job_family")
    t = jf.Tables(scale=gold["scale"])
    ran, with_min = [], 0
    live0 = capi.device_bytes_live()
    for name in sorted(SHAPES):
        wl = jf.workload(name, t, SHAPES[name])
        if jf.fused_select_on_build_sides(wl):
            continue
        g = gold["queries"][name]
        with pytest.raises(ValueError):  # (the default is what it was)
            jf.run_fused_device(gpu_ctx, wl, _paths(wl))
        res = jf.run_fused_device(gpu_ctx, wl, _paths(wl), probe_dictionary=True)
        assert res["count_star"] == g["count_star"], name
        assert [None if m is None else m.decode() for m in res["select_min"]] == g["select_min"], (name, res["select_min"])
        assert res["rows_written"] == 0, name
        ran.append(name)
        with_min += any(m is not None for m in res["select_min"])
    assert len(ran) == 9, ran
    assert with_min == 5  # (57 of the 113 shapes have a non-NULL MIN at this scale, 52 of them among the other 104)
    assert capi.device_bytes_live() == live0


@pytest.mark.parametrize("n_tables", [10, 17])
def test_chained_plans_with_the_last_stage_fused(gpu_ctx, n_tables):
    _q, plan, data = jobchain.instance(n_tables)
    assert len(plan["stages"]) >= 2
    cpu = jf.run_chain_host(plan, data, jobchain.oracle_stage)
    assert cpu["count"] >= 1 and any(m is not None for m in cpu["mins"])
    live0 = capi.device_bytes_live()
    got = jf.run_chain_fused_device(gpu_ctx, plan, data, chunk_capacity=jobchain.CHUNK)
    assert got["count"] == cpu["count"] and got["mins"] == cpu["mins"]
    assert got["stage_rows"] == cpu["stage_rows"] and got["rows_written"] == 0
    assert capi.device_bytes_live() == live0
