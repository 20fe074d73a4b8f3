"""tools/spill_report.py on the K = 4 counting build of the flat pool kernel (the headline's kernel): the router's
step loop touches no scratch memory, and the probe loop has not paid for it.  A cross-compile of about ten seconds; no
GPU."""
import importlib.util
import os

import pytest

import common

_spec = importlib.util.spec_from_file_location("spill_report", os.path.join(common.ROOT, "tools", "spill_report.py"))
spill_report = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(spill_report)

# polr_pool_flat_kernel<4, 0> before the router's state moved to LDS (profiles/spill_report_parent.txt)
PARENT_VGPR_SPILLS = 137
PARENT_PRIVATE_BYTES = 576
PARENT_PROBE_SPILLS = 5


@pytest.mark.skipif(not spill_report.have_hipcc(), reason="hipcc is not installed")
def test_router_step_loop_of_k4_counting_build_does_not_spill(tmp_path):
    rows = spill_report.report(["k4"], tmpdir=str(tmp_path))["k4"]
    assert len(rows) == 1 and "polr_pool_flat_kernelILi4ELi0EE" in rows[0]["kernel"]
    r = rows[0]
    text = open(os.path.join(str(tmp_path), "k4.s")).read()
    # the markers the classification rests on are there (else every spill would count as "probe side")
    assert spill_report.STEPS_BEGIN in text and spill_report.STEPS_END in text and spill_report.ROUTER_END in text
    assert r["router_step_spills"] == 0, r
    assert r["probe_spills"] <= PARENT_PROBE_SPILLS, r
    assert r["vgpr_spill_count"] <= PARENT_VGPR_SPILLS, r
    assert r["private_segment"] <= PARENT_PRIVATE_BYTES, r
    assert r["vgpr_count"] <= 128, r  # (16 waves per workgroup, one workgroup per CU)
