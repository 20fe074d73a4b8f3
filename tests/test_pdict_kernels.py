"""The dictionary encoder's kernels as the compiler builds them for gfx950 (tools/spill_report.py --build dict, a
cross-compile: no GPU needed): none of them, the through-selection forms included, uses scratch memory or spills a
register."""
import importlib.util
import os

import pytest

import common

_spec = importlib.util.spec_from_file_location("spill_report", os.path.join(common.ROOT, "tools", "spill_report.py"))
spill_report = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(spill_report)

NEW = ["polr_dict_insert_kernelILb1E", "polr_dict_count_long_kernelILb1E", "polr_dict_sel_valid_kernel"]


@pytest.mark.skipif(not spill_report.have_hipcc(), reason="hipcc is not installed")
def test_no_kernel_of_the_encoder_uses_scratch(tmp_path):
    rows = spill_report.report(["dict"], tmpdir=str(tmp_path))["dict"]
    names = [r["kernel"] for r in rows]
    for new in NEW:
        assert any(new in n for n in names), (new, names)
    assert any("polr_dict_insert_kernelILb0E" in n for n in names)  # (the build side's form is still there)
    for r in rows:
        assert (r["private_segment"], r["vgpr_spill_count"], r["sgpr_spill_count"], r["probe_spills"]) == (0, 0, 0, 0), r
        assert r["vgpr_count"] <= 64, r  # (8 waves per SIMD: the insert kernel hides its probe latency by occupancy)
