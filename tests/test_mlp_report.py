"""tools/mlp_report.py on the K = 4 counting build of the flat pool kernel (the headline's kernel): on the plain path (no
selection vector, no validity column on a deeper stage) a sweep issues the key gathers of ALL deeper stages without
waiting for any of them, and likewise the bit words of all tables; with a selection vector there is ONE wait, between
the rows and the keys.  A cross-compile of about ten seconds; no GPU."""
import importlib.util
import os
import re

import pytest

import common

_spec = importlib.util.spec_from_file_location("mlp_report", os.path.join(common.ROOT, "tools", "mlp_report.py"))
mlp_report = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mlp_report)
spill_report = mlp_report.spill_report


def _sweep_f(k):
    """flat_sweep_f<K>() of polr_flat_device.h, read from the source"""
    src = open(os.path.join(common.ROOT, "duckdb-polr_amd", "csrc", "polr_flat_device.h")).read()
    m = re.search(r"flat_sweep_f\(\) \{\s*return K <= (\d+) \? (\d+) : (\d+);", src)
    assert m, "flat_sweep_f not found"
    return int(m.group(2)) if k <= int(m.group(1)) else int(m.group(3))


@pytest.mark.skipif(not spill_report.have_hipcc(), reason="hipcc is not installed")
def test_plain_sweep_of_k4_counting_build_waits_for_no_load(tmp_path):
    rows = mlp_report.report(["k4"], tmpdir=str(tmp_path))["k4"]
    assert len(rows) == 1 and "polr_pool_flat_kernelILi4ELi0EE" in rows[0]["kernel"]
    text = open(os.path.join(str(tmp_path), "k4.s")).read()
    for region in mlp_report.REGIONS:
        assert region + "-begin" in text and region + "-end" in text, region
    reg = rows[0]["regions"]
    # the sweep is inlined where the source phase and where the drain calls it
    copies = reg["polr-sweep-keys"]["copies"]
    assert copies >= 1 and all(reg[r]["copies"] == copies for r in mlp_report.PLAIN_REGIONS + [mlp_report.SEL_REGION]), reg
    for r in mlp_report.PLAIN_REGIONS:
        assert reg[r]["waits"] == 0, (r, reg[r])
    # K - 1 = 3 deeper stages x flat_sweep_f<4>() gathers per lane, in every copy
    assert reg["polr-sweep-keys"]["loads"] >= copies * 3 * _sweep_f(4), reg["polr-sweep-keys"]
    # ... and as many table words (either address space is compiled in: the global-memory loads are counted here)
    assert reg["polr-sweep-tables"]["loads"] >= copies * 3 * _sweep_f(4), reg["polr-sweep-tables"]
    # a selection vector: rows, one wait, keys (and validity bytes)
    assert reg[mlp_report.SEL_REGION]["waits"] == copies, reg[mlp_report.SEL_REGION]
    assert reg[mlp_report.SEL_REGION]["loads"] >= copies * 3 * 3 * _sweep_f(4), reg[mlp_report.SEL_REGION]
    assert rows[0]["probe_insts"] > 0
