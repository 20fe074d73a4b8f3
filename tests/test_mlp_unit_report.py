"""tools/mlp_report.py on what a probe wave of the K = 4 counting build does AROUND a unit: the join-order switch asks for
all stage records before it waits for one, a look at the queues is one batch of loads, and an arrival is one returning
counter atomic with at most one wait in front of the arrival add.  A cross-compile of about ten seconds; no GPU."""
import importlib.util
import os
import re

import pytest

import common

_spec = importlib.util.spec_from_file_location("mlp_report_unit", os.path.join(common.ROOT, "tools", "mlp_report.py"))
mlp_report = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mlp_report)
spill_report = mlp_report.spill_report

K = 4


def _flat_stage_words():
    """the dwords of a FlatStage (polr_flat_device.h), counted from the source: 2 per pointer, 1 per uint32_t"""
    src = open(os.path.join(common.ROOT, "duckdb-polr_amd", "csrc", "polr_flat_device.h")).read()
    m = re.search(r"struct FlatStage \{(.*?)\n\};", src, re.S)
    assert m, "struct FlatStage not found"
    words = 0
    for decl in re.sub(r"//.*", "", m.group(1)).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        names = decl.count(",") + 1
        words += names * (2 if "*" in decl else 1)
    return words


@pytest.fixture(scope="module")
def k4(tmp_path_factory):
    if not spill_report.have_hipcc():
        pytest.skip("hipcc is not installed")
    tmp = str(tmp_path_factory.mktemp("mlp_unit"))
    rows = mlp_report.unit_report(["k4"], tmpdir=tmp)["k4"]
    assert len(rows) == 1 and "polr_pool_flat_kernelILi4ELi0EE" in rows[0]["kernel"]
    text = open(os.path.join(tmp, "k4.s")).read()
    return rows[0]["regions"], text, spill_report.report_file(os.path.join(tmp, "k4.s"))


def test_markers_are_planted(k4):
    _, text, _ = k4
    for region in mlp_report.UNIT_REGIONS:
        assert region + "-begin" in text and region + "-end" in text, region


def test_path_switch_requests_every_record_before_it_waits(k4):
    reg = k4[0][mlp_report.SWITCH_REGION]
    print("path switch:", reg)
    assert reg["copies"] >= 1
    assert _flat_stage_words() == 10
    # no wait on vmcnt or lgkmcnt between the first and the last descriptor load of a copy
    assert reg["inner"] == 0, reg
    # all K stages' words are asked for, in every copy
    assert reg["words"] >= reg["copies"] * K * _flat_stage_words(), reg


def test_poll_is_one_batch_of_loads(k4):
    """polr_pool_look.  What was asked of a look is ONE round trip; what ships is two (three when both tickets are lacking):
    the ticket adds stand in front of the load, because a ticket taken at consumption and held through the next unit made
    the latency-bound workloads slower (profiles/README.md).  So `loads == copies` and `inner == 0` are the requirement --
    one load, nothing between a first and a last one -- while the bound on the waits only pins what the compiler emits
    for that shape today, so that a further wait in the look shows up here."""
    reg = k4[0][mlp_report.POLL_REGION]
    print("poll:", reg)
    assert reg["copies"] >= 1
    # ONE load per look (a lane per word) ...
    assert reg["loads"] == reg["copies"] and reg["words"] == 2 * reg["copies"], reg
    assert reg["inner"] == 0, reg
    # ... and the region shows what a look costs: the wait for the load, and one for each of the two tickets it may lack (a
    # look consumes at most one ticket, so the next look lacks at most one: the compiler's wave-reduced form of an add at a
    # uniform address waits for it on the spot)
    assert 1 <= reg["waits"] <= 3 * reg["copies"], reg
    assert reg["ret_atomics"] == 2 * reg["copies"], reg


def test_arrival_is_one_returning_atomic_and_one_wait(k4):
    reg = k4[0][mlp_report.ARRIVE_REGION]
    print("arrive:", reg)
    assert reg["copies"] >= 1
    assert reg["ret_atomics"] == reg["copies"], reg
    assert reg["ret_waits"] <= reg["copies"], reg


def test_k4_counting_build_keeps_its_registers(k4):
    rows = k4[2]
    assert len(rows) == 1
    print("registers:", {key: rows[0][key] for key in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count")})
    assert rows[0]["vgpr_spill_count"] == 0, rows[0]
    assert rows[0]["vgpr_count"] <= 128, rows[0]
