"""Range stealing, the part that needs no GPU: the claim / steal protocol of duckdb-polr_amd/csrc/polr_steal.h as a
stand-alone host program (tests/steal/steal_protocol_main.cpp: known answers on one thread, 8 threads over 4 096
chunks), built once with the thread sanitizer and once with the address + undefined-behaviour sanitizers and run
directly; and the declarations of the launch mode in header, library and binding."""
import os
import re
import subprocess

import pytest

import common

SRC = os.path.join(common.ROOT, "tests", "steal", "steal_protocol_main.cpp")
HEADER = os.path.join(common.ROOT, "duckdb-polr_amd", "csrc", "polr_steal.h")
NAMES = ["polr_mpx_run_resident_stealing", "polr_mpx_steal_stats"]


@pytest.mark.parametrize("sanitize", ["thread", "address,undefined"])
def test_protocol_program_under_sanitizers(tmp_path, sanitize):
    assert os.path.isfile(HEADER), "duckdb-polr_amd/csrc/polr_steal.h is missing"
    exe = str(tmp_path / "steal_protocol")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=" + sanitize,
                            "-fno-sanitize-recover=all", SRC, "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(run.stdout)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    lines = run.stdout.strip().splitlines()
    assert lines[-1] == "ok"
    # three layouts x grants 1, 3, 64: every chunk of the union exactly once, none outside it
    rows = [l for l in lines if "chunks claimed" in l]
    assert len(rows) == 9
    want = {"owner0": 4096, "even": 4096, "gaps": 690 + 1 + 1501 + 596 + 125}
    for l in rows:
        m = re.match(r"(\w+)\s+grant\s+(\d+): (\d+) chunks claimed, (\d+) stolen, (\d+) miscounted", l)
        assert m, l
        assert int(m.group(3)) == want[m.group(1)] and int(m.group(5)) == 0, l
        assert int(m.group(4)) % int(m.group(2)) == 0, l
    assert "WARNING: ThreadSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]


def test_header_library_and_binding_declare_the_launch_mode():
    from polr_amd import capi
    header = open(os.path.join(common.ROOT, "include", "polr_hip.h")).read()
    lib = capi.load()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in capi.EXPORTS, name
        assert hasattr(lib, name), name
    assert "polr_steal_stats" in header
    assert callable(capi.run_resident_stealing) and callable(capi.DeviceMultiplexer.steal_stats)
