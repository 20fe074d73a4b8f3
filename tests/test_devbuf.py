"""The owner of device memory (duckdb-polr_amd/csrc/polr_devbuf.h), the part that needs no GPU: the header compiled
against a stand-in hip/hip_runtime.h (tests/devbuf/hip) into a stand-alone host program (tests/devbuf/devbuf_main.cpp)
whose hipMalloc / hipFree keep the set of live blocks and can fail on demand; built plain and with the address +
undefined-behaviour sanitizers, and run directly."""
import os
import re
import subprocess

import pytest

import common

DIR = os.path.join(common.ROOT, "tests", "devbuf")
SRC = os.path.join(DIR, "devbuf_main.cpp")
HEADER = os.path.join(common.ROOT, "duckdb-polr_amd", "csrc", "polr_devbuf.h")


@pytest.mark.parametrize("sanitize", [None, "address,undefined"], ids=["plain", "asan-ubsan"])
def test_every_block_is_freed_exactly_once(tmp_path, sanitize):
    assert os.path.isfile(HEADER), "duckdb-polr_amd/csrc/polr_devbuf.h is missing"
    exe = str(tmp_path / "devbuf")
    flags = ["-fsanitize=" + sanitize, "-fno-sanitize-recover=all"] if sanitize else []
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-I", DIR] + flags + [SRC, "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    lines = run.stdout.strip().splitlines()
    assert lines[-1] == "ok"
    m = re.match(r"(\d+) allocations, (\d+) frees, (\d+) failed allocations, (\d+) null frees, (\d+) bad frees, "
                 r"(\d+) live blocks, (\d+) live bytes, (\d+) steps checked", lines[-2])
    assert m, lines[-2]
    allocs, frees, failed, null_frees, bad_frees, live_blocks, live_bytes, steps = [int(g) for g in m.groups()]
    # what the program does, counted by hand: 2 + 1 + 2 + 2 + 2 + 1 + 100 allocations that succeed, 3 that are made to fail
    assert (allocs, failed) == (110, 3)
    assert frees == allocs and live_blocks == 0 and live_bytes == 0
    assert null_frees == 0 and bad_frees == 0
    assert steps == 24  # the CHECK() lines of the program, each passed once
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-4000:]


def test_the_header_stands_alone():
    """polr_devbuf.h includes the HIP runtime header and standard headers only (so that it compiles on a host)"""
    text = open(HEADER).read()
    includes = re.findall(r'^#include\s+([<"][^>"]+[>"])', text, flags=re.M)
    assert "<hip/hip_runtime.h>" in includes
    assert not [i for i in includes if i.startswith('"')], includes
