"""The order of two string_t cells (polr_str_cell_cmp3 of duckdb-polr_amd/csrc/polr_strcmp.h, the order of the sorted
dictionary codes), the part that needs no GPU: the header compiled into a stand-alone host program
(tests/strcmp/str_cell_cmp_main.cpp) that runs every ordered pair of scanstr.EDGES as cell against cell -- inline cells also
with garbage padding, every long string in an allocation of exactly its size -- against memcmp-then-length; built plain and
with the address + undefined-behaviour sanitizers, and run directly."""
import os
import re
import subprocess

import pytest

import common
import scanstr

SRC = os.path.join(common.ROOT, "tests", "strcmp", "str_cell_cmp_main.cpp")
HEADER = os.path.join(common.ROOT, "duckdb-polr_amd", "csrc", "polr_strcmp.h")


@pytest.mark.parametrize("sanitize", [None, "address,undefined"], ids=["plain", "asan-ubsan"])
def test_every_ordered_pair_of_cells_of_the_edge_set(tmp_path, sanitize):
    assert "polr_str_cell_cmp3" in open(HEADER).read(), "polr_strcmp.h has no cell-against-cell comparison"
    exe, edges = str(tmp_path / "str_cell_cmp"), str(tmp_path / "edges.bin")
    scanstr.write_edges(edges)
    flags = ["-fsanitize=" + sanitize, "-fno-sanitize-recover=all"] if sanitize else []
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall"] + flags + [SRC, "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe, edges], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    lines = run.stdout.strip().splitlines()
    assert lines[-1] == "ok"
    m = re.match(r"(\d+) strings, (\d+) inline cells, (\d+) heap cells, (\d+) pairs compared, (\d+) mismatches", lines[-2])
    assert m, lines[-2]
    n = len(scanstr.EDGES)
    n_inline, n_padded = sum(len(e) <= 12 for e in scanstr.EDGES), sum(len(e) < 12 for e in scanstr.EDGES)
    assert [int(g) for g in m.groups()] == [n, n_inline + n_padded, n - n_inline, (n + n_padded) ** 2, 0]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-4000:]
