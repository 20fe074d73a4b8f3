"""The comparison of a string_t cell against a constant (duckdb-polr_amd/csrc/polr_strcmp.h), the part that needs no GPU:
the header compiled into a stand-alone host program (tests/strcmp/str_cmp_main.cpp) that runs every ordered pair of
scanstr.EDGES -- inline cells also with garbage padding, every string in an allocation of exactly its size -- against
memcmp-then-length; built plain and with the address + undefined-behaviour sanitizers, and run directly."""
import os
import re
import subprocess

import pytest

import common
import scanstr

SRC = os.path.join(common.ROOT, "tests", "strcmp", "str_cmp_main.cpp")
HEADER = os.path.join(common.ROOT, "duckdb-polr_amd", "csrc", "polr_strcmp.h")


@pytest.mark.parametrize("sanitize", [None, "address,undefined"], ids=["plain", "asan-ubsan"])
def test_every_ordered_pair_of_the_edge_set(tmp_path, sanitize):
    assert os.path.isfile(HEADER), "duckdb-polr_amd/csrc/polr_strcmp.h is missing"
    exe, edges = str(tmp_path / "str_cmp"), str(tmp_path / "edges.bin")
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
    assert [int(g) for g in m.groups()] == [n, n_inline + n_padded, n - n_inline, (n + n_padded) * n, 0]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-4000:]


def test_edge_set_holds_what_the_comparison_can_get_wrong():
    e = scanstr.EDGES
    assert len(set(e)) == len(e)
    assert b"" in e and b"\0" in e and b"ab" in e and b"ab\0" in e  # a trailing NUL is a character
    assert {12, 13, 40, 41, 300} <= {len(s) for s in e}
    assert any(len(a) == len(b) == 13 and a[:12] == b[:12] and a != b for a in e for b in e)
    assert any(len(a) == len(b) == 40 and a[:4] == b[:4] and a[4] != b[4] for a in e for b in e)
    assert any(len(a) == len(b) == 40 and a[:39] == b[:39] and a != b for a in e for b in e)
    assert any(len(a) == 40 and len(b) == 41 and b.startswith(a) for a in e for b in e)
    assert {b"\x7f", b"\x80", b"\xff"} <= set(e)
