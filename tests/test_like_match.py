"""The LIKE matcher (duckdb-polr_amd/csrc/polr_like.h) over patterns lowered by polr_filter_plan.h, the part that needs no
GPU: both headers compiled into a stand-alone host program (tests/like/like_main.cpp) that matches every pattern of
scanexpr.LIKE_EDGES against every string -- inline cells also with garbage padding, heap strings at every alignment 0..7 in
an allocation of exactly the words that contain them -- compared with scanexpr's regular expression; built plain and with
the address + undefined-behaviour sanitizers, and run directly."""
import os
import re
import subprocess

import pytest

import common
import scanexpr
import scanstr

SRC = os.path.join(common.ROOT, "tests", "like", "like_main.cpp")
CSRC = os.path.join(common.ROOT, "duckdb-polr_amd", "csrc")


def write_edges(path):
    """the patterns, then the strings, each as scanstr.write_edges writes a list"""
    parts = []
    for strings in (scanexpr.LIKE_PATTERNS, scanexpr.LIKE_STRINGS):
        scanstr.write_edges(path, strings)
        parts.append(open(path, "rb").read())
    open(path, "wb").write(b"".join(parts))


@pytest.mark.parametrize("sanitize", [None, "address,undefined"], ids=["plain", "asan-ubsan"])
def test_every_pattern_against_every_string(tmp_path, sanitize):
    for h in ("polr_like.h", "polr_filter_plan.h"):
        assert os.path.isfile(os.path.join(CSRC, h)), h + " is missing"
    exe, edges = str(tmp_path / "like_match"), str(tmp_path / "edges.bin")
    write_edges(edges)
    flags = ["-fsanitize=" + sanitize, "-fno-sanitize-recover=all"] if sanitize else []
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall"] + flags + [SRC, "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe, edges], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    lines = run.stdout.strip().splitlines()
    assert lines[-1] == "ok"
    m = re.match(r"(\d+) patterns, (\d+) strings, (\d+) forms matched, 0 disagreements", lines[-2])
    strings, patterns = scanexpr.LIKE_STRINGS, scanexpr.LIKE_PATTERNS
    n_forms = sum(2 if len(s) < 12 else 1 if len(s) == 12 else 8 for s in strings)
    assert m and [int(g) for g in m.groups()] == [len(patterns), len(strings), n_forms * len(patterns)], lines[-2]
    assert len(lines) == len(patterns) + 2
    bad = []
    for p, line in zip(patterns, lines):
        want = "".join("1" if scanexpr.like(s, p) else "0" for s in strings)
        if line != want:
            bad.append((p, [s for s, a, b in zip(strings, line, want) if a != b][:5]))
    assert not bad, bad[:5]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-4000:]


def test_edge_set_holds_what_the_matcher_can_get_wrong():
    p, s = scanexpr.LIKE_PATTERNS, scanexpr.LIKE_STRINGS
    assert len(set(p)) == len(p) and len(set(s)) == len(s)
    assert {b"", b"%", b"%%", b"_", b"__", b"%_", b"_%", b"a%", b"%a", b"%a%", b"a%a", b"%ab%ab", b"%ab%b", b"a_c",
            b"%_b_%", b"M_nchen", b"M__nchen", "%語%".encode()} <= set(p)
    assert set(scanstr.EDGES) | {b"abab", b"ababab", b"aab", "München".encode(), "日本語".encode()} <= set(s)
    assert sum(24 <= len(x) <= 40 and x.startswith(b"(") for x in s) >= 4  # JOB-like notes
    assert not scanexpr.like("München".encode(), b"M_nchen") and scanexpr.like("München".encode(), b"M__nchen")
    assert any(len(x) > max(map(len, s)) for x in p)
    assert not any(0 in x for x in p)
    # every pattern but the over-long ones separates the strings
    for x in p:
        n = sum(bool(scanexpr.like(v, x)) for v in s)
        assert (0 < n < len(s)) or x in (b"%", b"%%") or len(x) > 300, x
    # a segment that straddles byte 12 of a 40-byte string, one that occurs only at its very end
    assert scanstr._S40.find(b"abcde") == 10 and scanstr._S40.endswith(b"ABCD") and scanstr._S40.count(b"ABCD") == 1
    # leftmost is not enough for the last segment: 'ab' occurs twice in 'abab', only the second occurrence ends it
    assert scanexpr.like(b"abab", b"%ab") and scanexpr.like(b"ababab", b"ab%ab") and not scanexpr.like(b"aab", b"%ab%b")
