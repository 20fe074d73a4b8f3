"""The string copy routine and the packed-offset arithmetic of polr_out_materialize_strings (duckdb-polr_amd/csrc/
polr_strcopy.h), the part that needs no GPU: the header compiled into a stand-alone host program (tests/strcopy/
strcopy_main.cpp), built plain and with the address + undefined-behaviour sanitizers, and run directly.

Copies: every length 13..80, the cut-over between "a lane alone" and "the whole wave" and its neighbours, 4097 and 100 000
bytes, each at every source alignment x destination alignment and as 1 lane and as 64 lanes in turn; the source in an
allocation of exactly the aligned words that contain it (the sanitizer proves nothing else is read), the destination
between canaries (nothing but the string's own bytes is written).  Offsets: lists of (length, validity) whose packed
offsets and totals this file computes in Python, one of them with a running total beyond 2^32."""
import os
import re
import subprocess

import numpy as np
import pytest

import common

SRC = os.path.join(common.ROOT, "tests", "strcopy", "strcopy_main.cpp")
HEADER = os.path.join(common.ROOT, "duckdb-polr_amd", "csrc", "polr_strcopy.h")


def cut_over():
    """POLR_STRCOPY_LANE_MAX as the header defines it"""
    m = re.search(r"#define POLR_STRCOPY_LANE_MAX (\d+)u", open(HEADER).read())
    assert m, "polr_strcopy.h does not define POLR_STRCOPY_LANE_MAX"
    return int(m.group(1))


def offset_lists():
    """[(lengths, validity)]: the inline / heap boundary, NULL rows with long 'lengths', an empty list, a list of huge
    lengths whose running total passes 2^32 with rows still to come"""
    rng = np.random.default_rng(7)
    lists = [([], []),
             ([0, 1, 12, 13, 14, 12, 13, 100, 5, 4097], [1] * 10),
             ([13, 20, 500, 13, 12, 0xFFFFFFFF, 40], [0, 1, 0, 1, 1, 0, 1]),
             ([12] * 9, [1] * 9),
             ([0xFFFFFFF0, 13, 0xFFFFFFFF, 7, 0x80000000, 13, 0xFFFFFFFF, 100], [1, 1, 1, 1, 1, 0, 1, 1])]
    lens = rng.choice([0, 5, 12, 13, 31, 64, 65, 4096, 1 << 20], 3000)
    lists.append((lens.tolist(), (rng.random(3000) > 0.2).astype(int).tolist()))
    return lists


def packed(lens, valid):
    """exact Python: offsets and total of the packed heap"""
    offs, at = [], 0
    for ln, ok in zip(lens, valid):
        offs.append(at)
        at += ln if ok and ln > 12 else 0
    return offs, at


def write_offsets(path):
    totals = []
    with open(path, "w") as f:
        for lens, valid in offset_lists():
            offs, total = packed(lens, valid)
            f.write("%d\n" % len(lens))
            for row in zip(lens, valid, offs):
                f.write("%d %d %d\n" % row)
            f.write("%d\n" % total)
            totals.append(total)
    return totals


@pytest.mark.parametrize("sanitize", [None, "address,undefined"], ids=["plain", "asan-ubsan"])
def test_copies_and_offsets(tmp_path, sanitize):
    assert os.path.isfile(HEADER), "polr_strcopy.h is missing"
    cut = cut_over()
    exe, offsets = str(tmp_path / "strcopy"), str(tmp_path / "offsets.txt")
    totals = write_offsets(offsets)
    assert max(totals) > 1 << 32
    flags = ["-fsanitize=" + sanitize, "-fno-sanitize-recover=all"] if sanitize else []
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall"] + flags + [SRC, "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe, offsets], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    lines = run.stdout.strip().splitlines()
    assert lines[-1] == "ok" and len(lines) == 3, lines[-5:]
    n_lengths = (80 - 13 + 1) + 5
    m = re.match(r"cut-over (\d+): (\d+) lengths, (\d+) copies, 0 differ", lines[0])
    assert m and [int(g) for g in m.groups()] == [cut, n_lengths, n_lengths * 8 * 8 * 2], lines[0]
    n_rows = sum(len(lens) for lens, _ in offset_lists())
    m = re.match(r"(\d+) offset lists, (\d+) rows, largest total (\d+), 0 wrong", lines[1])
    assert m and [int(g) for g in m.groups()] == [len(totals), n_rows, max(totals)], lines[1]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-4000:]


def test_cut_over_is_a_length_the_heap_can_hold():
    """a string of at most 12 bytes never reaches the heap: a cut-over below 13 would send every heap string to the wave"""
    assert 13 <= cut_over() <= 1 << 20
