"""The cell lists of an obstacle field (contract O1), on the CPU.

csrc/obstacle_cells.h builds, for a list of obstacles (x, y, r), a grid over their footprints and per cell the
obstacles an agent there has to visit so that its obstacle forces keep the flat list's bits.  It is pure host
arithmetic in a header without HIP includes, so a plain g++ program (tests/obstacle_cells/obstacle_cells_main.cpp)
drives it here.  For every accepted case the program checks that every list is ascending without duplicates,
that the pair count is the sum of the footprints' cell ranges, and -- for a lattice of probes, random probes,
probes at the cell boundaries and one ulp either side, at the rim of the obstacles' reach, and outside the box on
all eight sides, next to it and 1e6 away -- that every obstacle which passes the flat loop's pre-test at the probe
is in the list of the probe's cell.  (A dead obstacle, r <= -5, passes that pre-test near its centre and is in no
list by the footprint rule; for it the program checks instead that the flat loop's own d < 5.0 is false, so that
it adds no term in either form.)  No reference counterpart (agent.py walks the whole sensed list).
"""
import os
import subprocess

import pytest

from conftest import PKG, ROOT

SRC = os.path.join(ROOT, "tests", "obstacle_cells", "obstacle_cells_main.cpp")
CSRC = os.path.join(PKG, "csrc")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("obstacle_cells") / "obstacle_cells")
    # (-ffp-contract=off: the library's flag -- the footprints are the arithmetic the device repeats)
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                    "-o", exe, SRC], check=True, capture_output=True, text=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    return p.returncode, p.stdout


def test_program_passes(report):
    rc, out = report
    assert rc == 0 and out.rstrip().endswith("0 failed"), out


@pytest.mark.parametrize("case,m,live", [
    ("m0", 0, 0), ("m1", 1, 1), ("m7", 7, 7), ("m1025", 1025, 1025), ("radii", 17, 15), ("all_dead", 3, 0),
    ("r300_among_small", 41, 41), ("duplicates", 28, 28), ("one_line_x", 30, 30), ("one_line_y", 30, 30),
    ("one_point", 9, 9), ("near_1e9", 50, 50), ("near_minus_1e9", 50, 50), ("outlier", 31, 31)])
def test_lists_cover_the_flat_loop(report, case, m, live):
    assert f"ok {case} m={m} live={live} " in report[1], report[1]


def test_no_live_obstacle_is_one_empty_cell(report):
    for case in ("m0 m=0", "all_dead m=3"):
        assert f"ok {case} live=0 ncx=1 ncy=1 cell=1 pairs=0 longest=0 " in report[1], report[1]


@pytest.mark.parametrize("case,status", [("nan_x", 1), ("inf_y", 1), ("minus_inf_r", 1), ("nan_r", 1),
                                         ("extent_overflows_x", 2), ("extent_overflows_y", 2)])
def test_bad_lists_are_refused_with_nothing_created(report, case, status):
    assert f"ok {case} refused status={status}\n" in report[1], report[1]


def test_too_many_pairs_are_refused_before_any_list(report):
    """200 000 obstacles over an arena of 1 400, 224 of them with r = 1e6: ~890 x 890 cells (the cell cap) that each
    of the 224 reaches, 1.8e8 pairs > 2^26.  Refused by the count, which is arithmetic: no list was allocated."""
    assert "ok too_many_pairs refused status=3\n" in report[1], report[1]


def test_70000_obstacles_of_r_1e6_are_refused_by_the_pair_count(report):
    """70 000 obstacles of r = 1e6 over [0, 1400]^2: the start side (10) does not grow with the radii, so the cell
    cap 4 m + 1024 makes ~530 x 530 cells over the 2e6-wide box and every obstacle reaches all of them -- 2e10
    pairs.  Refused by the count alone: the lists' vectors were never given any memory."""
    assert "case huge_70000 status=3 lists_empty=1 " in report[1], report[1]


def test_header_has_no_hip_includes():
    with open(os.path.join(CSRC, "obstacle_cells.h")) as f:
        inc = [ln.split()[1] for ln in f if ln.startswith("#include")]
    assert inc == ["<cmath>", "<cstdint>", "<new>", "<vector>", '"grid_shape.h"']
