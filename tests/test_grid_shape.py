"""The grid shaping of csrc/grid_shape.h, on the CPU: it refuses a box without a finite extent and ends for
every other one.

shape_grid grows the cells by sqrt(2) until the grid fits its cell cap.  For finite positions whose extent
overflows a double (one agent at -1e308, one at +1e308) the extent is inf, the cell grows to inf, inf / inf
is NaN and the comparison that ends the loop is false for ever: every entry point that grids positions
(swarm_build_rgg, swarm_cell_order, swarm_cell_index, the sensed physics and loop, the auction's task grid)
hung on the host.  The shaping is pure host arithmetic in a header without HIP includes, so a plain g++
program (tests/grid_shape/grid_shape_main.cpp) drives it here, before anything of it runs next to a GPU.
No reference counterpart (agent.py has no grid).
"""
import os
import subprocess

import pytest

from conftest import PKG, ROOT

SRC = os.path.join(ROOT, "tests", "grid_shape", "grid_shape_main.cpp")
CSRC = os.path.join(PKG, "csrc")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("grid_shape") / "grid_shape")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", exe, SRC],
                   check=True, capture_output=True, text=True)
    # a shaping loop that does not end is the defect under test: the limit turns it into a failure
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    return p.returncode, p.stdout


def test_program_passes(report):
    rc, out = report
    assert rc == 0 and out.rstrip().endswith("0 failed"), out


@pytest.mark.parametrize("case", ["x_pm1e308", "y_pm1e308", "both_pm1e308", "dbl_max", "inf_corner", "nan_corner"])
def test_box_without_finite_extent_is_refused(report, case):
    assert f"ok {case} refused\n" in report[1], report[1]


@pytest.mark.parametrize("case", ["extent_1e300", "extent_1e300_x_only", "cell_1e-300_extent_1e308",
                                  "extent_largest_finite", "cell_largest_double", "cell_overflows_while_growing",
                                  "one_row"])
def test_large_finite_boxes_end(report, case):
    assert f"ok {case} ncx=" in report[1], report[1]


def test_zero_extent_is_one_cell(report):
    assert "ok zero_extent ncx=1 ncy=1 cell=1.0000000010000001\n" in report[1], report[1]


def test_sparse_box_grows_its_cells(report):
    """64 agents over 1e4 x 1e4 at radius 1: 4 * 64 + 1024 = 1280 cells at most, so 28 x 28 cells of 2^8.5."""
    assert "ok sparse_64_agents ncx=28 ncy=28 cell=362.03867232955105\n" in report[1], report[1]


def test_header_has_no_hip_includes():
    with open(os.path.join(CSRC, "grid_shape.h")) as f:
        inc = [ln.split()[1] for ln in f if ln.startswith("#include")]
    assert inc == ["<cmath>", "<cstdint>"]
