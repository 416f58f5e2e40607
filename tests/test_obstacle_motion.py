"""The host arithmetic of moving obstacle fields (contract O2), on the CPU.

csrc/obstacle_motion.h plans a call over a moving field: the call's grid (over the live footprints at entry and
wherever the velocities put them) and the capacity of the device builder's pair buffers, a bound from the radii and
the grid alone.  It is pure host arithmetic in a header without HIP includes, so a plain g++ program
(tests/obstacle_motion/obstacle_motion_main.cpp) drives it here: it iterates the contract's advance exactly and
checks, per tick, that the counted pairs never exceed the capacity, that no obstacle's per-axis cell range exceeds
its per-axis bound (also snapped to the cell boundaries, one ulp either side), and that the call's box holds every
footprint of every tick.  No reference counterpart (the reference's obstacles do not move).
"""
import os
import subprocess

import pytest

from conftest import PKG, ROOT

SRC = os.path.join(ROOT, "tests", "obstacle_motion", "obstacle_motion_main.cpp")
CSRC = os.path.join(PKG, "csrc")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("obstacle_motion") / "obstacle_motion")
    # (-ffp-contract=off: the library's flag -- the advance is the arithmetic the device repeats)
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                    "-o", exe, SRC], check=True, capture_output=True, text=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    return p.returncode, p.stdout


def test_program_passes(report):
    rc, out = report
    assert rc == 0 and out.rstrip().endswith("0 failed"), out


@pytest.mark.parametrize("case,m,live,ticks", [
    ("random_300", 300, 300, 40), ("random_1025", 1025, 1025, 25), ("m1", 1, 1, 30), ("m0", 0, 0, 10),
    ("radii", 200, None, 20), ("near_1e9", 100, 100, 30), ("near_minus_1e9", 100, None, 30),
    ("one_line", 30, 30, 30), ("one_line_across", 30, 30, 30), ("velocity_zero", 300, 300, 30),
    ("velocity_null", 300, 300, 30), ("all_leave_the_entry_box", 64, 64, 50), ("all_dead", 3, 0, 10),
    ("negative_dt", 50, 50, 20), ("many_ticks", 20, 20, 2000)])
def test_capacity_and_box_hold_on_every_tick(report, case, m, live, ticks):
    line = [ln for ln in report[1].splitlines() if ln.startswith(f"ok {case} m={m} ")]
    assert len(line) == 1, report[1]
    assert f" ticks={ticks} " in line[0]
    if live is not None:
        assert f" live={live} " in line[0]
    f = dict(kv.split("=") for kv in line[0].split()[2:])
    assert int(f["max_pairs"]) <= int(f["capacity"])


def test_every_obstacle_leaves_the_entry_box_in_that_case(report):
    assert " m=64 live=64 ticks=50 " in report[1] and "left_entry_box=64\n" in report[1], report[1]


@pytest.mark.parametrize("case,status", [("nan_velocity", 1), ("inf_velocity", 1), ("nan_entry", 1),
                                         ("extent_overflows", 2), ("product_overflows", 2), ("bound_over_2_26", 3)])
def test_bad_calls_are_refused_with_nothing_planned(report, case, status):
    assert f"ok {case} refused status={status}\n" in report[1], report[1]


def test_header_has_no_hip_includes():
    with open(os.path.join(CSRC, "obstacle_motion.h")) as f:
        inc = [ln.split()[1] for ln in f if ln.startswith("#include")]
    assert inc == ["<cmath>", "<cstdint>", '"obstacle_cells.h"']
