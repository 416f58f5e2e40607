"""The sender-segment capacities of csrc/tick_segments.h, on the CPU: no workgroup of k_tick is ever dealt
more agents than its segment holds, and the segments do not overlap.

Every workgroup of k_tick (push mode, csrc/protocol.hip) lists the agents that sent something in a segment
of its own; a capacity below what the workgroup can be dealt is an out-of-bounds write on the GPU.  The
capacities are pure host integer arithmetic in a header without HIP includes, so a plain g++ program
(tests/tick_segments/tick_segments_main.cpp) restates how the kernel deals chunks, groups and units to its
workgroups -- with and without the XCD-grouped order -- and checks every combination of
  n           1, 3, 4 095, 4 096, 4 097, 32 767, 32 768 xg +- 1, 1 000 003
  sweep grid  1, 8, 16, 2 560
  SWARM_FSM_RECV_WGS    0 (unset), 1, 8, 1 280
  SWARM_TICK_XCD_GROUP  0 (unset), 1, 2, 3, 5
No reference counterpart (agent.py has no workgroups).
"""
import os
import subprocess

import pytest

from conftest import PKG, ROOT

SRC = os.path.join(ROOT, "tests", "tick_segments", "tick_segments_main.cpp")
CSRC = os.path.join(PKG, "csrc")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tick_segments") / "tick_segments")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", exe, SRC],
                   check=True, capture_output=True, text=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    return p.returncode, p.stdout


def test_no_segment_overflows_or_overlaps(report):
    rc, out = report
    assert rc == 0 and out.rstrip().endswith("0 failed") and "FAIL" not in out, out


def test_every_combination_ran_and_some_are_grouped(report):
    """7 sizes x 16 without the grouped order, 9 sizes x 16 for each of the four group sizes; the grouped
    order takes effect only where both role grids are multiples of 8, which 96 of the combinations are."""
    assert "688 cases, 96 in the grouped order\n" in report[1], report[1]


def test_header_has_no_hip_includes():
    with open(os.path.join(CSRC, "tick_segments.h")) as f:
        inc = [ln.split()[1] for ln in f if ln.startswith("#include")]
    assert inc == ["<algorithm>", "<cstdint>"]
