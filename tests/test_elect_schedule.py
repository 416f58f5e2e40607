"""The election's round schedule (csrc/elect_schedule.h), on the CPU.

Which leader buffer a launch reads and writes once launches and rounds are counted apart, which buffer holds
the final state, and how far a batch runs ahead of the read-back are integer bookkeeping over the history of
per-round change counts; nothing of it touches the device.  The schedule lives in a header without HIP includes,
and a plain g++ program (tests/elect_schedule/elect_schedule_main.cpp) drives it over synthetic histories
(linear and geometric decay, a long flat noisy tail, one that never reaches zero; first zero round R in 1..12,
255..260, 510..516 and 1100; max_rounds around R; 0/1/2/9/10 dense rounds; look-ahead 0/1/8/64; both modes;
with and without the initial copies; pair rounds off, from the first sparse round, from the middle of a run and
never; the one-workgroup tail adopted and handed back) against a model of the two leader buffers written from
the rules in elect.hip's header comment.  No reference counterpart (agent.py has no rounds to schedule).
"""
import os
import re
import subprocess

import pytest

from conftest import PKG, ROOT

SRC = os.path.join(ROOT, "tests", "elect_schedule", "elect_schedule_main.cpp")
CSRC = os.path.join(PKG, "csrc")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("elect_schedule") / "elect_schedule")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", exe, SRC],
                   check=True, capture_output=True, text=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    return p.returncode, p.stdout


def figure(out, name):
    m = re.search(r"^%s (\d+)$" % name, out, re.M)
    assert m, out
    return int(m.group(1))


def test_program_passes(report):
    """Coverage of the rounds, guard rounds, buffer preconditions, reads of launched rounds only, the final state
    in `leader`, rounds_exec and converged: every case."""
    rc, out = report
    assert rc == 0 and out.rstrip().endswith("\n0 failed"), out


@pytest.mark.parametrize("family", ["ended_on_pair_first_round", "ended_on_pair_second_round",
                                    "cut_in_pair_mode_odd_launches", "cut_in_pair_mode_even_launches"])
def test_no_pair_ending_is_empty(report, family):
    assert figure(report[1], family) > 0, report[1]


@pytest.mark.parametrize("family", ["pair_switch_on_first_sparse_batch", "pair_switch_through_trend_cap",
                                    "pair_switch_never", "tail_adopted", "tail_handed_back", "tail_refused_first",
                                    "final_copy_from_buffer_1"])
def test_no_other_family_is_empty(report, family):
    assert figure(report[1], family) > 0, report[1]


def test_launches_stay_less_than_half_the_ring_ahead(report):
    """The newest launched round is never kRing/2 = 256 or more rounds ahead of read_upto (the program fails a
    case that gets there): round t recycles the counter slot of round t - 256, read by then with a round to
    spare.  The longest batches reach 255."""
    assert figure(report[1], "max_rounds_ahead_of_read_upto") == 255, report[1]


def test_header_has_no_hip_includes():
    with open(os.path.join(CSRC, "elect_schedule.h")) as f:
        text = f.read()
    inc = [ln.split()[1] for ln in text.split("\n") if ln.startswith("#include")]
    assert inc == ["<algorithm>", "<climits>", "<cstddef>", "<cstdint>", "<vector>"]
    assert "getenv" not in text
