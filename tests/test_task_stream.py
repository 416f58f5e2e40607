"""Task boards that reuse the slots of closed tasks (contract U1-P): swarm_board_place /
swarm_board_last_tick, Swarm.place_board_tasks / board_free_slots.

Between calls a slot whose task was absent at the last two ticks run takes a new task (position, requirement,
velocity, window), and every claim-table entry about the slot is purged unless keep_tables.  The yardstick is
tests/loop_stream_model.py, a thin driver over the unchanged loop_lifetimes_model in two forms: the board of T slots
with places between segments, and the "virtual" board with one index per life.  tests/golden/
loop_stream_board_n200.npz comes from real SwarmAgent objects whose arrivals get fresh dict keys
(tools/gen_golden_task_stream.py).  The GPU must equal the slot form with its own x*x squares bit for bit over its
storage order.
"""
import ctypes
import os
import subprocess
import types

import numpy as np
import pytest

from conftest import PKG, ROOT, load_golden
import board_census_model as bcm
import loop_lifetimes_model as llm
import loop_stream_model as lsm
from loop_model import OUT_KEYS
from test_moving_tasks import _check, _result, _run
from test_update_loop_board import ROWS, _assert_rows, _rows, _storage_case
from test_update_loop_sensed import EXACT, _state
from test_update_loop_tasks import _hand, _kw, _swarm

CSRC = os.path.join(PKG, "csrc")
OPEN, TENTATIVE, LOCKED, ASSIGNED = 0, 1, 2, 3
FIXTURE = "loop_stream_board_n200"
FOREVER = lsm.FOREVER
FAR = 10 ** 6  # a window that opens long after every run here


def _place(slot, pos, open_tick, close_tick, tick, life=None, vel=None, req=None):
    slot = np.atleast_1d(np.asarray(slot, np.int64))
    m = len(slot)
    full = lambda v, d: np.full(m, d, np.int64) if v is None else np.broadcast_to(np.asarray(v, np.int64), (m,)).copy()  # noqa: E731
    return dict(tick=int(tick), slot=slot, life=full(life, -1), pos=np.asarray(pos, np.float64).reshape(m, 2),
                vel=np.zeros((m, 2)) if vel is None else np.asarray(vel, np.float64).reshape(m, 2), req=full(req, -1),
                open=full(open_tick, 0), close=full(close_tick, 0))


def _number_lives(T, places):
    """Fresh life numbers T, T + 1, ... in the order of the places."""
    nxt = T
    for e in places:
        e["life"] = np.arange(nxt, nxt + len(e["slot"]))
        nxt += len(e["slot"])
    return places


def _hand2():
    """Claimer A (ID 1, bit 0) at the origin, leader R (ID 9, without the capability) at (0, 2); two slots, three
    lives, all needing bit 0: life 0 in slot 0 at distance 1 (U = 50) closes at tick 3, life 1 in slot 1 never
    closes, life 2 takes slot 0 after tick 4 at distance 1.5 (U = 40), open from tick 5.  (A run of t ticks ends
    with the places after tick t made.)"""
    g = _hand([(0, 0), (0, 2)], [1, 9], lead=(1,), caps=[1, 0], tasks=[(1, 0, 0), (0, 1, 0)])
    init = dict(pos=np.array([[1.0, 0.0], [0.0, 1.0]]), vel=np.zeros((2, 2)), req=np.array([0, 0]),
                open=np.array([0, 0], np.int64), close=np.array([3, FOREVER], np.int64))
    places = [_place([0], [[-1.5, 0.0]], 5, FOREVER, tick=4, life=[2], req=[0])]
    return g, init, places


def _hand_three_agents():
    """The same with a new claimant: A (ID 1) at the origin, C (ID 2) at (3, 0), both with bit 0, leader R (ID 9) at
    (1.5, 1.5) hears both.  Life 0 in slot 0 at (-1.5, 0) is A's (U = 40; C is 4.5 away: no claim) and closes at
    tick 3; life 1 in slot 1 is far from everyone; life 2 takes slot 0 after tick 4 at (4.5, 0): C's (U = 40)."""
    g = _hand([(0, 0), (3, 0), (1.5, 1.5)], [1, 2, 9], lead=(2,), caps=[1, 1, 0], tasks=[(-1.5, 0, 0), (100, 100, 0)])
    init = dict(pos=np.array([[-1.5, 0.0], [100.0, 100.0]]), vel=np.zeros((2, 2)), req=np.array([0, 0]),
                open=np.array([0, 0], np.int64), close=np.array([3, FOREVER], np.int64))
    places = [_place([0], [[4.5, 0.0]], 5, FOREVER, tick=4, life=[2], req=[0])]
    return g, init, places


# ----------------------------------------------------------------------------- CPU

def test_exports_and_struct_sizes():
    from swarm_amd import _lib
    lib = _lib.load()
    for name in ("swarm_board_place", "swarm_board_last_tick"):
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert ctypes.sizeof(_lib.BoardState) == 64 and ctypes.sizeof(_lib.BoardDesc) == 56
    assert len(lib.swarm_board_place.argtypes) == 14 and len(lib.swarm_board_last_tick.argtypes) == 2
    assert _lib.PLACE_KEEP_TABLES == 1
    with open(os.path.join(ROOT, "include", "swarm.h")) as f:
        text = f.read()
    assert "int swarm_board_place(swarm_ctx *ctx, swarm_board *board, int64_t n, const swarm_board_state *state," in text
    assert "int swarm_board_last_tick(const swarm_board *board, int64_t *last_tick);" in text
    assert "#define SWARM_PLACE_KEEP_TABLES 1u" in text


def test_entry_points_refuse_bad_arguments_without_a_device():
    from swarm_amd import _lib
    from swarm_amd.swarm import Swarm
    lib = _lib.load()
    fake = ctypes.c_void_p(8)  # never dereferenced: the arguments below are refused first
    st = _lib.BoardState(4, 4, None, fake, fake, fake, fake, fake, fake)
    out = ctypes.c_int64(-5)

    def place(ctx=fake, board=fake, n=3, state=st, m=1, arrays=(fake,) * 6, flags=0):
        return lib.swarm_board_place(ctx, board, n, ctypes.byref(state) if state is not None else None, m, *arrays,
                                     flags, ctypes.byref(out), None)
    for kw, text in ((dict(ctx=None), "ctx, board or state is NULL"), (dict(board=None), "ctx, board or state is NULL"),
                     (dict(state=None), "ctx, board or state is NULL"), (dict(flags=2), "unknown flag"),
                     (dict(flags=1 << 31), "unknown flag"), (dict(n=-1), "n must be in"), (dict(n=1 << 31), "n must be in"),
                     (dict(m=-1), "m must not be negative"),
                     (dict(arrays=(None, fake, fake, fake, fake, fake)), "NULL request array"),
                     (dict(arrays=(fake, None, fake, fake, fake, fake)), "NULL request array"),
                     (dict(arrays=(fake, fake, None, fake, fake, fake)), "NULL request array"),
                     (dict(arrays=(fake, fake, fake, fake, None, fake)), "NULL request array"),
                     (dict(arrays=(fake, fake, fake, fake, fake, None)), "NULL request array"),
                     (dict(state=_lib.BoardState(0, 4, None, fake, fake, fake, fake, fake, fake)), "slots must be in"),
                     (dict(state=_lib.BoardState(4, 4097, None, fake, fake, fake, fake, fake, fake)), "slots must be in"),
                     (dict(state=_lib.BoardState(4097, 1, None, fake, fake, fake, fake, fake, fake)), "slots must be in"),
                     (dict(state=_lib.BoardState(4, 0, None, fake, fake, fake, fake, fake, fake)), "slots must be in")):
        assert place(**kw) == _lib.ERR_ARG and text in _lib.last_error(), kw
    assert out.value == -5  # a refusal writes nothing
    t = ctypes.c_int64(-5)
    assert lib.swarm_board_last_tick(None, ctypes.byref(t)) == _lib.ERR_ARG
    assert lib.swarm_board_last_tick(fake, None) == _lib.ERR_ARG and t.value == -5
    # the Python layer, before the device is touched
    s = Swarm.__new__(Swarm)
    s.n, s.device = 4, "cpu"
    with pytest.raises(RuntimeError, match="no task board"):
        s.place_board_tasks([0], [1.0], [1.0])
    with pytest.raises(RuntimeError, match="no task board"):
        s.board_free_slots()
    s.board = dict(moving=False, T=4)
    with pytest.raises(RuntimeError, match="needs a task board with lifetimes"):
        s.place_board_tasks([0], [1.0], [1.0])
    s.board = dict(moving=True, T=4)
    with pytest.raises(RuntimeError, match="needs a task board with lifetimes"):
        s.board_free_slots()
    # slot 0 closed at 8, slot 1 closes at 9 (heard at the last tick), slot 2 opens later, slot 3 is never present
    s.board = dict(moving=True, T=4, life=(np.array([0, 2, 12, 6]), np.array([8, 9, 20, 6])))
    s.board_task_ids = np.arange(4)
    s.fsm_tick = 9
    np.testing.assert_array_equal(s.board_free_slots(), [0, 2, 3])
    np.testing.assert_array_equal(s.board_free_slots(8), [2, 3])
    np.testing.assert_array_equal(s.board_free_slots(10), [0, 1, 2, 3])
    np.testing.assert_array_equal(s.board_free_slots(12), [0, 1, 3])
    for args, kw, text in ((([4], [1.0], [1.0]), {}, r"a slot outside \[0, 4\)"), (([-1], [1.0], [1.0]), {}, "a slot outside"),
                           (([0, 0], [1.0, 2.0], [1.0, 2.0]), {}, "listed twice"),
                           (([0.5], [1.0], [1.0]), {}, "integer slots"),
                           (([0], [1.0, 2.0], [1.0]), {}, "expected 1 values each"),
                           (([0], [np.nan], [1.0]), {}, "must be finite"), (([0], [1.0], [np.inf]), {}, "must be finite"),
                           (([0], [1.0], [1.0], [32]), {}, r"treq must be in \[-1, 31\]"),
                           (([0], [1.0], [1.0], [-2]), {}, r"treq must be in"),
                           (([0], [1.0], [1.0], [1, 2]), {}, "treq: expected 1 values"),
                           (([0], [1.0], [1.0]), dict(velocities=[[np.nan, 0.0]]), "velocities must be finite"),
                           (([0], [1.0], [1.0]), dict(velocities=[[0.0, 0.0, 0.0]]), "velocities: expected shape"),
                           (([0], [1.0], [1.0]), dict(open_tick=9), "opens at or before the last tick run"),
                           (([0, 2], [1.0, 1.0], [1.0, 1.0]), dict(open_tick=[10, 3]), "task 1 opens at or before"),
                           (([0], [1.0], [1.0]), dict(open_tick=12, close_tick=11), "opens after it closes"),
                           (([0], [1.0], [1.0]), dict(close_tick=-1), "must not be negative"),
                           (([0], [1.0], [1.0]), dict(open_tick=[10.5]), "integer ticks"),
                           (([0], [1.0], [1.0]), dict(task_ids=[1, 2]), "task_ids: expected 1 keys"),
                           (([1], [1.0], [1.0]), {}, "slot 1 is not free"),
                           (([0, 3, 1], [1.0] * 3, [1.0] * 3), {}, "slot 1 is not free")):
        with pytest.raises(ValueError, match=text):
            s.place_board_tasks(*args, **kw)
    assert s.place_board_tasks([], [], []) == {"purged": 0, "next_tick": 10}  # m == 0 touches nothing


@pytest.fixture(scope="module")
def place_report(tmp_path_factory):
    """The placing header through a plain host program, with the address and undefined-behaviour sanitizers on that
    program only."""
    exe = str(tmp_path_factory.mktemp("task_place") / "task_place")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "task_place", "task_place_main.cpp")], check=True, capture_output=True,
                   text=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    return p.returncode, p.stdout + p.stderr


def test_task_place_program_passes(place_report):
    rc, out = place_report
    assert rc == 0 and out.rstrip().endswith("0 failed") and "FAIL" not in out and "runtime error" not in out, out


@pytest.mark.parametrize("case", [
    "eligible_closed_at_last_minus_2", "eligible_closed_at_last_minus_1", "busy_closed_at_last",
    "busy_last_tick_of_the_window", "busy_open_at_last", "eligible_opens_after_last", "busy_one_tick_window_at_last",
    "open_equals_close_always_eligible", "forever_is_never_eligible_once_open", "near_max_close", "near_max_open",
    "last_zero", "eligible_iff_absent_at_last_and_the_tick_before", "request_ok", "request_index", "request_busy",
    "request_negative", "request_early", "request_order", "request_non_finite", "request_req",
    "list_names_the_first_bad_request", "list_then_the_next", "list_ok_with_null_velocities", "list_empty",
    "no_duplicate", "duplicate_found", "closes_by_hand", "closes_empty", "closes_all_dropped",
    "closes_random_sequences_equal_the_recomputation", "closes_cover_every_close_to_come", "reasons_have_text"])
def test_task_place_cases(place_report, case):
    assert f"ok {case}\n" in place_report[1], place_report[1]


def test_task_place_header_has_no_hip_includes():
    with open(os.path.join(CSRC, "task_place.h")) as f:
        inc = [ln.split()[1] for ln in f if ln.startswith("#include")]
    assert inc == ["<algorithm>", "<cmath>", "<cstdint>", "<iterator>", "<vector>"]


_cpu = {}


def _fixture_models(oracle_mod):
    """The fixture through the slot form (purge and keep_tables) and the virtual form, with pow: once."""
    if not _cpu:
        g = load_golden(FIXTURE)
        init, places, T = lsm.case_from_fixture(g)
        first, ticks = int(g["task_tick"]) - 1, int(g["ticks"])
        kw = dict(first=first, use_pow=True)
        _cpu.update(g=g, init=init, places=places, T=T, a=lsm.drive_slots(oracle_mod, g, init, places, ticks, **kw),
                    v=lsm.drive_virtual(oracle_mod, g, init, places, ticks, **kw),
                    k=lsm.drive_slots(oracle_mod, g, init, places, ticks, keep_tables=True, **kw))
    return _cpu


def test_slot_model_with_pow_equals_the_fixture(oracle_mod):
    """Real agents, fresh dict keys: the slot form equals their run, read through the slot map."""
    c = _fixture_models(oracle_mod)
    g, a, T = c["g"], c["a"], c["T"]
    o, life = a["o"], a["life"]
    assert g["status_out"].shape == (200, 680) and T == 120 and int(g["task_seed"]) == 5150
    for k in OUT_KEYS:  # the thirteen arrays
        np.testing.assert_array_equal(o[k], g[k + "_out"], err_msg=k)
    for k in ("status", "tab_winner"):
        np.testing.assert_array_equal(o[k], g[k + "_out"][:, life], err_msg=k)
    np.testing.assert_array_equal(o["tab_util"].view(np.uint32), g["tab_util_out"][:, life].view(np.uint32))
    np.testing.assert_array_equal(np.concatenate(a["acc"]["counts"]), g["counts"])
    np.testing.assert_array_equal(np.concatenate(a["acc"]["task_counts"]), g["task_counts"])
    np.testing.assert_array_equal(a["cur"][:, 0], g["task_x_end"][life])
    np.testing.assert_array_equal(a["cur"][:, 1], g["task_y_end"][life])
    # the last two ticks' message records: the reference's keys are lives, the board's are slots
    slot = np.asarray(g["life_slot"], np.int64)
    want = {key: [[set() for _ in range(200)] for _ in range(2)] for key in ("claim_idx", "conflict_idx")}
    for key in want:
        for h, i, k in g[key]:
            want[key][h][i].add(int(slot[k]))
    end = int(g["ticks"])
    view = lsm.slot_view(a)
    for key, cur, prev in (("claim_idx", "claims", "claims_prev"), ("conflict_idx", "conflicts", "conflicts_prev")):
        assert [sorted(x) for x in want[key][end & 1]] == view[cur], key
        assert [sorted(x) for x in want[key][(end - 1) & 1]] == view[prev], key
    # the generator's conditions, on the reference's run and on the model's
    n = dict(zip(("lives", "placed", "waited", "most", "reuses", "stale_reuses", "stale_entries", "other_winner",
                  "within", "handled", "guard"), (int(v) for v in g["stream_counts"])))
    assert sorted(set(g["status_out"].ravel().tolist())) == [0, 1, 2, 3] and sorted(set(o["status"].ravel().tolist())) == [0, 1, 2, 3]
    assert n["lives"] == 630 and n["placed"] == 560 and n["most"] >= 3 and n["waited"] >= 1 and n["guard"] == 0
    assert n["stale_reuses"] >= 1 and n["other_winner"] >= 1 and n["within"] >= 1
    assert n["handled"] == g["task_counts"][:, 1].sum() >= 100
    assert len(a["stale"]) == n["stale_entries"] == sum(a["purged"]) and len({(p, k) for p, k, _, _ in a["stale"]}) == n["stale_reuses"]
    assert a["acc"]["guard"] == 0 and a["acc"]["singular"] == 0 and lsm.peaks(a)[0] <= 16 and lsm.peaks(a)[1] <= 16
    assert np.bincount(slot[np.asarray(g["open_tick"]) != np.asarray(g["close_tick"])]).max() == n["most"]
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", FIXTURE + ".npz")) < 400000


def test_slot_model_equals_the_virtual_model(oracle_mod):
    """Contract U1-P.4 with no device involved: places with purge are the board with one index per life."""
    c = _fixture_models(oracle_mod)
    a, v = c["a"], c["v"]
    lsm.assert_same(lsm.slot_view(a), lsm.to_slots(v, a["life"]))
    lsm.assert_same_counts(a, v)
    for k in OUT_KEYS:
        np.testing.assert_array_equal(a["o"][k], v["o"][k], err_msg=k)
    g = c["g"]
    np.testing.assert_array_equal(v["o"]["status"], g["status_out"])  # the virtual form is the reference's own run
    np.testing.assert_array_equal(v["o"]["tab_winner"], g["tab_winner_out"])
    assert v["o"]["status"].shape[1] == 680 and a["o"]["status"].shape[1] == 120
    # the virtual tables keep what the slot form purged
    dead = np.setdiff1d(np.arange(680), a["life"])
    assert (v["o"]["tab_winner"][:, dead] >= 0).sum() >= sum(a["purged"]) > 100


def test_keep_tables_differs_from_purge_on_the_fixture(oracle_mod):
    """The purge matters: with the tables kept a new life meets its slot's old winner and utility."""
    c = _fixture_models(oracle_mod)
    a, k = c["a"], c["k"]
    assert sum(k["purged"]) == 0 and len(k["stale"]) >= len(a["stale"])
    ta, tk = np.concatenate(a["acc"]["task_counts"]), np.concatenate(k["acc"]["task_counts"])
    assert (ta != tk).any()  # conflicts that a stale entry swallowed
    assert (a["o"]["tab_winner"] != k["o"]["tab_winner"]).sum() > 50
    with pytest.raises(AssertionError):
        lsm.assert_same(lsm.slot_view(k), lsm.to_slots(c["v"], k["life"]))


def test_two_agents_two_slots_three_lives_by_hand(oracle_mod):
    """Slot 0 is reused while R's table still names life 0's winner with U = 50.  With the purge life 2's claim
    (U = 40) makes a new entry, R sends the conflict and A is ASSIGNED; with keep_tables the claim is 40 <= 50 + 5
    against the stale entry of the same sender: nothing is sent, A stays TENTATIVE for ever and the table keeps 50.
    (With two agents the stale entry's winner is always the new claimant: a leader hears nobody else.)"""
    g, init, places = _hand2()
    sent = {1: [2, 0, 0], 2: [0, 2, 2], 3: [0, 0, 0], 4: [0, 0, 0], 5: [1, 0, 0], 6: [0, 1, 1], 7: [0, 0, 0]}
    a_row = {1: [TENTATIVE, TENTATIVE], 2: [TENTATIVE, TENTATIVE], 3: [OPEN, ASSIGNED], 4: [OPEN, ASSIGNED],
             5: [TENTATIVE, ASSIGNED], 6: [TENTATIVE, ASSIGNED], 7: [ASSIGNED, ASSIGNED]}
    r_win = {1: [-1, -1], 2: [1, 1], 3: [1, 1], 4: [-1, 1], 5: [-1, 1], 6: [1, 1], 7: [1, 1]}
    r_util = {3: [50.0, 50.0], 4: [0.0, 50.0], 5: [0.0, 50.0], 6: [40.0, 50.0], 7: [40.0, 50.0]}
    for t in range(1, 8):
        d = lsm.drive_slots(oracle_mod, g, init, places, t)
        o = d["o"]
        np.testing.assert_array_equal(np.concatenate(d["acc"]["task_counts"])[-1], sent[t], err_msg=str(t))
        np.testing.assert_array_equal(o["status"], [a_row[t], [OPEN, OPEN]], err_msg=str(t))
        np.testing.assert_array_equal(o["tab_winner"], [[-1, -1], r_win[t]], err_msg=str(t))
        if t in r_util:
            np.testing.assert_array_equal(o["tab_util"], np.array([[0.0, 0.0], r_util[t]], np.float32), err_msg=str(t))
    assert d["purged"] == [1] and d["stale"] == [(0, 0, 1, 1)]
    np.testing.assert_array_equal(d["open"], [5, 0])
    np.testing.assert_array_equal(d["close"], [FOREVER, FOREVER])
    rows = lsm.lbm.sparse_state(o, 2, 2)
    np.testing.assert_array_equal(rows["status"], [[0 << 2 | ASSIGNED, 1 << 2 | ASSIGNED], [-1, -1]])
    np.testing.assert_array_equal(rows["tab_task"], [[-1, -1], [0, 1]])
    np.testing.assert_array_equal(rows["conflict_out"], [[[-1, -1], [0, -1]], [[-1, -1]] * 2])  # (tick 6: R's)
    k = lsm.drive_slots(oracle_mod, g, init, places, 7, keep_tables=True)
    sent[6] = [0, 1, 0]  # the claim is handled, nothing is sent
    np.testing.assert_array_equal(np.concatenate(k["acc"]["task_counts"]), [sent[t] for t in range(1, 8)])
    np.testing.assert_array_equal(k["o"]["status"], [[TENTATIVE, ASSIGNED], [OPEN, OPEN]])
    np.testing.assert_array_equal(k["o"]["tab_winner"], [[-1, -1], [1, 1]])
    np.testing.assert_array_equal(k["o"]["tab_util"], np.array([[0.0, 0.0], [50.0, 50.0]], np.float32))
    assert k["purged"] == [0] and k["stale"] == d["stale"]
    # the virtual board: three indices, one window each
    v = lsm.drive_virtual(oracle_mod, g, init, places, 7)
    np.testing.assert_array_equal(v["o"]["status"], [[OPEN, ASSIGNED, ASSIGNED], [OPEN] * 3])
    np.testing.assert_array_equal(v["o"]["tab_winner"], [[-1] * 3, [1, 1, 1]])
    lsm.assert_same(lsm.slot_view(d), lsm.to_slots(v, d["life"]))
    lsm.assert_same_counts(d, v)


def test_three_agents_a_new_claimant_wins_only_with_the_purge(oracle_mod):
    """The new claimant C wins life 2 with the purge; with keep_tables its U = 40 is not above the stale entry's
    40 + 5, R's conflict names the old winner A, and C is LOCKED."""
    g, init, places = _hand_three_agents()
    d = lsm.drive_slots(oracle_mod, g, init, places, 7)
    np.testing.assert_array_equal(d["o"]["status"], [[LOCKED, OPEN], [ASSIGNED, OPEN], [OPEN, OPEN]])  # (A hears R too)
    np.testing.assert_array_equal(d["o"]["tab_winner"], [[-1, -1], [-1, -1], [2, -1]])
    assert d["purged"] == [1] and d["stale"] == [(0, 0, 2, 1)]
    k = lsm.drive_slots(oracle_mod, g, init, places, 7, keep_tables=True)
    np.testing.assert_array_equal(k["o"]["status"], [[ASSIGNED, OPEN], [LOCKED, OPEN], [OPEN, OPEN]])
    np.testing.assert_array_equal(k["o"]["tab_winner"], [[-1, -1], [-1, -1], [1, -1]])
    np.testing.assert_array_equal(np.concatenate(d["acc"]["task_counts"]), np.concatenate(k["acc"]["task_counts"]))
    v = lsm.drive_virtual(oracle_mod, g, init, places, 7)
    lsm.assert_same(lsm.slot_view(d), lsm.to_slots(v, d["life"]))


# ----------------------------------------------------------------------------- GPU

_models = {}


def _board(s, init, Ks, Kt):
    return s.set_task_board(init["pos"][:, 0], init["pos"][:, 1], init["req"], status_slots=Ks, table_slots=Kt,
                            velocities=init["vel"], open_tick=init["open"], close_tick=init["close"])


def _do_place(s, e, keep=False, **kw):
    return s.place_board_tasks(e["slot"], e["pos"][:, 0], e["pos"][:, 1], e["req"], velocities=e["vel"],
                               open_tick=e["open"], close_tick=e["close"], keep_tables=keep, **kw)


def _play(s, g, places, total, *, now=0, cuts=(), keep=False, **kw):
    """Runs the board of s from tick `now` to `total` with the places between the calls (cuts: further call
    boundaries) -> (the joined results, the places' purged counts)."""
    stops = sorted({int(e["tick"]) for e in places if e["tick"] >= now} | {int(c) for c in cuts} | {total})
    rs, purged = [], []
    for stop in stops:
        if stop > now:
            rs.append(_run(s, g, stop - now, **kw))
            now = stop
        for e in places:
            if e["tick"] == stop:
                info = _do_place(s, e, keep)
                assert info["next_tick"] == stop + 1 == s.board_last_tick() + 1
                purged.append(info["purged"])
    return _join(rs), purged


def _join(rs):
    out = dict(counts=np.concatenate([r["counts"] for r in rs]),
               task_counts=np.concatenate([r["task_counts"] for r in rs]), guard=sum(r["guard"] for r in rs),
               singular=sum(r["singular"] for r in rs))
    if "link_counts" in rs[0]:
        out["link_counts"] = np.concatenate([r["link_counts"] for r in rs])
    return out


def _same_swarm(a, b, rows=True):
    import torch
    for t in ("pos", "pos_prev", "vel", "target", "has_target", "state", "leader"):
        assert torch.equal(getattr(a, t), getattr(b, t)), t
    for k in a.fsm:
        assert torch.equal(a.fsm[k], b.fsm[k]), k
    for k in ROWS if rows else ():
        assert torch.equal(a.board[k].view(torch.int32), b.board[k].view(torch.int32)), k


def _fixture_gpu(oracle_mod, layout, loss, keep=False, cuts=()):
    g = load_golden(FIXTURE)
    init, places, T = lsm.case_from_fixture(g)
    first, ticks = int(g["task_tick"]) - 1, int(g["ticks"])
    s = _swarm(g, layout, board=False)
    kw = dict(loss=loss, loss_seed=77) if loss else {}
    r0 = s.update_loop_radio(first, float(g["radio_radius"]), float(g["sense_radius"]), **_kw(g), **kw)
    _board(s, init, 16, 16)
    r1, purged = _play(s, g, places, ticks, now=first, cuts=cuts, keep=keep, **kw)
    key = (layout, loss, keep)
    if key not in _models:  # once per storage order, left unchanged
        q, perm = _storage_case(s, g)
        d = lsm.drive_slots(oracle_mod, q, init, places, ticks, first=first, keep_tables=keep, loss=loss or None,
                            loss_seed=77)
        _models[key] = _result(d, perm, 16, 16), d
    want, d = _models[key]
    r = dict(r1)
    r["counts"] = np.concatenate([r0["counts"], r1["counts"]])
    r["task_counts"] = np.concatenate([np.zeros((first, 3), np.int64), r1["task_counts"]])
    r["singular"] = r0["singular"] + r1["singular"]
    _check(s, r, want)
    if loss:
        np.testing.assert_array_equal(np.concatenate([r0["link_counts"], r1["link_counts"]]), want["link_counts"])
    assert purged == d["purged"] and s.fsm_tick == ticks == s.board_last_tick() and s.last_refused_tick == -1
    for got, w in zip(s.board_lifetimes(), (d["open"], d["close"])):
        np.testing.assert_array_equal(got, w)
    for got, w in zip(s.board["life"], (d["open"], d["close"])):  # the host copy
        np.testing.assert_array_equal(got, w)
    return s, g, r, want, d


# 1. the fixture, both layouts, the ideal channel and a lossy one
@pytest.mark.gpu
@pytest.mark.parametrize("loss", [0.0, 0.2])
@pytest.mark.parametrize("layout", ["input", "spatial"])
def test_gpu_equals_the_slot_model_on_the_fixture(oracle_mod, layout, loss):
    s, g, r, want, d = _fixture_gpu(oracle_mod, layout, loss)
    assert want["task_counts"][:, 1].sum() >= (100 if not loss else 50) and sum(d["purged"]) >= 50
    if layout == "input" and not loss:  # real agents, in everything the squares cannot reach
        got = _state(s)
        for k in EXACT:
            np.testing.assert_array_equal(got[k], g[k + "_out"], err_msg=k)
        life = d["life"]
        rows = _rows(s)
        tt, tw, tu = lsm.lbm.sparse_tables(g["tab_winner_out"][:, life], g["tab_util_out"][:, life], 16)
        np.testing.assert_array_equal(rows["status"], lsm.lbm.sparse_status(g["status_out"][:, life], 16))
        np.testing.assert_array_equal(rows["tab_task"], tt)
        np.testing.assert_array_equal(rows["tab_winner"], tw)
        np.testing.assert_array_equal(r["task_counts"], g["task_counts"])


# 2. the same run as 1-tick chunks and as uneven chunks; 3. keep_tables
@pytest.mark.gpu
@pytest.mark.parametrize("cuts", ["every tick", "uneven"])
def test_gpu_chunked_run_with_the_same_places_is_the_same_run(oracle_mod, cuts):
    cuts = range(45, 260) if cuts == "every tick" else (50, 51, 64, 131, 257)
    _fixture_gpu(oracle_mod, "spatial", 0.0, cuts=cuts)


@pytest.mark.gpu
def test_gpu_keep_tables_equals_the_model_and_differs_from_the_purge(oracle_mod):
    s, g, r, want, d = _fixture_gpu(oracle_mod, "spatial", 0.0, keep=True)
    assert d["purged"] == [0] * len(d["purged"])
    if ("spatial", 0.0, False) in _models:
        other = _models["spatial", 0.0, False][0]
        assert (other["task_counts"] != want["task_counts"]).any()


# 4. swarm sizes around the workgroup; boards of 1 and 65 slots
def _random_stream(n, T, seed, ticks=30):
    rng = np.random.default_rng(seed)
    side = max(np.sqrt(n * np.pi * 2.5 ** 2 / 12.0), 3.0)
    g = _hand(np.stack([rng.uniform(0, side, n), rng.uniform(0, side, n)], 1), rng.permutation(n) + 1,
              lead=tuple(range(0, n, 9)), caps=rng.integers(0, 8, n))
    spot = lambda m: np.stack([rng.uniform(-2.0, side + 2.0, m), rng.uniform(-2.0, side + 2.0, m)], 1).reshape(m, 2)  # noqa: E731
    there = rng.uniform(size=T) < 0.6
    lo = np.where(there, 0, 0).astype(np.int64)
    hi = np.where(there, rng.integers(3, 10, T), 0).astype(np.int64)
    init = dict(pos=spot(T), vel=rng.uniform(-3.0, 3.0, (T, 2)), req=rng.integers(-1, 3, T), open=lo.copy(),
                close=hi.copy())
    g.update(task_x=init["pos"][:, 0].copy(), task_y=init["pos"][:, 1].copy(), task_req=init["req"].astype(np.int8),
             ticks=np.int64(ticks))
    places = []
    for last in range(2, ticks - 2, 3):
        free = np.flatnonzero(lsm.eligible(lo, hi, last))
        k = free[rng.uniform(size=len(free)) < 0.7]
        if not len(k):
            continue
        o = last + 1 + rng.integers(0, 2, len(k))
        c = np.where(rng.uniform(size=len(k)) < 0.1, FOREVER, o + rng.integers(0, 9, len(k)))
        lo[k], hi[k] = o, c
        places.append(_place(k, spot(len(k)), o, c, tick=last, vel=rng.uniform(-3.0, 3.0, (len(k), 2)),
                             req=rng.integers(-1, 3, len(k))))
    return g, init, _number_lives(T, places)


@pytest.mark.gpu
@pytest.mark.parametrize("n,T", [(1, 40), (255, 40), (256, 40), (257, 40), (120, 1), (120, 65)])
def test_gpu_swarm_and_board_sizes_equal_the_model(oracle_mod, n, T):
    g, init, places = _random_stream(n, T, 100 * n + T)
    s = _swarm(g, "spatial", board=False)
    _board(s, init, T, T)
    q, perm = _storage_case(s, g)
    d = lsm.drive_slots(oracle_mod, q, init, places, 30)
    want = _result(d, perm, T, T)
    r, purged = _play(s, g, places, 30)
    _check(s, r, want)
    assert purged == d["purged"] and len(places) >= (5 if T > 1 else 1)
    assert want["task_counts"][:, 0].sum() > 0 and (n == 1 or want["task_counts"][:, 1].sum() > 0)
    assert n == 1 or T == 1 or sum(purged) > 0
    assert T == 1 or np.bincount(np.concatenate([e["slot"] for e in places])).max() >= 2  # a slot placed twice


# 5. the purge pass on table rows set by hand
@pytest.mark.gpu
@pytest.mark.parametrize("Kt", [1, 5, 64, 67, 130, 4096])
def test_gpu_purge_pass_on_rows_set_by_hand(Kt):
    """Tasks far from every agent and never present, table rows written by hand with guard words behind each of the
    three arrays: row 0 full and purged whole; row 1 full, losing every second entry; row 2 full, losing nothing;
    row 3 holds an entry outside [0, T), which is kept; the rest random.  First a place of two slots no row names
    (nothing purged: every byte as it was), then the place that purges."""
    import torch
    n, T, G = 70, 3 * Kt + 2, 64
    rng = np.random.default_rng(Kt)
    g = _hand(np.stack([rng.uniform(0, 6, n), rng.uniform(0, 6, n)], 1), rng.permutation(n) + 1, lead=(0, 9))
    Q0 = np.stack([rng.uniform(500, 600, T), rng.uniform(500, 600, T)], 1)
    k = np.arange(T)
    placed = (k < Kt) | ((k < 2 * Kt) & ((k - Kt) % 2 == 0))  # the first Kt slots, every second of the next Kt
    held = [np.arange(Kt), Kt + np.arange(Kt), 2 * Kt + np.arange(Kt)] + \
        [np.sort(rng.choice(3 * Kt, rng.integers(0, Kt + 1), replace=False)) for _ in range(n - 3)]
    if Kt > 1:
        held[3] = np.concatenate([held[3][:Kt - 1], [T + 7]])
    rows = {key: np.full((n, Kt), fill, dt) for key, fill, dt in (("tab_task", -1, np.int32), ("tab_winner", -1, np.int32),
                                                                  ("tab_util", 0, np.float32))}
    want = {key: v.copy() for key, v in rows.items()}
    removed = 0
    for i, tasks in enumerate(held):
        w, u = rng.integers(1, 1000, len(tasks)), rng.uniform(20, 100, len(tasks)).astype(np.float32)
        rows["tab_task"][i, :len(tasks)], rows["tab_winner"][i, :len(tasks)], rows["tab_util"][i, :len(tasks)] = tasks, w, u
        keep = ~((tasks < T) & placed[np.minimum(tasks, T - 1)])
        removed += int((~keep).sum())
        want["tab_task"][i, :keep.sum()], want["tab_winner"][i, :keep.sum()] = tasks[keep], w[keep]
        want["tab_util"][i, :keep.sum()] = u[keep]
    assert (want["tab_task"][0] == -1).all() and (want["tab_task"][2] == rows["tab_task"][2]).all()
    assert Kt == 1 or ((want["tab_task"][1] >= 0).sum() == Kt // 2 and (want["tab_task"][3:] != rows["tab_task"][3:]).any())
    assert Kt == 1 or (want["tab_task"][3] == T + 7).sum() == 1
    s = _swarm(g, "input", board=False)
    s.set_task_board(Q0[:, 0], Q0[:, 1], None, status_slots=4, table_slots=Kt, open_tick=0, close_tick=0)
    _run(s, g, 1)  # a tick has run: the lifetimes are no longer fresh (and the rows below never meet an entry check)
    big = {}
    for key, v in rows.items():  # each array in front of G guard words
        flat = torch.full((n * Kt + G,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        flat[:n * Kt] = torch.as_tensor(v.view(np.int32).ravel(), device="cuda")
        big[key] = flat
        s.board[key] = flat[:n * Kt].view(n, Kt).view(torch.float32 if key == "tab_util" else torch.int32)
    before = {key: v.clone() for key, v in big.items()}
    info = s.place_board_tasks([T - 2, T - 1], [1.0, 2.0], [3.0, 4.0], open_tick=FAR)
    assert info == {"purged": 0, "next_tick": 2}
    for key in big:  # nothing purged: the rows' bytes and the guard words unchanged
        assert torch.equal(big[key], before[key]), key
    idx = np.flatnonzero(placed)
    info = s.place_board_tasks(idx, np.full(len(idx), 550.0), np.full(len(idx), 550.0), open_tick=FAR)
    assert info["purged"] == removed
    for key in big:
        got = big[key].cpu().numpy()
        np.testing.assert_array_equal(got[:n * Kt].reshape(n, Kt), want[key].view(np.int32), err_msg=key)
        assert (got[n * Kt:] == 0x5A5A5A5A).all(), key
    assert (s.board["status"] == -1).all() and (s.board["claim_out"] == -1).all()
    again = s.place_board_tasks(idx, np.full(len(idx), 551.0), np.full(len(idx), 551.0), open_tick=FAR)
    assert again["purged"] == 0  # (a slot that opens later is free: placed again, nothing left to purge)
    for key in big:
        np.testing.assert_array_equal(big[key].cpu().numpy()[:n * Kt].reshape(n, Kt), want[key].view(np.int32), err_msg=key)


# 6. m = 0, m = 1 and m = T
@pytest.mark.gpu
def test_gpu_place_none_one_and_every_slot():
    g, init, _ = _random_stream(40, 5, 7)
    s = _swarm(g, "input", board=False)
    init.update(open=np.zeros(5, np.int64), close=np.zeros(5, np.int64))
    _board(s, init, 4, 4)
    _run(s, g, 2)
    life, pos = s.board_lifetimes(), s.board_positions()
    assert s.place_board_tasks([], [], []) == {"purged": 0, "next_tick": 3}
    for got, w in zip(s.board_lifetimes() + s.board_positions(), life + pos):
        np.testing.assert_array_equal(got, w)
    np.testing.assert_array_equal(s.board_free_slots(), np.arange(5))
    s.place_board_tasks([3], [1.5], [2.5], [2], velocities=[[0.5, -0.5]], open_tick=4, close_tick=9)
    lo, hi = s.board_lifetimes()
    np.testing.assert_array_equal(lo, [0, 0, 0, 4, 0])
    np.testing.assert_array_equal(hi, [0, 0, 0, 9, 0])
    cur, lag = s.board_positions()
    np.testing.assert_array_equal(cur[3], [1.5, 2.5])
    np.testing.assert_array_equal(lag[3], [1.5, 2.5])
    np.testing.assert_array_equal(np.delete(cur, 3, 0), np.delete(pos[0], 3, 0))
    x = np.arange(5) + 0.25
    s.place_board_tasks(np.arange(5)[::-1], x, -x, open_tick=3)  # every slot, in descending order
    cur, lag = s.board_positions()
    np.testing.assert_array_equal(cur, np.stack([x, -x], 1)[::-1])
    np.testing.assert_array_equal(lag, cur)
    lo, hi = s.board_lifetimes()
    assert (lo == 3).all() and (hi == FOREVER).all()
    assert len(s.board_free_slots()) == 5  # (a slot that has not opened yet may still be given to another task)
    r = _run(s, g, 3)
    assert not len(s.board_free_slots())
    np.testing.assert_array_equal(s.board_positions()[0], cur)  # at rest: the velocities were replaced by zero
    assert r["task_counts"].shape == (3, 3) and s.board_last_tick() == 5


# 7. a place followed by a status overflow; grow_board and the repeated call
@pytest.mark.gpu
def test_gpu_overflow_after_a_place_restores_the_placed_board(oracle_mod):
    import torch
    from swarm_amd import _lib
    g, init, places = _hand2()
    places = [_place([0], [[-1.5, 0.0]], 6, FOREVER, tick=4, life=[2], req=[0])]
    init["close"] = np.array([3, 3], np.int64)  # both lives close at tick 3; the place leaves slot 1 to the second place
    places.append(_place([1], [[0.0, -1.5]], 6, FOREVER, tick=5, life=[3], req=[0]))
    s = _swarm(g, "input", board=False)
    _board(s, init, 1, 2)  # one status slot: ticks 1 - 3 need two
    with pytest.raises(_lib.SwarmError) as e:
        _run(s, g, 4)
    assert e.value.code == _lib.ERR_RANGE and s.last_board_overflow[0] == "status" and s.board_last_tick() == -1
    s.grow_board(status_slots=2)
    q, perm = _storage_case(s, g)
    _run(s, g, 4)
    _do_place(s, places[0])
    _run(s, g, 1)
    _do_place(s, places[1])
    s.board["status"] = s.board["status"][:, :1].contiguous()  # back to one slot: tick 6 needs two again
    s.board["claim_out"] = s.board["claim_out"][:, :1].contiguous()
    s.board["Ks"] = 1
    s._motion_state()
    keep = dict(pos=s.pos, pos_prev=s.pos_prev, vel=s.vel, state=s.state, leader=s.leader, **s.fsm,
                **{k: s.board[k] for k in ROWS})
    before = {k: v.clone() for k, v in keep.items()}
    entry, life = s.board_positions(), s.board_lifetimes()
    np.testing.assert_array_equal(entry[0], [[-1.5, 0.0], [0.0, -1.5]])
    with pytest.raises(_lib.SwarmError) as e:
        _run(s, g, 3)
    assert e.value.code == _lib.ERR_RANGE and "status slots at tick 6 " in str(e.value)
    assert s.last_refused_tick == 6 and s.fsm_tick == 5 == s.board_last_tick()
    for k, v in keep.items():  # state and positions as after the place
        assert torch.equal(v, before[k]), k
    for a, w in zip(s.board_positions() + s.board_lifetimes(), entry + life):
        np.testing.assert_array_equal(a, w)
    s.grow_board(status_slots=2)
    r = _run(s, g, 3)
    d = lsm.drive_slots(oracle_mod, q, init, places, 8)
    want = _result(d, perm, 2, 2)
    _assert_rows(_rows(s), want["rows"])
    np.testing.assert_array_equal(r["task_counts"], want["task_counts"][5:])
    np.testing.assert_array_equal(lsm.lbm.dense_status(_rows(s)["status"], 2), [[ASSIGNED, ASSIGNED], [OPEN, OPEN]])


# 8. a resort between a place and the next call
@pytest.mark.gpu
def test_gpu_a_resort_between_a_place_and_the_next_call():
    from test_resort import _assert_same_swarm, _board_case, _fresh_twin
    g = _board_case(5001, 23, ticks=60, kills=(10, 50), T=200)
    rng = np.random.default_rng(9)
    Q0 = np.stack([g["task_x"], g["task_y"]], 1)
    init = dict(pos=Q0, vel=rng.uniform(-3.0, 3.0, Q0.shape), req=g["task_req"], open=np.zeros(200, np.int64),
                close=rng.integers(5, 27, 200).astype(np.int64))
    a, b = _swarm(g, "spatial", board=False), _swarm(g, "spatial", board=False)
    for s in (a, b):
        _board(s, init, 64, 32)
    run = lambda s, k: s.update_loop_board(k, 2.5, 2.5, loss=0.1, loss_seed=5, **_kw(g))  # noqa: E731
    ra, rb = run(a, 30), run(b, 30)
    np.testing.assert_array_equal(ra["task_counts"], rb["task_counts"])
    free = a.board_free_slots()
    assert len(free) >= 100 and (a.board["tab_task"] >= 0).any()
    e = _place(free, np.stack([rng.uniform(Q0.min(), Q0.max(), len(free))] * 2, 1), 31, FOREVER, tick=30,
               req=rng.integers(-1, 3, len(free)))
    pa, pb = _do_place(a, e), _do_place(b, e)
    assert pa == pb and pa["purged"] > 0
    a.resort()
    assert a.last_resort_moved > 0
    c = _fresh_twin(b)  # (it shares b's board handle: b is not run again)
    _assert_same_swarm(a, c)
    ra, rc = run(a, 30), run(c, 30)
    for k in ("counts", "task_counts", "link_counts"):
        np.testing.assert_array_equal(ra[k], rc[k], err_msg=k)
    assert ra["task_counts"][:, 0].sum() > 0 and ra["task_counts"][:, 1].sum() > 0
    _assert_same_swarm(a, c)


# 9. the census after a purge; 10. the bridge with new keys
@pytest.mark.gpu
def test_gpu_census_after_a_purge_shows_no_table_entry_of_the_slot(oracle_mod):
    from test_board_census import _assert_census
    g, init, places = _random_stream(257, 40, 11, ticks=20)
    s = _swarm(g, "input", board=False)
    _board(s, init, 40, 40)
    q, perm = _storage_case(s, g)
    stop = places[-1]["tick"]
    d = lsm.drive_slots(oracle_mod, q, init, places, stop)
    want = _result(d, perm, 40, 40)
    r, purged = _play(s, g, places, stop)
    assert purged == d["purged"] and purged[-1] > 0
    c = bcm.census(want["status"], want["tab_winner"], want["tab_util"], g["ids"])
    _assert_census(s.board_census(holders=True), c, holders=True)
    k = places[-1]["slot"]
    assert (want["tab_winner"][:, k] < 0).all() and (want["status"][:, k] == 0).all()
    w, u = lsm.lbm.dense_tables(*(_rows(s)[key] for key in ("tab_task", "tab_winner", "tab_util")), 40)
    assert (w[:, k] < 0).all() and (w >= 0).any()
    got = {key: v.cpu().numpy() for key, v in s.board_census().items() if hasattr(v, "cpu")}
    for key in ("tentative", "locked", "assigned"):
        assert (got[key][k] == 0).all(), key


@pytest.mark.gpu
def test_gpu_write_back_board_names_the_new_keys():
    g, init, places = _hand2()
    s = _swarm(g, "spatial", board=False)
    pos = {10: (1.0, 0.0), 20: (0.0, 1.0)}
    task = lambda p: {"status": "OPEN", "pos": p, "required_cap": "extinguisher"}  # noqa: E731
    agents = [types.SimpleNamespace(agent_id=int(i), task_claims={}, tasks={k: task(p) for k, p in pos.items()})
              for i in g["ids"]]
    s.set_task_board(s.tasks_from_dict(agents[0].tasks), status_slots=2, table_slots=2, open_tick=init["open"],
                     close_tick=init["close"])
    np.testing.assert_array_equal(s.board_task_ids, [10, 20])
    _run(s, g, 4)
    info = _do_place(s, places[0], task_ids=[30])
    assert info == {"purged": 1, "next_tick": 5}
    np.testing.assert_array_equal(s.board_task_ids, [30, 20])
    for a in agents:  # the simulator adds the new key
        a.tasks[30] = task((-1.5, 0.0))
    _run(s, g, 3)
    s.write_back_board(agents)
    assert [sorted(a.tasks) for a in agents] == [[20, 30], [20, 30]]  # key 10 has left with its slot
    assert [a.tasks[30]["status"] for a in agents] == ["ASSIGNED", "OPEN"]
    assert [a.tasks[20]["status"] for a in agents] == ["ASSIGNED", "OPEN"]
    assert agents[1].task_claims == {30: {"winner": 1, "utility": 40.0}, 20: {"winner": 1, "utility": 50.0}}


# 11. every refusal the library makes with the device at hand: nothing changes
@pytest.mark.gpu
def test_gpu_refusals_change_nothing():
    import torch
    from swarm_amd import _lib
    g, init, _ = _random_stream(60, 6, 3)
    # slot 0 closed at tick 2, slot 1 closes at 3, slot 2 closes at 5, slot 3 is open for ever, 4 opens later, 5 never
    init.update(open=np.array([0, 0, 0, 0, 50, 7], np.int64), close=np.array([2, 3, 5, FOREVER, 60, 7], np.int64))
    s = _swarm(g, "input", board=False)
    lib, ctx = _lib.lib(), _lib.ctx()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    dev = lambda a: torch.as_tensor(a, device="cuda")  # noqa: E731

    def state(b, Ks=None, Kt=None):
        return _lib.BoardState(Ks or b["Ks"], Kt or b["Kt"], None, *[_lib.ptr(b[k]) for k in ROWS])

    def place(idx, pos=None, req=None, vel=None, lo=None, hi=None, *, handle=None, ctx_=None, st=None, flags=0, device=False):
        m = len(idx)
        arrays = [np.asarray(idx, np.int32), np.ones((m, 2)) if pos is None else np.asarray(pos, np.float64),
                  np.full(m, -1, np.int8) if req is None else np.asarray(req, np.int8),
                  None if vel is None else np.asarray(vel, np.float64),
                  np.full(m, 10, np.int64) if lo is None else np.asarray(lo, np.int64),
                  np.full(m, 20, np.int64) if hi is None else np.asarray(hi, np.int64)]
        hold = [None if a is None else (dev(a) if device else a) for a in arrays]
        ptrs = [None if a is None else (_lib.ptr(a) if device else p(a)) for a in hold]
        out = ctypes.c_int64(-5)
        rc = lib.swarm_board_place(ctx_ or ctx, handle or s.board["handle"], s.n, ctypes.byref(st or state(s.board)),
                                   m, *ptrs, flags, ctypes.byref(out), _lib.stream())
        return rc, out.value, _lib.last_error()

    # a static board; a moving board without lifetimes; fresh lifetimes
    s.set_task_board(init["pos"][:, 0], init["pos"][:, 1], init["req"], status_slots=6, table_slots=6)
    assert place([0])[::2] == (_lib.ERR_ARG, "invalid argument: placing needs a moving board with lifetimes "
                               "(swarm_board_set_lifetimes)")
    s.set_task_board(init["pos"][:, 0], init["pos"][:, 1], init["req"], status_slots=6, table_slots=6,
                     velocities=init["vel"])
    rc, _, text = place([0])
    assert rc == _lib.ERR_ARG and "needs a moving board with lifetimes" in text
    _board(s, init, 6, 6)
    rc, _, text = place([5])
    assert rc == _lib.ERR_ARG and "no tick has run since" in text
    dead = ctypes.c_void_p(s.board["handle"].value)
    _board(s, init, 6, 6)  # destroys the board before
    rc, _, text = place([5], handle=dead)
    assert rc == _lib.ERR_ARG and "not a live board" in text
    _run(s, g, 4)  # last = 4: slots 0, 1, 4 and 5 are free; 2 and 3 are open
    np.testing.assert_array_equal(s.board_free_slots(), [0, 1, 4, 5])
    s.set_board_lifetimes(*s.board_lifetimes())  # the same windows, set again: fresh until a tick has run
    rc, _, text = place([5])
    assert rc == _lib.ERR_ARG and "no tick has run since" in text
    _run(s, g, 1)  # last = 5: slot 2 closed at the last tick -- its last claim may be in flight
    np.testing.assert_array_equal(s.board_free_slots(), [0, 1, 4, 5])
    s.board["tab_task"][:, 0] = 0  # table entries about slot 0 at every agent: a purge would remove them
    s.board["tab_winner"][:, 0] = 7
    rows = {k: s.board[k].clone() for k in ROWS}
    life, pos = s.board_lifetimes(), s.board_positions()
    treq = s.board_dense()  # (reads only)
    other = _lib.Ctx()
    nan, inf, big = float("nan"), float("inf"), 2 ** 62
    cases = [(dict(idx=[0], ctx_=other), "not a live board"),
             (dict(idx=[6]), "request 0 (slot 6) names a slot outside"), (dict(idx=[0, -1]), "request 1 (slot -1) names a slot outside"),
             (dict(idx=[0, 1, 0]), "slot 0 is listed twice"), (dict(idx=[0, 1, 4, 5, 0, 1, 4]), "more requests than slots"),
             (dict(idx=[0, 2]), "request 1 (slot 2) names a slot that is not free"), (dict(idx=[3]), "request 0 (slot 3) names a slot that is not free"),
             (dict(idx=[0, 1], lo=[6, 5]), "request 1 (slot 1) opens at or before the last tick run"),
             (dict(idx=[0], lo=[0]), "opens at or before"), (dict(idx=[0], lo=[-3]), "has a negative open or close tick"),
             (dict(idx=[0], hi=[-1]), "has a negative"), (dict(idx=[0], lo=[9], hi=[8]), "opens after it closes"),
             (dict(idx=[0], lo=[big + 1], hi=[big]), "opens after it closes"),
             (dict(idx=[0, 1], pos=[[1, 1], [nan, 1]]), "request 1 (slot 1) has a position or velocity that is not finite"),
             (dict(idx=[0], pos=[[1, -inf]]), "not finite"), (dict(idx=[0], vel=[[inf, 0]]), "not finite"),
             (dict(idx=[0], vel=[[0, nan]]), "not finite"), (dict(idx=[0], req=[32]), "has a treq outside [-1, 31]"),
             (dict(idx=[0], req=[-2]), "has a treq outside"), (dict(idx=[0], flags=4), "unknown flag"),
             (dict(idx=[0], st=state(s.board, Kt=4097)), "slots must be in"), (dict(idx=[0], st=state(s.board, Ks=0x10000)), "slots must be in")]
    for kw, text in cases:
        for device in (False, True):
            rc, out, msg = place(kw.pop("idx") if device else kw["idx"], device=device, **{k: v for k, v in kw.items() if k != "idx"})
            assert rc == _lib.ERR_ARG and text in msg, (kw, msg)
            assert out in (-5, 0)
            for k in ROWS:
                assert torch.equal(s.board[k], rows[k]), (kw, k)
            for a, w in zip(s.board_lifetimes() + s.board_positions(), life + pos):
                np.testing.assert_array_equal(a, w, err_msg=str(kw))
    assert all(torch.equal(a, b) for a, b in zip(s.board_dense(), treq)) and s.board_last_tick() == 5
    r = _run(s, g, 2)  # the board runs on, never placed on: any start would do
    assert r["task_counts"].shape == (2, 3)
    rc, out, _ = place([0, 5], device=True)  # and the same arrays do place once they are right
    assert rc == _lib.OK and out == s.n


# 12. the loop on a board that has been placed on
@pytest.mark.gpu
def test_gpu_loop_on_a_placed_board_must_start_at_the_next_tick():
    import torch
    from swarm_amd import _lib
    g, init, places = _hand2()
    s = _swarm(g, "input", board=False)
    _board(s, init, 2, 2)
    _run(s, g, 4)
    s.fsm_tick = 7  # a board never placed on takes any start
    _run(s, g, 1)
    assert s.board_last_tick() == 8 and s.fsm_tick == 8
    _do_place(s, _place([0], [[-1.5, 0.0]], 9, FOREVER, tick=8, req=[0]))
    s._motion_state()
    rows = {k: s.board[k].clone() for k in ROWS}
    pos = s.board_positions()
    for start in (7, 9, 0):
        s.fsm_tick = start
        with pytest.raises(_lib.SwarmError, match="tasks have been placed on this board") as e:
            _run(s, g, 2)
        assert e.value.code == _lib.ERR_ARG
        for k in ROWS:
            assert torch.equal(s.board[k], rows[k]), k
        for a, w in zip(s.board_positions(), pos):
            np.testing.assert_array_equal(a, w)
    s.fsm_tick = 8
    r = _run(s, g, 2)
    assert r["task_counts"][0, 0] == 1 and s.board_last_tick() == 10


# 13. a twin swarm on the virtual board agrees slot for slot
@pytest.mark.gpu
def test_gpu_twin_on_the_virtual_board_agrees_slot_for_slot(oracle_mod):
    """Contract U1-P.4 on the device: the twin's board has one index per life, every index placed once at the tick
    its life was placed (an index that has not opened yet is free) -- nothing is ever reused there and nothing
    purged, its tables keep every dead life."""
    g = load_golden(FIXTURE)
    init, places, T = lsm.case_from_fixture(g)
    first, ticks = int(g["task_tick"]) - 1, int(g["ticks"])
    vb = lsm.virtual_board(init, places)
    L = len(vb["slot"])
    a, b = _swarm(g, "spatial", board=False), _swarm(g, "spatial", board=False)
    for s in (a, b):
        s.update_loop_radio(first, float(g["radio_radius"]), float(g["sense_radius"]), **_kw(g))
    _board(a, init, 16, 16)
    vinit = {k: vb[k].copy() for k in ("pos", "vel", "req", "open", "close")}
    vinit["open"][T:], vinit["close"][T:] = FAR, FAR  # not there yet
    _board(b, vinit, 16, 64)
    vplaces = [dict(e, slot=e["life"]) for e in places]
    ra, pa = _play(a, g, places, ticks, now=first)
    rb, pb = _play(b, g, vplaces, ticks, now=first)
    assert sum(pa) > 100 and sum(pb) == 0
    _same_swarm(a, b, rows=False)
    for k in ("counts", "task_counts"):
        np.testing.assert_array_equal(ra[k], rb[k], err_msg=k)
    assert ra["guard"] == rb["guard"] == 0
    life = np.array(np.arange(T))
    for e in places:
        life[e["slot"]] = e["life"]
    sa, wa, ua = (t.cpu().numpy() for t in a.board_dense())
    sb, wb, ub = (t.cpu().numpy() for t in b.board_dense())
    np.testing.assert_array_equal(sa, sb[:, life])
    np.testing.assert_array_equal(wa, wb[:, life])
    np.testing.assert_array_equal(ua.view(np.uint32), ub[:, life].view(np.uint32))
    for x, y in zip(a.board_positions(), b.board_positions()):
        np.testing.assert_array_equal(x, y[life])
    slot = vb["slot"]
    for key in ("claim_out", "conflict_out"):  # the message records, life -> slot
        x, y = a.board[key].cpu().numpy(), b.board[key].cpu().numpy()
        for i in range(2 * a.n):
            assert sorted(x[i][x[i] >= 0].tolist()) == sorted(slot[y[i][y[i] >= 0]].tolist()), (key, i)
    dead = np.setdiff1d(np.arange(L), life)
    assert (wb[:, dead] >= 0).sum() > 100 and (sa != 0).any()
    assert llm.present(a.board["life"][0], a.board["life"][1], ticks).sum() >= 20
