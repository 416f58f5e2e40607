"""Agent lifetimes (contract U1-J): swarm_agent_life_create / _set / _events / _destroy,
Swarm.set_agent_lifetimes, agent_lifetimes, agents_up.

Agent i is up at tick t iff boot[i] <= t < death[i].  At the start of tick t the agents with death == t die as a
kill_ticks victim does, then the agents with boot == t become a fresh SwarmAgent constructed at the clock of tick
t - 1.  The yardstick on the GPU is the loops themselves, already verified against the oracle: one call with
lifetimes must equal, bit for bit, the same ticks run one loop call at a time with the documented torch edits of
the swarm's arrays from Python in between (_edit below writes them out).  The host schedule (csrc/agent_life.h)
is driven on the CPU by tests/agent_life/agent_life_main.cpp.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT, load_golden
import board_census_model as bcm
from test_moving_tasks import _case48, _mboard
from test_update_loop_board import ROWS
from test_update_loop_tasks import _kw, _swarm

CSRC = os.path.join(PKG, "csrc")
FOREVER = np.iinfo(np.int64).max
NEW = ("swarm_agent_life_create", "swarm_agent_life_set", "swarm_agent_life_events", "swarm_agent_life_destroy")


# ----------------------------------------------------------------------------- CPU

def test_exports_and_header():
    from swarm_amd import _lib
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert [len(getattr(lib, name).argtypes) for name in NEW] == [7, 7, 5, 2]
    with open(os.path.join(ROOT, "include", "swarm.h")) as f:
        text = f.read()
    assert "int swarm_agent_life_create(swarm_ctx *ctx, int64_t n, const int64_t *boot, const int64_t *death, " \
           "uint8_t *alive,\n" in text
    assert "int swarm_agent_life_set(swarm_ctx *ctx, swarm_agent_life *life, int64_t n, const int64_t *boot, " \
           "const int64_t *death,\n" in text
    assert "int swarm_agent_life_events(swarm_ctx *ctx, const swarm_agent_life *life, int64_t t0, int32_t ticks, " \
           "int64_t *events);" in text
    assert "int swarm_agent_life_destroy(swarm_ctx *ctx, swarm_agent_life *life);" in text
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
    for name in NEW:
        assert f" T {name}\n" in out.stdout, name


def test_entry_points_refuse_bad_arguments_without_a_device():
    from swarm_amd import _lib
    from swarm_amd.swarm import Swarm
    lib = _lib.load()
    fake = ctypes.c_void_p(8)  # never dereferenced: the arguments below are refused first
    out = ctypes.c_void_p(5)
    i64 = lambda *v: np.array(v, np.int64).ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    ok_b, ok_d = np.zeros(3, np.int64), np.full(3, FOREVER)
    hb, hd = ok_b.ctypes.data_as(ctypes.c_void_p), ok_d.ctypes.data_as(ctypes.c_void_p)
    assert lib.swarm_agent_life_create(None, 3, hb, hd, fake, fake, ctypes.byref(out)) == _lib.ERR_ARG
    assert b"ctx or out is NULL" in lib.swarm_last_error()
    assert lib.swarm_agent_life_create(fake, 3, hb, hd, fake, fake, None) == _lib.ERR_ARG
    for n in (-1, 1 << 31):
        assert lib.swarm_agent_life_create(fake, n, hb, hd, fake, fake, ctypes.byref(out)) == _lib.ERR_ARG
        assert b"n out of range" in lib.swarm_last_error() and not out.value
    for args in ((None, hd, fake, fake), (hb, None, fake, fake), (hb, hd, None, fake), (hb, hd, fake, None)):
        assert lib.swarm_agent_life_create(fake, 3, *args, ctypes.byref(out)) == _lib.ERR_ARG
        assert b"NULL agent array" in lib.swarm_last_error()
    for bad in (-1, 1 << 31, FOREVER):
        assert lib.swarm_agent_life_create(fake, 3, i64(0, bad, 0), hd, fake, fake, ctypes.byref(out)) == _lib.ERR_ARG
        assert b"agent 1 (storage index) boots at tick" in lib.swarm_last_error()
    assert lib.swarm_agent_life_create(fake, 3, hb, i64(5, 5, -2), fake, fake, ctypes.byref(out)) == _lib.ERR_ARG
    assert b"agent 2 (storage index) dies at a negative tick" in lib.swarm_last_error()
    assert lib.swarm_agent_life_set(None, fake, 3, hb, hd, 0, None) == _lib.ERR_ARG
    assert lib.swarm_agent_life_set(fake, None, 3, hb, hd, 0, None) == _lib.ERR_ARG
    assert b"ctx or life is NULL" in lib.swarm_last_error()
    assert lib.swarm_agent_life_events(None, fake, 0, 1, hb) == _lib.ERR_ARG
    assert lib.swarm_agent_life_events(fake, None, 0, 1, hb) == _lib.ERR_ARG
    assert lib.swarm_agent_life_destroy(None, fake) == _lib.ERR_ARG
    # the Python layer, before the device is touched
    s = Swarm.__new__(Swarm)
    s.n, s.device, s.layout = 4, "cpu", "input"
    with pytest.raises(ValueError, match=r"boot_tick must be in \[0, 2\^31\)"):
        s.set_agent_lifetimes([0, -1, 0, 0], None)
    with pytest.raises(ValueError, match=r"boot_tick must be in \[0, 2\^31\)"):
        s.set_agent_lifetimes(1 << 31, None)
    with pytest.raises(ValueError, match="death_tick must not be negative"):
        s.set_agent_lifetimes(None, [3, 4, -5, 6])
    with pytest.raises(ValueError, match=r"boot_tick: expected 4 ticks or a scalar, got shape \(3,\)"):
        s.set_agent_lifetimes([0, 1, 2], None)
    with pytest.raises(ValueError, match="integer ticks"):
        s.set_agent_lifetimes(None, [1.5, 2.0, 3.0, 4.0])
    with pytest.raises(ValueError, match="signed 64-bit"):
        s.set_agent_lifetimes(None, np.array([2 ** 63, 5, 5, 5], np.uint64))
    # without lifetimes: nothing to read back, everybody up; removing what is not there is no error
    assert s.agent_lifetimes() is None and s.agents_up().all() and s.set_agent_lifetimes(None, None) is s
    # agents_up: the windows' edges; the default tick is the next one to run
    s.agent_life = dict(boot=np.array([0, 5, 7, 6]), death=np.array([5, 7, FOREVER, 6]), finalizer=lambda: None)
    s.fsm_tick = 4
    np.testing.assert_array_equal(s.agents_up(), [False, True, False, False])
    np.testing.assert_array_equal(s.agents_up(4), [True, False, False, False])
    np.testing.assert_array_equal(s.agents_up(7), [False, False, True, False])
    boot, death = s.agent_lifetimes()
    np.testing.assert_array_equal(boot, [0, 5, 7, 6])
    np.testing.assert_array_equal(death, [5, 7, FOREVER, 6])


@pytest.fixture(scope="module")
def life_report(tmp_path_factory):
    """The schedule header through a plain host program, with the address and undefined-behaviour sanitizers on
    that program only."""
    exe = str(tmp_path_factory.mktemp("agent_life") / "agent_life")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "agent_life", "agent_life_main.cpp")], check=True, capture_output=True,
                   text=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    return p.returncode, p.stdout + p.stderr


def test_agent_life_program_passes(life_report):
    rc, out = life_report
    assert rc == 0 and out.rstrip().endswith("0 failed") and "FAIL" not in out and "runtime error" not in out, out


@pytest.mark.parametrize("case", [
    "up_edges", "up_defaults", "up_empty_window", "set_time_rule", "valid_windows", "refuses_negative_boot",
    "refuses_boot_at_2_31", "refuses_negative_death", "valid_empty", "defaults_have_no_events", "empty_schedule",
    "empty_swarm", "death_sorts_before_boot_on_one_tick", "boot_equals_death_never_fires", "entry_round_trip",
    "events_at_first_and_last_tick", "events_at_or_before_t0_do_not_fire", "events_beyond_the_call_do_not_fire",
    "a_call_after_every_event", "a_call_of_no_ticks", "chunks_fire_every_event_once", "near_max_death",
    "near_max_no_overflow", "segments_equal_the_definition_random"])
def test_agent_life_cases(life_report, case):
    assert f"ok {case}\n" in life_report[1], life_report[1]


def test_agent_life_header_has_no_hip_includes():
    with open(os.path.join(CSRC, "agent_life.h")) as f:
        inc = [ln.split()[1] for ln in f if ln.startswith("#include")]
    assert inc == ["<algorithm>", "<cstdint>", "<vector>"]


def _hand3():
    """Three agents in a row, all within radio range: A (ID 1), B (ID 5), C (ID 9).  C starts late, at tick 7; B dies
    at tick 9.  timeout 0.25 s, no jitter, lock-step tick counters: every step below follows from agent.py."""
    g = dict(ids=np.array([1, 5, 9], np.int32), x=np.array([0.0, 1.0, 2.0]), y=np.zeros(3),
             tick_off=np.zeros(3, np.int32), last_hb0=np.zeros(3), tx=np.zeros(3), ty=np.zeros(3),
             has_t=np.zeros(3, np.uint8), obs=np.zeros((0, 3)), kill_ticks=np.zeros(0, np.int64), seed=1, dt=0.1,
             max_speed=5.0, radio_radius=10.0, sense_radius=0.5)
    return g, np.array([0, 0, 7], np.int64), np.array([FOREVER, 9, FOREVER], np.int64)


F_, W_, L_ = 1, 2, 3
# after each tick: states, leaders, alive flags, has_leader_pos, the tick's outbox bytes (1 ACCLAIM, 2 HEARTBEAT)
HAND3 = {
    1: ([F_, F_, F_], [-1, -1, -1], [1, 1, 0], [0, 0, 0], [0, 0, 0]),   # C is down from the start (boot 7 > 0)
    2: ([F_, F_, F_], [-1, -1, -1], [1, 1, 0], [0, 0, 0], [0, 0, 0]),
    3: ([W_, W_, F_], [-1, -1, -1], [1, 1, 0], [0, 0, 0], [0, 0, 0]),   # 0.3 - 0.0 > 0.25: A and B start to wait
    4: ([L_, L_, F_], [1, 5, -1], [1, 1, 0], [0, 0, 0], [1, 1, 0]),     # no jitter: both acclaim
    5: ([F_, F_, F_], [5, 1, -1], [1, 1, 0], [0, 0, 0], [0, 0, 0]),     # each takes the other's COORDINATOR
    6: ([F_, F_, F_], [5, 1, -1], [1, 1, 0], [0, 0, 0], [0, 0, 0]),
    7: ([F_, F_, F_], [5, 1, -1], [1, 1, 1], [0, 0, 0], [0, 0, 0]),     # C boots: last_hb 0.6, its tick counter 1
    8: ([W_, W_, F_], [-1, -1, -1], [1, 1, 1], [0, 0, 0], [0, 0, 0]),   # 0.8 - 0.5 > 0.25; C: 0.8 - 0.6 is not
    9: ([L_, W_, W_], [1, -1, -1], [1, 0, 1], [0, 0, 0], [1, 0, 0]),    # B dies waiting and stays so; C waits
    10: ([L_, W_, F_], [1, -1, 1], [1, 0, 1], [0, 0, 0], [2, 0, 0]),    # C takes A's COORDINATOR (its own tick is
                                                                         # 4: no bully heartbeat); A's tick 10: HEARTBEAT
    11: ([L_, W_, F_], [1, -1, 1], [1, 0, 1], [0, 0, 1], [0, 0, 0]),    # C has A's position and starts to move
    12: ([L_, W_, F_], [1, -1, 1], [1, 0, 1], [0, 0, 1], [0, 0, 0]),
    13: ([L_, W_, F_], [1, -1, 1], [1, 0, 1], [0, 0, 1], [0, 0, 0]),
    14: ([L_, W_, W_], [1, -1, -1], [1, 0, 1], [0, 0, 0], [0, 0, 0]),   # 1.4 - 1.1 > 0.25: A beats every 10 ticks only
    15: ([L_, W_, L_], [1, -1, 9], [1, 0, 1], [0, 0, 0], [0, 0, 1]),    # the late high ID acclaims
    16: ([F_, W_, L_], [9, -1, 9], [1, 0, 1], [0, 0, 0], [0, 0, 2]),    # and takes over from the living lower leader;
}                                                                        # C's own tick 10: its first HEARTBEAT


def test_three_agents_by_hand(oracle_mod):
    import agent_life_model as alm
    g, boot, death = _hand3()
    seen = {}

    def on_tick(t, o):
        f = o["fsm"]
        half = (t & 1) * 3
        seen[t] = tuple(f[k].tolist() for k in ("state", "leader", "alive", "has_lpos")) + \
            (f["outbox"][half:half + 3].tolist(),)
        want_off = [0, 0, -6 if t >= 7 else 0]
        assert o["tick_off"].tolist() == want_off, t
        if t == 7:  # the fresh agent: constructed at the clock of tick 6, standing where it stood
            assert f["last_hb"][2] == 6 * 0.1 and f["wait_start"][2] == 0 and f["delay"][2] == 0
            assert o["x"][2] == 2.0 and o["vx"][2] == 0
    o = alm.set_time(alm.fresh(oracle_mod, g), boot, death)
    assert o["fsm"]["alive"].tolist() == [1, 1, 0]
    o = alm.drive(oracle_mod, g, boot, death, 16, start=o, on_tick=on_tick, timeout=0.25, jitter=0.0, use_pow=True)
    for t, want in HAND3.items():
        assert seen[t] == tuple(list(w) for w in want), (t, seen[t])
    assert o["agent_events"].tolist() == [[int(t == 7), int(t == 9)] for t in range(1, 17)]
    assert o["counts"][:, 0].tolist() == [0, 0, 0, 2, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 2, 1]
    assert o["fsm"]["last_hb"][0] == 16 * 0.1 and o["x"][2] < 0.0 and o["x"][0] == 0.0  # C moved past A's position
    # default windows are the loop itself
    M = np.full(3, FOREVER)
    a = alm.drive(oracle_mod, g, np.zeros(3, np.int64), M, 12, timeout=0.25, jitter=0.0)
    import loop_radio_model
    b = loop_radio_model.run(oracle_mod, g, 12, timeout=0.25, jitter=0.0)
    for k in b["fsm"]:
        np.testing.assert_array_equal(a["fsm"][k], b["fsm"][k], err_msg=k)
    np.testing.assert_array_equal(a["counts"], b["counts"])
    assert not a["agent_events"].any()


FIXTURES = ("agent_life_radio_n200", "agent_life_board_n200", "agent_life_wide_n400")


@pytest.mark.parametrize("name", FIXTURES)
def test_model_with_pow_equals_the_real_agents(oracle_mod, name):
    """Real SwarmAgent objects constructed anew and stopped mid-run (tools/gen_golden_agent_lifetimes.py) against
    the model: every final array, tick_off, the per-tick counts and the events."""
    import agent_life_model as alm
    from loop_model import OUT_KEYS
    g = load_golden(name)
    boot, death, ticks = g["boot"], g["death"], int(g["ticks"])
    hist = {}

    board = "task_x" in g
    claimed = np.zeros(len(boot), bool)  # agents that sent a TASK_CLAIM after they booted

    def on_tick(t, o):
        hist[t] = (o["fsm"]["state"].copy(), o["fsm"]["alive"].copy(), o["fsm"]["leader"].copy(),
                   (o["tasks"]["status"] == 3).any(1) if board else None)
        if board:
            claimed[:] |= np.array([bool(c) for c in o["tasks"]["claims"]]) & (boot > 0) & (boot <= t)
    o = alm.set_time(alm.fresh(oracle_mod, g), boot, death)
    o["fsm"]["alive"][g["restart"] != 0] = 1  # up when they boot: restarts
    o = alm.drive(oracle_mod, g, boot, death, ticks, start=o, on_tick=on_tick, use_pow=True)
    if board:
        for k in ("status", "tab_winner", "claim_out", "conflict_out", "task_counts"):
            np.testing.assert_array_equal(o[k], g[k + "_out"] if k + "_out" in g else g[k], err_msg=k)
        np.testing.assert_array_equal(o["tab_util"].view(np.uint32), g["tab_util_out"].view(np.uint32))
        again = np.flatnonzero(g["restart"])
        # a restart of agents that held an ASSIGNED task; booted agents that claim; arbitration went on meanwhile
        assert len(again) == 5 and (boot[again] == 71).all() and hist[70][3][again].all() and hist[70][1][again].all()
        assert claimed.sum() >= 3 and claimed[again].any()
        assert o["task_counts"][:, 1].sum() >= 20 and (o["status"] == 3).any()
    for k in OUT_KEYS:  # the thirteen arrays
        got = o["fsm"][k] if k in o["fsm"] else o[k]
        np.testing.assert_array_equal(got, g[k + "_out"], err_msg=k)
    np.testing.assert_array_equal(o["tick_off"], g["tick_off_out"])
    np.testing.assert_array_equal(o["counts"], g["counts"])
    np.testing.assert_array_equal(o["agent_events"], g["agent_events"])
    assert o["singular"] == 0
    # what the fixture must exercise, asserted again on the data: a fixture that exercises nothing cannot pass
    ids, st, al = g["ids"], g["state_out"], g["alive_out"].astype(bool)
    late = (boot > 0) & (death > ticks)
    took_over = [i for i in np.flatnonzero(late & al & (st == 3))
                 if any(((hist[t][0] == 3) & (hist[t][1] != 0) & (ids < ids[i]) & (hist[t + 1][2] == ids[i]) &
                         (hist[t + 1][1] != 0)).any() for t in range(int(boot[i]), ticks))]
    assert took_over  # a booted agent ends LEADER, having taken over from a living lower leader
    assert (late & al & (st == 1) & (g["has_lpos_out"] == 1)).any()  # a booted FOLLOWER with a leader position
    dying = np.flatnonzero((boot < death) & (death <= ticks) & (death > 1))
    was = np.array([hist[int(death[i]) - 1][0][i] for i in dying])
    up = np.array([hist[int(death[i]) - 1][1][i] for i in dying]).astype(bool)
    assert (up & (was != 3)).any() and (up & (was == 3)).sum() >= 2  # non-leader deaths and leader deaths
    orphans = [j for i in dying[up & (was == 3)] for j in np.flatnonzero(hist[int(death[i])][2] == ids[i])]
    assert any(hist[t][0][j] == 2 for j in orphans for t in range(52, ticks + 1))  # ... and a timeout re-election
    ev = g["agent_events"]
    assert ev[0, 0] >= 1 and ev[-1, 0] >= 1 and ((ev[:, 0] >= 1) & (ev[:, 1] >= 1)).any()
    assert (int(ids.max()) > 255) == ("wide" in name)


# ----------------------------------------------------------------------------- GPU

LOOPS = ("protocol", "csr", "sensed", "radio", "tasks", "board", "moving board")
FIRST = 44  # the ticks every case has run before its lifetimes are set: leaders stand, heartbeats are in flight


def _case():
    """loop_tasks_n200's agents with test_moving_tasks' 48 drifting tasks, a leader kill inside the event ticks."""
    g, Q0, V = _case48()
    g["kill_ticks"] = np.array([FIRST + 9], np.int64)
    return g, Q0, V


def _make(g, Q0, V, loop, layout="spatial"):
    """A swarm of the case after FIRST ticks of its loop family, with the loop's task state in flight."""
    s = _swarm(g, layout, board=False)
    if loop in ("protocol", "csr", "sensed"):
        s.set_graph(g["row_ptr"], g["col"])
    if loop == "tasks":
        s.set_tasks(g["task_x"][:40], g["task_y"][:40], g["task_req"][:40])
    elif loop == "board":
        s.set_task_board(Q0[:, 0], Q0[:, 1], g["task_req"], status_slots=32, table_slots=16)
    elif loop == "moving board":
        _mboard(s, Q0, V, g["task_req"], 32, 16)
    _step(s, g, loop, FIRST)
    return s


def _step(s, g, loop, ticks, mode="hybrid", loss=0.0):
    """`ticks` ticks of the loop; returns every per-tick array of the call, by name."""
    kw = _kw(g)
    ch = dict(loss=loss, loss_seed=77) if loss else {}
    rc, rs = float(g["radio_radius"]), float(g["sense_radius"])
    if loop == "protocol":
        counts = s.protocol_run(ticks, kill_ticks=kw["kill_ticks"], dt=kw["dt"], seed=kw["seed"], mode=mode)
        return dict(counts=counts, agent_events=s.last_agent_events)
    if loop == "csr":
        r = s.update_loop(ticks, mode=mode, **kw)
    elif loop == "sensed":
        r = s.update_loop_sensed(ticks, rs, mode=mode, **kw)
    elif loop == "radio":
        r = s.update_loop_radio(ticks, rc, rs, **kw, **ch)
    elif loop == "tasks":
        r = s.update_loop_tasks(ticks, rc, rs, **kw, **ch)
    else:
        r = s.update_loop_board(ticks, rc, rs, **kw, **ch)
    return {k: v for k, v in r.items() if isinstance(v, np.ndarray)}


def _rows_of(s, mask):
    """Storage rows of the agents `mask` (input order) names."""
    import torch
    perm = s.perm.cpu().numpy().astype(np.int64)
    return torch.as_tensor(np.flatnonzero(mask[perm]), device=s.device)


def _edit(s, t, boot, death, dt, motion=True):
    """The per-tick workaround the contract replaces, before tick t: the agents that die, then the agents that boot,
    by torch edits of the swarm's arrays (boot / death in input order).  motion: the call is given the motion
    state (every update loop; swarm_protocol_run is not, and leaves it alone)."""
    n = s.n
    up = boot < death
    dies, boots = _rows_of(s, up & (death == t)), _rows_of(s, up & (boot == t))
    f = s.fsm
    if len(dies):
        f["alive"][dies] = 0
    if not len(boots):
        return
    f["alive"][boots] = 1
    s.state[boots] = 1  # FOLLOWER
    s.leader[boots] = -1
    f["leader_pos"][boots] = 0.0
    f["has_leader_pos"][boots] = 0
    f["last_hb"][boots] = float(t - 1) * dt
    f["wait_start"][boots] = 0.0
    f["delay"][boots] = 0.0
    s.tick_off[boots] = 1 - t
    if motion and hasattr(s, "vel"):
        s.vel[boots] = 0.0
        s.target[boots] = 0.0
        s.has_target[boots] = 0
    for half in (boots, boots + n):
        f["outbox"][half] = 0
    if hasattr(s, "tasks"):
        b = s.tasks
        for k in ("status_lo", "status_hi"):
            b[k][boots] = 0
        for half in (boots, boots + n):
            b["claim_out"][half] = 0
            b["conflict_out"][half] = 0
        b["tab_winner"][boots] = -1
        b["tab_util"][boots] = 0.0
    if hasattr(s, "board"):
        b = s.board
        for k in ("status", "tab_task", "tab_winner"):
            b[k][boots] = -1
        b["tab_util"][boots] = 0.0
        for half in (boots, boots + n):
            b["claim_out"][half] = -1
            b["conflict_out"][half] = -1


def _set_by_hand(s, boot, death):
    """The set-time rule by hand: whoever is not up at the last tick run loses its alive flag."""
    T = s.fsm_tick
    down = _rows_of(s, (boot > T) | (death <= T))
    if len(down):
        s.fsm["alive"][down] = 0


def _per_tick(s, g, loop, ticks, boot, death, **kw):
    """The run one loop call at a time, with _edit before each."""
    out = []
    for _ in range(ticks):
        _edit(s, s.fsm_tick + 1, boot, death, float(g["dt"]), motion=loop != "protocol")
        out.append(_step(s, g, loop, 1, **kw))
    return {k: np.concatenate([r[k] for r in out]) for k in out[0] if k != "agent_events"}


def _tensors(s):
    out = dict(pos=s.pos, state=s.state, leader=s.leader, tick_off=s.tick_off, **s.fsm)
    for k in ("pos_prev", "vel", "target", "has_target"):
        if hasattr(s, k):
            out[k] = getattr(s, k)
    if hasattr(s, "tasks"):
        out.update({"tasks." + k: v for k, v in s.tasks.items() if hasattr(v, "view") and k not in ("tpos", "treq")})
    if hasattr(s, "board"):
        out.update({"board." + k: s.board[k] for k in ROWS})
    return out


def _same(a, b):
    """Every array of the two swarms, bit for bit."""
    import torch
    ta, tb = _tensors(a), _tensors(b)
    assert ta.keys() == tb.keys()
    for k in ta:
        x, y = ta[k], tb[k]
        if x.dtype.is_floating_point:
            x, y = (v.view(torch.int64 if v.dtype == torch.float64 else torch.int32) for v in (x, y))
        assert torch.equal(x, y), k


def _windows(s, ticks, seed=3):
    """Windows over the ticks FIRST+1 .. FIRST+ticks of a swarm that has run FIRST ticks: a tenth of the agents
    boots late, a tenth dies, with a boot at the first tick and at the last tick of the run, a death and a boot of
    different agents on one tick, a dying LEADER and a LEADER that restarts.  Returns boot, death, and the agents
    that restart (up when they boot: their alive flag is put back after the set-time rule took it)."""
    n, T = s.n, s.fsm_tick
    rng = np.random.default_rng(seed)
    boot, death = np.zeros(n, np.int64), np.full(n, FOREVER)
    who = rng.permutation(n)
    k = max(n // 10, 1)
    late, dying, again = who[:k], who[k:2 * k], who[2 * k:3 * k]
    boot[late] = rng.integers(T + 1, T + ticks + 1, len(late))
    death[dying] = rng.integers(T + 1, T + ticks + 1, len(dying))
    boot[again] = rng.integers(T + 2, T + ticks + 1, len(again))
    state = s.to_input_order(s.state)
    lead = np.flatnonzero(state == 3)
    if n >= 30:
        assert len(lead) >= 2, "the case has no leaders to lose"
        boot[late[0]], boot[late[1]], boot[late[2]] = T + 1, T + ticks, T + 5
        death[dying[0]] = T + 5
        boot[lead[0]], death[lead[0]] = T + 4, FOREVER  # a LEADER restarts
        again = np.union1d(np.setdiff1d(again, lead[1:2]), lead[:1])
        boot[lead[1]], death[lead[1]] = 0, T + 3  # a LEADER dies
    restart = np.zeros(n, bool)
    restart[again] = True
    restart &= boot > T
    return boot, death, restart


def _twins(loop, layout="spatial"):
    g, Q0, V = _case()
    return g, _make(g, Q0, V, loop, layout), _make(g, Q0, V, loop, layout)


def _start(a, b, boot, death, restart):
    """Lifetimes on a, the set-time rule by hand on b; the restarting agents stay up on both."""
    a.set_agent_lifetimes(boot, death)
    _set_by_hand(b, boot, death)
    for s in (a, b):
        s.fsm["alive"][_rows_of(s, restart)] = 1
    _same(a, b)


# 1. one call == the per-tick workaround, on every loop
@pytest.mark.gpu
@pytest.mark.parametrize("loop,mode,loss,layout", [
    ("protocol", "push", 0.0, "spatial"), ("protocol", "pull", 0.0, "input"), ("protocol", "hybrid", 0.0, "spatial"),
    ("csr", "push", 0.0, "input"), ("csr", "pull", 0.0, "spatial"), ("csr", "hybrid", 0.0, "spatial"),
    ("sensed", "push", 0.0, "spatial"), ("sensed", "pull", 0.0, "spatial"), ("sensed", "hybrid", 0.0, "input"),
    ("radio", "", 0.0, "input"), ("radio", "", 0.0, "spatial"), ("radio", "", 0.2, "spatial"),
    ("tasks", "", 0.0, "spatial"), ("tasks", "", 0.2, "input"),
    ("board", "", 0.0, "input"), ("board", "", 0.0, "spatial"), ("board", "", 0.2, "spatial"),
    ("moving board", "", 0.0, "spatial"), ("moving board", "", 0.2, "input")])
def test_gpu_one_call_equals_per_tick_calls_with_edits(loop, mode, loss, layout):
    ticks = 24
    g, a, b = _twins(loop, layout)
    boot, death, restart = _windows(a, ticks)
    _start(a, b, boot, death, restart)
    kw = dict(mode=mode) if mode else dict(loss=loss)
    ra = _step(a, g, loop, ticks, **kw)
    rb = _per_tick(b, g, loop, ticks, boot, death, **kw)
    _same(a, b)
    for k in rb:
        np.testing.assert_array_equal(ra[k], rb[k], err_msg=k)
    # the events the call reports are the windows'
    t = np.arange(FIRST + 1, FIRST + ticks + 1)[:, None]
    up = boot < death
    want = np.stack([((boot[None, :] == t) & up).sum(1), ((death[None, :] == t) & up).sum(1)], 1)
    np.testing.assert_array_equal(ra["agent_events"], want)
    assert want[0, 0] >= 1 and want[-1, 0] >= 1 and (want.min(1) >= 1).any() and want.sum() >= 40
    # what the events did is there to see: booted agents that follow a leader again, and dead ones
    alive = a.to_input_order(a.fsm["alive"]).astype(bool)
    late = (boot > FIRST) & up & (death > FIRST + ticks)
    assert alive[late].all() and not alive[up & (death <= FIRST + ticks)].any()
    assert (a.to_input_order(a.leader)[late] >= 0).any()
    np.testing.assert_array_equal(a.to_input_order(a.tick_off)[late], 1 - boot[late])
    if "task_counts" in ra:
        assert ra["task_counts"][:, 1].sum() > 0  # claims were handled while agents came and went
    np.testing.assert_array_equal(a.agents_up(FIRST + ticks), (boot <= FIRST + ticks) & (FIRST + ticks < death))


# 2. the three modes of the graph loops give the same bits
@pytest.mark.gpu
@pytest.mark.parametrize("loop", ["protocol", "csr", "sensed"])
def test_gpu_push_pull_and_hybrid_give_the_same_bits(loop):
    g, Q0, V = _case()
    runs = []
    for mode in ("push", "pull", "hybrid"):
        s = _make(g, Q0, V, loop)
        if not runs:
            boot, death, _ = _windows(s, 24)
        s.set_agent_lifetimes(boot, death)
        runs.append((s, _step(s, g, loop, 24, mode=mode)))
    for s, r in runs[1:]:
        _same(runs[0][0], s)
        np.testing.assert_array_equal(r["counts"], runs[0][1]["counts"])


# 3. default lifetimes, and lifetimes set and removed again: the bits of a swarm without
@pytest.mark.gpu
@pytest.mark.parametrize("loop", ["radio", "moving board"])
@pytest.mark.parametrize("how", ["arrays", "scalars", "removed again"])
def test_gpu_default_lifetimes_equal_the_swarm_without(loop, how):
    g, a, b = _twins(loop)
    if how == "arrays":
        b.set_agent_lifetimes(np.zeros(b.n, np.int64), np.full(b.n, FOREVER))
    elif how == "scalars":
        b.set_agent_lifetimes(0, None)
    else:
        b.set_agent_lifetimes(np.full(b.n, 0), np.full(b.n, FIRST + 3))
        boot, death = b.agent_lifetimes()
        assert (boot == 0).all() and (death == FIRST + 3).all()
        b.set_agent_lifetimes(None, None)
        assert b.agent_lifetimes() is None and b.agents_up().all()
    assert (b.agent_lifetimes() is None) == (how == "removed again") and a.agent_lifetimes() is None
    _same(a, b)
    ra, rb = _step(a, g, loop, 20, loss=0.1), _step(b, g, loop, 20, loss=0.1)
    _same(a, b)
    for k in ra:
        np.testing.assert_array_equal(ra[k], rb[k], err_msg=k)
    assert not ra["agent_events"].any()


# 4. a chunked run is the same run, events on the first and on the last tick of a chunk included
@pytest.mark.gpu
@pytest.mark.parametrize("loop", ["radio", "board"])
@pytest.mark.parametrize("chunks", [(1,) * 24, (7, 17)])
def test_gpu_chunked_run_is_the_same_run(loop, chunks):
    g, a, b = _twins(loop)
    boot, death, restart = _windows(a, 24)
    late = np.flatnonzero((boot > FIRST) & (death == FOREVER))
    boot[late[3]], boot[late[4]] = FIRST + 7, FIRST + 8  # the last tick of the chunk of 7, the first of the next
    a.set_agent_lifetimes(boot, death)
    b.set_agent_lifetimes(boot, death)
    for s in (a, b):
        s.fsm["alive"][_rows_of(s, restart)] = 1
    ra = _step(a, g, loop, 24)
    rb = [_step(b, g, loop, c) for c in chunks]
    _same(a, b)
    for k in ra:
        np.testing.assert_array_equal(ra[k], np.concatenate([r[k] for r in rb]), err_msg=k)
    assert ra["agent_events"][6, 0] >= 1 and ra["agent_events"][7, 0] >= 1


# 5. set_agent_lifetimes between calls: a second window for an agent that died is a rebirth
@pytest.mark.gpu
def test_gpu_a_second_window_gives_a_rebirth():
    g, a, b = _twins("board")
    n = a.n
    boot, death = np.zeros(n, np.int64), np.full(n, FOREVER)
    who = np.flatnonzero(a.to_input_order(a.board["status"])[:, 0] >= 0)[:5]  # agents that hold statuses
    assert len(who) == 5
    death[who] = FIRST + 2
    a.set_agent_lifetimes(boot, death)
    _set_by_hand(b, boot, death)
    ra = [_step(a, g, "board", 6)]
    rb = [_per_tick(b, g, "board", 6, boot, death)]
    alive = a.to_input_order(a.fsm["alive"])
    assert not alive[who].any() and alive.sum() >= n - 5 - 20  # (the leader kill has not come yet)
    assert (a.to_input_order(a.board["status"])[who, 0] >= 0).all()  # a death keeps the rows
    boot2, death2 = boot.copy(), death.copy()
    boot2[who], death2[who] = FIRST + 9, FOREVER
    a.set_agent_lifetimes(boot2, death2)  # the set-time rule finds them dead already and writes nothing new
    _set_by_hand(b, boot2, death2)
    _same(a, b)
    ra.append(_step(a, g, "board", 10))
    rb.append(_per_tick(b, g, "board", 10, boot2, death2))
    _same(a, b)
    for k in rb[0]:
        np.testing.assert_array_equal(np.concatenate([r[k] for r in ra]), np.concatenate([r[k] for r in rb]), err_msg=k)
    assert a.to_input_order(a.fsm["alive"])[who].all()
    np.testing.assert_array_equal(a.to_input_order(a.tick_off)[who], 1 - (FIRST + 9))
    np.testing.assert_array_equal(ra[1]["agent_events"][2], [5, 0])


# 6. sizes at which the event kernel can go wrong: everybody dies on one tick, everybody boots on one tick
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_gpu_every_agent_dies_and_boots_on_one_tick(n):
    import torch
    g, _, _ = _case()
    rng = np.random.default_rng(n)
    side = max(np.sqrt(n) * 1.2, 1.0)
    q = dict(g, ids=rng.permutation(4 * n)[:n].astype(np.int32), x=rng.uniform(0, side, n), y=rng.uniform(0, side, n),
             caps=np.ones(n, np.uint32), tick_off=rng.integers(0, 10, n).astype(np.int32),
             last_hb0=rng.uniform(-2.9, 0.0, n), tx=np.zeros(n), ty=np.zeros(n), has_t=np.zeros(n, np.uint8),
             kill_ticks=np.zeros(0, np.int64))
    a, b = _swarm(q, "spatial", board=False), _swarm(q, "spatial", board=False)
    for s in (a, b):
        _step(s, q, "radio", 36)  # elections have run: leaders and followers with leader positions
    T = a.fsm_tick
    boot, death = np.full(n, T + 8, np.int64), np.full(n, T + 3, np.int64)  # (two windows in a row: see below)
    # first window [0, T+3): everybody dies at T+3, a segment of n deaths
    a.set_agent_lifetimes(0, death)
    _set_by_hand(b, np.zeros(n, np.int64), death)
    ra = _step(a, q, "radio", 5)
    rb = _per_tick(b, q, "radio", 5, np.zeros(n, np.int64), death)
    _same(a, b)
    assert not a.fsm["alive"].any() and (ra["counts"][2:] == 0).all()
    np.testing.assert_array_equal(ra["agent_events"][2], [0, n])
    # nobody is up: the radio loop stays a no-op
    before = {k: v.clone() for k, v in _tensors(a).items() if k != "pos_prev"}
    a.set_agent_lifetimes(boot, None)
    _set_by_hand(b, boot, np.full(n, FOREVER))
    r = _step(a, q, "radio", 2)
    _per_tick(b, q, "radio", 2, boot, np.full(n, FOREVER))
    assert not r["counts"].any() and not r["agent_events"].any()
    for k, v in before.items():
        assert torch.equal(_tensors(a)[k], v), k
    # second window [T+8, forever): everybody boots on one tick, a segment of n boots
    ra = _step(a, q, "radio", 6)
    rb = _per_tick(b, q, "radio", 6, boot, np.full(n, FOREVER))
    _same(a, b)
    np.testing.assert_array_equal(ra["counts"], rb["counts"])
    np.testing.assert_array_equal(ra["agent_events"][0], [n, 0])
    assert a.fsm["alive"].all() and (a.tick_off == 1 - (T + 8)).all() and (a.state == 1).all()


# 7. a segment of one event on rows of every width: only the booted agent's rows change
@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 5, 64, 67, 4096])
def test_gpu_full_rows_set_by_hand_are_emptied_for_the_booted_agent_alone(K):
    import torch
    from swarm_amd.swarm import Swarm
    n, T = 5, 4096
    tx = 1000.0 + np.arange(T, dtype=np.float64)  # far from every agent: nobody claims
    twins = []
    for with_life in (True, False):
        s = Swarm(np.arange(n, dtype=np.int32) + 10, 100.0 * np.arange(n), np.zeros(n), layout="input", device="cuda")
        s.protocol_reset()
        s.set_task_board(tx, np.zeros(T), status_slots=K, table_slots=K)
        b = s.board
        slots = torch.arange(K, dtype=torch.int32, device="cuda")
        b["status"][:] = (slots << 2) | 2
        b["tab_task"][:] = slots
        b["tab_winner"][:] = 7
        b["tab_util"][:] = 33.5
        b["claim_out"][:] = slots
        b["conflict_out"][:] = slots
        s._motion_state()
        s.vel[:] = 0.25
        s.fsm["outbox"][:] = 2
        if with_life:
            s.set_agent_lifetimes([0, 0, 1, 0, 0], None)
            s.fsm["alive"][2] = 1  # up when it boots: a restart
        r = s.update_loop_board(1, 2.5, 2.5)
        twins.append(s)
    a, b = twins
    np.testing.assert_array_equal(r["agent_events"], [[0, 0]])
    others = torch.tensor([0, 1, 3, 4], device="cuda")
    for k in ROWS:
        x, y = (s.board[k].view(torch.int32).reshape(-1, n, K) for s in (a, b))
        assert torch.equal(x[:, others], y[:, others]), k
        want = 0 if k == "tab_util" else -1
        assert (x[:, 2] == want).all(), k
    # (the twin's agent 2 still holds its full rows; its out rows of this tick's parity were cleared by the tick)
    assert (b.board["status"][2] >= 0).all() and (b.board["tab_task"][2] >= 0).all()
    assert (a.vel[2] == 0).all() and torch.equal(a.vel[others], b.vel[others])
    assert a.fsm["outbox"][2] == 0 and a.fsm["outbox"][n + 2] == 0 and a.tick_off[2] == 0


# 8. a refused call leaves every array, tick_off included, as it was
def _keep(s):
    out = dict(_tensors(s))
    return out, {k: v.clone() for k, v in out.items()}


@pytest.mark.gpu
def test_gpu_board_overflow_after_an_event_tick_writes_nothing_and_the_repeated_call_is_the_run():
    import torch
    from swarm_amd import _lib
    g, Q0, V = _case()
    a, c = (_swarm(g, "spatial", board=False) for _ in range(2))
    for s in (a, c):
        _step(s, g, "radio", FIRST)
    boot, death, restart = _windows(a, 24)
    # the unrefused run on rows of 32 slots, a tick at a time: after every tick the fullest status row
    _mboard(c, Q0, V, g["task_req"], 32, 16)
    c.set_agent_lifetimes(boot, death)
    c.fsm["alive"][_rows_of(c, restart)] = 1
    rc, peaks = [], []
    for _ in range(24):
        rc.append(_step(c, g, "moving board", 1))
        peaks.append(int((c.board["status"] >= 0).sum(1).max()))
    # rows that hold the first tick (an event tick) and not the whole run: the refused tick is known exactly
    Ks = peaks[0]
    over = [k for k, p in enumerate(peaks) if p > Ks]
    assert Ks >= 1 and over and rc[0]["agent_events"].sum() >= 1, peaks
    _mboard(a, Q0, V, g["task_req"], Ks, 16)
    a.set_agent_lifetimes(boot, death)
    a.fsm["alive"][_rows_of(a, restart)] = 1
    keep, before = _keep(a)
    with pytest.raises(_lib.SwarmError) as e:
        _step(a, g, "moving board", 24)
    assert e.value.code == _lib.ERR_RANGE and f"status slots at tick {FIRST + 1 + over[0]} " in str(e.value)
    assert a.last_refused_tick == FIRST + 1 + over[0] and a.fsm_tick == FIRST
    for k, v in keep.items():
        assert torch.equal(v, before[k]), k
    a.grow_board(status_slots=32)
    ra = _step(a, g, "moving board", 24)  # the repeated call fires the same events
    _same(a, c)
    for k in ra:
        np.testing.assert_array_equal(ra[k], np.concatenate([r[k] for r in rc]), err_msg=k)
    assert ra["agent_events"].sum() >= 40


@pytest.mark.gpu
def test_gpu_too_dense_tick_writes_nothing():
    import torch
    from swarm_amd import _lib
    from swarm_amd.swarm import Swarm
    n = 1_200_000
    rng = np.random.default_rng(2)
    x, y = 3.0 + rng.uniform(0, 1e-3, n), -2.0 + rng.uniform(0, 1e-3, n)
    s = Swarm(np.arange(n, dtype=np.int32), x, y, layout="input", device="cuda")
    s.protocol_reset(tick_off=rng.integers(0, 10, n).astype(np.int32), last_hb=np.full(n, -2.95))
    s._motion_state()
    s.vel[:] = 0.5
    boot = np.zeros(n, np.int64)
    boot[::3] = 1
    s.set_agent_lifetimes(boot, None)
    assert int(s.fsm["alive"].sum()) == n - len(boot[::3])
    keep, before = _keep(s)
    with pytest.raises(_lib.SwarmError) as e:
        s.update_loop_radio(3, 1.0, 1.0)
    assert e.value.code == _lib.ERR_RANGE and "too dense" in str(e.value) and "tick 1" in str(e.value)
    assert s.last_refused_tick == 1 and s.fsm_tick == 0
    for k, v in keep.items():
        assert torch.equal(v, before[k]), k


# 9. a run with a resort() in the middle equals the run rebuilt from its input-order state
@pytest.mark.gpu
def test_gpu_a_run_with_a_resort_equals_the_run_rebuilt_from_its_input_order_state():
    from test_resort import _assert_same_swarm, _board_case, _fresh_twin
    g = _board_case(5001, 23, ticks=60, kills=(10, 30), T=200)
    n = 5001
    rng = np.random.default_rng(8)
    boot, death = np.zeros(n, np.int64), np.full(n, FOREVER)
    who = rng.permutation(n)
    boot[who[:500]] = rng.integers(1, 41, 500)
    death[who[500:1000]] = rng.integers(1, 41, 500)
    death[who[:100]] = boot[who[:100]] + rng.integers(0, 12, 100)  # short lives, some of them empty windows
    a, b = _swarm(g, "spatial", board=False), _swarm(g, "spatial", board=False)
    for s in (a, b):
        s.set_task_board(g["task_x"], g["task_y"], g["task_req"], status_slots=64, table_slots=32)
        s.set_agent_lifetimes(boot, death)
    run = lambda s, k: s.update_loop_board(k, 2.5, 2.5, loss=0.1, loss_seed=5, **_kw(g))  # noqa: E731
    ra, rb = run(a, 20), run(b, 20)
    np.testing.assert_array_equal(ra["task_counts"], rb["task_counts"])
    a.resort()
    assert a.last_resort_moved > 0
    for got, want in zip(a.agent_lifetimes(), (boot, death)):  # the windows stay with their agents
        np.testing.assert_array_equal(got, want)
    c = _fresh_twin(b)  # (it shares b's board handle: b is not run again)
    c.set_agent_lifetimes(boot, death)  # the set-time rule at tick 20 finds every flag as it is
    _assert_same_swarm(a, c)
    ra, rc = run(a, 20), run(c, 20)
    for k in ("counts", "task_counts", "link_counts", "agent_events"):
        np.testing.assert_array_equal(ra[k], rc[k], err_msg=k)
    assert ra["agent_events"][:, 0].sum() > 100 and ra["agent_events"][:, 1].sum() > 100
    assert ra["task_counts"][:, 0].sum() > 0 and ra["task_counts"][:, 1].sum() > 0
    _assert_same_swarm(a, c)
    import torch
    assert torch.equal(a.tick_off, c.tick_off)
    up = (boot <= 40) & (40 < death)
    np.testing.assert_array_equal(a.agents_up(40), up)
    assert not a.to_input_order(a.fsm["alive"])[~up].any()


# 10. the census counts the survivors
@pytest.mark.gpu
def test_gpu_census_after_deaths_counts_the_survivors():
    g, a, _ = _twins("board")
    n = a.n
    boot, death = np.zeros(n, np.int64), np.full(n, FOREVER)
    death[np.random.default_rng(1).permutation(n)[:60]] = FIRST + 4
    a.set_agent_lifetimes(boot, death)
    _step(a, g, "board", 12)
    alive = a.to_input_order(a.fsm["alive"]).astype(bool)
    assert (~alive).sum() >= 60
    from test_board_census import _assert_census
    st, w, u = (t.cpu().numpy() for t in a.board_dense())  # storage order, like the mask and the IDs
    mask = a.fsm["alive"].cpu().numpy()
    want = bcm.census(st, w, u, a.ids.cpu().numpy(), mask=mask)
    _assert_census(a.board_census(alive_only=True, holders=True), want, holders=True)
    everyone = bcm.census(st, w, u, a.ids.cpu().numpy())
    _assert_census(a.board_census(), everyone)
    assert (everyone["tables"] > want["tables"]).any() and want["tables"].sum() > 0  # the dead keep their tables


# 11. the library's own refusals that need a ctx
@pytest.mark.gpu
def test_gpu_another_n_a_dead_handle_and_another_tick_off_are_refused():
    import torch
    from swarm_amd import _lib
    g, a, _ = _twins("radio")
    n = a.n
    a.set_agent_lifetimes(0, FIRST + 5)
    life = a.agent_life
    lib, ctx, h = _lib.lib(), life["ctx"], life["handle"]
    ok_b, ok_d = np.zeros(n + 1, np.int64), np.full(n + 1, FOREVER)
    hb, hd = ok_b.ctypes.data_as(ctypes.c_void_p), ok_d.ctypes.data_as(ctypes.c_void_p)
    alive0 = a.fsm["alive"].clone()
    assert lib.swarm_agent_life_set(ctx, h, n + 1, hb, hd, FIRST, _lib.stream()) == _lib.ERR_ARG
    assert b"n is not the handle's" in lib.swarm_last_error()
    out = ctypes.c_void_p()
    assert lib.swarm_agent_life_create(ctx, n, hb, hd, _lib.ptr(a.fsm["alive"]), _lib.ptr(a.tick_off),
                                       ctypes.byref(out)) == _lib.ERR_ARG
    assert b"already has agent lifetimes" in lib.swarm_last_error() and not out.value
    assert torch.equal(a.fsm["alive"], alive0)
    # another tick_off than the handle's: the loop is refused before anything is written
    mine, a.tick_off = a.tick_off, a.tick_off.clone()
    life["tick_off"] = a.tick_off  # (keep the Python layer from rebuilding the handle)
    keep, before = _keep(a)
    with pytest.raises(_lib.SwarmError, match="tick_off is not the array"):
        _step(a, g, "radio", 3)
    for k, v in keep.items():
        assert torch.equal(v, before[k]), k
    a.tick_off = life["tick_off"] = mine
    # a dead handle
    raw = ctypes.c_void_p(h.value)
    a.set_agent_lifetimes(None, None)
    assert lib.swarm_agent_life_set(ctx, raw, n, hb, hd, FIRST, _lib.stream()) == _lib.ERR_ARG
    assert b"no live agent-lifetime handle" in lib.swarm_last_error()
    ev = np.zeros((3, 2), np.int64)
    assert lib.swarm_agent_life_events(ctx, raw, FIRST, 3, ev.ctypes.data_as(ctypes.c_void_p)) == _lib.ERR_ARG
    assert lib.swarm_agent_life_destroy(ctx, raw) == _lib.ERR_ARG
    r = _step(a, g, "radio", 8)  # the loops run as without lifetimes: nobody dies at FIRST + 5
    assert a.fsm["alive"].sum() >= n - 30 and not r["agent_events"].any()


# 12. protocol_reset drops the lifetimes
@pytest.mark.gpu
def test_gpu_protocol_reset_drops_the_lifetimes():
    g, a, _ = _twins("radio")
    a.set_agent_lifetimes(FIRST + 2, None)
    assert not a.fsm["alive"].any() and a.agent_lifetimes() is not None
    a.protocol_reset()
    assert a.agent_lifetimes() is None and a.fsm["alive"].all() and a.agents_up().all()
    r = _step(a, g, "radio", 4)
    assert not r["agent_events"].any() and a.fsm["alive"].all()


# 13. the GPU equals the CPU model (tests/agent_life_model.py over the storage order), hand case and random swarms
def _model_run(oracle_mod, s, g, boot, death, ticks, restart=None, **kw):
    import agent_life_model as alm
    from test_update_loop_sensed import PER_AGENT
    perm = s.perm.cpu().numpy().astype(np.int64)
    q = dict(g)
    for k in PER_AGENT + (("caps",) if "caps" in g else ()):
        q[k] = np.asarray(g[k])[perm]
    o = alm.set_time(alm.fresh(oracle_mod, q), boot[perm], death[perm])
    if restart is not None:
        o["fsm"]["alive"][restart[perm] != 0] = 1
    o = alm.drive(oracle_mod, q, boot[perm], death[perm], ticks, start=o, **kw)
    out = {k: o[k] for k in ("counts", "agent_events", "task_counts", "link_counts", "guard") if k in o}
    for k in ("state", "leader", "last_hb", "wait_start", "delay", "has_lpos", "alive"):
        out[k] = np.empty_like(o["fsm"][k])
        out[k][perm] = o["fsm"][k]
    for k in ("x", "y", "vx", "vy", "tx", "ty", "has_t", "tick_off") + \
            (("status", "tab_winner", "tab_util") if "task_x" in g else ()):
        out[k] = np.empty_like(o[k])
        out[k][perm] = o[k]
    if "task_x" in g:
        for k in ("claim_out", "conflict_out"):
            out[k] = np.empty_like(o[k])
            out[k][:, perm] = o[k]
    return out


def _check_model(s, r, want):
    from test_update_loop_sensed import _state
    got = _state(s)
    got["tick_off"] = s.to_input_order(s.tick_off)
    for k in ("state", "leader", "last_hb", "wait_start", "delay", "has_lpos", "alive", "x", "y", "vx", "vy", "tx",
              "ty", "has_t", "tick_off"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    for k in ("counts", "agent_events", "task_counts", "link_counts"):
        if k in r:
            np.testing.assert_array_equal(r[k], want[k], err_msg=k)
    if "guard" in r:
        assert r["guard"] == want["guard"]


@pytest.mark.gpu
def test_gpu_three_agents_by_hand(oracle_mod):
    from swarm_amd.swarm import Swarm
    g, boot, death = _hand3()
    s = Swarm(g["ids"], g["x"], g["y"], layout="input", device="cuda")
    s.protocol_reset(tick_off=g["tick_off"], last_hb=g["last_hb0"])
    s.set_agent_lifetimes(boot, death)
    r = s.update_loop_radio(16, 10.0, 0.5, dt=0.1, timeout=0.25, jitter=0.0, seed=1, max_speed=5.0)
    _check_model(s, r, _model_run(oracle_mod, s, g, boot, death, 16, timeout=0.25, jitter=0.0))
    want = HAND3[16]
    assert s.state.tolist() == want[0] and s.leader.tolist() == want[1] and s.fsm["alive"].tolist() == want[2]
    assert s.tick_off.tolist() == [0, 0, -6]


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["input", "spatial"])
@pytest.mark.parametrize("n", [120, 257])
def test_gpu_equals_the_model_on_random_swarms(oracle_mod, n, layout):
    from test_update_loop_radio import _case, _run, _swarm as _radio_swarm
    ticks = 50
    g = _case(n, 40 + n, 2.5, 1.5, ticks=ticks)
    g["kill_ticks"] = np.array([10, 36], np.int64)
    rng = np.random.default_rng(n)
    boot, death = np.zeros(n, np.int64), np.full(n, FOREVER)
    who = rng.permutation(n)
    k = n // 6
    boot[who[:k]] = rng.integers(1, ticks + 1, k)
    death[who[k:2 * k]] = rng.integers(1, ticks + 1, k)
    boot[who[2 * k:3 * k]] = rng.integers(1, ticks, k)
    death[who[2 * k:3 * k]] = boot[who[2 * k:3 * k]] + rng.integers(0, 15, k)  # short lives, empty windows too
    boot[who[0]], boot[who[1]], death[who[k]] = 1, ticks, ticks
    s = _radio_swarm(g, layout)
    s.set_agent_lifetimes(boot, death)
    r = _run(s, g, ticks)
    want = _model_run(oracle_mod, s, g, boot, death, ticks)
    _check_model(s, r, want)
    assert want["counts"][:, 0].max() >= 1 and want["agent_events"].sum() >= 2 * k
    late = (boot > 0) & (death > ticks)
    assert (want["leader"][late] >= 0).any()  # booted agents found a leader


_fixture_models = {}


@pytest.mark.gpu
@pytest.mark.parametrize("loss", [0.0, 0.2])
@pytest.mark.parametrize("layout", ["input", "spatial"])
@pytest.mark.parametrize("name,loop", [("agent_life_radio_n200", "radio"), ("agent_life_wide_n400", "radio"),
                                       ("agent_life_board_n200", "tasks"), ("agent_life_board_n200", "board")])
def test_gpu_equals_the_model_on_the_fixtures(oracle_mod, name, loop, layout, loss):
    """Every fixture on the loop it was made for -- the board fixture on the 64-task loop and on the sparse board
    with rows that hold all its tasks -- in both layouts, over the ideal channel and at loss 0.2, against the model
    run over the swarm's storage order: every array, the per-tick counts, the link counts and the events."""
    from test_update_loop_board import _assert_rows, _rows
    from test_update_loop_radio import _swarm as _radio_swarm
    from test_update_loop_sensed import EXACT, _state
    from test_update_loop_tasks import _assert_tasks, _task_state
    import loop_board_model as lbm
    g = load_golden(name)
    boot, death, ticks, restart = g["boot"], g["death"], int(g["ticks"]), g["restart"]
    T = len(g["task_x"]) if "task_x" in g else 0
    s = _swarm(g, layout, board=False) if T else _radio_swarm(g, layout)
    if loop == "tasks":
        s.set_tasks(g["task_x"], g["task_y"], g["task_req"])
    elif loop == "board":
        s.set_task_board(g["task_x"], g["task_y"], g["task_req"], status_slots=T, table_slots=T)
    s.set_agent_lifetimes(boot, death)
    s.fsm["alive"][_rows_of(s, restart != 0)] = 1
    # the board is handed out at the fixture's task tick: the radio loop until then
    first = int(g["task_tick"]) - 1 if T else 0
    r0 = _step(s, g, "radio", first, loss=loss) if first else None
    r = _step(s, g, loop, ticks - first, loss=loss)
    if r0 is not None:
        z = dict(task_counts=np.zeros((first, 3), np.int64))
        r = {k: np.concatenate([r0[k] if k in r0 else z[k], v]) for k, v in r.items()}
    key = (name, layout, loss)
    if key not in _fixture_models:  # once per storage order and channel, left unchanged
        kw = dict(loss=loss, loss_seed=77) if loss else {}
        _fixture_models[key] = _model_run(oracle_mod, s, g, boot, death, ticks, restart=restart, **kw)
    want = _fixture_models[key]
    if not loss:
        want = {k: v for k, v in want.items() if k != "link_counts"}
        r.pop("link_counts", None)
    r.pop("guard", None)
    _check_model(s, r, want)
    if loop == "tasks":
        _assert_tasks(_task_state(s), want)
    elif loop == "board":
        sets = {k: [[np.flatnonzero((int(w) >> np.arange(64)) & 1).tolist() for w in want[k][h]] for h in (0, 1)]
                for k in ("claim_out", "conflict_out")}
        tt, tw, tu = lbm.sparse_tables(want["tab_winner"], want["tab_util"], T)
        _assert_rows(_rows(s), dict(status=lbm.sparse_status(want["status"], T), tab_task=tt, tab_winner=tw,
                                    tab_util=tu, claim_out=np.stack([lbm.sparse_sets(sets["claim_out"][h], T)
                                                                     for h in (0, 1)]),
                                    conflict_out=np.stack([lbm.sparse_sets(sets["conflict_out"][h], T)
                                                           for h in (0, 1)])))
    if layout == "input" and not loss:  # real agents, in everything the squares cannot reach
        got = _state(s)
        for k in EXACT:
            np.testing.assert_array_equal(got[k], g[k + "_out"], err_msg=k)
        np.testing.assert_array_equal(s.to_input_order(s.tick_off), g["tick_off_out"])
        np.testing.assert_array_equal(r["agent_events"], g["agent_events"])
        if loop == "tasks":
            np.testing.assert_array_equal(_task_state(s)["status"], g["status_out"])
            np.testing.assert_array_equal(r["task_counts"], g["task_counts"])
