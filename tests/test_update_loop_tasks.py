"""The update loop that claims and resolves tasks every tick (contract U1-T):
swarm_update_loop_tasks / Swarm.set_tasks + Swarm.update_loop_tasks(ticks, Rc, Rs).

tests/golden/loop_tasks_*.npz were produced by real SwarmAgent objects driven through the radio loop with all
five message types dispatched and a board of 24 tasks handed to every agent at task_tick
(tools/gen_golden_loop_tasks.py).  The CPU model (tests/loop_tasks_model.py: the handlers restated over
explicit messages) must reproduce them bit for bit with the reference's libm pow; the GPU must equal the same
model with its own x*x squares bit for bit, over the GPU's storage order, and the fixture itself in layout
"input".  The hand-built cases are resting agents (max_speed 0) in layout "input", so that the walk order is
the order they are listed in, with the expected values written out.
"""
import ctypes
import re
import time

import numpy as np
import pytest

from conftest import load_golden
import loop_radio_model
import loop_tasks_model
from loop_model import OUT_KEYS, F, L
from test_update_loop_sensed import EXACT, PER_AGENT, _assert_equal, _state

TASKS = ("loop_tasks_n200", "loop_tasks_wide_n400", "loop_tasks_r12_n250")
ALL = OUT_KEYS + ("px", "py")
TASK_ARRAYS = ("status", "tab_winner", "tab_util", "claim_out", "conflict_out")
OPEN, TENTATIVE, LOCKED, ASSIGNED = 0, 1, 2, 3
DISCRETE = ("state", "leader", "has_lpos", "alive", "has_t")


# ----------------------------------------------------------------------------- CPU

_pow_models = {}


def _pow_model(oracle_mod, name):
    if name not in _pow_models:  # computed once, shared, left unchanged
        _pow_models[name] = loop_tasks_model.run(oracle_mod, load_golden(name), use_pow=True)
    return _pow_models[name]


@pytest.mark.parametrize("name", TASKS)
def test_model_with_pow_equals_the_reference_fixture(oracle_mod, name):
    g = load_golden(name)
    o = _pow_model(oracle_mod, name)
    for k in OUT_KEYS:  # the thirteen arrays
        np.testing.assert_array_equal(o[k], g[k + "_out"], err_msg=k)
    np.testing.assert_array_equal(o["counts"], g["counts"])
    for k in ("status", "tab_winner"):
        np.testing.assert_array_equal(o[k], g[k + "_out"], err_msg=k)
    np.testing.assert_array_equal(o["tab_util"].view(np.uint32), g["tab_util_out"].view(np.uint32))
    for k in ("claim_out", "conflict_out", "task_counts"):
        np.testing.assert_array_equal(o[k], g[k], err_msg=k)
    assert o["singular"] == 0 and o["guard"] == 0


@pytest.mark.parametrize("name", TASKS)
def test_fixtures_exercise_every_branch_of_the_handlers(name):
    g = load_golden(name)
    tc = g["task_counts"]
    assert sorted(set(g["status_out"].ravel().tolist())) == [OPEN, TENTATIVE, LOCKED, ASSIGNED]
    assert tc[:int(g["task_tick"]) - 1].sum() == 0 and tc[int(g["task_tick"]) - 1, 0] > 0
    assert tc[:, 1].sum() >= 20 and tc[:, 2].sum() >= 20 and tc[:, 0].sum() - tc[:, 1].sum() >= 20
    assert (g["tab_winner_out"] >= 0).any(axis=1).sum() >= 3  # several leaders kept a table of their own


@pytest.mark.parametrize("name", TASKS)
def test_squares_model_equals_the_pow_model_in_everything_discrete(oracle_mod, name):
    g = load_golden(name)
    a, b = _pow_model(oracle_mod, name), loop_tasks_model.run(oracle_mod, g, use_pow=False)
    for k in TASK_ARRAYS + ("task_counts", "counts") + DISCRETE:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert b["guard"] == 0


def test_model_without_tasks_equals_the_radio_model(oracle_mod):
    g = dict(load_golden("loop_tasks_n200"))
    g["task_x"] = g["task_y"] = np.zeros(0)
    g["task_req"] = np.zeros(0, np.int8)
    a, b = loop_tasks_model.run(oracle_mod, g, 120), loop_radio_model.run(oracle_mod, g, 120)
    _assert_equal(a, b, ALL)
    np.testing.assert_array_equal(a["counts"], b["counts"])
    assert a["task_counts"].sum() == 0 and a["status"].shape == (200, 0)


def test_model_in_chunks_equals_one_run(oracle_mod):
    g = load_golden("loop_tasks_n200")
    one = loop_tasks_model.run(oracle_mod, g, 60)
    o = None
    for chunk in (44, 1, 1, 3, 11):
        o = loop_tasks_model.run(oracle_mod, g, chunk, start=o)
    _assert_equal(o, one, ALL + TASK_ARRAYS)


def test_header_exports_equal_the_library_binding():
    from swarm_amd import _lib
    with open(_lib.INCLUDE_H) as f:
        declared = set(re.findall(r"^(?:int|const char \*)\s*(swarm_\w+)\(", f.read(), re.M))
    assert declared == set(_lib.EXPORTS)
    lib = _lib.load()
    for name in _lib.EXPORTS:
        assert hasattr(lib, name), name
    assert "swarm_update_loop_tasks" in declared
    assert ctypes.sizeof(_lib.Tasks) == 80  # int32 + padding, nine pointers


def test_entry_point_rejects_bad_boards_without_gpu():
    from swarm_amd import _lib
    lib = _lib.load()

    def call(ctx, tasks):
        return lib.swarm_update_loop_tasks(ctx, 4, None, None, None, None, None, 0, 1, 0.1, 3.0, 0.2,
                                           ctypes.c_uint64(0), None, 0, None, None, None, 0, None, 2.5, 2.5, 5.0,
                                           None, 0, None, None, None, tasks, None, None, None)
    assert call(None, None) == _lib.ERR_ARG and b"ctx is NULL" in lib.swarm_last_error()
    fake = ctypes.c_void_p(8)  # never dereferenced: the board is refused first
    assert call(fake, None) == _lib.ERR_ARG and b"tasks is NULL" in lib.swarm_last_error()
    for T in (-1, 65):
        assert call(fake, ctypes.byref(_lib.Tasks(T))) == _lib.ERR_ARG and b"[0, 64]" in lib.swarm_last_error()
    assert call(fake, ctypes.byref(_lib.Tasks(3))) == _lib.ERR_ARG and b"NULL task array" in lib.swarm_last_error()


def test_update_loop_tasks_needs_a_board_and_good_radii_without_a_device():
    from swarm_amd.swarm import Swarm
    s = Swarm.__new__(Swarm)
    with pytest.raises(RuntimeError, match="set_tasks"):
        s.update_loop_tasks(3, 2.5, 2.5)
    s.tasks = {}
    with pytest.raises(ValueError, match="radio_radius must be positive and finite"):
        s.update_loop_tasks(3, 0.0, 1.0)
    with pytest.raises(ValueError, match="sense_radius must be positive and finite"):
        s.update_loop_tasks(3, 2.5, float("nan"))


# ----------------------------------------------------------------------------- GPU

def _swarm(g, layout="input", board=True):
    """test_update_loop_radio._swarm with the agents' capabilities, and the case's board unless told not to."""
    import torch
    from swarm_amd.swarm import Swarm
    s = Swarm(g["ids"], g["x"], g["y"], g["caps"], layout=layout, device="cuda")
    s.protocol_reset(tick_off=g["tick_off"], last_hb=g["last_hb0"])
    idx = np.flatnonzero(g["has_t"])
    if len(idx):
        s.set_target(g["tx"][idx], g["ty"][idx], index=idx)
    where = dict(state=(s.state, torch.uint8), leader=(s.leader, torch.int32), alive=(s.fsm["alive"], torch.uint8))
    for k, v in g.get("fsm0", {}).items():  # input order -> storage order
        where[k][0].copy_(s._storage(v, where[k][1]))
    if board:
        s.set_tasks(g["task_x"], g["task_y"], g["task_req"])
    return s


def _kw(g):
    return dict(obstacles=g["obs"], kill_ticks=g["kill_ticks"], dt=float(g["dt"]), seed=int(g["seed"]),
                max_speed=float(g["max_speed"]))


def _run(s, g, ticks, **kw):
    return s.update_loop_tasks(ticks, float(g["radio_radius"]), float(g["sense_radius"]), **_kw(g), **kw)


def _run_radio(s, g, ticks):
    return s.update_loop_radio(ticks, float(g["radio_radius"]), float(g["sense_radius"]), **_kw(g))


def _task_state(s):
    """The task arrays in input order: status (n, T), the tables, the two sets as (2, n) uint64."""
    w, u = s.task_tables()
    out = dict(status=s.to_input_order(s.task_status()), tab_winner=s.to_input_order(w),
               tab_util=s.to_input_order(u))
    for k in ("claim_out", "conflict_out"):
        a = s.tasks[k].cpu().numpy().view(np.uint64).reshape(2, s.n)
        out[k] = np.stack([s.to_input_order(s.tasks[k][h * s.n:(h + 1) * s.n]).view(np.uint64) for h in (0, 1)])
        assert a.shape == out[k].shape
    return out


def _assert_tasks(got, want):
    for k in ("status", "tab_winner", "claim_out", "conflict_out"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    np.testing.assert_array_equal(got["tab_util"].view(np.uint32), np.asarray(want["tab_util"]).view(np.uint32),
                                  err_msg="tab_util bits")


def _model(oracle_mod, s, g, ticks=None, plan=None, **kw):
    """loop_tasks_model.run over s's storage order, its per-agent results put back into input order."""
    perm = s.perm.cpu().numpy().astype(np.int64)
    q = dict(g)
    for k in PER_AGENT + ("caps",):
        q[k] = np.asarray(g[k])[perm]
    if "fsm0" in g:
        q["fsm0"] = {k: np.asarray(v)[perm] for k, v in g["fsm0"].items()}
    o, counts, tcounts, singular, guard = None, [], [], 0, 0
    for chunk in (plan or [ticks]):
        o = loop_tasks_model.run(oracle_mod, q, chunk, start=o, **kw)
        counts.append(o["counts"])
        tcounts.append(o["task_counts"])
        singular += o["singular"]
        guard += o["guard"]
    out = {}
    for k, v in o.items():
        if k in ("claim_out", "conflict_out"):
            out[k] = np.empty_like(v)
            out[k][:, perm] = v
        elif isinstance(v, np.ndarray) and k not in ("counts", "task_counts"):
            out[k] = np.empty_like(v)
            out[k][perm] = v
        else:
            out[k] = v
    out.update(counts=np.concatenate(counts), task_counts=np.concatenate(tcounts), singular=singular, guard=guard)
    return out


_models = {}


def _fixture_model(oracle_mod, s, name, layout, use_pow=False):
    key = (name, layout, use_pow)
    if key not in _models:  # once per storage order, shared, left unchanged
        _models[key] = _model(oracle_mod, s, load_golden(name), int(load_golden(name)["ticks"]), use_pow=use_pow)
    return _models[key]


def _check_fixture(oracle_mod, s, g, name, layout, counts, tcounts, guard, singular):
    want = _fixture_model(oracle_mod, s, name, layout)
    got = _state(s)
    _assert_equal(got, want, ALL)
    tk = _task_state(s)
    _assert_tasks(tk, want)
    np.testing.assert_array_equal(counts, want["counts"])
    np.testing.assert_array_equal(tcounts, want["task_counts"])
    assert guard == want["guard"] == 0 and singular == want["singular"] == 0
    if layout == "input":  # the fixture's own order: real agents, in everything the squares cannot reach
        for k in EXACT:
            np.testing.assert_array_equal(got[k], g[k + "_out"], err_msg=k)
        _assert_tasks(tk, dict(status=g["status_out"], tab_winner=g["tab_winner_out"], tab_util=g["tab_util_out"],
                               claim_out=g["claim_out"], conflict_out=g["conflict_out"]))
        np.testing.assert_array_equal(counts, g["counts"])
        np.testing.assert_array_equal(tcounts, g["task_counts"])
    else:  # another order: the reference is the pow model over it (pinned to real agents above)
        ref = _fixture_model(oracle_mod, s, name, layout, use_pow=True)
        for k in EXACT:
            np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
        _assert_tasks(tk, ref)
        np.testing.assert_array_equal(tcounts, ref["task_counts"])
    assert s.fsm_tick == int(g["ticks"]) and s.last_refused_tick == -1 and s.row_ptr is None


# 1. fixtures: an empty board up to the hand-out, then the board
@pytest.mark.gpu
@pytest.mark.parametrize("name", TASKS)
@pytest.mark.parametrize("layout", ["input", "spatial"])
def test_gpu_equals_the_model_and_the_reference_fixture(oracle_mod, name, layout):
    g = load_golden(name)
    s = _swarm(g, layout, board=False)
    first, ticks = int(g["task_tick"]) - 1, int(g["ticks"])
    s.set_tasks([], [])
    r0 = _run(s, g, first)  # T = 0
    assert r0["task_counts"].shape == (first, 3) and r0["task_counts"].sum() == 0 and r0["guard"] == 0
    s.set_tasks(g["task_x"], g["task_y"], g["task_req"])
    r1 = _run(s, g, ticks - first)
    _check_fixture(oracle_mod, s, g, name, layout, np.concatenate([r0["counts"], r1["counts"]]),
                   np.concatenate([r0["task_counts"], r1["task_counts"]]), r1["guard"],
                   r0["singular"] + r1["singular"])


# 2. fixtures: the radio loop up to the hand-out (the loops chain)
@pytest.mark.gpu
@pytest.mark.parametrize("name", TASKS)
def test_gpu_radio_loop_then_set_tasks_then_task_loop(oracle_mod, name):
    g = load_golden(name)
    s = _swarm(g, "input", board=False)
    first, ticks = int(g["task_tick"]) - 1, int(g["ticks"])
    r0 = _run_radio(s, g, first)
    s.set_tasks(g["task_x"], g["task_y"], g["task_req"])
    r1 = _run(s, g, ticks - first)
    _check_fixture(oracle_mod, s, g, name, "input", np.concatenate([r0["counts"], r1["counts"]]),
                   np.concatenate([np.zeros((first, 3), np.int64), r1["task_counts"]]), r1["guard"],
                   r0["singular"] + r1["singular"])


# 3. chunks
@pytest.mark.gpu
@pytest.mark.parametrize("chunks", [(1, 1, 1, 1, 3, 8), (2, 2, 2, 9), (3, 12)])
def test_gpu_chunked_run_is_the_same_run(chunks):
    """From the hand-out on: the first claims leave at tick 45, the first conflicts at tick 46, so every
    boundary of the first chunks has claims or conflicts in flight, at odd and at even ticks."""
    import torch
    g = load_golden("loop_tasks_n200")
    first = int(g["task_tick"]) - 1
    a, b = _swarm(g, "spatial"), _swarm(g, "spatial")
    _run_radio(a, g, first)
    _run_radio(b, g, first)
    ra = _run(a, g, sum(chunks))
    rb = [_run(b, g, c) for c in chunks]
    assert ra["task_counts"][0, 0] > 0 and ra["task_counts"][1, 1] > 0 and ra["task_counts"][1, 2] > 0
    for t in ("pos", "pos_prev", "vel", "target", "has_target", "state", "leader"):
        assert torch.equal(getattr(a, t), getattr(b, t)), t
    for k in a.fsm:
        assert torch.equal(a.fsm[k], b.fsm[k]), k
    for k in a.tasks:
        if isinstance(a.tasks[k], torch.Tensor):
            assert torch.equal(a.tasks[k], b.tasks[k]), k
    np.testing.assert_array_equal(ra["task_counts"], np.concatenate([r["task_counts"] for r in rb]))
    np.testing.assert_array_equal(ra["counts"], np.concatenate([r["counts"] for r in rb]))
    assert ra["guard"] == sum(r["guard"] for r in rb)


# 4. hand-built cases
def _hand(xy, ids, lead=(), caps=None, tasks=(), off=None, rc=2.5, kill=()):
    """Resting agents (no targets, max_speed 0: nobody moves) in the order given; `lead`: the indices that
    start as LEADERs of themselves; tick_off 0 (a LEADER heartbeats at tick 10) unless given; tasks:
    (x, y, required capability bit or -1)."""
    n = len(ids)
    xy = np.asarray(xy, np.float64).reshape(n, 2)
    state = np.full(n, F, np.uint8)
    leader = np.full(n, -1, np.int32)
    for i in lead:
        state[i], leader[i] = L, ids[i]
    tasks = np.asarray(tasks, np.float64).reshape(-1, 3)
    return dict(ids=np.asarray(ids, np.int32), x=xy[:, 0].copy(), y=xy[:, 1].copy(),
                tick_off=np.zeros(n, np.int32) if off is None else np.asarray(off, np.int32), last_hb0=np.zeros(n),
                tx=np.zeros(n), ty=np.zeros(n), has_t=np.zeros(n, np.uint8), obs=np.array([[1000.0, 1000.0, 0.5]]),
                kill_ticks=np.asarray(kill, np.int64), seed=np.uint64(3), dt=np.float64(0.1),
                max_speed=np.float64(0.0), radio_radius=np.float64(rc), sense_radius=np.float64(1.0),
                fsm0=dict(state=state, leader=leader),
                caps=np.zeros(n, np.uint32) if caps is None else np.asarray(caps, np.uint32),
                task_x=tasks[:, 0].copy(), task_y=tasks[:, 1].copy(), task_req=tasks[:, 2].astype(np.int8))


def _go(g, ticks):
    s = _swarm(g, "input")
    r = _run(s, g, ticks)
    st, tk = _state(s), _task_state(s)
    np.testing.assert_array_equal(st["x"], g["x"])  # at rest
    np.testing.assert_array_equal(st["y"], g["y"])
    return s, r, st, tk


def _u32(dx, dy):
    """The claim's '!f' utility for an offset (dx, dy), the GPU's arithmetic."""
    return np.float32(100.0 / (1.0 + np.sqrt(np.float64(dx) * dx + np.float64(dy) * dy)))


@pytest.mark.gpu
def test_gpu_leader_that_yields_mid_walk_keeps_the_claims_before_and_ignores_those_after():
    # walk order of receiver R (ID 5, index 3): claimer C1 (ID 1), leader H (ID 9, heartbeats at tick 1),
    # claimer C2 (ID 2).  H hears neither claimer (4.0 and 2.83 away).  Task 0 needs bit 0 (C1 only), task 1
    # bit 1 (C2 only), each 1.0 from its claimer: U = 50.
    g = _hand([(-2, 0), (2, 0), (0, -2), (0, 0)], [1, 9, 2, 5], lead=(1, 3), caps=[1, 0, 2, 0],
              tasks=[(-2, 1, 0), (1, -2, 1)], off=[0, 9, 0, 0])
    s, r, st, tk = _go(g, 3)
    np.testing.assert_array_equal(r["task_counts"], [[2, 0, 0], [0, 1, 1], [0, 0, 0]])
    np.testing.assert_array_equal(st["state"], [F, L, F, F])
    assert st["leader"][3] == 9
    np.testing.assert_array_equal(tk["tab_winner"], [[-1, -1], [-1, -1], [-1, -1], [1, -1]])
    np.testing.assert_array_equal(tk["tab_util"], np.array([[0, 0], [0, 0], [0, 0], [50, 0]], np.float32))
    # tick 3: R's conflict on task 0 names ID 1 -- C1 ASSIGNED, H and C2 LOCKED; C2's claim was lost
    np.testing.assert_array_equal(tk["status"], [[ASSIGNED, OPEN], [LOCKED, OPEN], [LOCKED, TENTATIVE], [OPEN, OPEN]])
    np.testing.assert_array_equal(tk["conflict_out"], [[0, 0, 0, 1], [0, 0, 0, 0]])  # tick 2's sets at parity 0
    assert r["guard"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["near first", "far first"])
@pytest.mark.parametrize("gap", ["more than 5", "less than 5"])
def test_gpu_two_claims_of_one_tick_meet_the_hysteresis_in_walk_order(order, gap):
    # leader R (ID 9, lacks the capability) at the origin, the task at (0, 1); the near claimer (ID 1) at
    # (-1, 0): U = 100 / (1 + sqrt 2) = 41.42; the far one (ID 2) at (1.2, 0): 39.03, or at (2, 0): 30.90
    far_x = 1.2 if gap == "less than 5" else 2.0
    near, far = ((-1.0, 0.0), 1), ((far_x, 0.0), 2)
    a, b = (near, far) if order == "near first" else (far, near)
    g = _hand([a[0], b[0], (0, 0)], [a[1], b[1], 9], lead=(2,), caps=[1, 1, 0], tasks=[(0, 1, 0)])
    s, r, st, tk = _go(g, 3)
    u_near, u_far = _u32(-1.0, -1.0), _u32(far_x, -1.0)
    assert (float(u_near) - float(u_far) > 5.0) == (gap == "more than 5")
    # more than 5 apart the near claim wins in either order (taken, or replacing); less, the first one heard
    win = 1 if gap == "more than 5" or order == "near first" else 2
    assert tk["tab_winner"][2, 0] == win
    assert tk["tab_util"][2, 0].view(np.uint32) == (u_near if win == 1 else u_far).view(np.uint32)
    np.testing.assert_array_equal(r["task_counts"], [[2, 0, 0], [0, 2, 2], [0, 0, 0]])
    want = {1: ASSIGNED if win == 1 else LOCKED, 2: ASSIGNED if win == 2 else LOCKED}
    np.testing.assert_array_equal(tk["status"][:, 0], [want[a[1]], want[b[1]], OPEN])


@pytest.mark.gpu
@pytest.mark.parametrize("first", ["L1", "L2"])
def test_gpu_bystander_of_two_leaders_keeps_the_last_conflict_in_walk_order(first):
    # L1 (ID 8) at (-2, 0) hears only B (ID 3, origin); L2 (ID 9) at (2, 0) hears B and C2 (ID 4, at (4, 0)).
    # The task at (3, 0) needs bit 0 (B and C2): B claims with U = 25, C2 with 50.  L1's table names B; L2's
    # takes B, then C2 (50 > 25 + 5).  At tick 3 B hears both leaders' conflicts in index order.
    l1, l2 = ((-2.0, 0.0), 8), ((2.0, 0.0), 9)
    a, b = (l1, l2) if first == "L1" else (l2, l1)
    g = _hand([a[0], b[0], (0, 0), (4, 0)], [a[1], b[1], 3, 4], lead=(0, 1), caps=[0, 0, 1, 1], tasks=[(3, 0, 0)])
    s, r, st, tk = _go(g, 3)
    i1, i2 = (0, 1) if first == "L1" else (1, 0)
    assert tk["tab_winner"][i1, 0] == 3 and tk["tab_util"][i1, 0] == np.float32(25.0)
    assert tk["tab_winner"][i2, 0] == 4 and tk["tab_util"][i2, 0] == np.float32(50.0)
    np.testing.assert_array_equal(r["task_counts"], [[2, 0, 0], [0, 3, 3], [0, 0, 0]])
    # L1 then L2: ASSIGNED, overwritten by LOCKED; L2 then L1: LOCKED, overwritten by ASSIGNED
    assert tk["status"][2, 0] == (LOCKED if first == "L1" else ASSIGNED)
    assert tk["status"][3, 0] == ASSIGNED and tk["status"][0, 0] == OPEN and tk["status"][1, 0] == OPEN


@pytest.mark.gpu
def test_gpu_claim_no_leader_hears_stays_tentative_and_is_never_sent_again():
    g = _hand([(0, 0), (10, 0)], [1, 9], lead=(1,), tasks=[(1, 0, -1)])  # the leader is 10 away
    s, r, st, tk = _go(g, 6)
    np.testing.assert_array_equal(r["task_counts"], [[1, 0, 0]] + [[0, 0, 0]] * 5)
    np.testing.assert_array_equal(tk["status"][:, 0], [TENTATIVE, OPEN])
    assert (tk["tab_winner"] == -1).all() and not tk["claim_out"].any() and not tk["conflict_out"].any()


@pytest.mark.gpu
def test_gpu_utility_of_exactly_20_is_no_claim_and_counts_in_the_guard_band():
    # 4.0 away: U = 100 / 5 = 20.0, not > 20; evaluated again at each of the three ticks
    g = _hand([(0, 0)], [1], tasks=[(4, 0, -1)])
    s, r, st, tk = _go(g, 3)
    assert r["guard"] == 3 and r["task_counts"].sum() == 0 and tk["status"][0, 0] == OPEN
    # one ulp nearer: whatever fp64 makes of it (the separately rounded square, IEEE sqrt and division), and
    # inside the guard band while it is evaluated
    tx = np.nextafter(4.0, 0.0)
    U = 100.0 / (1.0 + np.sqrt((0.0 - tx) * (0.0 - tx) + 0.0))
    g = _hand([(0, 0)], [1], tasks=[(tx, 0, -1)])
    s, r, st, tk = _go(g, 3)
    claims = bool(U > 20.0)
    assert r["task_counts"][:, 0].tolist() == ([1, 0, 0] if claims else [0, 0, 0])
    assert tk["status"][0, 0] == (TENTATIVE if claims else OPEN) and r["guard"] == (1 if claims else 3)


@pytest.mark.gpu
def test_gpu_claimer_at_exactly_the_radio_radius_is_heard_and_one_ulp_further_is_not():
    # two leader / claimer pairs 100 apart; the tasks 1.0 beyond their claimers, out of the leaders' reach
    # (the leaders lack the capability; the second pair keeps x small so that the coordinate holds the ulp)
    far = np.nextafter(2.5, 3.0)
    g = _hand([(0, 0), (2.5, 0), (0, 100), (far, 100)], [8, 1, 9, 2], lead=(0, 2), caps=[0, 1, 0, 1],
              tasks=[(3.5, 0, 0), (far + 1.0, 100, 0)])
    assert (0.0 - far) * (0.0 - far) > 2.5 * 2.5
    s, r, st, tk = _go(g, 3)
    np.testing.assert_array_equal(r["task_counts"], [[2, 0, 0], [0, 1, 1], [0, 0, 0]])
    np.testing.assert_array_equal(tk["tab_winner"], [[1, -1], [-1, -1], [-1, -1], [-1, -1]])
    np.testing.assert_array_equal(tk["status"], [[OPEN, OPEN], [ASSIGNED, OPEN], [OPEN, OPEN], [OPEN, TENTATIVE]])


@pytest.mark.gpu
def test_gpu_missing_capability_claims_nothing():
    g = _hand([(0, 0), (0.5, 0)], [1, 2], caps=[0b10, 0b01], tasks=[(0, 1, 0)])  # bit 0: agent 2 only
    s, r, st, tk = _go(g, 2)
    np.testing.assert_array_equal(tk["status"][:, 0], [OPEN, TENTATIVE])
    assert r["task_counts"][:, 0].tolist() == [1, 0] and r["guard"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 64])
def test_gpu_smallest_and_largest_board(T):
    # the last task of the board 1.0 from the claimer, the others far away; bit T - 1 of every word
    tasks = [(1000.0 + 10 * k, 0, -1) for k in range(T - 1)] + [(1, 0, -1)]
    g = _hand([(0, 0), (0, 2)], [1, 9], lead=(1,), tasks=tasks)
    s, r, st, tk = _go(g, 3)
    bit = np.uint64(1) << np.uint64(T - 1)
    want = np.zeros((2, T), np.uint8)
    want[0, T - 1] = ASSIGNED  # (the leader, sqrt 5 away, claimed it too: TENTATIVE, nobody arbitrates for it)
    want[1, T - 1] = TENTATIVE
    np.testing.assert_array_equal(tk["status"], want)
    np.testing.assert_array_equal(tk["conflict_out"], [[0, bit], [0, 0]])
    assert tk["tab_winner"][1, T - 1] == 1 and tk["tab_util"][1, T - 1] == np.float32(50.0)
    assert (np.delete(tk["tab_winner"].ravel(), T + T - 1) == -1).all()
    np.testing.assert_array_equal(r["task_counts"], [[2, 0, 0], [0, 1, 1], [0, 0, 0]])
    assert int(s.tasks["status_hi"].cpu().numpy().view(np.uint64)[0]) == int(bit)


@pytest.mark.gpu
@pytest.mark.parametrize("bad", ["T = 65", "treq = 32", "treq = -2"])
def test_gpu_bad_board_is_refused_and_nothing_is_written(bad):
    import torch
    from swarm_amd import _lib
    T = 65 if bad == "T = 65" else 3
    tasks = [(1, 0, -1)] * T
    if bad != "T = 65":
        tasks[1] = (1, 0, 32 if bad == "treq = 32" else -2)
    g = _hand([(0, 0), (0, 2)], [1, 9], lead=(1,), tasks=tasks)
    s = _swarm(g, "input")
    keep = dict(pos=s.pos, state=s.state, **s.fsm, **{k: v for k, v in s.tasks.items() if isinstance(v, torch.Tensor)})
    before = {k: v.clone() for k, v in keep.items()}
    with pytest.raises(_lib.SwarmError) as e:
        _run(s, g, 3)
    assert e.value.code == _lib.ERR_ARG and ("[0, 64]" if bad == "T = 65" else "[-1, 31]") in str(e.value)
    assert s.fsm_tick == 0
    for k, v in keep.items():
        assert torch.equal(v, before[k]), k


@pytest.mark.gpu
def test_gpu_conflicts_of_a_leader_killed_a_tick_later_still_arrive():
    g = _hand([(0, 0), (0, 2)], [1, 9], lead=(1,), caps=[1, 0], tasks=[(1, 0, 0)], kill=(3,))
    s, r, st, tk = _go(g, 4)
    np.testing.assert_array_equal(st["alive"], [1, 0])
    np.testing.assert_array_equal(r["task_counts"], [[1, 0, 0], [0, 1, 1], [0, 0, 0], [0, 0, 0]])
    np.testing.assert_array_equal(tk["status"][:, 0], [ASSIGNED, OPEN])
    assert tk["tab_winner"][1, 0] == 1  # the table outlives its owner
    assert not tk["conflict_out"].any() and not tk["claim_out"].any()  # the dead send nothing more


@pytest.mark.gpu
@pytest.mark.parametrize("m", [1, 2, 3, 4, 5, 6, 7])
def test_gpu_one_to_seven_claimers_around_one_leader(oracle_mod, m):
    """The sorted list of four heard senders fills up and overflows into the merge.  Claimer k (index k, ID
    k + 1) sits 0.3 (k + 1) from the leader on a ray, the task at the leader's place (the leader lacks the
    capability): U falls with k, so the first claimer heard takes the entry and every other one is re-affirmed
    against (U_0 = 76.9 against at most U_1 + 5 = 67.5)."""
    ang = 2.0 * np.pi * np.arange(m) / 7.0
    rad = 0.3 * (np.arange(m) + 1.0)
    xy = [(50.0 + r_ * np.cos(a), 50.0 + r_ * np.sin(a)) for r_, a in zip(rad, ang)] + [(50.0, 50.0)]
    g = _hand(xy, list(range(1, m + 1)) + [99], lead=(m,), caps=[1] * m + [0], tasks=[(50.0, 50.0, 0)])
    s, r, st, tk = _go(g, 3)
    np.testing.assert_array_equal(r["task_counts"], [[m, 0, 0], [0, m, m], [0, 0, 0]])
    assert tk["tab_winner"][m, 0] == 1
    u0 = _u32(xy[0][0] - 50.0, xy[0][1] - 50.0)
    assert tk["tab_util"][m, 0].view(np.uint32) == u0.view(np.uint32)
    np.testing.assert_array_equal(tk["status"][:, 0], [ASSIGNED] + [LOCKED] * (m - 1) + [OPEN])
    want = _model(oracle_mod, s, g, 3)
    _assert_tasks(tk, want)


@pytest.mark.gpu
def test_gpu_dense_block_of_claimers_and_leaders_over_all_nine_cells(oracle_mod):
    """300 agents at random in a 7.4 x 7.4 block (three cells of side 2.5 each way), every fifth a LEADER, the
    rest claimers of 12 tasks scattered over the block: receivers with claimers in all nine cells of their
    windows, dozens of claims per leader walk (the merge), leaders that hear each other's conflicts."""
    rng = np.random.default_rng(12)
    n = 300
    xy = np.stack([20.0 + rng.uniform(0.0, 7.4, n), 30.0 + rng.uniform(0.0, 7.4, n)], 1)
    tasks = [(20.0 + rng.uniform(0.0, 7.4), 30.0 + rng.uniform(0.0, 7.4), int(rng.integers(-1, 3))) for _ in range(12)]
    g = _hand(xy, rng.permutation(n), lead=tuple(range(0, n, 5)), caps=rng.integers(0, 8, n), tasks=tasks)
    s = _swarm(g, "input")
    want = _model(oracle_mod, s, g, 5)
    tc = want["task_counts"]
    assert want["max_heard"] >= 80 and tc[0, 0] >= 500 and tc[1, 1] >= 1000 and tc[1, 2] >= 1000
    r = _run(s, g, 5)
    _assert_equal(_state(s), want, ALL)
    _assert_tasks(_task_state(s), want)
    np.testing.assert_array_equal(r["task_counts"], tc)
    np.testing.assert_array_equal(r["counts"], want["counts"])
    assert r["guard"] == want["guard"]


@pytest.mark.gpu
def test_gpu_follower_among_claimers_hears_its_one_heartbeat_and_the_leader_beside_it_the_claims(oracle_mod):
    """What a receiver listens to decides which window cells and which sender bytes count for it.  FOLLOWER R
    (index 12) and LEADER H (index 13, heartbeats at tick 1) share the middle cell of a 3 x 3 grid of side 2.5;
    three claimers sit in each of the eight cells around them, all within Rc of both, each with a task of its
    own 0.5 away.  At tick 2 R's window holds claimers in eight cells -- for a LEADER more than the sorted list
    is tried for -- but the only sender R listens to is H: it takes the heartbeat and handles no claim.  H, in
    the same crowd, handles all 24.  An anchor at the origin fixes the grid's corner."""
    rc, n_cl = 2.5, 24
    ring = [(dx, dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy) != (0, 0)]
    jit = [(0.0, 0.0), (-0.2, 0.1), (0.15, -0.2)]
    cl = [(3.75 + 1.55 * dx + jx, 3.75 + 1.55 * dy + jy) for dx, dy in ring for jx, jy in jit]
    xy = cl[:12] + [(3.75, 3.75), (3.8, 3.75)] + cl[12:] + [(0.0, 0.0)]
    ids = list(range(1, 13)) + [50, 99] + list(range(13, 25)) + [60]
    bit = list(range(12)) + [None, None] + list(range(12, 24)) + [None]
    caps = [0 if b is None else 1 << b for b in bit]
    tasks = [(x, y + 0.5, b) for (x, y), b in zip(xy, bit) if b is not None]
    n, R, H = len(ids), 12, 13
    g = _hand(xy, ids, lead=(H,), caps=caps, tasks=tasks, off=[9 if i == H else 0 for i in range(n)], rc=rc)
    s = _swarm(g, "input")
    # the precondition, from the model's first tick: who claimed, who sent an election packet
    one = _model(oracle_mod, s, g, 1)
    claimed = one["claim_out"][1] != 0
    sent = (np.asarray(one["fsm"]["outbox"])[n:] & 3) != 0
    side = rc * (1.0 + 1e-9)  # the run's cells: max(Rc, min(Rs, 2)) widened by 1e-9, from the bounding box's corner
    cx, cy = (np.minimum(np.floor((g[k] - g[k].min()) * (1.0 / side)), 2).astype(int) for k in ("x", "y"))
    assert (cx[R], cy[R]) == (cx[H], cy[H]) == (1, 1) and claimed.sum() == n_cl
    assert len({(a, b) for a, b in zip(cx[claimed], cy[claimed])}) >= 5  # (every cell of the grid is in R's window)
    near = (g["x"] - g["x"][R]) ** 2 + (g["y"] - g["y"][R]) ** 2 <= rc * rc
    near[R] = False
    assert (near & claimed).sum() == n_cl and np.flatnonzero(near & sent).tolist() == [H]
    want = _model(oracle_mod, s, g, 3)
    np.testing.assert_array_equal(want["task_counts"], [[n_cl, 0, 0], [0, n_cl, n_cl], [0, 0, 0]])
    r = _run(s, g, 3)
    st = _state(s)
    _assert_equal(st, want, ALL)
    _assert_tasks(_task_state(s), want)
    np.testing.assert_array_equal(r["task_counts"], want["task_counts"])
    np.testing.assert_array_equal(r["counts"], want["counts"])
    assert r["guard"] == want["guard"]
    assert st["state"][R] == F and st["leader"][R] == 99 and st["state"][H] == L


# 5. a large random swarm
@pytest.mark.gpu
def test_gpu_random_swarm_of_20001_agents_equals_the_model(oracle_mod):
    from test_update_loop_sensed import _random_case
    g = _random_case(20001, 23, ticks=40)
    rng = np.random.default_rng(5)
    lo, hi = g["x"].min(), g["x"].max()
    g.update(radio_radius=np.float64(2.5), sense_radius=np.float64(2.5), caps=rng.integers(0, 8, 20001).astype(np.uint32),
             task_x=rng.uniform(lo, hi, 24), task_y=rng.uniform(lo, hi, 24),
             task_req=rng.integers(-1, 3, 24).astype(np.int8))
    s = _swarm(g, "spatial")
    want = _model(oracle_mod, s, g, 40)
    tc = want["task_counts"]
    assert tc[:, 0].sum() >= 100 and tc[:, 1].sum() >= 20 and tc[:, 2].sum() >= 20 and want["guard"] == 0
    r = _run(s, g, 40)
    _assert_equal(_state(s), want, ALL)
    _assert_tasks(_task_state(s), want)
    np.testing.assert_array_equal(r["task_counts"], tc)
    np.testing.assert_array_equal(r["counts"], want["counts"])
    assert r["guard"] == 0 and r["singular"] == want["singular"]


# 6. the all-or-nothing refusal
@pytest.mark.gpu
def test_gpu_refused_tick_leaves_every_task_array_as_it_was():
    """test_update_loop_radio's too-dense swarm (a window work limit is only reached by a million agents in one
    cell), with a board, claims and conflicts in flight, statuses and table entries to keep."""
    import torch
    from swarm_amd import _lib
    from swarm_amd.swarm import Swarm
    n = 1_200_000
    rng = np.random.default_rng(2)
    x, y = 3.0 + rng.uniform(0, 1e-3, n), -2.0 + rng.uniform(0, 1e-3, n)
    s = Swarm(np.arange(n, dtype=np.int32), x, y, layout="input", device="cuda")
    s.protocol_reset(last_hb=np.full(n, -2.95))
    s.set_tasks([3.0, 4.0, 50.0], [-2.0, -2.0, 0.0])
    b = s.tasks
    b["status_lo"][::2] = 1
    b["status_hi"][::3] = 5
    b["claim_out"][::5] = 2
    b["conflict_out"][::7] = 1
    b["tab_winner"][::4, 0] = 7
    b["tab_util"][::4, 0] = 33.0
    keep = dict(pos=s.pos, state=s.state, leader=s.leader, **s.fsm,
                **{k: v for k, v in b.items() if isinstance(v, torch.Tensor)})
    before = {k: v.clone() for k, v in keep.items()}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with pytest.raises(_lib.SwarmError) as e:
        s.update_loop_tasks(3, 1.0, 1.0)
    torch.cuda.synchronize()
    assert time.perf_counter() - t0 < 20.0
    assert e.value.code == _lib.ERR_RANGE and "too dense" in str(e.value) and "tick 1" in str(e.value)
    assert s.last_refused_tick == 1 and s.fsm_tick == 0
    for k, v in keep.items():
        assert torch.equal(v, before[k]), k


# 7. nothing to do: the radio loop, bit for bit
@pytest.mark.gpu
@pytest.mark.parametrize("board", ["out of reach", "T = 0"])
def test_gpu_idle_board_equals_the_radio_loop_on_a_twin_swarm(board):
    import torch
    g = load_golden("loop_tasks_n200")
    a, b = _swarm(g, "spatial", board=False), _swarm(g, "spatial", board=False)
    if board == "T = 0":
        a.set_tasks([], [])
    else:
        a.set_tasks(np.full(24, 1.0e4), np.linspace(-1.0e4, 1.0e4, 24), g["task_req"])
    ra, rb = _run(a, g, 120), _run_radio(b, g, 120)
    for t in ("pos", "pos_prev", "vel", "target", "has_target", "state", "leader"):
        assert torch.equal(getattr(a, t), getattr(b, t)), t
    for k in a.fsm:
        assert torch.equal(a.fsm[k], b.fsm[k]), k
    np.testing.assert_array_equal(ra["counts"], rb["counts"])
    assert ra["singular"] == rb["singular"] and ra["task_counts"].sum() == 0 and ra["guard"] == 0
    assert not a.task_status().any() and not a.tasks["claim_out"].any()


# 8. the bridge
@pytest.mark.gpu
def test_gpu_write_back_tasks_fills_the_agent_objects():
    import types
    g = _hand([(0, 0), (0, 2)], [1, 9], lead=(1,), caps=[1, 0], tasks=[(1, 0, 0), (500, 0, -1)])
    s = _swarm(g, "spatial", board=False)
    agents = [types.SimpleNamespace(agent_id=int(i), tasks={10: {"status": "OPEN", "pos": (1.0, 0.0),
                                                                "required_cap": "extinguisher"},
                                                           20: {"status": "OPEN", "pos": (500.0, 0.0)}},
                                    task_claims={}) for i in g["ids"]]
    s.set_tasks(s.tasks_from_dict(agents[0].tasks))
    np.testing.assert_array_equal(s.task_ids, [10, 20])
    _run(s, g, 3)
    s.write_back_tasks(agents)
    assert [a.tasks[10]["status"] for a in agents] == ["ASSIGNED", "OPEN"]
    assert [a.tasks[20]["status"] for a in agents] == ["OPEN", "OPEN"]
    assert agents[0].task_claims == {} and agents[1].task_claims == {10: {"winner": 1, "utility": 50.0}}
