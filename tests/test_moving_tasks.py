"""Moving tasks (contract U1-M): swarm_board_create_moving / swarm_update_loop_board_moving,
Swarm.set_task_board(..., velocities=) + Swarm.update_loop_board.

Tick t of a call runs U1-B (U1-L when lossy) with the board at cur = Q_{t-1}; the claims of tick t-1 are heard with
lag = Q_{t-2}; then lag <- cur and cur <- fl(cur + fl(v * dt)).  The yardsticks are the unchanged CPU models
(loop_tasks_model, loop_lossy_model), driven one tick at a time through start= with that tick's task_x / task_y:
they carry the utility in the message and owe nothing to the recomputation.  tests/golden/
loop_moving_board_n200.npz comes from real SwarmAgent objects whose tasks[k]['pos'] is moved before every tick
(tools/gen_golden_moving_tasks.py).  The GPU must equal the model with its own x*x squares bit for bit over its
storage order -- tab_util included, which a build without the lag list misses.
"""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT, load_golden
import loop_board_model as lbm
import loop_lossy_model
import loop_tasks_model
from loop_model import OUT_KEYS
from test_update_loop_board import ALL, ROWS, _assert_rows, _rows, _storage_case, _to_input
from test_update_loop_sensed import EXACT, _assert_equal, _state
from test_update_loop_tasks import _hand, _kw, _swarm

CSRC = os.path.join(PKG, "csrc")
OPEN, TENTATIVE, LOCKED, ASSIGNED = 0, 1, 2, 3
FIXTURE = "loop_moving_board_n200"


def _advance(q, v, dt, k=1):
    """Q after k advances: fl(q + fl(v * dt)) per coordinate (numpy float64: two roundings)."""
    q = np.array(q, np.float64)
    for _ in range(k):
        q = q + v * dt
    return q


def _drive(oracle_mod, q, Q0, V, ticks, *, first=0, loss=None, loss_seed=0, use_pow=False, recompute=False,
           start=None):
    """The model over case q (the order of its arrays), `first` ticks in one piece (before the hand-out), then
    `ticks` ticks one at a time with the board at Q_0, Q_1, ... (start: a result of this function: goes on from its
    positions).  recompute: every claim's payload recomputed from the advanced positions before it is heard -- what
    a board without a lag list computes.  -> the last model result plus the concatenated counts, per-tick peaks,
    the leader-handled and sent claims and the board positions (cur, lag)."""
    dt = float(q["dt"])
    run = (lambda g, k, st: loop_tasks_model.run(oracle_mod, g, k, start=st, use_pow=use_pow)) if loss is None else \
        (lambda g, k, st: loop_lossy_model.run(oracle_mod, g, k, start=st, use_pow=use_pow, loss=loss,
                                               loss_seed=loss_seed))
    acc = dict(counts=[], task_counts=[], link_counts=[], peaks=[], singular=0, guard=0) if start is None else \
        {k: (list(v) if isinstance(v, list) else v) for k, v in start["acc"].items()}
    o = None if start is None else start["o"]
    cur = np.array(Q0, np.float64) if start is None else start["cur"]
    lag = cur.copy() if start is None else start["lag"]

    def note(o):
        acc["counts"].append(o["counts"])
        acc["task_counts"].append(o["task_counts"])
        if loss is not None:
            acc["link_counts"].append(o["link_counts"])
        acc["singular"] += o["singular"]
        acc["guard"] += o["guard"]
    if first:
        o = run(q, first, o)
        note(o)
    g = dict(q)
    for _ in range(ticks):
        g["task_x"], g["task_y"] = cur[:, 0].copy(), cur[:, 1].copy()
        o = run(g, 1, o)
        note(o)
        acc["peaks"].append(lbm.peak_slots(o))
        lag, cur = cur, cur + V * dt
        if recompute:
            for j, msgs in enumerate(o["tasks"]["claims"]):
                o["tasks"]["claims"][j] = [
                    (k, np.float32(loop_tasks_model.utility(float(o["px"][j]), float(o["py"][j]), q["caps"][j],
                                                            float(cur[k, 0]), float(cur[k, 1]), int(q["task_req"][k]),
                                                            use_pow))) for k, _ in msgs]
    return dict(o=o, acc=acc, cur=cur, lag=lag)


def _result(d, perm, Ks, Kt):
    """_drive's result in input order, as test_update_loop_board's _model returns one."""
    out = _to_input(d["o"], perm, Ks, Kt)
    a = d["acc"]
    out.update(counts=np.concatenate(a["counts"]), task_counts=np.concatenate(a["task_counts"]),
               singular=a["singular"], guard=a["guard"], peaks=np.asarray(a["peaks"]), cur=d["cur"], lag=d["lag"])
    if a["link_counts"]:
        out["link_counts"] = np.concatenate(a["link_counts"])
    return out


def _case48():
    """The issue's case: loop_tasks_n200's agents, 48 tasks over the arena widened by 5, drifting at up to 3
    units/s, there from the first tick."""
    g = dict(load_golden("loop_tasks_n200"))
    rng = np.random.default_rng(5)
    T = 48
    pos = np.stack([rng.uniform(g["x"].min() - 5.0, g["x"].max() + 5.0, T),
                    rng.uniform(g["y"].min() - 5.0, g["y"].max() + 5.0, T)], 1)
    vel = rng.uniform(-3.0, 3.0, (T, 2))
    g.update(task_x=pos[:, 0].copy(), task_y=pos[:, 1].copy(), task_req=np.full(T, -1, np.int8),
             task_tick=np.int64(1), ticks=np.int64(120))
    return g, pos, vel


# ----------------------------------------------------------------------------- CPU

def test_exports_and_struct_sizes():
    from swarm_amd import _lib
    lib = _lib.load()
    for name in ("swarm_board_create_moving", "swarm_board_set_velocities", "swarm_board_positions",
                 "swarm_board_refresh", "swarm_board_call_box", "swarm_update_loop_board_moving"):
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert ctypes.sizeof(_lib.BoardState) == 64 and ctypes.sizeof(_lib.BoardDesc) == 56
    assert ctypes.sizeof(_lib.BoardOverflow) == 16
    assert lib.swarm_update_loop_board_moving.argtypes == lib.swarm_update_loop_board.argtypes


def test_entry_points_refuse_bad_arguments_without_a_device():
    from swarm_amd import _lib
    from swarm_amd.swarm import Swarm
    lib = _lib.load()
    fake = ctypes.c_void_p(8)  # never dereferenced: the arguments below are refused first
    out = ctypes.c_void_p()
    for T in (-1, (1 << 24) + 1):
        assert lib.swarm_board_create_moving(fake, T, fake, fake, fake, ctypes.byref(out), None, None) == _lib.ERR_ARG
        assert b"[0, 2^24]" in lib.swarm_last_error() and not out.value
    assert lib.swarm_board_create_moving(None, 3, fake, fake, fake, ctypes.byref(out), None, None) == _lib.ERR_ARG
    assert lib.swarm_board_create_moving(fake, 3, fake, fake, fake, None, None, None) == _lib.ERR_ARG
    assert lib.swarm_board_create_moving(fake, 3, None, fake, fake, ctypes.byref(out), None, None) == _lib.ERR_ARG
    assert b"NULL task array" in lib.swarm_last_error()
    assert lib.swarm_board_set_velocities(None, fake, fake, None) == _lib.ERR_ARG
    assert lib.swarm_board_set_velocities(fake, None, fake, None) == _lib.ERR_ARG
    assert lib.swarm_board_positions(None, ctypes.byref(out), ctypes.byref(out)) == _lib.ERR_ARG
    assert lib.swarm_board_positions(fake, None, ctypes.byref(out)) == _lib.ERR_ARG
    assert lib.swarm_board_refresh(None, fake, None, None) == _lib.ERR_ARG
    assert lib.swarm_board_refresh(fake, None, None, None) == _lib.ERR_ARG
    assert lib.swarm_board_call_box(fake, None, 0.1, 3, fake, None) == _lib.ERR_ARG
    good = _lib.BoardState(8, 8)
    args = (4, None, None, None, None, None, 0, 1, 0.1, 3.0, 0.2, ctypes.c_uint64(0), None, 0, None, None, None, 0, None,
            2.5, 2.5, 5.0, None, 0, None, None, None)
    loop = lambda ctx, board, state: lib.swarm_update_loop_board_moving(  # noqa: E731
        ctx, *args, board, state, None, None, None, None, None, None)
    assert loop(None, fake, ctypes.byref(good)) == _lib.ERR_ARG and b"ctx is NULL" in lib.swarm_last_error()
    assert loop(fake, None, ctypes.byref(good)) == _lib.ERR_ARG and b"board is NULL" in lib.swarm_last_error()
    assert loop(fake, fake, None) == _lib.ERR_ARG and b"state is NULL" in lib.swarm_last_error()
    # the Python layer: velocities of the wrong shape, or not finite, before the device is touched
    s = Swarm.__new__(Swarm)
    s.n, s.device = 4, "cpu"
    with pytest.raises(ValueError, match=r"expected shape \(2, 2\)"):
        s.set_task_board([1.0, 2.0], [2.0, 3.0], velocities=[1.0, 2.0])
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="velocities must be finite"):
            s.set_task_board([1.0, 2.0], [2.0, 3.0], velocities=[[0.0, 1.0], [bad, 0.0]])
    s.board = dict(moving=False, T=2)
    with pytest.raises(RuntimeError, match="does not move"):
        s.set_board_velocities(np.zeros((2, 2)))


@pytest.fixture(scope="module")
def motion_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("task_motion") / "task_motion")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                    "-o", exe, os.path.join(ROOT, "tests", "task_motion", "task_motion_main.cpp")], check=True,
                   capture_output=True, text=True)
    return exe


@pytest.fixture(scope="module")
def motion_report(motion_exe):
    p = subprocess.run([motion_exe], capture_output=True, text=True, timeout=120)
    return p.returncode, p.stdout


def test_task_motion_program_passes(motion_report):
    rc, out = motion_report
    assert rc == 0 and out.rstrip().endswith("0 failed") and "FAIL" not in out, out


@pytest.mark.parametrize("case,ticks", [
    ("random_300", 120), ("random_5000", 40), ("t1", 30), ("t0", 10), ("velocity_null", 30), ("velocity_zero", 30),
    ("negative_dt", 20), ("ticks_1", 1), ("ticks_0", 0), ("near_1e9_ticks_1", 1), ("near_1e9_ticks_1000", 1000),
    ("near_1e9_ticks_1e6", 1000000), ("opposite_signs", 500), ("opposite_signs_ticks_1e6", 1000000),
    ("all_leave_the_entry_box", 50), ("scales_0", None), ("scales_39", None)])
def test_every_position_of_a_call_stays_inside_its_span_the_box_and_the_grid(motion_report, case, ticks):
    """The program iterates the advance and checks containment at every tick, and the advance's bits."""
    line = [ln for ln in motion_report[1].splitlines() if ln.startswith(f"ok {case} T=")]
    assert len(line) == 1, motion_report[1]
    if ticks is not None:
        assert f" ticks={ticks} " in line[0]
    if case == "all_leave_the_entry_box":
        assert line[0].endswith("left_entry_box=64")


@pytest.mark.parametrize("case,status", [("nan_velocity", 1), ("inf_velocity", 1), ("nan_position", 1),
                                         ("extent_overflows", 2), ("span_overflows", 2),
                                         ("static_extent_overflows", 2)])
def test_task_motion_refuses_and_writes_nothing(motion_report, case, status):
    assert f"ok {case} refused status={status}\n" in motion_report[1], motion_report[1]


def test_task_motion_header_has_no_hip_includes():
    with open(os.path.join(CSRC, "task_motion.h")) as f:
        inc = [ln.split()[1] for ln in f if ln.startswith("#include")]
    assert inc == ["<cmath>", "<cstdint>", '"task_grid.h"']


_pow = {}


def test_model_with_pow_driven_per_tick_equals_the_fixture(oracle_mod):
    g = load_golden(FIXTURE)
    first, ticks = int(g["task_tick"]) - 1, int(g["ticks"])
    Q0, V = np.stack([g["task_x"], g["task_y"]], 1), np.stack([g["task_vx"], g["task_vy"]], 1)
    d = _drive(oracle_mod, g, Q0, V, ticks - first, first=first, use_pow=True)
    o, acc = d["o"], d["acc"]
    assert g["status_out"].shape == (200, 300) and ticks - first == 216
    for k in OUT_KEYS:  # the thirteen arrays
        np.testing.assert_array_equal(o[k], g[k + "_out"], err_msg=k)
    for k in ("status", "tab_winner"):
        np.testing.assert_array_equal(o[k], g[k + "_out"], err_msg=k)
    np.testing.assert_array_equal(o["tab_util"].view(np.uint32), g["tab_util_out"].view(np.uint32))
    np.testing.assert_array_equal(np.concatenate(acc["counts"]), g["counts"])
    np.testing.assert_array_equal(np.concatenate(acc["task_counts"]), g["task_counts"])
    from test_update_loop_board import _fixture_rows
    want, got = _fixture_rows(g, 300, 300), lbm.out_rows(o, 300, 300)
    np.testing.assert_array_equal(got[0], want["claim_out"])
    np.testing.assert_array_equal(got[1], want["conflict_out"])
    np.testing.assert_array_equal(d["cur"][:, 0], g["task_x_end"])
    np.testing.assert_array_equal(d["cur"][:, 1], g["task_y_end"])
    tc = g["task_counts"]
    assert acc["singular"] == 0 and acc["guard"] == 0 and tc[:, 1].sum() >= 100 and tc[:, 2].sum() >= 100
    # the tasks do move: the frozen board of the hand-out computes something else
    frozen = loop_tasks_model.run(oracle_mod, g, use_pow=True)
    assert (frozen["status"] != g["status_out"]).sum() > 100
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", FIXTURE + ".npz")) < 790802


def test_recomputing_a_claims_payload_from_the_advanced_positions_changes_the_tables(oracle_mod):
    """Why the board keeps a lag list: hear_claims_board recomputes a claim's utility from the task's position,
    and at the tick it is heard the board has advanced once since the claim was sent."""
    g, Q0, V = _case48()
    exact = _drive(oracle_mod, g, Q0, V, 120)
    wrong = _drive(oracle_mod, g, Q0, V, 120, recompute=True)
    tc = np.concatenate(exact["acc"]["task_counts"])
    eu, wu = exact["o"]["tab_util"].view(np.uint32), wrong["o"]["tab_util"].view(np.uint32)
    peaks = np.asarray(exact["acc"]["peaks"])
    print("claims sent", tc[:, 0].sum(), "leader-handled", tc[:, 1].sum(), "tab_util entries changed",
          int((eu != wu).sum()), "peak rows", peaks.max(0))
    assert tc[:, 1].sum() >= 100
    assert (eu != wu).sum() > 0
    np.testing.assert_array_equal(exact["cur"], _advance(Q0, V, 0.1, 120))
    np.testing.assert_array_equal(exact["lag"], _advance(Q0, V, 0.1, 119))


# ----------------------------------------------------------------------------- GPU

def _mboard(s, pos, vel, req=None, Ks=64, Kt=32):
    return s.set_task_board(pos[:, 0], pos[:, 1], req, status_slots=Ks, table_slots=Kt, velocities=vel)


def _run(s, g, ticks, **kw):
    return s.update_loop_board(ticks, float(g["radio_radius"]), float(g["sense_radius"]), **_kw(g), **kw)


def _read_lists(s):
    from swarm_amd import _lib
    lib, h = _lib.lib(), s.board["handle"]
    d = _lib.BoardDesc()
    _lib.check(lib.swarm_board_info(h, ctypes.byref(d)))
    off, idx = np.zeros(d.ncx * d.ncy + 1, np.uint32), np.zeros(max(d.T, 1), np.int32)
    _lib.check(lib.swarm_board_read(h, off.ctypes.data_as(ctypes.c_void_p), idx.ctypes.data_as(ctypes.c_void_p)))
    return {k: getattr(d, k) for k, _ in _lib.BoardDesc._fields_}, off, idx[:d.T]


def _refresh(s):
    from swarm_amd import _lib
    d = _lib.BoardDesc()
    _lib.check(_lib.lib().swarm_board_refresh(_lib.ctx(), s.board["handle"], ctypes.byref(d), _lib.stream()))
    return {k: getattr(d, k) for k, _ in _lib.BoardDesc._fields_}


def _lists_case(case):
    rng = np.random.default_rng(11)
    if isinstance(case, int):
        return np.stack([rng.uniform(-40.0, 90.0, case), rng.uniform(5.0, 60.0, case)], 1).reshape(case, 2)
    if case == "one cell":
        return np.stack([rng.uniform(3.0, 4.0, 500), rng.uniform(-1.0, 0.0, 500)], 1)
    if case == "cell edge":  # the grid's corner is the lowest position: tasks exactly k cells from it, +- an ulp
        c = 5.0 * (1.0 + 1e-9)
        e = np.array([c * k for k in range(1, 9)])
        xs = np.concatenate([[0.0, 60.0], e, np.nextafter(e, 0.0), np.nextafter(e, 100.0)])
        return np.stack([xs, xs[::-1].copy()], 1)
    assert case == "shifted 1e9"
    return np.stack([1e9 + rng.uniform(0.0, 300.0, 400), -1e9 + rng.uniform(0.0, 300.0, 400)], 1)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [0, 1, 63, 64, 65, 257, 20_000, "one cell", "cell edge", "shifted 1e9"])
def test_gpu_refresh_builds_the_lists_of_build_task_cells(case, motion_exe, tmp_path):
    """The device builder against the host builder (a static board's lists) on the same list -- at creation, and
    after the tasks have moved; and the device's span box against the header's function."""
    from swarm_amd import _lib
    pos = _lists_case(case)
    T = len(pos)
    rng = np.random.default_rng(12)
    vel = rng.uniform(-30.0, 30.0, (T, 2))
    req = rng.integers(-1, 3, T).astype(np.int8)
    g = _hand([(-5.0e5, 7.0e5)], [1], tasks=[(0, 0, -1)])  # (nobody within reach of a task)
    a, b = _swarm(g, "input", board=False), _swarm(g, "input", board=False)
    _mboard(a, pos, vel, req, 1, 1)
    for step in (0, 3):
        if step:
            _run(a, g, step)
        cur, lag = a.board_positions()
        np.testing.assert_array_equal(cur, _advance(pos, vel, 0.1, step))
        np.testing.assert_array_equal(lag, _advance(pos, vel, 0.1, max(step - 1, 0)))
        b.set_task_board(cur[:, 0], cur[:, 1], req, status_slots=1, table_slots=1)
        want = _read_lists(b)
        info = _refresh(a)
        got = _read_lists(a)
        assert info == got[0] == want[0]
        np.testing.assert_array_equal(got[1], want[1])
        np.testing.assert_array_equal(got[2], want[2])
        if case == "one cell" and step == 0:
            assert info["ncx"] == info["ncy"] == 1 and info["longest"] == T
    # the box of the call's spans: the device's reduction against task_span_box, bit for bit
    for ticks, dt in ((1, 0.1), (200, 0.1), (1_000_000, 0.01)):
        cur = a.board_positions()[0]
        box = np.zeros(4)
        _lib.check(_lib.lib().swarm_board_call_box(_lib.ctx(), a.board["handle"], dt, ticks,
                                                   box.ctypes.data_as(ctypes.c_void_p), _lib.stream()))
        path = tmp_path / "box.bin"
        path.write_bytes(struct.pack("<qqd", T, ticks, dt) + cur.tobytes() + vel.tobytes())
        p = subprocess.run([motion_exe, "box", str(path)], capture_output=True, text=True, check=True)
        want = np.array([float.fromhex(w) for w in p.stdout.split()])
        np.testing.assert_array_equal(box, want)
        if T:
            end = _advance(cur, vel, dt, min(ticks, 300))
            assert (np.minimum(cur, end).min(0) >= box[:2]).all() and (np.maximum(cur, end).max(0) <= box[2:]).all()


_models = {}


def _fixture_case():
    g = load_golden(FIXTURE)
    return g, np.stack([g["task_x"], g["task_y"]], 1), np.stack([g["task_vx"], g["task_vy"]], 1)


def _check(s, r, want, cur_lag=True):
    _assert_equal(_state(s), want, ALL)
    _assert_rows(_rows(s), want["rows"])
    np.testing.assert_array_equal(r["counts"], want["counts"])
    np.testing.assert_array_equal(r["task_counts"], want["task_counts"])
    assert r["guard"] == want["guard"] and r["singular"] == want["singular"]
    if cur_lag:
        cur, lag = s.board_positions()
        np.testing.assert_array_equal(cur, want["cur"])
        np.testing.assert_array_equal(lag, want["lag"])


# 1. the fixture and the 48-task case, both layouts, the ideal channel and a lossy one
@pytest.mark.gpu
@pytest.mark.parametrize("loss", [0.0, 0.2])
@pytest.mark.parametrize("layout", ["input", "spatial"])
@pytest.mark.parametrize("name", [FIXTURE, "case48"])
def test_gpu_equals_the_model_driven_per_tick(oracle_mod, name, layout, loss):
    """Every array equals the per-tick model, tab_util included: this test fails without the lag list."""
    g, Q0, V = _fixture_case() if name == FIXTURE else _case48()
    T, first, ticks = len(Q0), int(g["task_tick"]) - 1, int(g["ticks"])
    s = _swarm(g, layout, board=False)
    kw = dict(loss=loss, loss_seed=77) if loss else {}
    r0 = s.update_loop_radio(first, float(g["radio_radius"]), float(g["sense_radius"]), **_kw(g), **kw) if first else None
    _mboard(s, Q0, V, g["task_req"], T, T)
    r1 = _run(s, g, ticks - first, **kw)
    if (name, layout, loss) not in _models:  # once per storage order, left unchanged
        q, perm = _storage_case(s, g)
        d = _drive(oracle_mod, q, Q0, V, ticks - first, first=first, loss=loss or None, loss_seed=77)
        _models[name, layout, loss] = _result(d, perm, T, T)
    want = _models[name, layout, loss]
    r = dict(r1)
    if first:
        r["counts"] = np.concatenate([r0["counts"], r1["counts"]])
        r["task_counts"] = np.concatenate([np.zeros((first, 3), np.int64), r1["task_counts"]])
        r["singular"] = r0["singular"] + r1["singular"]
    _check(s, r, want)
    assert want["task_counts"][:, 1].sum() >= (100 if not loss else 50)
    if loss:
        links = np.concatenate([r0["link_counts"], r1["link_counts"]]) if first else r1["link_counts"]
        np.testing.assert_array_equal(links, want["link_counts"])
    np.testing.assert_array_equal(want["cur"], _advance(Q0, V, 0.1, ticks - first))
    assert s.fsm_tick == ticks and s.last_refused_tick == -1 and s.last_board_overflow is None
    if name == FIXTURE and layout == "input" and not loss:  # real agents, in everything the squares cannot reach
        got = _state(s)
        for k in EXACT:
            np.testing.assert_array_equal(got[k], g[k + "_out"], err_msg=k)
        from test_update_loop_board import _fixture_rows
        _assert_rows(_rows(s), _fixture_rows(g, T, T))
        np.testing.assert_array_equal(r["task_counts"], g["task_counts"])


# 2. zero velocities: every bit of a static-board twin
@pytest.mark.gpu
@pytest.mark.parametrize("vel", ["zeros", "none given to the library"])
def test_gpu_zero_velocities_equal_the_static_board_on_a_twin_swarm(vel):
    import torch
    from swarm_amd import _lib
    g, Q0, V = _case48()
    a, b = _swarm(g, "spatial", board=False), _swarm(g, "spatial", board=False)
    a.set_task_board(Q0[:, 0], Q0[:, 1], g["task_req"], status_slots=32, table_slots=16)
    _mboard(b, Q0, np.zeros_like(V), g["task_req"], 32, 16)
    if vel != "zeros":  # NULL velocities mean all zero
        _lib.check(_lib.lib().swarm_board_set_velocities(_lib.ctx(), b.board["handle"], None, _lib.stream()))
    ra, rb = _run(a, g, 60, loss=0.1, loss_seed=3), _run(b, g, 60, loss=0.1, loss_seed=3)
    assert ra["task_counts"][:, 1].sum() >= 20
    for t in ("pos", "pos_prev", "vel", "target", "has_target", "state", "leader"):
        assert torch.equal(getattr(a, t), getattr(b, t)), t
    for k in a.fsm:
        assert torch.equal(a.fsm[k], b.fsm[k]), k
    for k in ROWS:
        assert torch.equal(a.board[k].view(torch.int32), b.board[k].view(torch.int32)), k
    for k in ("counts", "task_counts", "link_counts"):
        np.testing.assert_array_equal(ra[k], rb[k], err_msg=k)
    assert ra["guard"] == rb["guard"]
    for q in b.board_positions() + a.board_positions():
        np.testing.assert_array_equal(q, Q0)


# 3. chunks
@pytest.mark.gpu
@pytest.mark.parametrize("chunks", [(1,) * 24, (7, 113)])
def test_gpu_chunked_run_is_the_same_run(chunks):
    import torch
    g, Q0, V = _case48()
    a, b = _swarm(g, "spatial", board=False), _swarm(g, "spatial", board=False)
    for s in (a, b):
        _mboard(s, Q0, V, g["task_req"], 32, 16)
    total = sum(chunks)
    ra = _run(a, g, total)
    rb = [_run(b, g, c) for c in chunks]
    assert ra["task_counts"][:, 0].sum() > 0 and ra["task_counts"][:, 1].sum() > 0
    for t in ("pos", "pos_prev", "vel", "target", "has_target", "state", "leader"):
        assert torch.equal(getattr(a, t), getattr(b, t)), t
    for k in a.fsm:
        assert torch.equal(a.fsm[k], b.fsm[k]), k
    for k in ROWS:
        assert torch.equal(a.board[k].view(torch.int32), b.board[k].view(torch.int32)), k
    np.testing.assert_array_equal(ra["task_counts"], np.concatenate([r["task_counts"] for r in rb]))
    np.testing.assert_array_equal(ra["counts"], np.concatenate([r["counts"] for r in rb]))
    for s in (a, b):
        cur, lag = s.board_positions()
        np.testing.assert_array_equal(cur, _advance(Q0, V, 0.1, total))
        np.testing.assert_array_equal(lag, _advance(Q0, V, 0.1, total - 1))


# 4. one task passing one resting agent
@pytest.mark.gpu
def test_gpu_a_task_passing_a_resting_agent_is_claimed_when_it_comes_within_reach():
    from swarm_amd import _lib
    # claimer A (ID 1, bit 0) at the origin, leader R (ID 9, without the capability) at (0, 2); task 0 needs bit 0
    # and passes at y = 0.5 with 0.5 a tick (every sum exact); task 1 rests far away and gives the creation box
    g = _hand([(0, 0), (0, 2)], [1, 9], lead=(1,), caps=[1, 0], tasks=[(-8.0, 0.5, 0), (-8.0, 40.0, -1)])
    Q0 = np.array([[-8.0, 0.5], [-8.0, 40.0]])
    V = np.array([[5.0, 0.0], [0.0, 0.0]])
    Q = [_advance(Q0, V, 0.1, k) for k in range(31)]
    d2 = [float(q[0, 0] * q[0, 0] + q[0, 1] * q[0, 1]) for q in Q]
    U = [100.0 / (1.0 + np.sqrt(v)) for v in d2]
    j = next(k for k in range(31) if d2[k] <= 25.0 and U[k] > 20.0)  # tick j + 1 reads Q_j
    assert j == 9 and not U[j - 1] > 20.0 and np.float32(U[j]) != np.float32(U[j + 1])
    s = _swarm(g, "input", board=False)
    _mboard(s, Q0, V, g["task_req"], 4, 4)
    box = np.zeros(4)
    _lib.check(_lib.lib().swarm_board_call_box(_lib.ctx(), s.board["handle"], 0.1, 30,
                                               box.ctypes.data_as(ctypes.c_void_p), _lib.stream()))
    cell = 5.0 * (1.0 + 1e-9)  # (the call's grid: far below the cell cap)
    assert (np.floor((box[2] - box[0]) / cell) + 1) * (np.floor((box[3] - box[1]) / cell) + 1) <= 4 * 2 + 1024
    cx = [int(np.floor((q[0, 0] - box[0]) / cell)) for q in Q]
    assert cx[30] - cx[0] >= 2  # task-cell edges are crossed mid-call
    info = s.board["info"]  # the creation box is the line x = -8: the task leaves it with its first advance
    assert info["ncx"] == 1 and info["xmin"] == -8.0 and Q[1][0, 0] > -8.0
    r = _run(s, g, j)  # OPEN while out of reach
    assert r["task_counts"].sum() == 0 and all((s.board[k] == (0 if k == "tab_util" else -1)).all() for k in ROWS)
    r = _run(s, g, 1)  # tick j + 1: the exact pre-test and U > 20 hold for the first time
    np.testing.assert_array_equal(r["task_counts"], [[1, 0, 0]])
    np.testing.assert_array_equal(_rows(s)["status"], [[0 << 2 | TENTATIVE, -1, -1, -1], [-1] * 4])
    r = _run(s, g, 30 - j - 1)  # heard one tick later, with the sending tick's utility
    np.testing.assert_array_equal(r["task_counts"][:2], [[0, 1, 1], [0, 0, 0]])
    assert r["task_counts"][2:].sum() == 0 and r["guard"] == 0
    rows = _rows(s)
    np.testing.assert_array_equal(rows["status"], [[0 << 2 | ASSIGNED, -1, -1, -1], [-1] * 4])
    np.testing.assert_array_equal(rows["tab_task"], [[-1] * 4, [0, -1, -1, -1]])
    np.testing.assert_array_equal(rows["tab_winner"], [[-1] * 4, [1, -1, -1, -1]])
    assert rows["tab_util"][1, 0].view(np.uint32) == np.float32(U[j]).view(np.uint32)
    cur, lag = s.board_positions()
    np.testing.assert_array_equal(cur, Q[30])
    np.testing.assert_array_equal(lag, Q[29])
    assert cur[0, 0] == 7.0 and box[0] <= -8.0 and box[2] >= 7.0


# 5. new velocities between calls
@pytest.mark.gpu
def test_gpu_set_board_velocities_between_calls(oracle_mod):
    import torch
    from swarm_amd import _lib
    g, Q0, V = _case48()
    V2 = np.random.default_rng(8).uniform(-3.0, 3.0, V.shape)
    s = _swarm(g, "spatial", board=False)
    _mboard(s, Q0, V, g["task_req"], 48, 48)
    q, perm = _storage_case(s, g)
    ra = _run(s, g, 40)
    before = s.board_positions()
    s.set_board_velocities(V2)
    for a, b in zip(before, s.board_positions()):  # neither list changes
        np.testing.assert_array_equal(a, b)
    with pytest.raises(ValueError, match="finite"):
        s.set_board_velocities(np.full_like(V, np.nan))
    bad = torch.full((48, 2), float("inf"), dtype=torch.float64, device="cuda")
    assert _lib.lib().swarm_board_set_velocities(_lib.ctx(), s.board["handle"], _lib.ptr(bad), _lib.stream()) == \
        _lib.ERR_ARG and "not finite" in _lib.last_error()
    rb = _run(s, g, 40)
    d = _drive(oracle_mod, q, Q0, V, 40)
    d = _drive(oracle_mod, q, None, V2, 40, start=d)
    want = _result(d, perm, 48, 48)
    r = dict(counts=np.concatenate([ra["counts"], rb["counts"]]),
             task_counts=np.concatenate([ra["task_counts"], rb["task_counts"]]), guard=ra["guard"] + rb["guard"],
             singular=ra["singular"] + rb["singular"])
    _check(s, r, want)
    np.testing.assert_array_equal(want["cur"], _advance(_advance(Q0, V, 0.1, 40), V2, 0.1, 40))


# 6. a status overflow is a refusal that restores both lists
@pytest.mark.gpu
def test_gpu_status_overflow_restores_both_lists_and_grow_board_repeats_the_call(oracle_mod):
    import torch
    from swarm_amd import _lib
    g, Q0, V = _case48()
    s = _swarm(g, "spatial", board=False)
    q, perm = _storage_case(s, g)
    d5 = _drive(oracle_mod, q, Q0, V, 5)
    d = _drive(oracle_mod, q, None, V, 115, start=d5)
    want = _result(d, perm, 48, 48)
    peaks = want["peaks"]
    Ks = int(peaks[-1, 0]) - 2
    over = np.flatnonzero(peaks[:, 0] > Ks)
    tick = int(over[0]) + 1  # the first tick at whose end the exact run holds more than the rows do
    assert Ks >= 4 and tick > 6 and (peaks[:, 1] <= 48).all()
    _mboard(s, Q0, V, g["task_req"], Ks, 48)
    r5 = _run(s, g, 5)
    b = s.board
    s._motion_state()
    keep = dict(pos=s.pos, pos_prev=s.pos_prev, vel=s.vel, state=s.state, leader=s.leader, **s.fsm,
                **{k: b[k] for k in ROWS})
    before = {k: v.clone() for k, v in keep.items()}
    entry = s.board_positions()
    np.testing.assert_array_equal(entry[0], _advance(Q0, V, 0.1, 5))
    np.testing.assert_array_equal(entry[1], _advance(Q0, V, 0.1, 4))
    with pytest.raises(_lib.SwarmError) as e:
        _run(s, g, 115)
    assert e.value.code == _lib.ERR_RANGE and f"status slots at tick {tick} " in str(e.value)
    assert s.last_refused_tick == tick and s.fsm_tick == 5 and s.last_board_overflow[0] == "status"
    for k, v in keep.items():
        assert torch.equal(v, before[k]), k
    for a, w in zip(s.board_positions(), entry):  # both lists at their entry bytes
        np.testing.assert_array_equal(a, w)
    s.grow_board(status_slots=48)
    r = _run(s, g, 115)
    r = dict(counts=np.concatenate([r5["counts"], r["counts"]]),
             task_counts=np.concatenate([r5["task_counts"], r["task_counts"]]), guard=r5["guard"] + r["guard"],
             singular=r5["singular"] + r["singular"])
    _check(s, r, want)
    assert s.last_refused_tick == -1 and s.last_board_overflow is None


# 7. the static entry point refuses a moving board (and the moving one a static board)
@pytest.mark.gpu
def test_gpu_the_static_entry_point_refuses_a_moving_board_and_writes_nothing():
    import torch
    from swarm_amd import _lib
    g, Q0, V = _case48()
    s = _swarm(g, "spatial", board=False)
    _mboard(s, Q0, V, g["task_req"], 16, 16)
    s._motion_state()
    keep = dict(pos=s.pos, vel=s.vel, state=s.state, leader=s.leader, **s.fsm, **{k: s.board[k] for k in ROWS})
    before = {k: v.clone() for k, v in keep.items()}
    for moving, text in ((False, "a moving board needs swarm_update_loop_board_moving"), (True, "does not move")):
        if moving:
            s.set_task_board(Q0[:, 0], Q0[:, 1], g["task_req"], status_slots=16, table_slots=16)
        s.board["moving"] = moving  # the wrong entry point for the handle
        with pytest.raises(_lib.SwarmError) as e:
            _run(s, g, 3)
        assert e.value.code == _lib.ERR_ARG and text in str(e.value)
        assert s.fsm_tick == 0 and s.last_refused_tick == -1
        for k, v in keep.items():
            if k not in ROWS or not moving:
                assert torch.equal(v, before[k]), k
        if not moving:
            for a in s.board_positions():
                np.testing.assert_array_equal(a, Q0)


# 8. a resort in the middle of a run
@pytest.mark.gpu
def test_gpu_a_run_with_a_resort_equals_the_run_rebuilt_from_its_input_order_state():
    from test_resort import _assert_same_swarm, _board_case, _fresh_twin
    g = _board_case(5001, 23, ticks=60, kills=(10, 50), T=200)
    Q0 = np.stack([g["task_x"], g["task_y"]], 1)
    V = np.random.default_rng(9).uniform(-3.0, 3.0, Q0.shape)
    a, b = _swarm(g, "spatial", board=False), _swarm(g, "spatial", board=False)
    for s in (a, b):
        _mboard(s, Q0, V, g["task_req"], 64, 32)
    run = lambda s, k: s.update_loop_board(k, 2.5, 2.5, loss=0.1, loss_seed=5, **_kw(g))  # noqa: E731
    ra, rb = run(a, 30), run(b, 30)
    np.testing.assert_array_equal(ra["task_counts"], rb["task_counts"])
    a.resort()
    assert a.last_resort_moved > 0
    c = _fresh_twin(b)  # (it shares b's board handle: b is not run again)
    _assert_same_swarm(a, c)
    ra, rc = run(a, 30), run(c, 30)
    for k in ("counts", "task_counts", "link_counts"):
        np.testing.assert_array_equal(ra[k], rc[k], err_msg=k)
    assert ra["task_counts"][:, 0].sum() > 0 and ra["task_counts"][:, 1].sum() > 0
    _assert_same_swarm(a, c)
    for x, y in zip(a.board_positions(), c.board_positions()):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(a.board_positions()[0], _advance(Q0, V, 0.1, 60))


# 9. swarm sizes around the workgroup
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_gpu_swarm_sizes_around_a_workgroup_equal_the_model(oracle_mod, n):
    rng = np.random.default_rng(n)
    side = max(np.sqrt(n * np.pi * 2.5 ** 2 / 12.0), 3.0)
    lead = tuple(range(0, n, 9))
    g = _hand(np.stack([rng.uniform(0, side, n), rng.uniform(0, side, n)], 1), rng.permutation(n) + 1, lead=lead,
              caps=rng.integers(0, 8, n))
    T = 40
    Q0 = np.stack([rng.uniform(-4.0, side + 4.0, T), rng.uniform(-4.0, side + 4.0, T)], 1)
    V = rng.uniform(-3.0, 3.0, (T, 2))
    g.update(task_x=Q0[:, 0].copy(), task_y=Q0[:, 1].copy(), task_req=rng.integers(-1, 3, T).astype(np.int8),
             ticks=np.int64(30))
    s = _swarm(g, "spatial", board=False)
    _mboard(s, Q0, V, g["task_req"], T, T)
    q, perm = _storage_case(s, g)
    want = _result(_drive(oracle_mod, q, Q0, V, 30), perm, T, T)
    r = _run(s, g, 30)
    _check(s, r, want)
    assert want["task_counts"][:, 0].sum() > 0 and (n == 1 or want["task_counts"][:, 1].sum() > 0)
