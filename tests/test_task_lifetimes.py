"""Task lifetimes (contract U1-A): swarm_board_set_lifetimes / swarm_board_lifetimes,
Swarm.set_task_board(..., open_tick=, close_tick=), set_board_lifetimes, board_lifetimes, board_present.

Task k is present at tick t iff open[k] <= t < close[k].  Only present tasks are offered, a conflict about an
absent task writes nothing, a claim about one is arbitrated as ever, and at a retiring tick the status entries of
absent tasks leave their rows.  The yardstick is tests/loop_lifetimes_model.py, a thin driver over the unchanged
CPU models; tests/golden/loop_lifetime_board_n200.npz comes from real SwarmAgent objects whose `tasks` dicts are
filled and emptied before every tick (tools/gen_golden_task_lifetimes.py).  The GPU must equal the model with its
own x*x squares bit for bit over its storage order.
"""
import ctypes
import os
import subprocess
import types

import numpy as np
import pytest

from conftest import PKG, ROOT, load_golden
import board_census_model as bcm
import loop_board_model as lbm
import loop_lifetimes_model as llm
from loop_model import OUT_KEYS
from test_moving_tasks import _advance, _case48, _check, _drive, _mboard, _result, _run
from test_update_loop_board import ROWS, _assert_rows, _fixture_rows, _rows, _storage_case
from test_update_loop_sensed import EXACT, _state
from test_update_loop_tasks import _hand, _kw, _swarm

CSRC = os.path.join(PKG, "csrc")
OPEN, TENTATIVE, LOCKED, ASSIGNED = 0, 1, 2, 3
FIXTURE = "loop_lifetime_board_n200"
FOREVER = llm.FOREVER


def _windows(T, seed, last=80, first=1):
    """Random windows over a run that starts at tick 1: some tasks there from the start, some never closing."""
    rng = np.random.default_rng(seed)
    lo = rng.integers(first, last, T).astype(np.int64)
    lo[rng.uniform(size=T) < 0.3] = 0
    hi = lo + rng.integers(5, 50, T)
    hi[rng.uniform(size=T) < 0.2] = FOREVER
    return lo, hi


def _hand3():
    """Claimer A (ID 1, bit 0) at the origin, leader R (ID 9, without the capability) at (0, 2); three tasks that
    need bit 0, each 1.0 from A (U = 50): task 0 closes at tick 2, task 1 never, task 2 opens at tick 4."""
    g = _hand([(0, 0), (0, 2)], [1, 9], lead=(1,), caps=[1, 0], tasks=[(1, 0, 0), (0, 1, 0), (-1, 0, 0)])
    Q0 = np.array([[1.0, 0.0], [0.0, 1.0], [-1.0, 0.0]])
    return g, Q0, np.array([0, 0, 4], np.int64), np.array([2, FOREVER, FOREVER], np.int64)


# ----------------------------------------------------------------------------- CPU

def test_exports_and_struct_sizes():
    from swarm_amd import _lib
    lib = _lib.load()
    for name in ("swarm_board_set_lifetimes", "swarm_board_lifetimes"):
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert ctypes.sizeof(_lib.BoardState) == 64 and ctypes.sizeof(_lib.BoardDesc) == 56
    assert ctypes.sizeof(_lib.BoardOverflow) == 16
    assert len(lib.swarm_board_set_lifetimes.argtypes) == 5 and len(lib.swarm_board_lifetimes.argtypes) == 3
    with open(os.path.join(ROOT, "include", "swarm.h")) as f:
        text = f.read()
    assert "int swarm_board_set_lifetimes(swarm_ctx *ctx, swarm_board *board, const int64_t *open_tick," in text
    assert "int swarm_board_lifetimes(const swarm_board *board, const int64_t **open_tick," in text


def test_entry_points_refuse_bad_arguments_without_a_device():
    from swarm_amd import _lib
    from swarm_amd.swarm import Swarm
    lib = _lib.load()
    fake = ctypes.c_void_p(8)  # never dereferenced: the arguments below are refused first
    out = ctypes.c_void_p()
    assert lib.swarm_board_set_lifetimes(None, fake, fake, fake, None) == _lib.ERR_ARG
    assert b"ctx or board is NULL" in lib.swarm_last_error()
    assert lib.swarm_board_set_lifetimes(fake, None, fake, fake, None) == _lib.ERR_ARG
    assert lib.swarm_board_set_lifetimes(fake, fake, fake, None, None) == _lib.ERR_ARG
    assert b"both arrays, or both NULL" in lib.swarm_last_error()
    assert lib.swarm_board_set_lifetimes(fake, fake, None, fake, None) == _lib.ERR_ARG
    assert lib.swarm_board_lifetimes(None, ctypes.byref(out), ctypes.byref(out)) == _lib.ERR_ARG
    assert lib.swarm_board_lifetimes(fake, None, ctypes.byref(out)) == _lib.ERR_ARG
    assert lib.swarm_board_lifetimes(fake, ctypes.byref(out), None) == _lib.ERR_ARG and not out.value
    # the Python layer, before the device is touched
    s = Swarm.__new__(Swarm)
    s.n, s.device = 4, "cpu"
    xy = ([1.0, 2.0], [2.0, 3.0])
    with pytest.raises(ValueError, match="task 1 opens after it closes"):
        s.set_task_board(*xy, open_tick=[0, 5], close_tick=[3, 4])
    with pytest.raises(ValueError, match="must not be negative"):
        s.set_task_board(*xy, open_tick=[0, -1])
    with pytest.raises(ValueError, match="must not be negative"):
        s.set_task_board(*xy, close_tick=-3)
    with pytest.raises(ValueError, match=r"open_tick: expected 2 ticks or a scalar, got shape \(3,\)"):
        s.set_task_board(*xy, open_tick=[0, 1, 2])
    with pytest.raises(ValueError, match="integer ticks"):
        s.set_task_board(*xy, close_tick=[1.5, 2.0])
    with pytest.raises(ValueError, match="signed 64-bit"):
        s.set_task_board(*xy, close_tick=np.array([2 ** 63, 5], np.uint64))
    with pytest.raises(RuntimeError, match="no task board"):
        s.set_board_lifetimes(0, 5)
    s.board = dict(moving=False, T=2)
    with pytest.raises(RuntimeError, match="does not move"):
        s.set_board_lifetimes(0, 5)
    s.board = dict(moving=True, T=2)
    with pytest.raises(ValueError, match="opens after it closes"):
        s.set_board_lifetimes(7, [9, 6])
    # board_present: the windows' edges; the default tick is the next one to run
    s.board = dict(moving=True, T=3, life=(np.array([0, 5, 7]), np.array([5, 7, FOREVER])))
    s.fsm_tick = 4
    np.testing.assert_array_equal(s.board_present(), [False, True, False])
    np.testing.assert_array_equal(s.board_present(4), [True, False, False])
    np.testing.assert_array_equal(s.board_present(7), [False, False, True])
    s.board = dict(moving=True, T=3)
    np.testing.assert_array_equal(s.board_present(), [True] * 3)


@pytest.fixture(scope="module")
def life_report(tmp_path_factory):
    """The schedule header through a plain host program, with the address and undefined-behaviour sanitizers on
    that program only."""
    exe = str(tmp_path_factory.mktemp("task_life") / "task_life")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "task_life", "task_life_main.cpp")], check=True, capture_output=True,
                   text=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    return p.returncode, p.stdout + p.stderr


def test_task_life_program_passes(life_report):
    rc, out = life_report
    assert rc == 0 and out.rstrip().endswith("0 failed") and "FAIL" not in out and "runtime error" not in out, out


@pytest.mark.parametrize("case", [
    "edge_before_open", "edge_at_open", "edge_last_tick", "edge_at_close", "edge_after_close",
    "open_equals_close_never_present", "zero_zero_never_present", "all_open_window", "forever_absent_at_max",
    "near_max_open", "near_max_close", "max_max_never_present", "close_ticks_sorted_unique_without_forever",
    "retire_ticks", "retire_near_max", "retire_when_fresh", "retire_never_without_closes", "count_present",
    "empty_board", "retire_iff_a_task_stops_being_present_random", "valid_windows", "refuses_open_after_close",
    "refuses_negative_open", "refuses_negative_close", "valid_empty", "valid_max_max"])
def test_task_life_cases(life_report, case):
    assert f"ok {case}\n" in life_report[1], life_report[1]


def test_task_life_header_has_no_hip_includes():
    with open(os.path.join(CSRC, "task_life.h")) as f:
        inc = [ln.split()[1] for ln in f if ln.startswith("#include")]
    assert inc == ["<algorithm>", "<cstdint>", "<vector>"]


def _fixture_case():
    g = load_golden(FIXTURE)
    return g, np.stack([g["task_x"], g["task_y"]], 1), np.stack([g["task_vx"], g["task_vy"]], 1)


def test_model_with_pow_equals_the_fixture(oracle_mod):
    g, Q0, V = _fixture_case()
    first, ticks = int(g["task_tick"]) - 1, int(g["ticks"])
    lo, hi = g["open_tick"], g["close_tick"]
    d = llm.drive(oracle_mod, g, Q0, V, lo, hi, ticks - first, first=first, use_pow=True)
    o, acc = d["o"], d["acc"]
    assert g["status_out"].shape == (200, 300)
    for k in OUT_KEYS:  # the thirteen arrays
        np.testing.assert_array_equal(o[k], g[k + "_out"], err_msg=k)
    for k in ("status", "tab_winner"):
        np.testing.assert_array_equal(o[k], g[k + "_out"], err_msg=k)
    np.testing.assert_array_equal(o["tab_util"].view(np.uint32), g["tab_util_out"].view(np.uint32))
    np.testing.assert_array_equal(np.concatenate(acc["counts"]), g["counts"])
    np.testing.assert_array_equal(np.concatenate(acc["task_counts"]), g["task_counts"])
    want, got = _fixture_rows(g, 300, 300), lbm.out_rows(o, 300, 300)
    np.testing.assert_array_equal(got[0], want["claim_out"])
    np.testing.assert_array_equal(got[1], want["conflict_out"])
    np.testing.assert_array_equal(d["cur"][:, 0], g["task_x_end"])
    np.testing.assert_array_equal(d["cur"][:, 1], g["task_y_end"])
    # the generator's conditions, on the reference's run and on the model's
    handled, deleted, at_close, dropped, opened, closed, guard = (int(v) for v in g["life_counts"])
    tc = g["task_counts"]
    assert sorted(set(g["status_out"].ravel().tolist())) == [0, 1, 2, 3]
    assert handled == tc[:, 1].sum() >= 100 and deleted >= 20 and at_close >= 1 and dropped >= 1 and guard == 0
    assert acc["deleted"] == deleted and acc["dropped"] >= 1 and acc["guard"] == 0 and acc["singular"] == 0
    end = int(g["ticks"])
    gone = ~llm.present(lo, hi, end)
    assert opened > 0 and closed > 0 and gone.any() and (hi == FOREVER).any() and (V != 0).any()
    assert (g["status_out"][:, gone] == 0).all()  # absent at the end: in no agent's dict
    assert (g["tab_winner_out"][:, gone & (hi <= end)] >= 0).any()  # the tables of closed tasks are kept
    # the board does change: the same run with every task always present computes something else
    frozen = _drive(oracle_mod, g, Q0, V, ticks - first, first=first, use_pow=True)
    assert (frozen["o"]["status"] != g["status_out"]).sum() > 100
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", FIXTURE + ".npz")) < 790802


def test_two_agents_three_tasks_by_hand(oracle_mod):
    """A close with a claim in flight (task 0 closes at tick 2, the tick R hears A's claim of tick 1), a conflict
    arriving after the close (R's conflict about task 0 reaches A at tick 3 and writes nothing), and a status slot
    freed and taken by another task (A's row of two slots holds tasks 0, 1, then 1, then 1 and 2)."""
    g, Q0, lo, hi = _hand3()
    sent = {1: [2, 0, 0], 2: [0, 2, 2], 3: [0, 0, 0], 4: [1, 0, 0], 5: [0, 1, 1], 6: [0, 0, 0]}
    a_row = {1: [[TENTATIVE, TENTATIVE, OPEN]], 2: [[OPEN, TENTATIVE, OPEN]], 3: [[OPEN, ASSIGNED, OPEN]],
             4: [[OPEN, ASSIGNED, TENTATIVE]], 5: [[OPEN, ASSIGNED, TENTATIVE]], 6: [[OPEN, ASSIGNED, ASSIGNED]]}
    r_tab = {1: [-1, -1, -1], 2: [1, 1, -1], 3: [1, 1, -1], 4: [1, 1, -1], 5: [1, 1, 1], 6: [1, 1, 1]}
    d = None
    for t in range(1, 7):
        d = llm.drive(oracle_mod, g, Q0, None, lo, hi, 1, start=d)
        o = d["o"]
        np.testing.assert_array_equal(o["task_counts"], [sent[t]], err_msg=str(t))
        np.testing.assert_array_equal(o["status"], a_row[t] + [[OPEN] * 3], err_msg=str(t))
        np.testing.assert_array_equal(o["tab_winner"], [[-1] * 3, r_tab[t]], err_msg=str(t))
        assert lbm.peak_slots(o)[0] <= 2  # (three statuses over the run, never more than two at once)
    assert d["acc"]["deleted"] == 1 and d["acc"]["dropped"] == 1 and d["acc"]["guard"] == 0
    np.testing.assert_array_equal(o["tab_util"].view(np.uint32),
                                  np.array([[0.0] * 3, [50.0] * 3], np.float32).view(np.uint32))
    rows = lbm.sparse_state(o, 2, 3)
    np.testing.assert_array_equal(rows["status"], [[1 << 2 | ASSIGNED, 2 << 2 | ASSIGNED], [-1, -1]])
    np.testing.assert_array_equal(rows["tab_task"], [[-1] * 3, [0, 1, 2]])
    np.testing.assert_array_equal(rows["claim_out"], np.full((2, 2, 2), -1))
    np.testing.assert_array_equal(rows["conflict_out"], [[[-1] * 3] * 2, [[-1] * 3, [2, -1, -1]]])
    # without lifetimes the same board needs three slots and ASSIGNs task 0 as well
    f = _drive(oracle_mod, g, Q0, np.zeros_like(Q0), 6)
    np.testing.assert_array_equal(f["o"]["status"], [[ASSIGNED] * 3, [OPEN] * 3])


# ----------------------------------------------------------------------------- GPU

_models = {}


def _lboard(s, pos, vel, lo, hi, req=None, Ks=64, Kt=32):
    return s.set_task_board(pos[:, 0], pos[:, 1], req, status_slots=Ks, table_slots=Kt, velocities=vel,
                            open_tick=lo, close_tick=hi)


def _same_swarm(a, b, rows=True):
    import torch
    for t in ("pos", "pos_prev", "vel", "target", "has_target", "state", "leader"):
        assert torch.equal(getattr(a, t), getattr(b, t)), t
    for k in a.fsm:
        assert torch.equal(a.fsm[k], b.fsm[k]), k
    for k in ROWS if rows else ():
        assert torch.equal(a.board[k].view(torch.int32), b.board[k].view(torch.int32)), k


def _join(rs):
    return dict(counts=np.concatenate([r["counts"] for r in rs]),
                task_counts=np.concatenate([r["task_counts"] for r in rs]), guard=sum(r["guard"] for r in rs),
                singular=sum(r["singular"] for r in rs))


# 1. the fixture, both layouts, the ideal channel and a lossy one
@pytest.mark.gpu
@pytest.mark.parametrize("loss", [0.0, 0.2])
@pytest.mark.parametrize("layout", ["input", "spatial"])
def test_gpu_equals_the_model_on_the_fixture(oracle_mod, layout, loss):
    g, Q0, V = _fixture_case()
    lo, hi = g["open_tick"], g["close_tick"]
    T, first, ticks = len(Q0), int(g["task_tick"]) - 1, int(g["ticks"])
    s = _swarm(g, layout, board=False)
    kw = dict(loss=loss, loss_seed=77) if loss else {}
    r0 = s.update_loop_radio(first, float(g["radio_radius"]), float(g["sense_radius"]), **_kw(g), **kw)
    _lboard(s, Q0, V, lo, hi, g["task_req"], T, T)
    np.testing.assert_array_equal(s.board_present(), llm.present(lo, hi, first + 1))
    r1 = _run(s, g, ticks - first, **kw)
    if (layout, loss) not in _models:  # once per storage order, left unchanged
        q, perm = _storage_case(s, g)
        d = llm.drive(oracle_mod, q, Q0, V, lo, hi, ticks - first, first=first, loss=loss or None, loss_seed=77)
        _models[layout, loss] = _result(d, perm, T, T)
    want = _models[layout, loss]
    r = dict(r1)
    r["counts"] = np.concatenate([r0["counts"], r1["counts"]])
    r["task_counts"] = np.concatenate([np.zeros((first, 3), np.int64), r1["task_counts"]])
    r["singular"] = r0["singular"] + r1["singular"]
    _check(s, r, want)
    assert want["task_counts"][:, 1].sum() >= (100 if not loss else 50)
    if loss:
        np.testing.assert_array_equal(np.concatenate([r0["link_counts"], r1["link_counts"]]), want["link_counts"])
    assert s.fsm_tick == ticks and s.last_refused_tick == -1 and s.last_board_overflow is None
    for got, w in zip(s.board_lifetimes(), (lo, hi)):  # no call writes the lifetimes
        np.testing.assert_array_equal(got, w)
    if layout == "input" and not loss:  # real agents, in everything the squares cannot reach
        got = _state(s)
        for k in EXACT:
            np.testing.assert_array_equal(got[k], g[k + "_out"], err_msg=k)
        _assert_rows(_rows(s), _fixture_rows(g, T, T))
        np.testing.assert_array_equal(r["task_counts"], g["task_counts"])


# 2. all-open lifetimes: every bit of a twin board without lifetimes
@pytest.mark.gpu
@pytest.mark.parametrize("how", ["arrays", "scalars", "removed again"])
def test_gpu_all_open_lifetimes_equal_the_board_without(how):
    g, Q0, V = _case48()
    a, b = _swarm(g, "spatial", board=False), _swarm(g, "spatial", board=False)
    _mboard(a, Q0, V, g["task_req"], 32, 16)
    if how == "arrays":
        _lboard(b, Q0, V, np.zeros(48, np.int64), np.full(48, FOREVER), g["task_req"], 32, 16)
    elif how == "scalars":
        _lboard(b, Q0, V, 0, None, g["task_req"], 32, 16)
    else:
        _lboard(b, Q0, V, 3, 4, g["task_req"], 32, 16)
        b.set_board_lifetimes(None, None)
        assert b.board_lifetimes() is None and b.board_present().all()
    assert (b.board_lifetimes() is None) == (how == "removed again") and a.board_lifetimes() is None
    ra, rb = _run(a, g, 60, loss=0.1, loss_seed=3), _run(b, g, 60, loss=0.1, loss_seed=3)
    assert ra["task_counts"][:, 1].sum() >= 20
    _same_swarm(a, b)
    for k in ("counts", "task_counts", "link_counts"):
        np.testing.assert_array_equal(ra[k], rb[k], err_msg=k)
    assert ra["guard"] == rb["guard"]
    for x, y in zip(a.board_positions(), b.board_positions()):
        np.testing.assert_array_equal(x, y)


# 3. chunks
@pytest.mark.gpu
@pytest.mark.parametrize("chunks", [(1,) * 24, (7, 113)])
def test_gpu_chunked_run_is_the_same_run(chunks):
    g, Q0, V = _case48()
    lo, hi = _windows(48, 21, last=max(sum(chunks) - 10, 8))
    a, b = _swarm(g, "spatial", board=False), _swarm(g, "spatial", board=False)
    for s in (a, b):
        _lboard(s, Q0, V, lo, hi, g["task_req"], 32, 16)
    total = sum(chunks)
    closes = np.unique(hi[hi <= total])
    assert len(closes) >= 3
    ra = _run(a, g, total)
    rb = [_run(b, g, c) for c in chunks]
    assert ra["task_counts"][:, 0].sum() > 0 and ra["task_counts"][:, 1].sum() > 0
    _same_swarm(a, b)
    np.testing.assert_array_equal(ra["task_counts"], np.concatenate([r["task_counts"] for r in rb]))
    np.testing.assert_array_equal(ra["counts"], np.concatenate([r["counts"] for r in rb]))
    gone = ~a.board_present(total)
    st = a.board_dense()[0].cpu().numpy()
    assert gone.any() and (st[:, gone] == 0).all() and (st[:, ~gone] != 0).any()
    for s in (a, b):
        cur, lag = s.board_positions()
        np.testing.assert_array_equal(cur, _advance(Q0, V, 0.1, total))
        np.testing.assert_array_equal(lag, _advance(Q0, V, 0.1, total - 1))


# 4. new lifetimes between calls close a task that has statuses; the library's own refusals
@pytest.mark.gpu
def test_gpu_set_board_lifetimes_between_calls(oracle_mod):
    import torch
    from swarm_amd import _lib
    g, Q0, V = _case48()
    lo, hi = _windows(48, 22)
    s = _swarm(g, "spatial", board=False)
    _lboard(s, Q0, V, lo, hi, g["task_req"], 48, 48)
    q, perm = _storage_case(s, g)
    ra = _run(s, g, 40)
    d = llm.drive(oracle_mod, q, Q0, V, lo, hi, 40)
    held = np.flatnonzero((d["o"]["status"] != 0).any(0) & llm.present(lo, hi, 40))
    assert len(held) >= 4  # present tasks with statuses: half of them close now, without a closing tick to come
    lo2, hi2 = lo.copy(), hi.copy()
    hi2[held[::2]] = 40
    lo2[held[::2]] = np.minimum(lo2[held[::2]], 40)
    rows_before = {k: s.board[k].clone() for k in ROWS}
    pos_before = s.board_positions()
    lib, h = _lib.lib(), s.board["handle"]
    dev = lambda a: torch.as_tensor(np.asarray(a, np.int64), device="cuda")  # noqa: E731
    for bad_lo, bad_hi, text in ((np.where(np.arange(48) == 5, 9, 0), np.full(48, 8), "task 5 opens after it closes"),
                                 (np.where(np.arange(48) == 7, -1, 0), np.full(48, 8), "task 7 has a negative"),
                                 (np.zeros(48), np.where(np.arange(48) == 47, -2, 8), "task 47 has a negative")):
        blo, bhi = dev(bad_lo), dev(bad_hi)  # device arrays here, host arrays through the Python layer
        assert lib.swarm_board_set_lifetimes(_lib.ctx(), h, _lib.ptr(blo), _lib.ptr(bhi), _lib.stream()) == \
            _lib.ERR_ARG and text in _lib.last_error()
    other = _lib.Ctx()
    assert lib.swarm_board_set_lifetimes(other, h, _lib.ptr(dev(lo)), _lib.ptr(dev(hi)), _lib.stream()) == \
        _lib.ERR_ARG and "not a live board" in _lib.last_error()
    for got, w in zip(s.board_lifetimes(), (lo, hi)):  # a refusal changes nothing
        np.testing.assert_array_equal(got, w)
    s.set_board_lifetimes(lo2, hi2)
    for got, w in zip(s.board_lifetimes(), (lo2, hi2)):
        np.testing.assert_array_equal(got, w)
    for k in ROWS:  # setting lifetimes writes no row and no position: the next call's first tick retires
        assert torch.equal(s.board[k], rows_before[k]), k
    for x, y in zip(pos_before, s.board_positions()):
        np.testing.assert_array_equal(x, y)
    rb = _run(s, g, 40)
    d = llm.drive(oracle_mod, q, None, V, lo2, hi2, 40, start=d)
    want = _result(d, perm, 48, 48)
    _check(s, _join([ra, rb]), want)
    assert (want["status"][:, held[::2]] == 0).all() and d["acc"]["deleted"] > 0


@pytest.mark.gpu
def test_gpu_static_and_dead_boards_are_refused():
    from swarm_amd import _lib
    g, Q0, V = _case48()
    s = _swarm(g, "spatial", board=False)
    s.set_task_board(Q0[:, 0], Q0[:, 1], g["task_req"])
    lib, lo, hi = _lib.lib(), np.zeros(48, np.int64), np.full(48, 9, np.int64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    assert lib.swarm_board_set_lifetimes(_lib.ctx(), s.board["handle"], p(lo), p(hi), _lib.stream()) == _lib.ERR_ARG
    assert "lifetimes need a moving board" in _lib.last_error()
    with pytest.raises(RuntimeError, match="does not move"):
        s.set_board_lifetimes(lo, hi)
    _lboard(s, Q0, None, lo, hi, g["task_req"])  # lifetimes alone make the board a moving one, at rest
    assert s.board["moving"]
    dead = ctypes.c_void_p(s.board["handle"].value)
    with pytest.raises(_lib.SwarmError, match="a moving board needs swarm_update_loop_board_moving"):
        s.board["moving"] = False  # the static entry point refuses the handle as it refuses any moving board
        _run(s, g, 2)
    s.set_task_board([1.0], [1.0])  # destroys the board
    assert lib.swarm_board_set_lifetimes(_lib.ctx(), dead, p(lo), p(hi), _lib.stream()) == _lib.ERR_ARG
    assert "not a live board" in _lib.last_error()


# 5. swarm sizes around the workgroup; 6. boards of 0, 1 and 65 tasks
def _random_case(n, T, seed):
    rng = np.random.default_rng(seed)
    side = max(np.sqrt(n * np.pi * 2.5 ** 2 / 12.0), 3.0)
    g = _hand(np.stack([rng.uniform(0, side, n), rng.uniform(0, side, n)], 1), rng.permutation(n) + 1,
              lead=tuple(range(0, n, 9)), caps=rng.integers(0, 8, n))
    Q0 = np.stack([rng.uniform(-2.0, side + 2.0, T), rng.uniform(-2.0, side + 2.0, T)], 1).reshape(T, 2)
    V = rng.uniform(-3.0, 3.0, (T, 2))
    g.update(task_x=Q0[:, 0].copy(), task_y=Q0[:, 1].copy(), task_req=rng.integers(-1, 3, T).astype(np.int8),
             ticks=np.int64(30))
    lo, hi = _windows(T, seed + 1, last=20)
    hi = np.where(hi == FOREVER, hi, lo + (hi - lo) % 14 + 3)
    return g, Q0, V, lo, hi


@pytest.mark.gpu
@pytest.mark.parametrize("n,T", [(1, 40), (255, 40), (256, 40), (257, 40), (120, 1), (120, 65)])
def test_gpu_swarm_and_board_sizes_equal_the_model(oracle_mod, n, T):
    g, Q0, V, lo, hi = _random_case(n, T, 100 * n + T)
    s = _swarm(g, "spatial", board=False)
    _lboard(s, Q0, V, lo, hi, g["task_req"], T, T)
    q, perm = _storage_case(s, g)
    d = llm.drive(oracle_mod, q, Q0, V, lo, hi, 30)
    want = _result(d, perm, T, T)
    r = _run(s, g, 30)
    _check(s, r, want)
    assert want["task_counts"][:, 0].sum() > 0 and (n == 1 or want["task_counts"][:, 1].sum() > 0)
    assert T == 1 or d["acc"]["deleted"] > 0


@pytest.mark.gpu
def test_gpu_a_board_without_tasks_is_the_radio_loop():
    g, _, _, _, _ = _random_case(120, 1, 5)
    a, b = _swarm(g, "spatial", board=False), _swarm(g, "spatial", board=False)
    z = np.zeros(0)
    a.set_task_board(z, z, open_tick=np.zeros(0, np.int64), close_tick=np.zeros(0, np.int64))
    assert a.board["moving"] and a.board["T"] == 0 and a.board_present().shape == (0,)
    assert all(x.shape == (0,) for x in a.board_lifetimes())
    ra = _run(a, g, 30)
    rb = b.update_loop_radio(30, float(g["radio_radius"]), float(g["sense_radius"]), **_kw(g))
    _same_swarm(a, b, rows=False)
    np.testing.assert_array_equal(ra["counts"], rb["counts"])
    assert ra["task_counts"].sum() == 0


# 7. the retire pass on rows of 1, 5, 64, 67, 130 and 4 096 slots set by hand
@pytest.mark.gpu
@pytest.mark.parametrize("Ks", [1, 5, 64, 67, 130, 4096])
def test_gpu_retire_pass_on_rows_set_by_hand(Ks):
    """Tasks far from every agent (nothing is offered, nothing is sent), status rows written by hand: row 0 full, all
    of it retired at one tick; row 1 full, losing every second entry; row 2 full, losing nothing; the rest random.
    The tick before the closing one retires too (the first after the lifetimes were set) and must change nothing."""
    import torch
    n, T = 70, 3 * Ks
    rng = np.random.default_rng(Ks)
    g = _hand(np.stack([rng.uniform(0, 6, n), rng.uniform(0, 6, n)], 1), rng.permutation(n) + 1, lead=(0, 9))
    Q0 = np.stack([rng.uniform(500, 600, T), rng.uniform(500, 600, T)], 1)
    codes = rng.integers(1, 4, (n, T))
    k = np.arange(T)
    closing = (k < Ks) | ((k < 2 * Ks) & ((k - Ks) % 2 == 0))  # the first Ks tasks, every second of the next Ks
    held = [np.arange(Ks), Ks + np.arange(Ks), 2 * Ks + np.arange(Ks)] + \
        [np.sort(rng.choice(T, rng.integers(0, Ks + 1), replace=False)) for _ in range(n - 3)]
    rows = np.full((n, Ks), -1, np.int32)
    want = np.full((n, Ks), -1, np.int32)
    for i, k in enumerate(held):
        rows[i, :len(k)] = k << 2 | codes[i, k]
        keep = k[~closing[k]]
        want[i, :len(keep)] = keep << 2 | codes[i, keep]
    assert (want[0] == -1).all() and (want[2] == rows[2]).all() and (rows[:3] >= 0).all()
    assert Ks == 1 or ((want[1] >= 0).sum() == Ks // 2 and (want[3:] != rows[3:]).any())
    s = _swarm(g, "input", board=False)
    _lboard(s, Q0, None, 0, np.where(closing, 2, FOREVER), None, Ks, 4)
    s.board["status"].copy_(torch.as_tensor(rows, device="cuda"))
    r = _run(s, g, 1)  # tick 1 retires (the first tick with these lifetimes): every task is present
    np.testing.assert_array_equal(s.board["status"].cpu().numpy(), rows)
    r = _run(s, g, 1)  # tick 2 closes
    np.testing.assert_array_equal(s.board["status"].cpu().numpy(), want)
    assert r["task_counts"].sum() == 0
    for k in ("tab_task", "claim_out", "conflict_out"):
        assert (s.board[k] == -1).all(), k
    r = _run(s, g, 2)  # no retiring tick any more
    np.testing.assert_array_equal(s.board["status"].cpu().numpy(), want)


# 8. a tick that both opens and closes tasks; 9. every task absent
@pytest.mark.gpu
def test_gpu_a_tick_that_opens_and_closes_tasks(oracle_mod):
    g, Q0, V = _case48()
    lo = np.where(np.arange(48) % 2 == 0, 0, 20).astype(np.int64)
    hi = np.where(np.arange(48) % 2 == 0, 20, FOREVER).astype(np.int64)
    s = _swarm(g, "spatial", board=False)
    _lboard(s, Q0, V, lo, hi, g["task_req"], 48, 48)
    q, perm = _storage_case(s, g)
    d = llm.drive(oracle_mod, q, Q0, V, lo, hi, 19)
    at19 = d["o"]["status"].copy()
    d = llm.drive(oracle_mod, q, None, V, lo, hi, 21, start=d)
    want = _result(d, perm, 48, 48)
    assert (at19[:, ::2] != 0).any() and (at19[:, 1::2] == 0).all()
    assert (want["status"][:, ::2] == 0).all() and (want["status"][:, 1::2] != 0).any() and d["acc"]["deleted"] > 0
    r = _run(s, g, 40)
    _check(s, r, want)


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["never opened", "closed long ago", "open equals close"])
def test_gpu_every_task_absent_is_the_radio_loop(how):
    g, Q0, V = _case48()
    a, b = _swarm(g, "spatial", board=False), _swarm(g, "spatial", board=False)
    lo, hi = {"never opened": (10 ** 9, FOREVER), "closed long ago": (0, 1), "open equals close": (7, 7)}[how]
    _lboard(a, Q0, V, lo, hi, g["task_req"], 4, 4)
    assert not a.board_present().any()
    ra = _run(a, g, 40, loss=0.1, loss_seed=3)
    rb = b.update_loop_radio(40, float(g["radio_radius"]), float(g["sense_radius"]), loss=0.1, loss_seed=3, **_kw(g))
    _same_swarm(a, b, rows=False)
    for k in ("counts", "link_counts"):
        np.testing.assert_array_equal(ra[k], rb[k], err_msg=k)
    assert ra["task_counts"].sum() == 0 and ra["guard"] == 0
    assert all((a.board[k] == (0 if k == "tab_util" else -1)).all() for k in ROWS)
    np.testing.assert_array_equal(a.board_positions()[0], _advance(Q0, V, 0.1, 40))  # absent tasks advance too


# 10. a status overflow at the model's tick, later than without closes; 11. four slots are enough only with closes
def _overflow_case(oracle_mod, s, g, Q0, V, lo, hi):
    q, perm = _storage_case(s, g)
    d5 = llm.drive(oracle_mod, q, Q0, V, lo, hi, 5)
    d = llm.drive(oracle_mod, q, None, V, lo, hi, 115, start=d5)
    frozen = _drive(oracle_mod, q, Q0, V, 120)
    return _result(d, perm, 48, 48), np.asarray(frozen["acc"]["peaks"])


@pytest.mark.gpu
def test_gpu_status_overflow_comes_later_with_closes_and_grow_board_repeats_the_call(oracle_mod):
    import torch
    from swarm_amd import _lib
    g, Q0, V = _case48()
    lo, hi = _windows(48, 23, last=100)
    s = _swarm(g, "spatial", board=False)
    want, frozen = _overflow_case(oracle_mod, s, g, Q0, V, lo, hi)
    peaks = want["peaks"]
    Ks = int(peaks[:, 0].max()) - 1
    tick = int(np.flatnonzero(peaks[:, 0] > Ks)[0]) + 1  # the first tick at whose end the exact run holds more
    tick_frozen = int(np.flatnonzero(frozen[:, 0] > Ks)[0]) + 1
    print("Ks", Ks, "refused tick", tick, "without closes", tick_frozen)
    assert Ks >= 2 and tick_frozen < tick and tick > 6 and (peaks[:, 1] <= 48).all()
    assert (peaks[:tick - 1, 0] <= Ks).all() and np.unique(hi[hi < tick]).size >= 3  # closes freed slots before
    _lboard(s, Q0, V, lo, hi, g["task_req"], Ks, 48)
    r5 = _run(s, g, 5)
    b = s.board
    s._motion_state()
    keep = dict(pos=s.pos, pos_prev=s.pos_prev, vel=s.vel, state=s.state, leader=s.leader, **s.fsm,
                **{k: b[k] for k in ROWS})
    before = {k: v.clone() for k, v in keep.items()}
    entry = s.board_positions()
    with pytest.raises(_lib.SwarmError) as e:
        _run(s, g, 115)
    assert e.value.code == _lib.ERR_RANGE and f"status slots at tick {tick} " in str(e.value)
    assert s.last_refused_tick == tick and s.fsm_tick == 5 and s.last_board_overflow[0] == "status"
    for k, v in keep.items():
        assert torch.equal(v, before[k]), k
    for a, w in zip(s.board_positions(), entry):  # both lists at their entry bytes
        np.testing.assert_array_equal(a, w)
    for got, w in zip(s.board_lifetimes(), (lo, hi)):
        np.testing.assert_array_equal(got, w)
    s.grow_board(status_slots=48)
    r = _run(s, g, 115)
    _check(s, _join([r5, r]), want)
    assert s.last_refused_tick == -1 and s.last_board_overflow is None


@pytest.mark.gpu
def test_gpu_four_slots_are_enough_only_because_closes_free_them(oracle_mod):
    from swarm_amd import _lib
    # A (ID 1, bit 0) at the origin, leader R (ID 9) at (0, 2); eight tasks around A, one after the other
    ang = np.arange(8) * (np.pi / 4)
    Q0 = np.stack([np.cos(ang), np.sin(ang) * 0.5 - 0.5], 1)
    g = _hand([(0, 0), (0, 2)], [1, 9], lead=(1,), caps=[1, 0], tasks=[(x, y, 0) for x, y in Q0])
    lo = (1 + 4 * np.arange(8)).astype(np.int64)
    hi = lo + 7  # two windows overlap: at most two statuses at a time, eight over the run
    s = _swarm(g, "input", board=False)
    q, perm = _storage_case(s, g)
    want = _result(llm.drive(oracle_mod, q, Q0, None, lo, hi, 40), perm, 4, 8)
    frozen = np.asarray(_drive(oracle_mod, q, Q0, np.zeros_like(Q0), 40)["acc"]["peaks"])
    assert want["peaks"][:, 0].max() <= 4 < frozen[:, 0].max() and want["task_counts"][:, 0].sum() == 8
    _lboard(s, Q0, None, lo, hi, g["task_req"], 4, 8)
    r = _run(s, g, 40)
    _check(s, r, want)
    s2 = _swarm(g, "input", board=False)  # the same board without lifetimes is refused for full rows
    _mboard(s2, Q0, np.zeros_like(Q0), g["task_req"], 4, 8)
    with pytest.raises(_lib.SwarmError) as e:
        _run(s2, g, 40)
    assert e.value.code == _lib.ERR_RANGE and s2.last_board_overflow[0] == "status"


@pytest.mark.gpu
def test_gpu_the_hand_case_on_rows_of_two_slots(oracle_mod):
    g, Q0, lo, hi = _hand3()
    s = _swarm(g, "input", board=False)
    _lboard(s, Q0, None, lo, hi, g["task_req"], 2, 3)
    r = _run(s, g, 6)
    np.testing.assert_array_equal(r["task_counts"], [[2, 0, 0], [0, 2, 2], [0, 0, 0], [1, 0, 0], [0, 1, 1], [0, 0, 0]])
    rows = _rows(s)
    np.testing.assert_array_equal(rows["status"], [[1 << 2 | ASSIGNED, 2 << 2 | ASSIGNED], [-1, -1]])
    np.testing.assert_array_equal(rows["tab_task"], [[-1] * 3, [0, 1, 2]])
    np.testing.assert_array_equal(rows["tab_winner"], [[-1] * 3, [1, 1, 1]])
    np.testing.assert_array_equal(rows["conflict_out"], [[[-1] * 3] * 2, [[-1] * 3, [2, -1, -1]]])


# 12. a resort in the middle of a run
@pytest.mark.gpu
def test_gpu_a_run_with_a_resort_equals_the_run_rebuilt_from_its_input_order_state():
    from test_resort import _assert_same_swarm, _board_case, _fresh_twin
    g = _board_case(5001, 23, ticks=60, kills=(10, 50), T=200)
    Q0 = np.stack([g["task_x"], g["task_y"]], 1)
    V = np.random.default_rng(9).uniform(-3.0, 3.0, Q0.shape)
    lo, hi = _windows(200, 24, last=50)
    a, b = _swarm(g, "spatial", board=False), _swarm(g, "spatial", board=False)
    for s in (a, b):
        _lboard(s, Q0, V, lo, hi, g["task_req"], 64, 32)
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
    gone = ~a.board_present(60)
    st = a.board_dense()[0].cpu().numpy()
    assert gone.sum() > 20 and (st[:, gone] == 0).all() and (st[:, ~gone] != 0).any()


# 13. the census after closes; 14. the bridge
@pytest.mark.gpu
def test_gpu_census_after_closes_counts_tables_and_no_statuses(oracle_mod):
    from test_board_census import _assert_census
    g, Q0, V = _case48()
    lo, hi = _windows(48, 25, last=60)
    s = _swarm(g, "input", board=False)
    _lboard(s, Q0, V, lo, hi, g["task_req"], 48, 48)
    q, perm = _storage_case(s, g)
    want = _result(llm.drive(oracle_mod, q, Q0, V, lo, hi, 100), perm, 48, 48)
    _run(s, g, 100)
    c = bcm.census(want["status"], want["tab_winner"], want["tab_util"], g["ids"])
    _assert_census(s.board_census(holders=True), c, holders=True)
    closed = hi <= 100
    held = (want["status"] != 0).sum(0)
    tables = (want["tab_winner"] >= 0).sum(0)
    assert closed.sum() >= 10 and (held[closed] == 0).all() and (tables[closed] > 0).any() and held[~closed].sum() > 0
    got = {k: v.cpu().numpy() for k, v in s.board_census().items() if hasattr(v, "cpu")}
    for k in ("tentative", "locked", "assigned"):
        assert (got[k][closed] == 0).all(), k


@pytest.mark.gpu
def test_gpu_write_back_board_leaves_absent_tasks_out():
    g, Q0, lo, hi = _hand3()
    s = _swarm(g, "spatial", board=False)
    pos = {10: (1.0, 0.0), 20: (0.0, 1.0), 30: (-1.0, 0.0)}
    agents = [types.SimpleNamespace(agent_id=int(i), task_claims={},
                                    tasks={k: {"status": "OPEN", "pos": p, "required_cap": "extinguisher"}
                                           for k, p in pos.items()}) for i in g["ids"]]
    del agents[1].tasks[10]  # (already gone at this agent)
    s.set_task_board(s.tasks_from_dict(agents[0].tasks), status_slots=2, table_slots=3, open_tick=lo, close_tick=hi)
    np.testing.assert_array_equal(s.board_task_ids, [10, 20, 30])
    _run(s, g, 3)  # task 10 has closed, task 30 is not open yet
    s.write_back_board(agents)
    assert [sorted(a.tasks) for a in agents] == [[20], [20]]
    assert [a.tasks[20]["status"] for a in agents] == ["ASSIGNED", "OPEN"]
    assert agents[1].task_claims == {10: {"winner": 1, "utility": 50.0}, 20: {"winner": 1, "utility": 50.0}}
    s.set_board_lifetimes(None, None)  # a board without lifetimes: nothing is deleted
    s.write_back_board(agents)
    assert [sorted(a.tasks) for a in agents] == [[20], [20]]
