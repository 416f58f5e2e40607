"""The task loop on boards of any size (contract U1-B): swarm_update_loop_board /
Swarm.set_task_board + Swarm.update_loop_board(ticks, Rc, Rs).

U1-B is U1-T word for word on a board of up to 2^24 tasks, every agent's task state in sparse canonical rows.
The yardsticks are the unchanged CPU models (loop_tasks_model, loop_lossy_model: they run any T; only their
64-bit claim / conflict words mean nothing above 64 tasks, so the `tasks` lists they return are compared) and
tests/golden/loop_board_n200.npz, produced by real SwarmAgent objects on a board of 300 tasks
(tools/gen_golden_loop_board.py).  tests/loop_board_model.py only converts between the dense and the sparse
layout.  The GPU must equal the model with its own x*x squares bit for bit over its storage order, the fixtures
themselves in layout "input", and update_loop_tasks on a twin swarm wherever a board fits both.
"""
import ctypes
import os
import subprocess
import time

import numpy as np
import pytest

from conftest import PKG, ROOT, load_golden
import loop_board_model as lbm
import loop_lossy_model
import loop_tasks_model
from loop_model import OUT_KEYS, F, L
from test_update_loop_sensed import EXACT, PER_AGENT, _assert_equal, _state
from test_update_loop_tasks import _hand, _kw, _swarm, _u32

ALL = OUT_KEYS + ("px", "py")
ROWS = ("status", "tab_task", "tab_winner", "tab_util", "claim_out", "conflict_out")
OPEN, TENTATIVE, LOCKED, ASSIGNED = 0, 1, 2, 3
FIXTURES = ("loop_tasks_n200", "loop_tasks_wide_n400", "loop_tasks_r12_n250", "loop_board_n200")
CSRC = os.path.join(PKG, "csrc")


def _fixture_rows(g, Ks, Kt):
    """A fixture's final task state as sparse rows (input order): the 64-task ones keep their sets as words."""
    n, T = g["status_out"].shape
    tt, tw, tu = lbm.sparse_tables(g["tab_winner_out"], g["tab_util_out"], Kt)
    sets = {}
    for key, idx, K in (("claim_out", "claim_idx", Ks), ("conflict_out", "conflict_idx", Kt)):
        lists = [[[] for _ in range(n)] for _ in range(2)]
        if idx in g:
            for h, i, k in g[idx]:
                lists[h][i].append(int(k))
        else:
            for h in (0, 1):
                for i in range(n):
                    lists[h][i] = [k for k in range(T) if int(g[key][h, i]) >> k & 1]
        sets[key] = np.stack([lbm.sparse_sets(lists[h], K) for h in (0, 1)])
    return dict(status=lbm.sparse_status(g["status_out"], Ks), tab_task=tt, tab_winner=tw, tab_util=tu, **sets)


# ----------------------------------------------------------------------------- CPU

def test_exports_and_struct_sizes():
    from swarm_amd import _lib
    lib = _lib.load()
    for name in ("swarm_board_create", "swarm_board_info", "swarm_board_read", "swarm_board_destroy",
                 "swarm_update_loop_board"):
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert ctypes.sizeof(_lib.BoardState) == 64  # two int32, seven pointers
    assert ctypes.sizeof(_lib.BoardDesc) == 56 and ctypes.sizeof(_lib.BoardOverflow) == 16


def test_entry_points_refuse_bad_arguments_without_a_device():
    from swarm_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(8)  # never dereferenced: the arguments below are refused first

    def loop(ctx, board, state):
        return lib.swarm_update_loop_board(ctx, 4, None, None, None, None, None, 0, 1, 0.1, 3.0, 0.2,
                                           ctypes.c_uint64(0), None, 0, None, None, None, 0, None, 2.5, 2.5, 5.0,
                                           None, 0, None, None, None, board, state, None, None, None, None, None,
                                           None)
    good = _lib.BoardState(8, 8)
    assert loop(None, fake, ctypes.byref(good)) == _lib.ERR_ARG and b"ctx is NULL" in lib.swarm_last_error()
    assert loop(fake, None, ctypes.byref(good)) == _lib.ERR_ARG and b"board is NULL" in lib.swarm_last_error()
    assert loop(fake, fake, None) == _lib.ERR_ARG and b"state is NULL" in lib.swarm_last_error()
    for ks, kt in ((0, 8), (4097, 8), (8, 0), (8, 4097)):
        assert loop(fake, fake, ctypes.byref(_lib.BoardState(ks, kt))) == _lib.ERR_ARG
        assert b"[1, 4096]" in lib.swarm_last_error()
    out = ctypes.c_void_p()
    for T in (-1, (1 << 24) + 1):
        assert lib.swarm_board_create(fake, T, fake, fake, ctypes.byref(out), None, None) == _lib.ERR_ARG
        assert b"[0, 2^24]" in lib.swarm_last_error() and not out.value
    assert lib.swarm_board_create(None, 3, fake, fake, ctypes.byref(out), None, None) == _lib.ERR_ARG
    assert lib.swarm_board_create(fake, 3, None, fake, ctypes.byref(out), None, None) == _lib.ERR_ARG
    assert b"NULL task array" in lib.swarm_last_error()


def test_update_loop_board_needs_a_board_and_good_radii_without_a_device():
    from swarm_amd.swarm import Swarm
    s = Swarm.__new__(Swarm)
    with pytest.raises(RuntimeError, match="set_task_board"):
        s.update_loop_board(3, 2.5, 2.5)
    s.board = {}
    with pytest.raises(ValueError, match="radio_radius must be positive and finite"):
        s.update_loop_board(3, 0.0, 1.0)
    with pytest.raises(ValueError, match="loss must be in"):
        s.update_loop_board(3, 2.5, 2.5, loss=1.5)
    s.n, s.device = 4, "cpu"
    for kw in (dict(status_slots=0), dict(table_slots=4097)):
        with pytest.raises(ValueError, match=r"must be in \[1, 4096\]"):
            s.set_task_board([1.0], [2.0], **kw)


_pow_model = {}


def _board_pow_model(oracle_mod):
    if not _pow_model:  # computed once, shared, left unchanged
        _pow_model["o"] = loop_tasks_model.run(oracle_mod, load_golden("loop_board_n200"), use_pow=True)
    return _pow_model["o"]


def test_model_with_pow_equals_the_board_fixture(oracle_mod):
    g, o = load_golden("loop_board_n200"), _board_pow_model(oracle_mod)
    assert g["status_out"].shape == (200, 300)
    for k in OUT_KEYS:  # the thirteen arrays
        np.testing.assert_array_equal(o[k], g[k + "_out"], err_msg=k)
    for k in ("status", "tab_winner"):
        np.testing.assert_array_equal(o[k], g[k + "_out"], err_msg=k)
    np.testing.assert_array_equal(o["tab_util"].view(np.uint32), g["tab_util_out"].view(np.uint32))
    np.testing.assert_array_equal(o["counts"], g["counts"])
    np.testing.assert_array_equal(o["task_counts"], g["task_counts"])
    want, got = _fixture_rows(g, 300, 300), lbm.out_rows(o, 300, 300)
    np.testing.assert_array_equal(got[0], want["claim_out"])
    np.testing.assert_array_equal(got[1], want["conflict_out"])
    assert o["singular"] == 0 and o["guard"] == 0


def test_board_fixture_exercises_the_handlers_above_task_64():
    g = load_golden("loop_board_n200")
    hi = g["status_out"][:, 64:]
    assert sorted(set(hi.ravel().tolist())) == [OPEN, TENTATIVE, LOCKED, ASSIGNED]
    assert (hi != OPEN).any(0).sum() >= 100 and (g["tab_winner_out"][:, 64:] >= 0).any(1).sum() >= 3
    tc = g["task_counts"]
    assert tc[:44].sum() == 0 and tc[44, 0] > 64 and tc[:, 1].sum() >= 200 and tc[:, 2].sum() >= 200
    assert g["claim_idx"].shape[1] == 3 and g["conflict_idx"].shape[1] == 3  # (the run is quiet at its end)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "loop_board_n200.npz")) < 790802


def test_converters_round_trip(oracle_mod):
    o = _board_pow_model(oracle_mod)
    ks, kt = lbm.peak_slots(o)
    assert ks > 16 and kt > 4
    np.testing.assert_array_equal(lbm.dense_status(lbm.sparse_status(o["status"], ks), 300), o["status"])
    w, u = lbm.dense_tables(*lbm.sparse_tables(o["tab_winner"], o["tab_util"], kt), 300)
    np.testing.assert_array_equal(w, o["tab_winner"])
    np.testing.assert_array_equal(u.view(np.uint32), o["tab_util"].view(np.uint32))
    rows = lbm.sparse_status(o["status"], ks + 3)
    live = rows >= 0
    assert (rows[~live] == -1).all() and (live[:, :-1] >= live[:, 1:]).all()  # the empties last
    assert (np.diff(rows.astype(np.int64) >> 2, axis=1)[live[:, 1:]] >= 1).all()  # strictly ascending tasks
    with pytest.raises(ValueError):
        lbm.sparse_status(o["status"], ks - 1)
    lists = [[(7, 1.0), (3, 2.0), (7, 5.0)], [], [300, 2]]
    np.testing.assert_array_equal(lbm.sparse_sets(lists, 3), [[3, 7, -1], [-1, -1, -1], [2, 300, -1]])
    assert lbm.set_lists(lbm.sparse_sets(lists, 3)) == [[3, 7], [], [2, 300]]


@pytest.fixture(scope="module")
def grid_report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("task_grid") / "task_grid")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                    "-o", exe, os.path.join(ROOT, "tests", "task_grid", "task_grid_main.cpp")], check=True,
                   capture_output=True, text=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    return p.returncode, p.stdout


def test_task_grid_program_passes(grid_report):
    rc, out = grid_report
    assert rc == 0 and out.rstrip().endswith("0 failed"), out


@pytest.mark.parametrize("case,T,shape", [
    ("t0", 0, "ncx=1 ncy=1"), ("one_task", 1, "ncx=1 ncy=1"), ("co_located", 50, "ncx=1 ncy=1"),
    ("one_line_x", 60, "ncx=21 ncy=1"), ("one_line_y", 60, "ncx=1 ncy=21"), ("on_cell_borders", 16, "ncx=8 ncy=8"),
    ("scattered_300", 300, ""), ("scattered_5000", 5000, "ncx=80 ncy=80"), ("wide_cells_grown", 40, ""),
    ("near_1e9", 80, "")])
def test_task_grid_offers_every_task_within_reach_of_a_probe(grid_report, case, T, shape):
    line = [ln for ln in grid_report[1].splitlines() if ln.startswith(f"ok {case} T={T} ")]
    assert len(line) == 1 and shape in line[0], grid_report[1]
    if case == "wide_cells_grown":  # the cell cap 4 T + 1024 made the cells wider than 5
        assert float(line[0].split("cell=")[1].split()[0]) > 1000.0


@pytest.mark.parametrize("case,status", [("nan_x", 1), ("inf_y", 1), ("extent_overflows", 2)])
def test_task_grid_refuses_bad_boards(grid_report, case, status):
    assert f"ok {case} refused status={status} lists_empty=1\n" in grid_report[1], grid_report[1]


def test_task_grid_header_has_no_hip_includes():
    with open(os.path.join(CSRC, "task_grid.h")) as f:
        inc = [ln.split()[1] for ln in f if ln.startswith("#include")]
    assert inc == ["<cmath>", "<cstdint>", "<new>", "<vector>", '"grid_shape.h"']


# ----------------------------------------------------------------------------- GPU

def _board(s, g, Ks, Kt):
    return s.set_task_board(g["task_x"], g["task_y"], g["task_req"], status_slots=Ks, table_slots=Kt)


def _run(s, g, ticks, **kw):
    return s.update_loop_board(ticks, float(g["radio_radius"]), float(g["sense_radius"]), **_kw(g), **kw)


def _run_radio(s, g, ticks, **kw):
    return s.update_loop_radio(ticks, float(g["radio_radius"]), float(g["sense_radius"]), **_kw(g), **kw)


def _rows(s):
    """The six sparse arrays in input order; the two out arrays as (2, n, K)."""
    b, n = s.board, s.n
    out = {k: s.to_input_order(b[k]) for k in ("status", "tab_task", "tab_winner", "tab_util")}
    for k in ("claim_out", "conflict_out"):
        out[k] = np.stack([s.to_input_order(b[k][h * n:(h + 1) * n]) for h in (0, 1)])
    return out


def _assert_rows(got, want):
    for k in ROWS:
        a, w = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == w.shape, k
        np.testing.assert_array_equal(a.view(np.uint32) if k == "tab_util" else a,
                                      w.view(np.uint32) if k == "tab_util" else w, err_msg=k)


def _storage_case(s, g):
    perm = s.perm.cpu().numpy().astype(np.int64)
    q = dict(g)
    for k in PER_AGENT + ("caps",):
        q[k] = np.asarray(g[k])[perm]
    if "fsm0" in g:
        q["fsm0"] = {k: np.asarray(v)[perm] for k, v in g["fsm0"].items()}
    return q, perm


def _to_input(o, perm, Ks, Kt):
    """A model result over the storage order -> per-agent arrays in input order, `rows` the sparse state."""
    out = {}
    for k, v in o.items():
        if isinstance(v, np.ndarray) and k not in ("counts", "task_counts", "link_counts", "claim_out", "conflict_out"):
            out[k] = np.empty_like(v)
            out[k][perm] = v
        else:
            out[k] = v
    rows = lbm.sparse_state(o, Ks, Kt)
    out["rows"] = {}
    for k, v in rows.items():
        out["rows"][k] = np.empty_like(v)
        if v.ndim == 3:
            out["rows"][k][:, perm] = v
        else:
            out["rows"][k][perm] = v
    return out


def _model(oracle_mod, s, g, ticks=None, plan=None, Ks=None, Kt=None, loss=None, loss_seed=0, **kw):
    """The model over s's storage order (loop_lossy_model with loss=), in chunks when asked."""
    q, perm = _storage_case(s, g)
    o, counts, tcounts, lcounts, singular, guard = None, [], [], [], 0, 0
    for chunk in (plan or [ticks]):
        if loss is None:
            o = loop_tasks_model.run(oracle_mod, q, chunk, start=o, **kw)
        else:
            o = loop_lossy_model.run(oracle_mod, q, chunk, start=o, loss=loss, loss_seed=loss_seed, **kw)
            lcounts.append(o["link_counts"])
        counts.append(o["counts"])
        tcounts.append(o["task_counts"])
        singular += o["singular"]
        guard += o["guard"]
    T = len(g["task_x"])
    out = _to_input(o, perm, Ks or max(T, 1), Kt or max(T, 1))
    out.update(counts=np.concatenate(counts), task_counts=np.concatenate(tcounts), singular=singular, guard=guard)
    if lcounts:
        out["link_counts"] = np.concatenate(lcounts)
    return out


_models = {}


# 1. the four fixtures, both layouts: the radio loop up to the hand-out, then the board with rows that cannot overflow
@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("layout", ["input", "spatial"])
def test_gpu_equals_the_model_and_the_reference_fixture(oracle_mod, name, layout):
    g = load_golden(name)
    T, first, ticks = len(g["task_x"]), int(g["task_tick"]) - 1, int(g["ticks"])
    s = _swarm(g, layout, board=False)
    r0 = _run_radio(s, g, first)
    _board(s, g, T, T)
    r1 = _run(s, g, ticks - first)
    if (name, layout) not in _models:  # once per storage order, left unchanged
        _models[name, layout] = _model(oracle_mod, s, g, ticks)
    want = _models[name, layout]
    got, rows = _state(s), _rows(s)
    counts = np.concatenate([r0["counts"], r1["counts"]])
    tcounts = np.concatenate([np.zeros((first, 3), np.int64), r1["task_counts"]])
    _assert_equal(got, want, ALL)
    _assert_rows(rows, want["rows"])
    np.testing.assert_array_equal(counts, want["counts"])
    np.testing.assert_array_equal(tcounts, want["task_counts"])
    assert r1["guard"] == want["guard"] == 0 and r0["singular"] + r1["singular"] == want["singular"] == 0
    assert s.fsm_tick == ticks and s.last_refused_tick == -1 and s.last_board_overflow is None
    if layout == "input":  # the fixture's own order: real agents, in everything the squares cannot reach
        for k in EXACT:
            np.testing.assert_array_equal(got[k], g[k + "_out"], err_msg=k)
        _assert_rows(rows, _fixture_rows(g, T, T))
        np.testing.assert_array_equal(counts, g["counts"])
        np.testing.assert_array_equal(tcounts, g["task_counts"])
    st, w, u = (s.to_input_order(t) for t in s.board_dense())
    np.testing.assert_array_equal(st, lbm.dense_status(rows["status"], T))
    np.testing.assert_array_equal(w, lbm.dense_tables(rows["tab_task"], rows["tab_winner"], rows["tab_util"], T)[0])
    assert u.dtype == np.float32 and (u != 0).sum() > 0


# 2. twin swarms on a board both loops take
@pytest.mark.gpu
@pytest.mark.parametrize("loss", [0.0, 0.2])
def test_gpu_board_loop_equals_the_task_loop_on_a_twin_swarm(loss):
    import torch
    from test_update_loop_sensed import _random_case
    g = _random_case(20001, 23, ticks=40)
    rng = np.random.default_rng(5)
    lo, hi = g["x"].min(), g["x"].max()
    g.update(radio_radius=np.float64(2.5), sense_radius=np.float64(2.5), caps=rng.integers(0, 8, 20001).astype(np.uint32),
             task_x=rng.uniform(lo, hi, 24), task_y=rng.uniform(lo, hi, 24),
             task_req=rng.integers(-1, 3, 24).astype(np.int8))
    a, b = _swarm(g, "spatial"), _swarm(g, "spatial", board=False)
    _board(b, g, 24, 24)
    kw = dict(loss=loss, loss_seed=77) if loss else {}
    ra = a.update_loop_tasks(40, 2.5, 2.5, **_kw(g), **kw)
    rb = _run(b, g, 40, **kw)
    tc = ra["task_counts"]
    assert tc[:, 0].sum() >= 100 and tc[:, 1].sum() >= 20 and tc[:, 2].sum() >= 20
    for t in ("pos", "pos_prev", "vel", "target", "has_target", "state", "leader"):
        assert torch.equal(getattr(a, t), getattr(b, t)), t
    for k in a.fsm:
        assert torch.equal(a.fsm[k], b.fsm[k]), k
    for k in ("counts", "task_counts") + (("link_counts",) if loss else ()):
        np.testing.assert_array_equal(ra[k], rb[k], err_msg=k)
    assert ("link_counts" in rb) == bool(loss) and ra["guard"] == rb["guard"] and ra["singular"] == rb["singular"]
    st, w, u = b.board_dense()
    assert torch.equal(st, a.task_status()) and torch.equal(w, a.tasks["tab_winner"])
    assert torch.equal(u.view(torch.int32), a.tasks["tab_util"].view(torch.int32))
    n = a.n
    for key in ("claim_out", "conflict_out"):
        words = a.tasks[key].cpu().numpy().view(np.uint64)
        rows = b.board[key].cpu().numpy()
        got = np.zeros(2 * n, np.uint64)
        for c in range(rows.shape[1]):
            live = rows[:, c] >= 0
            got[live] |= np.uint64(1) << rows[live, c].astype(np.uint64)
        np.testing.assert_array_equal(got, words, err_msg=key)
        assert (np.diff(rows.astype(np.int64), axis=1)[(rows[:, 1:] >= 0)] > 0).all()


# 3. a scattered board of 5 000 tasks around the arena (shared with 6.)
def _scattered_case():
    g = dict(load_golden("loop_tasks_n200"))
    rng = np.random.default_rng(77)
    g.update(task_x=rng.uniform(17.5 - 200.0, 17.5 + 200.0, 5000), task_y=rng.uniform(17.5 - 200.0, 17.5 + 200.0, 5000),
             task_req=rng.integers(-1, 3, 5000).astype(np.int8), task_tick=np.int64(1))
    return g


def _scattered_model(oracle_mod, s, g):
    """The exact run tick by tick over s's storage order: the model's end state, and after every tick the
    fullest agent's status and table entries (both only grow)."""
    if "scattered" not in _models:
        q, perm = _storage_case(s, g)
        o, peaks, counts, tcounts = None, [], [], []
        for _ in range(int(g["ticks"])):
            o = loop_tasks_model.run(oracle_mod, q, 1, start=o)
            peaks.append(lbm.peak_slots(o))
            counts.append(o["counts"])
            tcounts.append(o["task_counts"])
        out = _to_input(o, perm, 64, 32)
        out.update(counts=np.concatenate(counts), task_counts=np.concatenate(tcounts), peaks=np.asarray(peaks))
        _models["scattered"] = out
    return _models["scattered"]


def _check_scattered(s, r, want):
    _assert_equal(_state(s), want, ALL)
    _assert_rows(_rows(s), want["rows"])
    np.testing.assert_array_equal(r["counts"], want["counts"])
    np.testing.assert_array_equal(r["task_counts"], want["task_counts"])


@pytest.mark.gpu
def test_gpu_scattered_board_of_5000_tasks_equals_the_model(oracle_mod):
    g = _scattered_case()
    s = _swarm(g, "spatial", board=False)
    _board(s, g, 64, 32)
    want = _scattered_model(oracle_mod, s, g)
    ks, kt = want["peaks"][-1]
    touched = int((lbm.dense_status(want["rows"]["status"], 5000) != 0).any(0).sum())
    print("scattered board: peak status", ks, "peak table", kt, "tasks touched", touched)
    assert 16 < ks <= 64 and 4 < kt <= 32 and touched >= 100
    assert (want["rows"]["status"] >> 2).max() >= 4097 and want["task_counts"][:, 1].sum() >= 100
    r = _run(s, g, int(g["ticks"]))
    _check_scattered(s, r, want)
    assert s.board["info"]["T"] == 5000 and r["guard"] == 0


@pytest.mark.gpu
def test_gpu_scattered_board_over_a_lossy_channel_equals_the_lossy_model(oracle_mod):
    g = _scattered_case()
    s = _swarm(g, "spatial", board=False)
    _board(s, g, 64, 32)
    want = _model(oracle_mod, s, g, int(g["ticks"]), Ks=64, Kt=32, loss=0.3, loss_seed=11)
    r = _run(s, g, int(g["ticks"]), loss=0.3, loss_seed=11)
    _check_scattered(s, r, want)
    np.testing.assert_array_equal(r["link_counts"], want["link_counts"])
    assert want["link_counts"][:, 1].sum() > 100 and want["task_counts"][:, 1].sum() >= 20


# 4. hand-built resting agents on task indices 64, 65, 4 097 and T - 1 of a board whose other tasks are out of reach
T_HAND = 4100


def _far_board(T, near):
    """T tasks far from everybody (x = 1e5 + 10 k), but for `near`: {index: (x, y, treq)}."""
    tasks = [(1.0e5 + 10.0 * k, 0.0, -1) for k in range(T)]
    for k, v in near.items():
        tasks[k] = v
    return tasks


def _go(g, ticks, Ks=4, Kt=4):
    s = _swarm(g, "input", board=False)
    _board(s, g, Ks, Kt)
    r = _run(s, g, ticks)
    st = _state(s)
    np.testing.assert_array_equal(st["x"], g["x"])  # at rest
    rows = _rows(s)
    T = len(g["task_x"])
    dense = dict(status=lbm.dense_status(rows["status"], T) if T <= 5000 else None, rows=rows)
    return s, r, st, dense


def _status_of(rows, i, k):
    e = [int(v) & 3 for v in rows["status"][i] if v >= 0 and int(v) >> 2 == k]
    return e[0] if e else OPEN


def _entry(rows, i, k):
    """(winner, utility) agent i's table holds for task k, or None."""
    for t, w, u in zip(rows["tab_task"][i], rows["tab_winner"][i], rows["tab_util"][i]):
        if t == k:
            return int(w), u
    return None


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["near first", "far first"])
@pytest.mark.parametrize("gap", ["more than 5", "less than 5"])
def test_gpu_two_claims_of_one_tick_meet_the_hysteresis_in_walk_order(order, gap):
    # test_update_loop_tasks' case on task 64: leader R (ID 9, lacks the capability) at the origin, the task at
    # (0, 1); the near claimer (ID 1) at (-1, 0): U = 41.42; the far one (ID 2) at (1.2, 0): 39.03, or (2, 0): 30.90
    far_x = 1.2 if gap == "less than 5" else 2.0
    near, far = ((-1.0, 0.0), 1), ((far_x, 0.0), 2)
    a, b = (near, far) if order == "near first" else (far, near)
    g = _hand([a[0], b[0], (0, 0)], [a[1], b[1], 9], lead=(2,), caps=[1, 1, 0],
              tasks=_far_board(T_HAND, {64: (0, 1, 0)}))
    s, r, st, d = _go(g, 3)
    u_near, u_far = _u32(-1.0, -1.0), _u32(far_x, -1.0)
    win = 1 if gap == "more than 5" or order == "near first" else 2
    w, u = _entry(d["rows"], 2, 64)
    assert w == win and u.view(np.uint32) == (u_near if win == 1 else u_far).view(np.uint32)
    np.testing.assert_array_equal(r["task_counts"], [[2, 0, 0], [0, 2, 2], [0, 0, 0]])
    want = {1: ASSIGNED if win == 1 else LOCKED, 2: ASSIGNED if win == 2 else LOCKED}
    np.testing.assert_array_equal(d["rows"]["status"], [[64 << 2 | want[a[1]], -1, -1, -1],
                                                        [64 << 2 | want[b[1]], -1, -1, -1], [-1] * 4])
    np.testing.assert_array_equal(d["rows"]["tab_task"], [[-1] * 4, [-1] * 4, [64, -1, -1, -1]])
    # tick 2's conflict row at parity 0; tick 3 sent nothing and tick 1's claim rows were cleared on demand
    np.testing.assert_array_equal(d["rows"]["conflict_out"], [[[-1] * 4, [-1] * 4, [64, -1, -1, -1]], [[-1] * 4] * 3])
    assert (d["rows"]["claim_out"] == -1).all()


@pytest.mark.gpu
def test_gpu_leader_that_yields_mid_walk_keeps_the_claims_before_and_ignores_those_after():
    # walk order of receiver R (ID 5, index 3): claimer C1 (ID 1), leader H (ID 9, heartbeats at tick 1),
    # claimer C2 (ID 2).  Task 4097 needs bit 0 (C1 only), task 65 bit 1 (C2 only), each 1.0 from its claimer.
    g = _hand([(-2, 0), (2, 0), (0, -2), (0, 0)], [1, 9, 2, 5], lead=(1, 3), caps=[1, 0, 2, 0],
              tasks=_far_board(T_HAND, {4097: (-2, 1, 0), 65: (1, -2, 1)}), off=[0, 9, 0, 0])
    s, r, st, d = _go(g, 3)
    np.testing.assert_array_equal(r["task_counts"], [[2, 0, 0], [0, 1, 1], [0, 0, 0]])
    np.testing.assert_array_equal(st["state"], [F, L, F, F])
    assert _entry(d["rows"], 3, 4097) == (1, np.float32(50.0)) and _entry(d["rows"], 3, 65) is None
    # tick 3: R's conflict on task 4097 names ID 1 -- C1 ASSIGNED, H and C2 LOCKED; C2's claim was lost
    np.testing.assert_array_equal(d["rows"]["status"], [[4097 << 2 | ASSIGNED, -1, -1, -1],
                                                        [4097 << 2 | LOCKED, -1, -1, -1],
                                                        [65 << 2 | TENTATIVE, 4097 << 2 | LOCKED, -1, -1], [-1] * 4])
    np.testing.assert_array_equal(d["rows"]["conflict_out"][0], [[-1] * 4] * 3 + [[4097, -1, -1, -1]])
    assert r["guard"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("first", ["L1", "L2"])
def test_gpu_bystander_of_two_leaders_keeps_the_last_conflict_in_walk_order(first):
    # L1 (ID 8) at (-2, 0) hears only B (ID 3, origin); L2 (ID 9) at (2, 0) hears B and C2 (ID 4, at (4, 0)).
    # The last task of the board, at (3, 0), needs bit 0: B claims with U = 25, C2 with 50.
    k = T_HAND - 1
    l1, l2 = ((-2.0, 0.0), 8), ((2.0, 0.0), 9)
    a, b = (l1, l2) if first == "L1" else (l2, l1)
    g = _hand([a[0], b[0], (0, 0), (4, 0)], [a[1], b[1], 3, 4], lead=(0, 1), caps=[0, 0, 1, 1],
              tasks=_far_board(T_HAND, {k: (3, 0, 0)}))
    s, r, st, d = _go(g, 3)
    i1, i2 = (0, 1) if first == "L1" else (1, 0)
    assert _entry(d["rows"], i1, k) == (3, np.float32(25.0)) and _entry(d["rows"], i2, k) == (4, np.float32(50.0))
    np.testing.assert_array_equal(r["task_counts"], [[2, 0, 0], [0, 3, 3], [0, 0, 0]])
    # L1 then L2: ASSIGNED, overwritten by LOCKED; L2 then L1: LOCKED, overwritten by ASSIGNED
    assert _status_of(d["rows"], 2, k) == (LOCKED if first == "L1" else ASSIGNED)
    assert _status_of(d["rows"], 3, k) == ASSIGNED and (d["rows"]["status"][:2] == -1).all()


@pytest.mark.gpu
def test_gpu_unheard_claim_exact_threshold_and_missing_capability():
    # a claim nobody hears (the leader is 10 away) stays TENTATIVE and is never sent again
    g = _hand([(0, 0), (10, 0)], [1, 9], lead=(1,), tasks=_far_board(T_HAND, {4097: (1, 0, -1)}))
    s, r, st, d = _go(g, 6)
    np.testing.assert_array_equal(r["task_counts"], [[1, 0, 0]] + [[0, 0, 0]] * 5)
    np.testing.assert_array_equal(d["rows"]["status"], [[4097 << 2 | TENTATIVE, -1, -1, -1], [-1] * 4])
    assert (d["rows"]["tab_task"] == -1).all() and (d["rows"]["claim_out"] == -1).all()
    # 4.0 away: U = 100 / 5 = 20.0, not > 20; evaluated again at each of the three ticks
    g = _hand([(0, 0)], [1], tasks=_far_board(T_HAND, {64: (4, 0, -1)}))
    s, r, st, d = _go(g, 3)
    assert r["guard"] == 3 and r["task_counts"].sum() == 0 and (d["rows"]["status"] == -1).all()
    # one ulp nearer: whatever fp64 makes of it, and inside the guard band while it is evaluated
    tx = np.nextafter(4.0, 0.0)
    U = 100.0 / (1.0 + np.sqrt((0.0 - tx) * (0.0 - tx) + 0.0))
    g = _hand([(0, 0)], [1], tasks=_far_board(T_HAND, {64: (tx, 0, -1)}))
    s, r, st, d = _go(g, 3)
    claims = bool(U > 20.0)
    assert r["task_counts"][:, 0].tolist() == ([1, 0, 0] if claims else [0, 0, 0])
    assert _status_of(d["rows"], 0, 64) == (TENTATIVE if claims else OPEN) and r["guard"] == (1 if claims else 3)
    # a missing capability claims nothing (bit 0: agent 2 only)
    g = _hand([(0, 0), (0.5, 0)], [1, 2], caps=[0b10, 0b01], tasks=_far_board(T_HAND, {65: (0, 1, 0)}))
    s, r, st, d = _go(g, 2)
    np.testing.assert_array_equal(d["rows"]["status"][:, 0], [-1, 65 << 2 | TENTATIVE])
    assert r["task_counts"][:, 0].tolist() == [1, 0] and r["guard"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["neighbouring cells", "diagonal cells"])
def test_gpu_claimer_and_task_in_different_task_cells(where):
    # the grid's corner is the lowest task position, its cells `cell` wide: a border 3 cells in, the task 0.5
    # beyond it and the claimer 0.5 before it, on one axis or on both
    probe = _hand([(0, 0)], [1], tasks=[(0.0, 0.0, -1), (200.0, 200.0, -1)])
    s = _swarm(probe, "input", board=False)
    _board(s, probe, 1, 1)
    info = s.board["info"]
    cell = info["cell"]
    assert info["xmin"] == 0.0 and info["ymin"] == 0.0 and info["ncx"] >= 8
    b = 3 * cell
    diag = where == "diagonal cells"
    task = (b + 0.5, b + 0.5 if diag else b - 0.5)
    agent = (b - 0.5, b - 0.5)
    g = _hand([agent], [1], tasks=[(0.0, 0.0, -1), (200.0, 200.0, -1), (task[0], task[1], -1)])
    cx = lambda v: int(np.floor((v - 0.0) * (1.0 / cell)))  # noqa: E731
    assert cx(task[0]) == cx(agent[0]) + 1 and cx(task[1]) == cx(agent[1]) + int(diag)
    s, r, st, d = _go(g, 2)
    assert s.board["info"]["cell"] == cell
    np.testing.assert_array_equal(d["rows"]["status"], [[2 << 2 | TENTATIVE, -1, -1, -1]])
    np.testing.assert_array_equal(r["task_counts"], [[1, 0, 0], [0, 0, 0]])
    np.testing.assert_array_equal(d["rows"]["claim_out"], [[[-1] * 4], [[2, -1, -1, -1]]])


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 65, 1 << 24])
def test_gpu_smallest_board_first_size_past_the_words_and_largest_board(T):
    # the last task of the board 1.0 from the claimer, the others co-located far away
    tx, ty = np.full(T, 1.0e5), np.zeros(T)
    tx[T - 1] = 1.0
    g = _hand([(0, 0), (0, 2)], [1, 9], lead=(1,), tasks=[(1, 0, -1)])
    g.update(task_x=tx, task_y=ty, task_req=np.full(T, -1, np.int8))
    t0 = time.perf_counter()
    s, r, st, d = _go(g, 3, Ks=2, Kt=2)
    assert time.perf_counter() - t0 < 30.0
    k = T - 1
    # (the leader, sqrt 5 away, claimed it too: TENTATIVE, nobody arbitrates for it)
    np.testing.assert_array_equal(d["rows"]["status"], [[k << 2 | ASSIGNED, -1], [k << 2 | TENTATIVE, -1]])
    np.testing.assert_array_equal(d["rows"]["tab_task"], [[-1, -1], [k, -1]])
    np.testing.assert_array_equal(d["rows"]["tab_winner"], [[-1, -1], [1, -1]])
    np.testing.assert_array_equal(d["rows"]["tab_util"], np.array([[0, 0], [50, 0]], np.float32))
    np.testing.assert_array_equal(d["rows"]["conflict_out"], [[[-1, -1], [k, -1]], [[-1, -1], [-1, -1]]])
    np.testing.assert_array_equal(r["task_counts"], [[2, 0, 0], [0, 1, 1], [0, 0, 0]])
    assert s.board["info"]["T"] == T and s.board["info"]["longest"] == max(T - 1, 1)


# 5. chunks
@pytest.mark.gpu
@pytest.mark.parametrize("chunks", [(1, 1, 1, 1, 3, 8), (2, 2, 2, 9), (3, 12)])
def test_gpu_chunked_run_is_the_same_run(chunks):
    """From the hand-out on: the first claims leave at tick 45, the first conflicts at tick 46, so every
    boundary of the first chunks has claims or conflicts in flight, at odd and at even ticks."""
    import torch
    g = load_golden("loop_board_n200")
    first = int(g["task_tick"]) - 1
    a, b = _swarm(g, "spatial", board=False), _swarm(g, "spatial", board=False)
    for s in (a, b):
        _run_radio(s, g, first)
        _board(s, g, 48, 32)
    ra = _run(a, g, sum(chunks))
    rb = [_run(b, g, c) for c in chunks]
    assert ra["task_counts"][0, 0] > 0 and ra["task_counts"][1, 1] > 0 and ra["task_counts"][1, 2] > 0
    for t in ("pos", "pos_prev", "vel", "target", "has_target", "state", "leader"):
        assert torch.equal(getattr(a, t), getattr(b, t)), t
    for k in a.fsm:
        assert torch.equal(a.fsm[k], b.fsm[k]), k
    for k in ROWS:
        assert torch.equal(a.board[k].view(torch.int32), b.board[k].view(torch.int32)), k
    np.testing.assert_array_equal(ra["task_counts"], np.concatenate([r["task_counts"] for r in rb]))
    np.testing.assert_array_equal(ra["counts"], np.concatenate([r["counts"] for r in rb]))
    assert ra["guard"] == sum(r["guard"] for r in rb)


# 6. overflow is a refusal
@pytest.mark.gpu
@pytest.mark.parametrize("kind,Ks,Kt", [("status", 16, 32), ("table", 64, 4)])
def test_gpu_overflow_refuses_the_call_and_grow_board_repeats_it(oracle_mod, kind, Ks, Kt):
    import torch
    from swarm_amd import _lib
    g = _scattered_case()
    s = _swarm(g, "spatial", board=False)
    _board(s, g, Ks, Kt)
    want = _scattered_model(oracle_mod, s, g)
    col, cap = (0, Ks) if kind == "status" else (1, Kt)
    over = np.flatnonzero(want["peaks"][:, col] > cap)
    assert len(over) and (want["peaks"][:, 1 - col] <= (Kt if kind == "status" else Ks)).all()
    tick = int(over[0]) + 1  # the first tick at whose end the exact run holds more than the rows do
    b = s.board
    s._motion_state()
    keep = dict(pos=s.pos, pos_prev=s.pos.clone(), vel=s.vel, state=s.state, leader=s.leader, **s.fsm,
                **{k: b[k] for k in ROWS})
    s.pos_prev = keep["pos_prev"]
    s._pos_prev_key = (s.pos, s.pos._version)
    before = {k: v.clone() for k, v in keep.items()}
    with pytest.raises(_lib.SwarmError) as e:
        _run(s, g, int(g["ticks"]))
    assert e.value.code == _lib.ERR_RANGE and f"{kind} slots at tick {tick} " in str(e.value)
    assert s.last_refused_tick == tick and s.fsm_tick == 0
    okind, agent = s.last_board_overflow
    assert okind == kind and 0 <= agent < s.n
    for k, v in keep.items():
        assert torch.equal(v, before[k]), k
    # the named agent does hold more than the rows at the end of that tick of the exact run
    assert want["peaks"][tick - 1, col] > cap
    s.grow_board(status_slots=64, table_slots=32)
    assert s.board["status"].shape == (s.n, 64) and s.board["conflict_out"].shape == (2 * s.n, 32)
    r = _run(s, g, int(g["ticks"]))
    _check_scattered(s, r, want)
    assert s.last_refused_tick == -1 and s.last_board_overflow is None


# 7. a too-dense tick restores the sparse arrays with the rest
@pytest.mark.gpu
def test_gpu_too_dense_tick_leaves_every_sparse_array_as_it_was():
    import torch
    from swarm_amd import _lib
    from swarm_amd.swarm import Swarm
    n = 1_200_000
    rng = np.random.default_rng(2)
    x, y = 3.0 + rng.uniform(0, 1e-3, n), -2.0 + rng.uniform(0, 1e-3, n)
    s = Swarm(np.arange(n, dtype=np.int32), x, y, layout="input", device="cuda")
    s.protocol_reset(last_hb=np.full(n, -2.95))
    tx = np.full(65, 50.0)
    tx[64], tx[3] = 3.0, 4.0
    s.set_task_board(tx, np.full(65, -2.0), status_slots=1, table_slots=1)
    b = s.board
    b["status"][::2, 0] = 64 << 2 | 1
    b["claim_out"][::5, 0] = 64
    b["conflict_out"][::7, 0] = 3
    b["tab_task"][::4, 0] = 3
    b["tab_winner"][::4, 0] = 7
    b["tab_util"][::4, 0] = 33.0
    keep = dict(pos=s.pos, state=s.state, leader=s.leader, **s.fsm, **{k: b[k] for k in ROWS})
    before = {k: v.clone() for k, v in keep.items()}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with pytest.raises(_lib.SwarmError) as e:
        s.update_loop_board(3, 1.0, 1.0)
    torch.cuda.synchronize()
    assert time.perf_counter() - t0 < 20.0
    assert e.value.code == _lib.ERR_RANGE and "too dense" in str(e.value) and "tick 1" in str(e.value)
    assert s.last_refused_tick == 1 and s.fsm_tick == 0 and s.last_board_overflow is None
    for k, v in keep.items():
        assert torch.equal(v, before[k]), k


# 8. entry checks
@pytest.mark.gpu
@pytest.mark.parametrize("bad", ["task index T", "task index -7", "row out of order", "status code 0",
                                 "live entry behind an empty slot", "equal tasks in a row", "treq = 32"])
def test_gpu_bad_rows_are_refused_and_nothing_is_written(bad):
    import torch
    from swarm_amd import _lib
    T = 70
    g = _hand([(0, 0), (0, 2), (5, 5)], [1, 9, 4], lead=(1,), tasks=_far_board(T, {69: (1, 0, -1)}))
    s = _swarm(g, "input", board=False)
    if bad == "treq = 32":
        g["task_req"][5] = 32
        with pytest.raises(_lib.SwarmError) as e:
            _board(s, g, 4, 4)
        assert e.value.code == _lib.ERR_ARG and "[-1, 31]" in str(e.value) and not hasattr(s, "board")
        return
    _board(s, g, 4, 4)
    b = s.board
    b["status"][0, :2] = torch.tensor([3 << 2 | 2, 68 << 2 | 1])  # good rows first
    b["tab_task"][1, :2] = torch.tensor([3, 68])
    b["tab_winner"][1, :2] = torch.tensor([1, 1])
    if bad == "task index T":
        b["claim_out"][2 * 3 - 1, 0] = T
    elif bad == "task index -7":
        b["conflict_out"][1, 0] = -7
    elif bad == "row out of order":
        b["tab_task"][1, :2] = torch.tensor([68, 3])
    elif bad == "status code 0":
        b["status"][2, 0] = 5 << 2
    elif bad == "live entry behind an empty slot":
        b["status"][2, 1] = 5 << 2 | 1
    else:
        b["conflict_out"][4, :2] = torch.tensor([9, 9])
    keep = dict(pos=s.pos, state=s.state, **s.fsm, **{k: b[k] for k in ROWS})
    before = {k: v.clone() for k, v in keep.items()}
    with pytest.raises(_lib.SwarmError) as e:
        _run(s, g, 3)
    assert e.value.code == _lib.ERR_ARG and "sparse task row" in str(e.value)
    assert s.fsm_tick == 0 and s.last_refused_tick == -1
    for k, v in keep.items():
        assert torch.equal(v, before[k]), k


@pytest.mark.gpu
def test_gpu_good_caller_rows_are_taken_and_a_conflict_without_a_table_entry_locks_everyone():
    # agent 1 (a FOLLOWER now) sent a conflict on task 68 at tick 0, but its table has no entry for it: winner -1
    g = _hand([(0, 0), (0, 2)], [1, 9], tasks=_far_board(70, {}))
    s = _swarm(g, "input", board=False)
    _board(s, g, 2, 2)
    s.board["conflict_out"][1, 0] = 68  # parity 0, agent 1
    r = _run(s, g, 1)
    rows = _rows(s)
    np.testing.assert_array_equal(rows["status"], [[68 << 2 | LOCKED, -1], [-1, -1]])
    assert r["task_counts"].sum() == 0 and (rows["conflict_out"][1] == -1).all()


# 9. nothing to do: the radio loop, bit for bit
@pytest.mark.gpu
@pytest.mark.parametrize("board", ["out of reach", "T = 0"])
def test_gpu_idle_board_equals_the_radio_loop_on_a_twin_swarm(board):
    import torch
    g = load_golden("loop_tasks_n200")
    a, b = _swarm(g, "spatial", board=False), _swarm(g, "spatial", board=False)
    if board == "T = 0":
        a.set_task_board([], [])
    else:
        a.set_task_board(np.full(300, 1.0e4), np.linspace(-1.0e4, 1.0e4, 300), status_slots=1, table_slots=1)
    ra, rb = _run(a, g, 120), _run_radio(b, g, 120)
    for t in ("pos", "pos_prev", "vel", "target", "has_target", "state", "leader"):
        assert torch.equal(getattr(a, t), getattr(b, t)), t
    for k in a.fsm:
        assert torch.equal(a.fsm[k], b.fsm[k]), k
    np.testing.assert_array_equal(ra["counts"], rb["counts"])
    assert ra["singular"] == rb["singular"] and ra["task_counts"].sum() == 0 and ra["guard"] == 0
    assert all((a.board[k] == (0 if k == "tab_util" else -1)).all() for k in ROWS)


# 10. the handle: its grid as the C-ABI reports it, against numpy
@pytest.mark.gpu
def test_gpu_board_handle_reports_its_grid_and_cell_lists():
    from swarm_amd import _lib
    rng = np.random.default_rng(3)
    T = 777
    tx, ty = rng.uniform(-40.0, 90.0, T), rng.uniform(5.0, 60.0, T)
    g = _hand([(0, 0)], [1], tasks=[(0, 0, -1)])
    s = _swarm(g, "input", board=False)
    s.set_task_board(tx, ty, rng.integers(-1, 3, T), status_slots=1, table_slots=1)
    lib, h = _lib.lib(), s.board["handle"]
    d = _lib.BoardDesc()
    _lib.check(lib.swarm_board_info(h, ctypes.byref(d)))
    assert {k: getattr(d, k) for k, _ in _lib.BoardDesc._fields_} == s.board["info"]
    assert d.T == T and d.cell >= 5.0 * (1.0 + 1e-9) and d.xmin == tx.min() and d.ymin == ty.min()
    assert d.ncx == int(np.floor((tx.max() - tx.min()) / d.cell)) + 1 and d.ncx * d.ncy <= 4 * T + 1024
    off, idx = np.zeros(d.ncx * d.ncy + 1, np.uint32), np.zeros(T, np.int32)
    _lib.check(lib.swarm_board_read(h, off.ctypes.data_as(ctypes.c_void_p), idx.ctypes.data_as(ctypes.c_void_p)))
    inv = 1.0 / d.cell
    cx = np.minimum(np.floor((tx - d.xmin) * inv), d.ncx - 1).astype(np.int64)
    cy = np.minimum(np.floor((ty - d.ymin) * inv), d.ncy - 1).astype(np.int64)
    cell = cy * d.ncx + cx
    order = np.argsort(cell, kind="stable")  # cell by cell, ascending task index within a cell
    np.testing.assert_array_equal(idx, order)
    np.testing.assert_array_equal(off, np.searchsorted(cell[order], np.arange(d.ncx * d.ncy + 1)))
    assert d.longest == np.diff(off.astype(np.int64)).max()
    gone = ctypes.c_void_p(h.value)  # (compared with the live handles only, never dereferenced)
    s.set_task_board([1.0], [2.0])  # a new board replaces (and destroys) the old one
    assert lib.swarm_board_destroy(_lib.ctx(), gone) == _lib.ERR_ARG and "not a live board" in _lib.last_error()


# 11. the bridge
@pytest.mark.gpu
def test_gpu_write_back_board_fills_the_agent_objects():
    import types
    g = _hand([(0, 0), (0, 2)], [1, 9], lead=(1,), caps=[1, 0], tasks=[(1, 0, 0), (500, 0, -1)])
    s = _swarm(g, "spatial", board=False)
    agents = [types.SimpleNamespace(agent_id=int(i), tasks={10: {"status": "OPEN", "pos": (1.0, 0.0),
                                                                "required_cap": "extinguisher"},
                                                           20: {"status": "OPEN", "pos": (500.0, 0.0)}},
                                    task_claims={}) for i in g["ids"]]
    s.set_task_board(s.tasks_from_dict(agents[0].tasks), status_slots=2, table_slots=2)
    np.testing.assert_array_equal(s.board_task_ids, [10, 20])
    _run(s, g, 3)
    s.write_back_board(agents)
    assert [a.tasks[10]["status"] for a in agents] == ["ASSIGNED", "OPEN"]
    assert [a.tasks[20]["status"] for a in agents] == ["OPEN", "OPEN"]
    assert agents[0].task_claims == {} and agents[1].task_claims == {10: {"winner": 1, "utility": 50.0}}
    tt, tw, tu = s.board_tables()
    assert tuple(tt.shape) == (2, 2) and tuple(s.board_status().shape) == (2, 2)
