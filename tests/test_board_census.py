"""Task census (contract U1-C): swarm_board_census / swarm_tasks_census,
Swarm.board_census() / Swarm.task_census().

The census is a transpose of the agents' task state into per-task records, every field a commutative integer
reduction: the GPU must equal tests/board_census_model.py (plain numpy, from the definition) bit for bit, applied to
board_dense() / task_status() + task_tables(), whatever the storage order.  The model itself is pinned to figures
counted from the committed reference fixtures and to a 4 x 3 case written out by hand.
"""
import ctypes

import numpy as np
import pytest

from conftest import load_golden
import board_census_model as bcm
from board_census_model import FIELDS
from test_update_loop_tasks import _kw, _swarm

OPEN, TENTATIVE, LOCKED, ASSIGNED = 0, 1, 2, 3


# ----------------------------------------------------------------------------- CPU

def test_exports_and_struct_size():
    from swarm_amd import _lib
    lib = _lib.load()
    for name in ("swarm_board_census", "swarm_tasks_census"):
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert ctypes.sizeof(_lib.Census) == 80 and _lib.CENSUS_FIELDS == FIELDS  # ten pointers, the model's order


def test_entry_points_refuse_bad_arguments_without_a_device():
    from swarm_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(8)  # never dereferenced: the arguments below are refused first
    state = _lib.BoardState(8, 8, None, fake, fake, fake, fake, None, None)
    out = _lib.Census(*[fake] * 10)
    total = ctypes.c_int64(7)

    def board(ctx=fake, n=4, ids=fake, bd=fake, st=state, o=out, holders=None, cap=0):
        return lib.swarm_board_census(ctx, n, ids, bd, ctypes.byref(st) if st is not None else None, None,
                                      ctypes.byref(o) if o is not None else None, holders, cap, ctypes.byref(total),
                                      None)

    def tasks(ctx=fake, n=4, ids=fake, T=8, arrays=(fake,) * 4, o=out, holders=None, cap=0):
        return lib.swarm_tasks_census(ctx, n, ids, T, *arrays, None, ctypes.byref(o) if o is not None else None,
                                      holders, cap, ctypes.byref(total), None)

    def refused(rc, text):
        assert rc == _lib.ERR_ARG and text in lib.swarm_last_error(), (rc, lib.swarm_last_error())

    for call in (board, tasks):
        refused(call(ctx=None), b"ctx is NULL")
        refused(call(o=None), b"out is NULL")
        refused(call(ids=None), b"ids is NULL")
        refused(call(n=-1), b"[0, 2^31)")
        refused(call(n=1 << 31), b"[0, 2^31)")
        refused(call(cap=-1), b"cap must not be negative")
        refused(call(holders=None, cap=5), b"holders is NULL")
        for k in range(10):
            refused(call(o=_lib.Census(*[None if j == k else fake for j in range(10)])), b"NULL census array")
    refused(board(bd=None), b"board is NULL")
    refused(board(st=None), b"state is NULL")
    for ks, kt in ((0, 8), (4097, 8), (8, 0), (8, 4097)):
        refused(board(st=_lib.BoardState(ks, kt, None, fake, fake, fake, fake, None, None)), b"[1, 4096]")
    for k in range(4):
        arrays = [None if j == k else fake for j in range(4)]
        refused(board(st=_lib.BoardState(8, 8, None, *arrays, None, None)), b"NULL board state array")
        refused(tasks(arrays=arrays), b"NULL task state array")
    for T in (-1, 65):
        refused(tasks(T=T), b"[0, 64]")
    assert total.value == 7  # a refused call writes nothing


def test_python_layer_refuses_without_a_device():
    from swarm_amd.swarm import Swarm
    s = Swarm.__new__(Swarm)
    s.n, s.device = 4, "cpu"
    with pytest.raises(RuntimeError, match="set_task_board"):
        s.board_census()
    with pytest.raises(RuntimeError, match="set_tasks"):
        s.task_census()
    s.board, s.tasks = dict(T=3), dict(T=3)
    with pytest.raises(RuntimeError, match="alive_only needs the protocol state"):
        s.board_census(alive_only=True)
    with pytest.raises(RuntimeError, match="alive_only needs the protocol state"):
        s.task_census(alive_only=True)
    assert s.board == dict(T=3) and s.tasks == dict(T=3)


def _by_hand(status, winner, ids, mask):
    """The four figures of the issue's table, counted agent by agent with sets -- not the model's code."""
    n, T = status.shape
    holders, winners = [set() for _ in range(T)], [set() for _ in range(T)]
    for i in range(n):
        if mask is not None and not mask[i]:
            continue
        for k in range(T):
            if status[i, k] == ASSIGNED:
                holders[k].add(int(ids[i]))
            if winner[i, k] >= 0:
                winners[k].add(int(winner[i, k]))
    return (sum(1 for h in holders if h), sum(1 for h in holders if len(h) >= 2), max(len(h) for h in holders),
            sum(1 for w in winners if len(w) >= 2))


@pytest.mark.parametrize("name,shape,want,dead,want_alive", [
    ("loop_board_n200", (200, 300), (140, 84, 8, 97), 124, (94, 41, 6, 3)),
    ("loop_moving_board_n200", (200, 300), (153, 101, 7, 111), 124, (108, 47, 6, 1)),
    ("loop_tasks_wide_n400", (400, 24), (11, 6, 11, 7), 172, (9, 4, 7, 0)),
])
def test_model_reproduces_the_fixture_figures(name, shape, want, dead, want_alive):
    g = load_golden(name)
    st, w, u, ids, alive = g["status_out"], g["tab_winner_out"], g["tab_util_out"], g["ids"], g["alive_out"]
    assert st.shape == shape and int((alive == 0).sum()) == dead
    for mask, figures in ((None, want), (alive, want_alive)):
        c = bcm.census(st, w, u, ids, mask)
        assert bcm.summary(c) == figures == _by_hand(st, w, ids, mask)
        assert len(c["holders"]) == c["assigned"].sum() and (c["tables"] > 0).sum() == (c["winner_lo"] >= 0).sum()
        assert ((c["holder_lo"] == c["holder_hi"]) == (c["assigned"] <= 1)).all()  # the IDs are distinct


def test_model_on_a_case_written_out_by_hand():
    f = np.float32
    up = np.nextafter(f(31.5), f(np.inf))
    ids = np.array([40, 10, 30, 5], np.int32)
    status = np.array([[ASSIGNED, TENTATIVE, OPEN], [ASSIGNED, LOCKED, OPEN], [LOCKED, LOCKED, OPEN],
                       [ASSIGNED, ASSIGNED, ASSIGNED]], np.uint8)
    winner = np.array([[30, 40, -1], [10, -1, -1], [-1, 30, -1], [5, 5, 5]], np.int32)
    util = np.array([[25.0, 31.5, 0], [25.0, 0, 0], [0, up, 0], [99.0, 99.0, 99.0]], f)
    # agent 3 (the lowest ID, the highest utility) masked out: task 0 an equal-utility tie (to the lowest winner),
    # task 1 two utilities 1 ulp apart (to the higher), task 2 empty
    c = bcm.census(status, winner, util, ids, np.array([1, 1, 1, 0], np.uint8))
    want = dict(tentative=[0, 1, 0], locked=[1, 2, 0], assigned=[2, 0, 0], tables=[2, 2, 0], holder_lo=[10, -1, -1],
                holder_hi=[40, -1, -1], winner_lo=[10, 30, -1], winner_hi=[30, 40, -1], best_winner=[10, 30, -1])
    for k, v in want.items():
        np.testing.assert_array_equal(c[k], np.array(v, np.int32), err_msg=k)
        assert c[k].dtype == np.int32
    np.testing.assert_array_equal(c["best_util"].view(np.uint32), np.array([25.0, up, 0.0], f).view(np.uint32))
    assert up != f(31.5) and c["best_util"].dtype == f
    np.testing.assert_array_equal(c["holders"], [[0, 10], [0, 40]])
    # counted, it wins every field it can
    c = bcm.census(status, winner, util, ids)
    want = dict(tentative=[0, 1, 0], locked=[1, 2, 0], assigned=[3, 1, 1], tables=[3, 3, 1], holder_lo=[5, 5, 5],
                holder_hi=[40, 5, 5], winner_lo=[5, 5, 5], winner_hi=[30, 40, 5], best_winner=[5, 5, 5])
    for k, v in want.items():
        np.testing.assert_array_equal(c[k], np.array(v, np.int32), err_msg=k)
    np.testing.assert_array_equal(c["best_util"], np.full(3, 99.0, f))
    np.testing.assert_array_equal(c["holders"], [[0, 5], [0, 10], [0, 40], [1, 5], [2, 5]])
    # the order of the images: negative values below positive ones, -0.0 below +0.0
    v = np.array([-np.inf, -3.0, -0.0, 0.0, 20.5, np.inf], f)
    assert (np.diff(bcm.util_image(v).astype(np.int64)) > 0).all()


# ----------------------------------------------------------------------------- GPU

def _np(c):
    return {k: v.cpu().numpy() for k, v in c.items()}


def _assert_census(got, want, holders=None):
    """Bit for bit; holders: whether the dict must hold the pairs."""
    got = _np(got) if not isinstance(next(iter(got.values())), np.ndarray) else got
    for k in FIELDS:
        a, w = got[k], want[k]
        assert a.dtype == w.dtype and a.shape == w.shape, k
        np.testing.assert_array_equal(a.view(np.uint32), w.view(np.uint32), err_msg=k)
    if holders is not None:
        assert ("holders" in got) == holders
    if "holders" in got:
        assert got["holders"].dtype == np.int32
        np.testing.assert_array_equal(got["holders"], want["holders"], err_msg="holders")


def _alive(s):
    return s.fsm["alive"].cpu().numpy()


def _board_model(s, alive_only=False):
    """The model on board_dense(), over the storage order; where a table holds an entry comes from tab_task."""
    st, w, u = (t.cpu().numpy() for t in s.board_dense())
    tt = s.board["tab_task"].cpu().numpy()
    entry = np.zeros(st.shape, bool)
    rows = np.repeat(np.arange(s.n), tt.shape[1]).reshape(tt.shape)
    entry[rows[tt >= 0], tt[tt >= 0]] = True
    return bcm.census(st, w, u, s.ids.cpu().numpy(), _alive(s) if alive_only else None, entry=entry)


def _tasks_model(s, alive_only=False):
    w, u = s.task_tables()
    return bcm.census(s.task_status().cpu().numpy(), w.cpu().numpy(), u.cpu().numpy(), s.ids.cpu().numpy(),
                      _alive(s) if alive_only else None)


def _check_board(s, want=None, want_alive=None):
    """board_census in its four forms against the model (or the dicts given); returns the two model dicts."""
    want = _board_model(s) if want is None else want
    want_alive = _board_model(s, True) if want_alive is None else want_alive
    _assert_census(s.board_census(), want, holders=False)
    _assert_census(s.board_census(holders=True), want, holders=True)
    _assert_census(s.board_census(alive_only=True), want_alive, holders=False)
    _assert_census(s.board_census(alive_only=True, holders=True), want_alive, holders=True)
    return want, want_alive


# 1. the board fixtures run to their end, both layouts; the same census after resort() and grow_board()
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["loop_board_n200", "loop_moving_board_n200"])
@pytest.mark.parametrize("layout", ["input", "spatial"])
def test_gpu_census_of_a_fixture_board_run(name, layout):
    g = load_golden(name)
    first, ticks = int(g["task_tick"]) - 1, int(g["ticks"])
    rc, rs = float(g["radio_radius"]), float(g["sense_radius"])
    s = _swarm(g, layout, board=False)
    if first:
        s.update_loop_radio(first, rc, rs, **_kw(g))
    vel = np.stack([g["task_vx"], g["task_vy"]], 1) if "task_vx" in g else None
    s.set_task_board(g["task_x"], g["task_y"], g["task_req"], status_slots=64, table_slots=32, velocities=vel)
    _assert_census(s.board_census(holders=True), bcm.census(np.zeros((s.n, 300), np.uint8), np.full((s.n, 300), -1),
                                                            np.zeros((s.n, 300)), g["ids"]))  # a fresh board
    s.update_loop_board(ticks - first, rc, rs, **_kw(g))
    want, want_alive = _check_board(s)
    assert 0 < want_alive["assigned"].sum() < want["assigned"].sum()
    if layout == "input":  # the fixture's own order: real agents, so the issue's figures
        _assert_census(want, bcm.census(g["status_out"], g["tab_winner_out"], g["tab_util_out"], g["ids"]))
        assert bcm.summary(want) == ((140, 84, 8, 97) if name == "loop_board_n200" else (153, 101, 7, 111))
    if layout == "spatial":  # the agents have moved: a new storage order, the same census
        s.resort()
        assert s.last_resort_moved > 0
        _check_board(s, want, want_alive)
        _check_board(s)
    s.grow_board(status_slots=66, table_slots=33)  # rows that are no multiple of four slots wide
    _check_board(s, want, want_alive)


# 2. the 64-task fixtures through update_loop_tasks + task_census and through a twin's board: equal
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["loop_tasks_n200", "loop_tasks_wide_n400"])
@pytest.mark.parametrize("layout", ["input", "spatial"])
def test_gpu_task_census_equals_the_board_census_of_a_twin(name, layout):
    g = load_golden(name)
    T, first, ticks = len(g["task_x"]), int(g["task_tick"]) - 1, int(g["ticks"])
    rc, rs = float(g["radio_radius"]), float(g["sense_radius"])
    a, b = _swarm(g, layout, board=False), _swarm(g, layout, board=False)
    for s in (a, b):
        if first:
            s.update_loop_radio(first, rc, rs, **_kw(g))
    a.set_tasks(g["task_x"], g["task_y"], g["task_req"])
    b.set_task_board(g["task_x"], g["task_y"], g["task_req"], status_slots=T, table_slots=T)
    a.update_loop_tasks(ticks - first, rc, rs, **_kw(g))
    b.update_loop_board(ticks - first, rc, rs, **_kw(g))
    for alive_only in (False, True):
        want = _tasks_model(a, alive_only)
        ca = a.task_census(alive_only=alive_only, holders=True)
        _assert_census(ca, want, holders=True)
        _assert_census(a.task_census(alive_only=alive_only), want, holders=False)
        cb = b.board_census(alive_only=alive_only, holders=True)
        _assert_census(cb, want, holders=True)
        assert want["assigned"].sum() > 0 and want["tables"].sum() > 0
    want = _tasks_model(a)
    if layout == "input":
        _assert_census(want, bcm.census(g["status_out"], g["tab_winner_out"], g["tab_util_out"], g["ids"]))
    if layout == "spatial":
        a.resort()
        _assert_census(a.task_census(holders=True), want, holders=True)
        _assert_census(_tasks_model(a), want)


# 3. hand-written rows, no loop run
UTILS = np.array([25.0, np.nextafter(np.float32(25.0), np.float32(np.inf)), 30.5, 30.5, 21.0, 77.25], np.float32)


def _hand_swarm(n, T, Ks, Kt, seed=1, layout="input"):
    """n agents with IDs that are a random permutation unrelated to the storage order, a board of T tasks."""
    from swarm_amd.swarm import Swarm
    rng = np.random.default_rng(seed)
    ids = (rng.permutation(n) * 3 + 7).astype(np.int32)
    s = Swarm(ids, rng.uniform(0, 30, n), rng.uniform(0, 30, n), layout=layout, device="cuda")
    s.protocol_reset()
    s.set_task_board(rng.uniform(0, 30, T), rng.uniform(0, 30, T), status_slots=Ks, table_slots=Kt)
    return s, rng


def _canonical(rng, n, T, K, fill):
    """(n, K) rows of distinct tasks, ascending, the empties (-1) last; about `fill` of the slots taken."""
    big = np.int64(1) << 40
    t = np.sort(rng.integers(0, T, (n, K)).astype(np.int64), axis=1)
    t[:, 1:][t[:, 1:] == t[:, :-1]] = big
    t[rng.random((n, K)) >= fill] = big
    t = np.sort(t, axis=1)
    t[t == big] = -1
    return t.astype(np.int32)


def _random_rows(s, rng, fill=0.6):
    """Canonical random rows into s.board; the winners are IDs of the swarm, the utilities come with ties and
    1-ulp neighbours; a third of the agents dead."""
    import torch
    b, n, T = s.board, s.n, s.board["T"]
    ids = s.ids.cpu().numpy()
    st = _canonical(rng, n, T, b["Ks"], fill)
    st = np.where(st >= 0, st << 2 | rng.integers(1, 4, st.shape).astype(np.int32), -1).astype(np.int32)
    tt = _canonical(rng, n, T, b["Kt"], fill)
    tw = np.where(tt >= 0, ids[rng.integers(0, n, tt.shape)], -1).astype(np.int32)
    tu = np.where(tt >= 0, UTILS[rng.integers(0, len(UTILS), tt.shape)], np.float32(0)).astype(np.float32)
    for k, v in (("status", st), ("tab_task", tt), ("tab_winner", tw), ("tab_util", tu)):
        b[k].copy_(torch.as_tensor(v))
    s.fsm["alive"].copy_(torch.as_tensor((rng.random(n) < 0.67).astype(np.uint8)))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1025])
def test_gpu_rows_of_one_slot_at_the_workgroup_edges(n):
    s, rng = _hand_swarm(n, 7, 1, 1, seed=n)
    empty = bcm.census(np.zeros((n, 7), np.uint8), np.full((n, 7), -1), np.zeros((n, 7)), s.ids.cpu().numpy())
    assert (empty["holder_lo"] == -1).all() and (empty["best_util"].view(np.uint32) == 0).all()
    _check_board(s, empty, empty)  # a fresh board: all zeros and -1
    _random_rows(s, rng, fill=0.9)
    want, _ = _check_board(s)
    assert n < 255 or (want["assigned"].max() >= 2 and (want["winner_lo"] != want["winner_hi"]).any())


@pytest.mark.gpu
@pytest.mark.parametrize("layout,Ks,Kt", [("input", 16, 16), ("spatial", 5, 3), ("spatial", 8, 6), ("input", 3, 12)])
def test_gpu_random_rows_with_ties_and_one_ulp_neighbours_across_workgroups(layout, Ks, Kt):
    s, rng = _hand_swarm(3000, 40, Ks, Kt, seed=Ks, layout=layout)
    _random_rows(s, rng)
    want, want_alive = _check_board(s)
    # 24 workgroups' worth of agents: every task meets both utilities of a tie and of a 1-ulp pair somewhere
    assert (want["tables"] > 100).all() and set(np.unique(want["best_util"])) == {np.float32(77.25)}
    u = s.board["tab_util"]
    u[u == 77.25] = 21.0  # now the best entries are the 30.5 ties: to the lowest winner of all workgroups
    want, _ = _check_board(s)
    tt, tw = s.board["tab_task"].cpu().numpy(), s.board["tab_winner"].cpu().numpy()
    lowest = np.full(40, 1 << 30)
    tied = u.cpu().numpy() == 30.5
    np.minimum.at(lowest, tt[tied], tw[tied])
    assert (want["best_util"] == 30.5).all() and (want["best_winner"] == lowest).all()
    assert (want["tables"] > 100).all() and (want["winner_hi"] > lowest).all()  # several name the tied utility
    u[u == 30.5] = 21.0  # and now 25.0 against its upper neighbour
    want, _ = _check_board(s)
    assert (want["best_util"] == UTILS[1]).all() and UTILS[1] > UTILS[0]


@pytest.mark.gpu
def test_gpu_one_agent_with_full_rows_of_4096_slots():
    import torch
    s, rng = _hand_swarm(1, 5000, 4096, 4096)
    tasks = np.sort(rng.choice(5000, 4096, replace=False)).astype(np.int32)
    s.board["status"].copy_(torch.as_tensor((tasks << 2 | rng.integers(1, 4, 4096)).astype(np.int32)[None]))
    s.board["tab_task"].copy_(torch.as_tensor(tasks[::-1].copy()[None]).flip(1))
    s.board["tab_winner"].fill_(int(s.ids[0]))
    s.board["tab_util"].copy_(torch.as_tensor(rng.uniform(21, 90, 4096).astype(np.float32)[None]))
    want, _ = _check_board(s)
    assert want["tables"].sum() == 4096 and (want["tentative"] + want["locked"] + want["assigned"]).sum() == 4096


@pytest.mark.gpu
def test_gpu_largest_board_with_entries_at_its_two_ends():
    import torch
    T = 1 << 24
    s, rng = _hand_swarm(3, T, 2, 2)
    ids = s.ids.cpu().numpy()
    last = T - 1
    # agent 0 holds both end tasks, agent 1 the last one, agent 2 is LOCKED on task 0; two tables name the last
    st = np.array([[0 << 2 | ASSIGNED, last << 2 | ASSIGNED], [last << 2 | ASSIGNED, -1], [0 << 2 | LOCKED, -1]], np.int32)
    tt = np.array([[0, last], [-1, -1], [last, -1]], np.int32)
    tw = np.array([[ids[1], ids[0]], [-1, -1], [ids[2], -1]], np.int32)
    tu = np.array([[40.0, 50.0], [0.0, 0.0], [50.0, 0.0]], np.float32)
    for k, v in (("status", st), ("tab_task", tt), ("tab_winner", tw), ("tab_util", tu)):
        s.board[k].copy_(torch.as_tensor(v))
    # the model on the two end columns; every task between them must read empty
    ends = bcm.census(np.array([[ASSIGNED, ASSIGNED], [OPEN, ASSIGNED], [LOCKED, OPEN]], np.uint8),
                      np.array([[ids[1], ids[0]], [-1, -1], [-1, ids[2]]], np.int32),
                      np.array([[40.0, 50.0], [0.0, 0.0], [0.0, 50.0]], np.float32), ids)
    c = s.board_census(holders=True)
    for k in FIELDS:
        a = c[k]
        assert a.shape == (T,)
        np.testing.assert_array_equal(a[[0, T - 1]].cpu().numpy().view(np.uint32), ends[k].view(np.uint32), err_msg=k)
        empty = 0 if k in FIELDS[:4] or k == "best_util" else -1
        assert bool((a[1:T - 1].view(torch.int32) == empty).all()), k
    np.testing.assert_array_equal(c["holders"].cpu().numpy(),
                                  [[0, ids[0]]] + sorted([last, i] for i in ids[:2].tolist()))
    assert ends["best_winner"][1] == min(ids[0], ids[2]) and ends["assigned"].tolist() == [1, 2]


@pytest.mark.gpu
def test_gpu_hot_task_locked_at_20000_agents():
    import torch
    n = 20004
    s, rng = _hand_swarm(n, 3, 1, 1)
    st = np.full((n, 1), 0 << 2 | LOCKED, np.int32)
    st[12345, 0] = 0 << 2 | ASSIGNED
    st[-3:, 0] = [2 << 2 | TENTATIVE, -1, 2 << 2 | LOCKED]
    s.board["status"].copy_(torch.as_tensor(st))
    ids = s.ids.cpu().numpy()
    for i, (w, u) in ((5, (ids[9], 30.0)), (9000, (ids[4], 31.0)), (19999, (ids[77], 31.0))):
        s.board["tab_task"][i, 0], s.board["tab_winner"][i, 0], s.board["tab_util"][i, 0] = 0, int(w), u
    want, _ = _check_board(s)
    assert want["locked"][0] == 20000 and want["assigned"][0] == 1 and want["holder_lo"][0] == ids[12345]
    assert want["tables"][0] == 3 and want["best_winner"][0] == min(ids[4], ids[77])
    assert want["winner_lo"][0] == min(ids[[9, 4, 77]]) and want["winner_hi"][0] == max(ids[[9, 4, 77]])


@pytest.mark.gpu
def test_gpu_more_distinct_tasks_in_one_workgroup_than_its_table_holds():
    import torch
    n, K = 256, 64
    T = n * K
    s, rng = _hand_swarm(n, T, K, K)
    tasks = np.sort(rng.permutation(T).astype(np.int32).reshape(n, K), axis=1)  # pairwise distinct
    ids = s.ids.cpu().numpy()
    s.board["status"].copy_(torch.as_tensor(tasks << 2 | rng.integers(1, 4, (n, K)).astype(np.int32)))
    other = np.sort(rng.permutation(T).astype(np.int32).reshape(n, K), axis=1)
    s.board["tab_task"].copy_(torch.as_tensor(other))
    s.board["tab_winner"].copy_(torch.as_tensor(ids[rng.integers(0, n, (n, K))]))
    s.board["tab_util"].copy_(torch.as_tensor(UTILS[rng.integers(0, len(UTILS), (n, K))]))
    s.fsm["alive"][::3] = 0
    want, _ = _check_board(s)
    assert ((want["tentative"] + want["locked"] + want["assigned"]) == 1).all() and (want["tables"] == 1).all()


# 4. rows that are not canonical (a table entry has no status code: its fourth defect is a task held twice)
@pytest.mark.gpu
@pytest.mark.parametrize("where,defect", [
    ("status", "task index T"), ("status", "code 0"), ("status", "descending row"), ("status", "hole before an entry"),
    ("tab_task", "task index T"), ("tab_task", "task twice"), ("tab_task", "descending row"),
    ("tab_task", "hole before an entry")])
def test_gpu_bad_rows_are_refused_and_the_state_is_untouched(where, defect):
    import torch
    from swarm_amd import _lib
    T = 70
    s, rng = _hand_swarm(700, T, 8, 8, seed=3)
    _random_rows(s, rng, fill=0.5)
    sh, code = (2, ASSIGNED) if where == "status" else (0, 0)
    row = {"task index T": [T << sh | code], "code 0": [5 << 2], "task twice": [5, 5],
           "descending row": [9 << sh | code, 4 << sh | code], "hole before an entry": [-1, 9 << sh | code]}[defect]
    s.board[where][611] = -1
    s.board[where][611, :len(row)] = torch.as_tensor(row, dtype=torch.int32, device="cuda")
    before = {k: v.clone() for k, v in s.board.items() if isinstance(v, torch.Tensor)}
    for kw in (dict(), dict(holders=True), dict(alive_only=True)):
        with pytest.raises(_lib.SwarmError) as e:
            s.board_census(**kw)
        assert e.value.code == _lib.ERR_ARG and "strictly ascending" in str(e.value)
    for k, v in before.items():
        assert torch.equal(v.view(torch.int32), s.board[k].view(torch.int32)), k
    s.board[where][611] = -1  # the row emptied: the census is back
    if where == "tab_task":
        s.board["tab_winner"][611], s.board["tab_util"][611] = -1, 0.0
    _check_board(s)


@pytest.mark.gpu
def test_gpu_a_board_of_another_ctx_and_a_dead_board_are_refused():
    from swarm_amd import _lib
    s, rng = _hand_swarm(10, 5, 2, 2)
    b = s.board
    other = _lib.Ctx()
    out = {k: s.board_census()[k] for k in FIELDS}
    cs = _lib.Census(*[_lib.ptr(out[k]) for k in FIELDS])
    bs = _lib.BoardState(2, 2, None, *[_lib.ptr(b[k]) for k in ("status", "tab_task", "tab_winner", "tab_util")],
                         None, None)

    def call(ctx, handle):
        return _lib.lib().swarm_board_census(ctx, s.n, _lib.ptr(s.ids), handle, ctypes.byref(bs), None,
                                             ctypes.byref(cs), None, 0, None, _lib.stream())
    assert call(_lib.ctx(), b["handle"]) == 0
    assert call(other, b["handle"]) == _lib.ERR_ARG and "not a live board" in _lib.last_error()
    handle = ctypes.c_void_p(b["handle"].value)
    s.set_task_board([1.0], [1.0])  # destroys the first board
    assert call(_lib.ctx(), handle) == _lib.ERR_ARG and "not a live board" in _lib.last_error()


# 5. the holder pairs
@pytest.mark.gpu
@pytest.mark.parametrize("form", ["board", "tasks"])
def test_gpu_holder_buffer_smaller_than_the_total(form):
    import torch
    from swarm_amd import _lib
    n, T, cap, guard = 3000, 4, 100, 64
    s, rng = _hand_swarm(n, T, 2, 1, seed=11)
    codes = rng.integers(1, 4, n).astype(np.int32)
    codes[:1500] = ASSIGNED
    task = rng.integers(0, T, n).astype(np.int32)
    if form == "board":
        st = np.full((n, 2), -1, np.int32)
        st[:, 0] = task << 2 | codes
        s.board["status"].copy_(torch.as_tensor(st))
        bs = _lib.BoardState(2, 1, None, *[_lib.ptr(s.board[k]) for k in ("status", "tab_task", "tab_winner",
                                                                          "tab_util")], None, None)
        want = _board_model(s)
    else:
        s.set_tasks(np.arange(T, dtype=np.float64), np.zeros(T))
        bit = np.uint64(1) << task.astype(np.uint64)
        s.tasks["status_lo"].copy_(torch.as_tensor(np.where(codes & 1, bit, 0).astype(np.uint64).view(np.int64)))
        s.tasks["status_hi"].copy_(torch.as_tensor(np.where(codes & 2, bit, 0).astype(np.uint64).view(np.int64)))
        want = _tasks_model(s)
    total_want = int(want["assigned"].sum())
    assert total_want >= 1500 > T + 1024 > cap
    out = {k: torch.empty(T, dtype=torch.float32 if k == "best_util" else torch.int32, device="cuda")
           for k in FIELDS}
    cs = _lib.Census(*[_lib.ptr(out[k]) for k in FIELDS])
    buf = torch.full((cap + guard, 2), -777, dtype=torch.int32, device="cuda")
    total = ctypes.c_int64(-1)
    if form == "board":
        rc = _lib.lib().swarm_board_census(_lib.ctx(), n, _lib.ptr(s.ids), s.board["handle"], ctypes.byref(bs), None,
                                           ctypes.byref(cs), _lib.ptr(buf), cap, ctypes.byref(total), _lib.stream())
    else:
        b = s.tasks
        rc = _lib.lib().swarm_tasks_census(_lib.ctx(), n, _lib.ptr(s.ids), T, _lib.ptr(b["status_lo"]),
                                           _lib.ptr(b["status_hi"]), _lib.ptr(b["tab_winner"]),
                                           _lib.ptr(b["tab_util"]), None, ctypes.byref(cs), _lib.ptr(buf), cap,
                                           ctypes.byref(total), _lib.stream())
    assert rc == 0 and total.value == total_want
    _assert_census(out, want)
    got = buf.cpu().numpy()
    assert (got[cap:] == -777).all()  # the guard region behind the buffer
    true = {tuple(p) for p in want["holders"].tolist()}
    pairs = [tuple(p) for p in got[:cap].tolist()]
    assert len(set(pairs)) == cap and set(pairs) <= true  # exactly cap pairs, each a true one
    c = s.board_census(holders=True) if form == "board" else s.task_census(holders=True)
    _assert_census(c, want, holders=True)  # Swarm repeats the call with the exact count
    assert c["holders"].shape == (total_want, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["board", "tasks"])
def test_gpu_more_holders_in_one_workgroup_than_it_stages(form):
    """Every slot ASSIGNED: 128 agents of one workgroup hold 2048 (board) / some 4000 (tasks) pairs, more than
    a workgroup collects before its one add to the cursor -- the others take the cursor wave by wave."""
    import torch
    n, T = 300, 64
    s, rng = _hand_swarm(n, T, 16, 1, seed=12)
    if form == "board":
        tasks = np.sort(np.argsort(rng.random((n, T)), axis=1)[:, :16], axis=1).astype(np.int32)
        s.board["status"].copy_(torch.as_tensor(tasks << 2 | ASSIGNED))
        census, want = s.board_census, _board_model(s)
    else:
        s.set_tasks(np.arange(T, dtype=np.float64), np.zeros(T))
        words = rng.integers(0, 1 << 62, n, dtype=np.int64) & rng.integers(0, 1 << 62, n, dtype=np.int64) | 0xFFFFF
        s.tasks["status_lo"].copy_(torch.as_tensor(words))
        s.tasks["status_hi"].copy_(torch.as_tensor(words))
        census, want = s.task_census, _tasks_model(s)
    assert want["assigned"].sum() >= n * 16
    _assert_census(census(holders=True), want, holders=True)
    s.fsm["alive"][1::2] = 0
    _assert_census(census(holders=True, alive_only=True), (_board_model if form == "board" else _tasks_model)(s, True),
                   holders=True)


# 6. read-only
@pytest.mark.gpu
def test_gpu_census_writes_nothing_of_the_swarm():
    import torch
    g = load_golden("loop_tasks_n200")
    rc, rs = float(g["radio_radius"]), float(g["sense_radius"])
    s = _swarm(g, "spatial")  # holds the 64-task board; the sparse one next to it
    s.set_task_board(g["task_x"], g["task_y"], g["task_req"], status_slots=24, table_slots=24)
    s.update_loop_radio(int(g["task_tick"]) - 1, rc, rs, **_kw(g))
    s.update_loop_tasks(60, rc, rs, **_kw(g))
    s.update_loop_board(60, rc, rs, **_kw(g))

    def tensors():
        out = dict(pos=s.pos, ids=s.ids, state=s.state, leader=s.leader)
        for name in ("fsm", "board", "tasks"):
            out.update({f"{name}.{k}": v for k, v in getattr(s, name).items() if isinstance(v, torch.Tensor)})
        return out
    before = {k: (v, v.data_ptr(), v.clone()) for k, v in tensors().items()}
    attrs = set(vars(s))
    for kw in (dict(), dict(holders=True), dict(alive_only=True, holders=True)):
        cb, ct = s.board_census(**kw), s.task_census(**kw)
        assert cb["assigned"].sum() > 0 and ct["assigned"].sum() > 0
    assert set(vars(s)) == attrs
    now = tensors()
    assert set(now) == set(before) and len(before) >= 25
    for k, (t, p, v) in before.items():
        assert now[k] is t and t.data_ptr() == p and torch.equal(t.view(torch.uint8), v.view(torch.uint8)), k
