"""Moving obstacles (contract O2): fields whose cell lists are rebuilt on the device every tick.

A moving field's tick is an O1 field of the list as it stands, and every obstacle then advances by fl(v * dt): a call
given a moving field must equal, bit for bit, the same entry point called one tick at a time with the current list as
a flat tensor, the list advanced by the caller in between (numpy float64: the product and the sum rounded
separately, as the contract says).  The device builder is held to the host builder's lists exactly
(refresh() + read() against a static field of positions()).  The sensed steps are held to the CPU oracle as well.
"""
import numpy as np
import pytest
import torch

from test_obstacle_field import _assert_same_loop, _join, _lists, _loop_case_2000, _loop_swarm
from test_physics_sensed import KEYS, _assert_bits, _random_case, _result, _rgg, _shift, _swarm

pytestmark = pytest.mark.gpu


def _advance(obs, vel, dt, times=1):
    """The contract's advance in numpy float64: x <- fl(x + fl(vx * dt)), r untouched."""
    obs = np.array(obs, np.float64, copy=True).reshape(-1, 3)
    step = np.asarray(vel, np.float64).reshape(-1, 2) * np.float64(dt)
    for _ in range(times):
        obs[:, :2] = obs[:, :2] + step
    return obs


def _tiny_swarm(n=1):
    from swarm_amd.swarm import Swarm
    return Swarm(np.arange(n, dtype=np.int32), np.zeros(n), np.zeros(n), layout="input", device="cuda")


# ---------------------------------------------------------------- 1. the device builder against the host builder
def _same_lists(moving, static):
    moving.refresh()
    for k in ("m", "live", "ncx", "ncy", "cell", "xmin", "ymin", "pairs", "longest"):
        assert moving.info[k] == static.info[k], (k, moving.info, static.info)
    (off_m, idx_m), (off_s, idx_s) = moving.read(), static.read()
    np.testing.assert_array_equal(off_m, off_s)
    np.testing.assert_array_equal(idx_m, idx_s)


def _random_list(m, rng):
    side = 20.0 + 3.0 * np.sqrt(m)
    return np.stack([rng.uniform(0, side, m), rng.uniform(0, side, m), rng.uniform(0.2, 2, m)], 1)


def _builder_case(obs):
    rng = np.random.default_rng(12)
    m = len(obs)
    vel = rng.uniform(-1, 1, (m, 2))
    vel *= rng.uniform(0, 8, (m, 1)) / np.maximum(np.hypot(vel[:, 0], vel[:, 1]), 1e-9)[:, None]  # speeds up to 8
    n = 256
    cx, cy = (obs[:, 0].mean(), obs[:, 1].mean()) if m else (0.0, 0.0)
    g = _random_case(n, 4, 30.0)
    g = _shift(g, 0.0)
    for k in ("x", "tx"):
        g[k] = g[k] - 15.0 + cx
    for k in ("y", "ty"):
        g[k] = g[k] - 15.0 + cy
    s, li = _swarm(g, "spatial")
    moving, static = s.obstacle_field(obs, vel), s.obstacle_field(obs)
    assert moving.moving and not static.moving
    _same_lists(moving, static)
    r = s.physics_step(moving, leader_index=li, dt=0.1, steps=10, sense_radius=1.0)
    assert r["steps_done"] == 10
    now = moving.positions()
    np.testing.assert_array_equal(now, _advance(obs, vel, 0.1, 10))
    np.testing.assert_array_equal(moving.obstacles, obs)  # .obstacles stays the creation list
    _same_lists(moving, s.obstacle_field(now))


@pytest.mark.parametrize("shift", [0.0, 1e9])
@pytest.mark.parametrize("name", ["r1", "radii", "r300", "duplicates", "one_line", "all_dead", "empty"])
def test_device_builder_equals_the_host_builder_on_hand_built_lists(name, shift):
    obs = _lists(name, np.random.default_rng(8))
    obs[:, :2] += shift
    _builder_case(obs)


@pytest.mark.parametrize("m", [1, 7, 1025, 20000])
def test_device_builder_equals_the_host_builder_on_random_lists(m):
    _builder_case(_random_list(m, np.random.default_rng(m)))


def test_device_builder_after_ten_ticks_of_a_sensed_loop():
    g = _loop_case_2000()
    rng = np.random.default_rng(3)
    vel = rng.uniform(-8, 8, (len(g["obs"]), 2))
    s = _loop_swarm(g)
    f = s.obstacle_field(g["obs"], vel)
    _run(s, g, "sensed", 10, f)
    now = f.positions()
    np.testing.assert_array_equal(now, _advance(g["obs"], vel, g["dt"], 10))
    _same_lists(f, s.obstacle_field(now))


# ---------------------------------------------------------------- 2. the loops
KINDS = ["sensed", "radio", "tasks", "radio_lossy", "tasks_lossy"]


def _run(s, g, kind, ticks, obstacles):
    kw = dict(obstacles=obstacles, kill_ticks=g["kill_ticks"], dt=float(g["dt"]), seed=int(g["seed"]),
              max_speed=float(g["max_speed"]))
    if kind == "sensed":
        return s.update_loop_sensed(ticks, 2.5, **kw)
    if kind.endswith("_lossy"):
        kw.update(loss=0.2, loss_seed=77)
    if kind.startswith("radio"):
        return s.update_loop_radio(ticks, 2.5, 2.5, **kw)
    return s.update_loop_tasks(ticks, 2.5, 2.5, **kw)


def _twin(g, kind, obs, schedule):
    """A swarm stepped one tick at a time with the list as a flat tensor, advanced here on the CPU; schedule:
    (ticks, velocities) legs.  Returns the swarm, the joined results and the final list."""
    s = _loop_swarm(g)
    obs = np.array(obs, np.float64, copy=True)
    parts = []
    for ticks, vel in schedule:
        for _ in range(ticks):
            parts.append(_run(s, g, kind, 1, torch.tensor(obs, device="cuda")))
            obs = _advance(obs, vel, g["dt"])
    return s, _join(parts), obs


def _cells(obs):
    return np.floor(obs[:, :2] / 10.0).astype(np.int64)


@pytest.mark.parametrize("kind", KINDS)
def test_loops_with_a_moving_field_equal_the_per_tick_flat_twin(kind):
    g = _loop_case_2000()
    m = len(g["obs"])
    rng = np.random.default_rng(17)
    v1, v2 = rng.uniform(-8, 8, (m, 2)), rng.uniform(-8, 8, (m, 2))
    base = "tasks" if kind.startswith("tasks") else kind
    # (a) one call, (b) the twin
    twin, r_twin, end = _twin(g, kind, g["obs"], [(40, v1)])
    whole = _loop_swarm(g)
    f = whole.obstacle_field(g["obs"], v1)
    r_whole = _run(whole, g, kind, 40, f)
    _assert_same_loop(whole, twin, r_whole, r_twin, base)
    np.testing.assert_array_equal(f.positions(), end)
    # (c) chunks of 7 + 8 + 25
    chunked = _loop_swarm(g)
    fc = chunked.obstacle_field(g["obs"], v1)
    parts = [_run(chunked, g, kind, t, fc) for t in (7, 8, 25)]
    _assert_same_loop(chunked, twin, _join(parts), r_twin, base)
    np.testing.assert_array_equal(fc.positions(), end)
    # (d) velocities switched between the chunks
    twin2, r_twin2, end2 = _twin(g, kind, g["obs"], [(7, v1), (8, v2), (25, v1)])
    sw = _loop_swarm(g)
    fs = sw.obstacle_field(g["obs"], v1)
    parts = []
    for t, v in ((7, v1), (8, v2), (25, v1)):
        fs.set_velocities(v)
        parts.append(_run(sw, g, kind, t, fs))
    _assert_same_loop(sw, twin2, _join(parts), r_twin2, base)
    np.testing.assert_array_equal(fs.positions(), end2)
    assert not np.array_equal(end, end2)
    # the run is a real one: a frozen list ends elsewhere, and obstacles changed cell
    frozen = _loop_swarm(g)
    _run(frozen, g, kind, 40, frozen.obstacle_field(g["obs"]))
    assert not torch.equal(frozen.pos, whole.pos)
    assert (_cells(end) != _cells(g["obs"])).any(axis=1).sum() >= 20


# ---------------------------------------------------------------- 3. sensed steps
def _steps_with_list(g, layout, steps, vel, single, max_speed=5.0):
    """physics_step(sense_radius=1.0) over `steps` steps: single False -- one call with a moving field; True --
    one step at a time with the advanced flat list."""
    s, li = _swarm(g, layout)
    kw = dict(leader_index=li, dt=float(g["dt"]), sense_radius=1.0, max_speed=max_speed)
    if not single:
        f = s.obstacle_field(g["obs"], vel)
        r = s.physics_step(f, steps=steps, **kw)
        return _result(s, r), f.positions()
    obs, sing = np.array(g["obs"], copy=True), 0
    for _ in range(steps):
        sing += s.physics_step(torch.tensor(obs, device="cuda"), steps=1, **kw)["singular"]
        obs = _advance(obs, vel, g["dt"])
    return _result(s, {"singular": sing, "steps_done": steps}), obs


def _oracle_moving(oracle_mod, g, layout, steps, vel, max_speed):
    """The oracle one step at a time with the list of that step, over the storage order of a swarm of that layout
    (test_obstacle_field._oracle_in_storage_order's permutation), the results put back into input order."""
    perm = _swarm(g, layout)[0].perm.cpu().numpy().astype(np.int64)
    inv = np.empty(len(perm), np.int64)
    inv[perm] = np.arange(len(perm))
    q = {k: np.asarray(g[k])[perm] for k in ("ids", "state", "x", "y", "vx", "vy", "tx", "ty", "has_t")}
    lead = np.asarray(g["leader"], np.int64)[perm]
    leader = np.where(lead >= 0, inv[np.maximum(lead, 0)], -1).astype(np.int32)
    cur, obs, sing = {k: q[k] for k in KEYS}, np.array(g["obs"], copy=True), 0
    for _ in range(steps):
        rp, col = _rgg(oracle_mod, cur["x"], cur["y"], 1.0)
        o = oracle_mod.physics(q["ids"], q["state"], leader, cur["x"], cur["y"], cur["vx"], cur["vy"], cur["tx"],
                               cur["ty"], cur["has_t"], obs, rp, col, float(g["dt"]), max_speed, 1, use_pow=False)
        sing += o.pop("singular")
        cur = o
        obs = _advance(obs, vel, g["dt"])
    out = {"singular": sing}
    for k in KEYS:
        out[k] = np.empty_like(cur[k])
        out[k][perm] = cur[k]
    return out


@pytest.mark.parametrize("max_speed", [5.0, 3.0])
def test_sensed_steps_with_a_moving_field_equal_single_steps_and_the_oracle(oracle_mod, max_speed):
    from test_obstacle_field import _obstacles
    g = _random_case(5000, 21, 40.0)
    g["obs"] = _obstacles(300)
    g = _shift(g, 10.0)
    vel = np.random.default_rng(23).uniform(-8, 8, (300, 2))
    got, end = _steps_with_list(g, "spatial", 12, vel, False, max_speed)
    twin, end_t = _steps_with_list(g, "spatial", 12, vel, True, max_speed)
    assert got["steps_done"] == 12
    _assert_bits(got, twin, "against 12 single steps")
    assert got["singular"] == twin["singular"]
    np.testing.assert_array_equal(end, end_t)
    want = _oracle_moving(oracle_mod, g, "spatial", 12, vel, max_speed)
    _assert_bits(got, want, "against the oracle, one step at a time")
    assert got["singular"] == want["singular"]
    still = _steps_with_list(g, "spatial", 12, np.zeros((300, 2)), False, max_speed)[0]
    assert ((still["x"] != got["x"]) | (still["y"] != got["y"])).sum() >= 50  # the motion matters


@pytest.mark.parametrize("n,steps", [(1, 3), (255, 4), (256, 5), (257, 6), (20001, 3)])
def test_swarm_sizes_around_a_workgroup(n, steps):
    from test_obstacle_field import _obstacles
    g = _random_case(max(n, 300), 13, 40.0 if n > 300 else 12.0)
    g = {k: (v[:n].copy() if isinstance(v, np.ndarray) and v.ndim == 1 else v) for k, v in g.items()}
    g["leader"][g["leader"] >= n] = -1
    g["obs"] = _obstacles(40) * ([1.0, 1.0, 1.0] if n > 300 else [0.3, 0.3, 1.0])
    g["has_t"][0] = 1
    g = _shift(g, 10.0)
    vel = np.random.default_rng(n).uniform(-8, 8, (40, 2))
    got, end = _steps_with_list(g, "spatial", steps, vel, single=False)
    twin, end_t = _steps_with_list(g, "spatial", steps, vel, single=True)
    _assert_bits(got, twin, f"n={n}")
    assert got["singular"] == twin["singular"] and got["steps_done"] == steps
    np.testing.assert_array_equal(end, end_t)


# ---------------------------------------------------------------- 4. zero velocities
@pytest.mark.parametrize("kind", KINDS)
def test_zero_velocities_equal_the_static_field_and_the_flat_list(kind):
    g = _loop_case_2000()
    base = "tasks" if kind.startswith("tasks") else kind
    a, b, c = _loop_swarm(g), _loop_swarm(g), _loop_swarm(g)
    f = a.obstacle_field(g["obs"], np.zeros((len(g["obs"]), 2)))
    ra = _run(a, g, kind, 30, f)
    rb = _run(b, g, kind, 30, b.obstacle_field(g["obs"]))
    rc = _run(c, g, kind, 30, g["obs"])
    _assert_same_loop(a, b, ra, rb, base)
    _assert_same_loop(a, c, ra, rc, base)
    np.testing.assert_array_equal(f.positions(), g["obs"])


# ---------------------------------------------------------------- 5. a hand-built pass
def test_one_obstacle_passing_one_resting_agent(oracle_mod):
    from swarm_amd.swarm import Swarm
    dt, ticks = 0.1, 60
    # the agent rests on its own target at (50, 50); the obstacle (r = 1) starts 20 units to the left on the
    # line y = 53 and passes at distance 3; a dead one (r = -6) moves straight over the agent
    obs0 = np.array([[30.0, 53.0, 1.0], [44.0, 50.0, -6.0]])
    vel = np.array([[8.0, 0.0], [2.0, 0.0]])
    s = Swarm(np.array([5], np.int32), np.array([50.0]), np.array([50.0]), layout="input", device="cuda")
    s.set_graph(np.zeros(2, np.int32), np.zeros(0, np.int32))
    s.protocol_reset()
    s.set_target(np.array([50.0]), np.array([50.0]))
    f = s.obstacle_field(obs0, vel)
    r = s.update_loop_sensed(ticks, 1.0, obstacles=f, dt=dt, trace_every=1)
    trace = r["trace"].cpu().numpy()[:, 0, :]
    # the oracle composed per tick: one agent, no neighbours, its own target; the obstacle list of that tick
    x, y, vx, vy = np.array([50.0]), np.array([50.0]), np.zeros(1), np.zeros(1)
    rp, col = np.zeros(2, np.int32), np.zeros(0, np.int32)
    obs, first, frames = obs0.copy(), None, []
    for t in range(ticks):
        o = oracle_mod.physics(np.array([5], np.int32), np.array([3], np.uint8), np.array([-1], np.int32), x, y, vx, vy,
                               np.array([50.0]), np.array([50.0]), np.ones(1, np.uint8), obs, rp, col, dt, 5.0, 1,
                               use_pow=False)
        free = oracle_mod.physics(np.array([5], np.int32), np.array([3], np.uint8), np.array([-1], np.int32), x, y, vx,
                                  vy, np.array([50.0]), np.array([50.0]), np.ones(1, np.uint8), np.zeros((0, 3)), rp,
                                  col, dt, 5.0, 1, use_pow=False)
        if first is None and (o["x"][0] != free["x"][0] or o["y"][0] != free["y"][0]):
            first = t
        x, y, vx, vy = o["x"], o["y"], o["vx"], o["vy"]
        frames.append((x[0], y[0]))
        obs = _advance(obs, vel, dt)
    frames = np.array(frames)
    assert first is not None and 5 <= first <= 30, first
    np.testing.assert_array_equal(trace[:first], np.tile([[50.0, 50.0]], (first, 1)))
    np.testing.assert_array_equal(trace, frames)
    assert (trace[first:] != 50.0).any()
    # the dead obstacle went over the agent (44 -> 56) and changed nothing; both advanced every tick
    np.testing.assert_array_equal(f.positions(), obs)
    assert f.positions()[1, 0] > 55.0


# ---------------------------------------------------------------- 6. refusals
def _pair_bound(obs, info):
    """csrc/obstacle_motion.h's capacity formula (obs_pair_capacity) on the grid `info` describes."""
    inv = 1.0 / info["cell"]
    h = (5.0 + obs[:, 2]) * (1.0 + 1e-9)
    live = (5.0 + obs[:, 2]) > 0

    def axis(vmin, nc):
        if not (abs(vmin) + (float(nc) + 2.0) * info["cell"]) * inv <= 2.0 ** 40:
            return np.full(len(obs), nc, np.int64)
        return np.minimum(np.floor(2.0 * h * inv) + 3.0, nc).astype(np.int64)
    return int((axis(info["xmin"], info["ncx"]) * axis(info["ymin"], info["ncy"]))[live].sum())


def test_bad_arguments_are_refused_with_nothing_written():
    from swarm_amd import _lib
    g = _loop_case_2000()
    m = len(g["obs"])
    s = _loop_swarm(g)
    vel = np.random.default_rng(1).uniform(-8, 8, (m, 2))
    for bad in (np.nan, np.inf, -np.inf):
        v = vel.copy()
        v[m // 2, 1] = bad
        with pytest.raises(_lib.SwarmError) as e:
            s.obstacle_field(g["obs"], v)
        assert e.value.code == _lib.ERR_ARG
    for shape in ((m, 3), (m - 1, 2), (2 * m,)):
        with pytest.raises(ValueError):
            s.obstacle_field(g["obs"], np.zeros(shape))
    f, static = s.obstacle_field(g["obs"], vel), s.obstacle_field(g["obs"])
    keep = dict(pos=s.pos, vel=s.vel, target=s.target, has_target=s.has_target, state=s.state, leader=s.leader, **s.fsm)
    before = {k: v.clone() for k, v in keep.items()}
    list0 = f.positions()

    def untouched():
        for k, v in keep.items():
            assert torch.equal(v, before[k]), k
        np.testing.assert_array_equal(f.positions(), list0)

    v = vel.copy()
    v[3, 0] = np.nan
    with pytest.raises(_lib.SwarmError) as e:
        f.set_velocities(v)
    assert e.value.code == _lib.ERR_ARG
    with pytest.raises(ValueError):
        f.set_velocities(np.zeros((m, 3)))
    with pytest.raises(ValueError):
        static.set_velocities(vel)
    untouched()
    # the velocities are the old ones still: one tick advances by them
    t = _loop_swarm(g)
    ft = t.obstacle_field(g["obs"], vel)
    with pytest.raises(_lib.SwarmError):
        ft.set_velocities(v)
    _run(t, g, "sensed", 1, ft)
    np.testing.assert_array_equal(ft.positions(), _advance(g["obs"], vel, g["dt"]))
    # the fixed-graph calls
    with pytest.raises(ValueError):
        s.physics_step(f)
    with pytest.raises(ValueError):
        s.update_loop(3, obstacles=f)
    untouched()
    # ... and the C-ABI under them (a sensor graph given, so that only the field is wrong)
    with torch.cuda.device(s.device):
        other = torch.empty_like(s.pos)
        li = s.leader_index()
        rc = _lib.lib().swarm_physics_step(
            _lib.ctx(), s.n, _lib.ptr(s.ids), _lib.ptr(s.state), _lib.ptr(li), _lib.ptr(s.pos), _lib.ptr(other),
            _lib.ptr(s.vel), _lib.ptr(s.target), _lib.ptr(s.has_target), f.m, f._ptr, _lib.ptr(s.row_ptr),
            _lib.ptr(s.col), 0.1, 5.0, None, _lib.stream())
    assert rc == _lib.ERR_ARG
    untouched()
    # a closed field
    f.close()
    for call in (f.positions, f.refresh, f.read, lambda: f.set_velocities(vel),
                 lambda: s.update_loop_sensed(1, 2.5, obstacles=f)):
        with pytest.raises(ValueError):
            call()
    for k, v in keep.items():
        assert torch.equal(v, before[k]), k


def test_create_is_refused_by_the_capacity_bound_where_the_static_field_is_not():
    from swarm_amd import _lib
    s = _tiny_swarm()
    rng = np.random.default_rng(9)
    # obstacles of r = 200 over [0, 1000]^2: about 142 x 142 cells of side 10 (the cell cap 4 m + 1024 is far away), a
    # footprint of 410 covers 42 of them per axis on average and at most 44 by the bound.  m from the header's
    # formula on that grid: the first m whose bound exceeds 2^26.
    cell = 10.0 * (1.0 + 1e-9)
    guess = dict(cell=cell, xmin=-205.0, ymin=-205.0, ncx=142, ncy=142)
    per = _pair_bound(np.array([[500.0, 500.0, 200.0]]), guess)
    m = 2 ** 26 // per + 1
    obs = np.stack([rng.uniform(0, 1000, m), rng.uniform(0, 1000, m), np.full(m, 200.0)], 1)
    static = s.obstacle_field(obs)  # accepted: its counted pairs are fewer
    assert static.info["cell"] == cell and min(static.info["ncx"], static.info["ncy"]) >= 44  # as guessed: 44 x 44
    assert static.info["pairs"] <= 2 ** 26 < _pair_bound(obs, static.info)
    assert _pair_bound(obs[:-1], static.info) <= 2 ** 26
    static.close()
    with pytest.raises(_lib.SwarmError) as e:
        s.obstacle_field(obs, np.zeros((m, 2)))
    assert e.value.code == _lib.ERR_RANGE
    f = s.obstacle_field(obs[:-1], np.zeros((m - 1, 2)))  # one obstacle fewer: at the bound, accepted
    assert f.moving and _pair_bound(obs[:-1], f.info) <= 2 ** 26
    f.close()


# ---------------------------------------------------------------- 7. a refused dense tick
def test_a_refused_dense_tick_leaves_the_list_as_it_was():
    from swarm_amd import _lib
    from swarm_amd.swarm import Swarm
    n = 1_200_000
    rng = np.random.default_rng(2)
    x, y = 3.0 + rng.uniform(0, 1e-3, n), -2.0 + rng.uniform(0, 1e-3, n)
    s = Swarm(np.arange(n, dtype=np.int32), x, y, layout="input", device="cuda")
    s.protocol_reset(last_hb=np.full(n, -2.95))
    s.set_target(np.full(n, 9.0), np.full(n, 9.0))
    s.vel.fill_(0.25)
    s.pos_prev = s.pos + 0.5
    s._pos_prev_key = (s.pos, s.pos._version)
    s.fsm["outbox"][::3] = 1
    obs = np.stack([rng.uniform(-10, 15, 16), rng.uniform(-15, 10, 16), rng.uniform(0.2, 2, 16)], 1)
    vel = rng.uniform(-8, 8, (16, 2))
    f = s.obstacle_field(obs, vel)
    keep = dict(pos=s.pos, pos_prev=s.pos_prev, vel=s.vel, target=s.target, has_target=s.has_target,
                state=s.state, leader=s.leader, **s.fsm)
    before = {k: v.clone() for k, v in keep.items()}
    with pytest.raises(_lib.SwarmError) as e:
        s.update_loop_radio(3, 1.0, 1.0, obstacles=f)
    assert e.value.code == _lib.ERR_RANGE and "too dense" in str(e.value)
    assert s.last_refused_tick == 1 and s.fsm_tick == 0
    for k, v in keep.items():
        assert torch.equal(v, before[k]), k
    np.testing.assert_array_equal(f.positions(), obs)
    # the same swarm through the sensed steps: the list advanced exactly steps_done times
    with pytest.raises(_lib.SwarmError) as e:
        s.physics_step(f, dt=0.1, steps=3, sense_radius=1.0)
    assert e.value.code == _lib.ERR_RANGE
    np.testing.assert_array_equal(f.positions(), _advance(obs, vel, 0.1, s.last_steps_done))
