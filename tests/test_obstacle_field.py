"""Obstacle fields (contract O1; Swarm.obstacle_field, swarm_obstacle_field_create): the sensed
physics visits only the obstacles in an agent's reach, and every output keeps the flat list's bits.

The yardstick is the flat list: the CPU oracle's obstacle loop (oracle.physics, the loop models), which walks
all m obstacles for every agent, and a twin swarm on the GPU that is given the same obstacles as a list.  Every
comparison is bit for bit (numpy's assert_array_equal: NaN equals NaN).  The reference has no counterpart of the
field itself: its simulator hands every agent the obstacles it senses (update_sensors, agent.py:59-65).
"""
import numpy as np
import pytest
import torch

from rgg_brute import rgg_brute
from test_physics_sensed import KEYS, _assert_bits, _oracle_steps, _random_case, _result, _shift, _singular_case, _swarm
from test_update_loop_sensed import _assert_equal, _model_in_storage_order, _state
from test_update_loop_sensed import _random_case as _loop_case
from test_update_loop_tasks import _assert_tasks, _task_state
from loop_model import OUT_KEYS

pytestmark = pytest.mark.gpu
ALL = OUT_KEYS + ("px", "py")


def _obstacles(m, seed=3):
    """m obstacles uniform over [-10, 50]^2 (the agents live on [0, 40]^2), r in U(0.2, 2)."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-10, 50, m), rng.uniform(-10, 50, m), rng.uniform(0.2, 2, m)], 1).reshape(m, 3)


def _sensed(g, obstacles, radius, steps, layout="input", field=True):
    """A sensed run of `steps` steps on a fresh swarm; field: given an ObstacleField of the list, else the list."""
    s, li = _swarm(g, layout)
    obs = s.obstacle_field(obstacles) if field else obstacles
    r = s.physics_step(obs, leader_index=li, dt=float(g["dt"]), steps=steps, sense_radius=radius)
    return _result(s, r)


# ---------------------------------------------------------------- 1. sensed steps against the oracle
_oracle_cache = {}


def _oracle_in_storage_order(oracle_mod, g, layout, radius, steps):
    """_oracle_steps over the storage order of a swarm of that layout (the sensed neighbours are applied in
    ascending storage index: agent k of the run is input agent perm[k]), the results put back into input order."""
    perm = _swarm(g, layout)[0].perm.cpu().numpy().astype(np.int64)
    inv = np.empty(len(perm), np.int64)
    inv[perm] = np.arange(len(perm))
    q = dict(g)
    for k in ("ids", "state", "x", "y", "vx", "vy", "tx", "ty", "has_t"):
        q[k] = np.asarray(g[k])[perm]
    lead = np.asarray(g["leader"], np.int64)[perm]
    q["leader"] = np.where(lead >= 0, inv[np.maximum(lead, 0)], -1).astype(np.int32)
    o = _oracle_steps(oracle_mod, q, radius, steps, resense=True)
    out = {"singular": o["singular"]}
    for k in KEYS:
        out[k] = np.empty_like(o[k])
        out[k][perm] = o[k]
    return out


def _steps_case(oracle_mod, m, layout):
    if (m, layout) not in _oracle_cache:  # computed once, left unchanged
        g = _random_case(3000, 21, 40.0)
        g["obs"] = _obstacles(m)
        g = _shift(g, 10.0)
        _oracle_cache[m, layout] = (g, _oracle_in_storage_order(oracle_mod, g, layout, 1.0, 5))
    return _oracle_cache[m, layout]


@pytest.mark.parametrize("layout", ["input", "spatial"])
@pytest.mark.parametrize("m", [0, 1, 16, 1025, 5000])
def test_sensed_steps_with_a_field_match_the_oracle_and_the_flat_twin(oracle_mod, m, layout):
    g, want = _steps_case(oracle_mod, m, layout)
    got = _sensed(g, g["obs"], 1.0, 5, layout)
    assert got["steps_done"] == 5
    _assert_bits(got, want, f"m={m} against the oracle")
    assert got["singular"] == want["singular"]
    twin = _sensed(g, g["obs"], 1.0, 5, layout, field=False)
    _assert_bits(got, twin, f"m={m} against the flat twin")
    assert got["singular"] == twin["singular"]
    if m >= 1025:  # the obstacles really act: without them the moving agents end elsewhere
        none = _sensed(g, np.zeros((0, 3)), 1.0, 5, layout, field=False)
        moving = want["has_t"] != 0
        assert ((none["x"] != got["x"]) | (none["y"] != got["y"]))[moving].sum() >= 0.5 * moving.sum()


# ---------------------------------------------------------------- 2. hand-built boundaries
def _lists(name, rng):
    """The obstacle lists of tests/obstacle_cells/obstacle_cells_main.cpp, around [0, 40]^2."""
    sc = lambda m, lo, hi: np.stack([rng.uniform(lo, hi, m), rng.uniform(lo, hi, m), rng.uniform(0.2, 2, m)], 1)  # noqa: E731
    if name == "r1":
        return np.array([[20.0, 20.0, 1.0], [33.0, 9.0, 1.0]])
    if name == "radii":
        return np.concatenate([sc(12, 0, 40), [[10, 10, 0.0], [20, 12, -1.0], [30, 14, -5.0], [16, 30, -7.0],
                                               [22, 22, np.nextafter(-5.0, 0.0)]]])
    if name == "r300":
        return np.concatenate([sc(40, 0, 60), [[31.0, 29.0, 300.0]]])
    if name == "duplicates":
        o = sc(20, 0, 30)
        return np.concatenate([o, np.tile([[12.5, 7.25, 1.5]], (5, 1)), np.tile(o[:1], (3, 1))])
    if name == "one_line":
        k = np.arange(30.0)
        return np.stack([3.0 * k, np.full(30, 7.0), 0.5 + 0.05 * k], 1)
    if name == "all_dead":
        return np.array([[1.0, 2.0, -5.0], [3.0, 4.0, -7.0], [-2.0, 0.0, -1e6]])
    assert name == "empty"
    return np.zeros((0, 3))


def _boundary_agents(obs, info, rng):
    """Agent positions where a field can go wrong: the distance at which d is 5 (and one ulp either side), on an
    axis and on the diagonal; on every cell edge of the field's grid and one ulp either side; outside the
    field's box on all eight sides, next to it and 1e6 away; on an obstacle's centre; and a scatter."""
    up = lambda v: np.nextafter(v, np.inf)  # noqa: E731
    dn = lambda v: np.nextafter(v, -np.inf)  # noqa: E731
    pts = []
    for ox, oy, r in obs[:6]:
        reach = 5.0 + r  # d = sqrt(s2) - r is 5 at this distance
        if not reach > 0:
            continue
        for a in (reach, up(reach), dn(reach)):
            pts += [(ox + a, oy), (ox - a, oy), (ox, oy + a), (ox, oy - a)]
        q = reach * np.sqrt(0.5)
        for a in (q, up(q), dn(q)):
            pts += [(ox + a, oy + q), (ox - a, oy - q), (ox + q, oy - a)]
    x0, y0, c = info["xmin"], info["ymin"], info["cell"]
    x1, y1 = x0 + info["ncx"] * c, y0 + info["ncy"] * c
    near_y = obs[0, 1] if len(obs) else 0.5 * (y0 + y1)
    near_x = obs[0, 0] if len(obs) else 0.5 * (x0 + x1)
    for k in np.unique(np.linspace(0, info["ncx"], min(info["ncx"], 24) + 1).round()):
        e = x0 + k * c
        for v in (e, up(e), dn(e)):
            pts += [(v, near_y + 0.3), (v, rng.uniform(y0, y1))]
    for k in np.unique(np.linspace(0, info["ncy"], min(info["ncy"], 24) + 1).round()):
        e = y0 + k * c
        for v in (e, up(e), dn(e)):
            pts += [(near_x - 0.3, v), (rng.uniform(x0, x1), v)]
    mx, my = 0.5 * (x0 + x1), 0.5 * (y0 + y1)
    for d in (None, 1.0, 1e6):  # None: one ulp outside
        for sx in (-1, 0, 1):
            for sy in (-1, 0, 1):
                if sx or sy:
                    px = mx if sx == 0 else (dn(x0) if sx < 0 else up(x1)) if d is None else (x0 - d if sx < 0 else x1 + d)
                    py = my if sy == 0 else (dn(y0) if sy < 0 else up(y1)) if d is None else (y0 - d if sy < 0 else y1 + d)
                    pts.append((px, py))
    if len(obs):
        pts.append((obs[0, 0], obs[0, 1]))  # on a centre: a zero distance
        pts += [(ox + rng.uniform(-7, 7), oy + rng.uniform(-7, 7)) for ox, oy, _ in obs[:40] for _ in range(4)]
    pts += [(rng.uniform(x0 - 3, x1 + 3), rng.uniform(y0 - 3, y1 + 3)) for _ in range(300)]
    return np.array(pts, np.float64)


@pytest.mark.parametrize("shift", [0.0, 1e9])
@pytest.mark.parametrize("name", ["r1", "radii", "r300", "duplicates", "one_line", "all_dead", "empty"])
def test_hand_built_boundaries_match_the_oracles_flat_loop_and_the_flat_twin(oracle_mod, name, shift):
    from swarm_amd.swarm import Swarm
    rng = np.random.default_rng(8)
    obs = _lists(name, rng)
    obs[:, :2] += shift
    probe = Swarm(np.zeros(1, np.int32), np.zeros(1), np.zeros(1), layout="input", device="cuda")
    info = probe.obstacle_field(obs).info
    xy = _boundary_agents(obs, info, rng)
    n = len(xy)
    g = dict(ids=rng.permutation(n).astype(np.int32), state=np.full(n, 3, np.uint8), leader=np.full(n, -1, np.int32),
             x=xy[:, 0].copy(), y=xy[:, 1].copy(), vx=np.zeros(n), vy=np.zeros(n), tx=xy[:, 0] + 3.0,
             ty=xy[:, 1] - 2.0, has_t=np.ones(n, np.uint8), obs=obs, dt=np.float64(0.1))
    rp, col = rgg_brute(g["x"], g["y"], 1.0)  # (the ulp neighbours sense each other: the same on both sides)
    want = oracle_mod.physics(g["ids"], g["state"], g["leader"], g["x"], g["y"], g["vx"], g["vy"], g["tx"], g["ty"],
                              g["has_t"], obs, rp, col, 0.1, 5.0, 1, use_pow=False)
    got = _sensed(g, obs, 1.0, 1)
    twin = _sensed(g, obs, 1.0, 1, field=False)
    _assert_bits(got, twin, f"{name} against the flat twin")
    assert got["singular"] == twin["singular"]
    _assert_bits(got, want, f"{name} against the oracle")
    assert got["singular"] == want["singular"]
    if name in ("r1", "radii", "r300", "duplicates", "one_line"):
        assert got["singular"] >= 1  # the agent on a centre
        # at the distance where d is 5 the term is skipped, one ulp nearer it is applied: some agent of each
        # kind was there (the oracle decides which)
        free = oracle_mod.physics(g["ids"], g["state"], g["leader"], g["x"], g["y"], g["vx"], g["vy"], g["tx"], g["ty"],
                                  g["has_t"], np.zeros((0, 3)), rp, col, 0.1, 5.0, 1, use_pow=False)
        pushed = (free["x"] != want["x"]) | (free["y"] != want["y"])
        assert pushed.sum() >= 10 and (~pushed).sum() >= 10, (int(pushed.sum()), n)


# ---------------------------------------------------------------- 3. non-finite agents
def test_agents_left_non_finite_by_a_singular_step_keep_the_flat_twins_bits():
    g = _singular_case()
    g["obs"] = np.concatenate([g["obs"], _obstacles(60, seed=5) * [0.3, 0.3, 1.0] + [10.0, 10.0, 0.0]])
    one = _sensed(g, g["obs"], 2.5, 1)
    assert one["singular"] >= 3 and not np.isfinite(one["x"][5]) and not np.isfinite(one["x"][8])
    for steps in (1, 4):  # the singular step, then three further steps with NaN positions in the swarm
        got, twin = _sensed(g, g["obs"], 2.5, steps), _sensed(g, g["obs"], 2.5, steps, field=False)
        assert got["steps_done"] == twin["steps_done"] == steps
        _assert_bits(got, twin, f"steps={steps}")
        assert got["singular"] == twin["singular"]


# ---------------------------------------------------------------- 4. sizes
@pytest.mark.parametrize("n", [1, 255, 256, 257, 20001])
def test_swarm_sizes_around_a_workgroup(oracle_mod, n):
    # (the first n agents of a case of at least 300: a leader beyond them is no leader)
    g = _random_case(max(n, 300), 13, 40.0 if n > 300 else 12.0)
    g = {k: (v[:n].copy() if isinstance(v, np.ndarray) and v.ndim == 1 else v) for k, v in g.items()}
    g["leader"][g["leader"] >= n] = -1
    g["obs"] = _obstacles(40) * ([1.0, 1.0, 1.0] if n > 300 else [0.3, 0.3, 1.0])
    g["has_t"][0] = 1
    g = _shift(g, 10.0)
    got = _sensed(g, g["obs"], 1.0, 3, "spatial")
    twin = _sensed(g, g["obs"], 1.0, 3, "spatial", field=False)
    _assert_bits(got, twin, f"n={n} against the flat twin")
    assert got["singular"] == twin["singular"]
    if n <= 257:
        want = _oracle_in_storage_order(oracle_mod, g, "spatial", 1.0, 3)
        _assert_bits(got, want, f"n={n} against the oracle")
        assert got["singular"] == want["singular"]


# ---------------------------------------------------------------- 5. the update loops
def _loop_swarm(g):
    """A swarm for any of the loops: message graph, timers, targets, capabilities and the board."""
    from swarm_amd.swarm import Swarm
    s = Swarm(g["ids"], g["x"], g["y"], g["caps"], layout="spatial", device="cuda")
    s.set_graph(g["row_ptr"], g["col"])
    s.protocol_reset(tick_off=g["tick_off"], last_hb=g["last_hb0"])
    idx = np.flatnonzero(g["has_t"])
    s.set_target(g["tx"][idx], g["ty"][idx], index=idx)
    s.set_tasks(g["task_x"], g["task_y"], g["task_req"])
    return s


def _loop_run(s, g, kind, ticks, obstacles):
    kw = dict(obstacles=obstacles, kill_ticks=g["kill_ticks"], dt=float(g["dt"]), seed=int(g["seed"]),
              max_speed=float(g["max_speed"]))
    if kind == "sensed":
        return s.update_loop_sensed(ticks, 2.5, **kw)
    if kind == "radio":
        return s.update_loop_radio(ticks, 2.5, 2.5, **kw)
    if kind == "tasks":
        return s.update_loop_tasks(ticks, 2.5, 2.5, **kw)
    assert kind == "csr"
    return s.update_loop(ticks, **kw)


def _loop_case_2000():
    g = _loop_case(2000, 41, ticks=60, n_obs=300)
    rng = np.random.default_rng(6)
    lo, hi = g["x"].min(), g["x"].max()
    g.update(kill_ticks=np.array([20, 40], np.int64), caps=rng.integers(0, 8, 2000).astype(np.uint32),
             task_x=rng.uniform(lo, hi, 24), task_y=rng.uniform(lo, hi, 24),
             task_req=rng.integers(-1, 3, 24).astype(np.int8))
    return g


def _assert_same_loop(a, b, ra, rb, kind):
    _assert_equal(_state(a), _state(b), ALL)
    np.testing.assert_array_equal(ra["counts"], rb["counts"])
    assert ra["singular"] == rb["singular"] and a.fsm_tick == b.fsm_tick
    for k in a.fsm:
        assert torch.equal(a.fsm[k], b.fsm[k]), k
    if kind == "tasks":
        _assert_tasks(_task_state(a), _task_state(b))
        np.testing.assert_array_equal(ra["task_counts"], rb["task_counts"])
        assert ra["guard"] == rb["guard"]


def _join(parts):
    out = {"counts": np.concatenate([p["counts"] for p in parts]), "singular": sum(p["singular"] for p in parts)}
    if "task_counts" in parts[0]:
        out.update(task_counts=np.concatenate([p["task_counts"] for p in parts]), guard=sum(p["guard"] for p in parts))
    return out


@pytest.mark.parametrize("kind", ["sensed", "radio", "tasks"])
def test_loops_with_a_field_equal_a_twin_swarm_with_the_list_whole_and_in_chunks(kind):
    g = _loop_case_2000()
    flat, whole, chunked = _loop_swarm(g), _loop_swarm(g), _loop_swarm(g)
    field = whole.obstacle_field(g["obs"])
    r_flat = _loop_run(flat, g, kind, 60, g["obs"])
    r_whole = _loop_run(whole, g, kind, 60, field)
    _assert_same_loop(whole, flat, r_whole, r_flat, kind)
    parts = [_loop_run(chunked, g, kind, 25, field), _loop_run(chunked, g, kind, 35, field)]
    _assert_same_loop(chunked, flat, _join(parts), r_flat, kind)
    # the run is a real one: both kills found leaders, followers travelled, the obstacles pushed somebody
    st = _state(flat)
    assert (st["alive"] == 0).sum() >= 1 and ((st["x"] != g["x"]) | (st["y"] != g["y"])).sum() >= 500
    bare = _loop_swarm(g)
    _loop_run(bare, g, kind, 60, None)
    assert not torch.equal(bare.pos, flat.pos)
    if kind == "tasks":
        assert r_flat["task_counts"][:, 0].sum() >= 1


def test_sensed_loop_with_a_field_equals_the_model(oracle_mod):
    g = _loop_case(400, 43, ticks=30, n_obs=1100)
    from test_update_loop_sensed import _swarm as _sensed_loop_swarm
    s = _sensed_loop_swarm(g)
    want = _model_in_storage_order(oracle_mod, s, g)
    kw = dict(kill_ticks=g["kill_ticks"], dt=float(g["dt"]), seed=int(g["seed"]), max_speed=float(g["max_speed"]))
    r = s.update_loop_sensed(30, float(g["sense_radius"]), obstacles=s.obstacle_field(g["obs"]), **kw)
    _assert_equal(_state(s), want, ALL)
    np.testing.assert_array_equal(r["counts"], want["counts"])
    assert r["singular"] == want["singular"]


# ---------------------------------------------------------------- 6. the fixed-graph calls read the list
def test_fixed_graph_calls_given_a_field_equal_the_list():
    g = _shift(_random_case(3000, 21, 40.0), 10.0)
    g["obs"] = _obstacles(300) + [10.0, 10.0, 0.0]
    res = []
    for field in (True, False):
        s, li = _swarm(g, "spatial")
        s.build_graph(1.0)
        r = s.physics_step(s.obstacle_field(g["obs"]) if field else g["obs"], leader_index=li, steps=3)
        res.append(_result(s, r))
    _assert_bits(res[0], res[1], "physics_step")
    assert res[0]["singular"] == res[1]["singular"]
    g = _loop_case_2000()
    a, b = _loop_swarm(g), _loop_swarm(g)
    ra, rb = _loop_run(a, g, "csr", 30, a.obstacle_field(g["obs"])), _loop_run(b, g, "csr", 30, g["obs"])
    _assert_same_loop(a, b, ra, rb, "csr")


# ---------------------------------------------------------------- 7. the field itself
def _cell(v, vmin, cell, nc):
    """cell_coord's arithmetic (swarm_common.h) in numpy."""
    with np.errstate(invalid="ignore"):
        f = np.floor((v - vmin) * (1.0 / cell))
    return np.where(f >= 0.0, np.minimum(f, nc - 1), 0).astype(np.int64)


def _tiny_swarm():
    from swarm_amd.swarm import Swarm
    return Swarm(np.arange(4, dtype=np.int32), np.arange(4.0), np.zeros(4), layout="input", device="cuda")


def test_read_is_ascending_and_covers_a_brute_force_over_10000_probes():
    rng = np.random.default_rng(4)
    obs = np.concatenate([_obstacles(700), [[5.0, 5.0, -5.0], [7.0, 7.0, -9.0], [20.0, 20.0, 40.0]]])
    f = _tiny_swarm().obstacle_field(obs)
    off, idx = f.read()
    i = f.info
    assert (f.m, i["m"], i["live"]) == (703, 703, 701)
    assert len(off) == i["ncx"] * i["ncy"] + 1 and off[0] == 0 and off[-1] == len(idx) == i["pairs"]
    assert i["ncx"] * i["ncy"] <= 4 * i["live"] + 1024 and (np.diff(off.astype(np.int64)) >= 0).all()
    assert np.diff(off.astype(np.int64)).max() == i["longest"]
    lists = [idx[off[c]:off[c + 1]] for c in range(len(off) - 1)]
    assert all((np.diff(q) > 0).all() for q in lists)  # ascending, no duplicates
    np.testing.assert_array_equal(f.obstacles, obs)
    # the footprints: h = (5 + r)(1 + 1e-9), the grid starts at their lower-left corner
    rr = 5.0 + obs[:, 2]
    live = rr > 0
    h = rr[live] * (1.0 + 1e-9)
    assert i["xmin"] == (obs[live, 0] - h).min() and i["ymin"] == (obs[live, 1] - h).min()
    assert i["cell"] >= 2.0 * (5.0 * (1.0 + 1e-9))  # the start side, grown only by the cell cap
    assert not np.isin(np.flatnonzero(~live), idx).any()
    # covering: every obstacle that passes the flat loop's pre-test at a probe is in the list of the probe's cell
    px = np.concatenate([rng.uniform(-25, 65, 9000), rng.uniform(-1e3, 1e3, 600), rng.uniform(-1e7, 1e7, 400)])
    py = np.concatenate([rng.uniform(-25, 65, 9000), rng.uniform(-1e3, 1e3, 600), rng.uniform(-1e7, 1e7, 400)])
    c = _cell(py, i["ymin"], i["cell"], i["ncy"]) * i["ncx"] + _cell(px, i["xmin"], i["cell"], i["ncx"])
    ex, ey = px[:, None] - obs[None, live, 0], py[:, None] - obs[None, live, 1]
    passes = ~(ex * ex + ey * ey > (rr[live] * rr[live] * (1.0 + 1e-12))[None, :])
    member = np.zeros((len(off) - 1, len(obs)), bool)
    for k, q in enumerate(lists):
        member[k, q] = True
    assert passes.sum() >= 20000
    assert member[c][:, live][passes].all()


def test_the_field_copies_its_list():
    g = _shift(_random_case(500, 9, 30.0), 10.0)
    obs = torch.as_tensor(_obstacles(200) * [0.6, 0.6, 1.0] + [10.0, 10.0, 0.0], device="cuda")
    keep = obs.cpu().numpy().copy()
    s, li = _swarm(g)
    f = s.obstacle_field(obs)
    obs.fill_(1e3)  # the caller's tensor afterwards: the field does not see it
    np.testing.assert_array_equal(f.obstacles, keep)
    r = s.physics_step(f, leader_index=li, steps=2, sense_radius=1.0)
    _assert_bits(_result(s, r), _sensed(g, keep, 1.0, 2, field=False))


def test_bad_lists_raise_and_a_closed_field_raises():
    from swarm_amd import _lib
    s = _tiny_swarm().build_graph(1.0)
    bad = _obstacles(9)
    bad[4, 1] = np.nan
    with pytest.raises(_lib.SwarmError) as e:
        s.obstacle_field(bad)
    assert e.value.code == _lib.ERR_ARG and "not finite" in str(e.value)
    with pytest.raises(_lib.SwarmError) as e:
        s.obstacle_field(np.array([[-1e308, 0.0, 1.0], [1e308, 0.0, 1.0]]))
    assert e.value.code == _lib.ERR_ARG and "finite extent" in str(e.value)
    # more than 2^26 pairs: 224 obstacles of r = 1e6 among 200 000 small ones (tests/test_obstacle_cells.py)
    rng = np.random.default_rng(1)
    many = np.stack([rng.uniform(0, 1400, 200000), rng.uniform(0, 1400, 200000), rng.uniform(0.2, 2, 200000)], 1)
    many[np.arange(224) * 890, 2] = 1e6
    with pytest.raises(_lib.SwarmError) as e:
        s.obstacle_field(many)
    assert e.value.code == _lib.ERR_RANGE and "pairs" in str(e.value)
    f = s.obstacle_field(_obstacles(9))
    assert not f.closed
    f.close()
    f.close()  # twice is fine
    assert f.closed
    with pytest.raises(ValueError, match="closed"):
        f.read()
    for call in (lambda: s.physics_step(f, steps=1, sense_radius=1.0), lambda: s.physics_step(f),
                 lambda: s.update_loop_sensed(1, 1.0, obstacles=f), lambda: s.update_loop_radio(1, 1.0, 1.0, obstacles=f)):
        with pytest.raises(ValueError, match="closed"):
            call()


def test_70000_obstacles_of_r_1e6_raise():
    """70 000 obstacles of r = 1e6 raise ERR_RANGE by the pair count: the grid's start side does not grow with
    the radii, so the cell cap makes ~530 x 530 cells over the 2e6-wide box and every obstacle reaches them all
    (2e10 pairs against the limit 2^26)."""
    from swarm_amd import _lib
    rng = np.random.default_rng(1)
    huge = np.stack([rng.uniform(0, 1400, 70000), rng.uniform(0, 1400, 70000), np.full(70000, 1e6)], 1)
    with pytest.raises(_lib.SwarmError) as e:
        _tiny_swarm().obstacle_field(huge)
    assert e.value.code == _lib.ERR_RANGE and "pairs" in str(e.value)


def test_an_empty_field_works():
    g = _shift(_random_case(500, 9, 30.0), 10.0)
    s, li = _swarm(g)
    f = s.obstacle_field(np.zeros((0, 3)))
    assert f.m == 0 and f.info["live"] == 0 and (f.info["ncx"], f.info["ncy"], f.info["pairs"]) == (1, 1, 0)
    off, idx = f.read()
    assert off.tolist() == [0, 0] and len(idx) == 0
    r = s.physics_step(f, leader_index=li, steps=2, sense_radius=1.0)
    _assert_bits(_result(s, r), _sensed(g, np.zeros((0, 3)), 1.0, 2, field=False))
