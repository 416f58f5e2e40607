"""Physics steps that sense their neighbours from the moving positions (contract S1,
swarm_physics_run_sensed; Swarm.physics_step(sense_radius=R)).

The reference's simulator refreshes every agent's neighbour list before each tick.  The CPU reference
here is that loop over the oracle: per step oracle.rgg_csr on the step's positions, then one
oracle.physics step on that graph (x*x arithmetic, the GPU's).  The sensed GPU run must give its bits.
orc_rgg_csr indexes cells from floor(x / r) >= 0, so every oracle-checked input is shifted to keep all
coordinates positive over the run (motion is <= max_speed * dt = 0.5 a step).
"""
import time

import numpy as np
import pytest
import torch

KEYS = ("x", "y", "vx", "vy", "tx", "ty", "has_t")


def _random_case(n, seed, side, m_obs=16):
    """tests/test_physics.py's _random_case (the same draws in the same order), without its graph."""
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(0, side, n), rng.uniform(0, side, n)
    ids = rng.permutation(n).astype(np.int32)
    state = np.where(rng.uniform(size=n) < 0.02, 3, 1).astype(np.uint8)
    leaders = np.nonzero(state == 3)[0]
    leader = np.where((state == 1) & (rng.uniform(size=n) < 0.7), rng.choice(leaders, n), -1).astype(np.int32)
    has_t = (rng.uniform(size=n) < 0.3).astype(np.uint8)
    tx, ty = rng.uniform(0, side, n), rng.uniform(0, side, n)
    obs = np.stack([rng.uniform(0, side, m_obs), rng.uniform(0, side, m_obs), rng.uniform(0.2, 2, m_obs)], 1)
    return dict(ids=ids, state=state, leader=leader, x=x, y=y, vx=np.zeros(n), vy=np.zeros(n), tx=tx, ty=ty,
                has_t=has_t, obs=obs, dt=np.float64(0.1))


def _shift(g, d):
    g = {k: np.array(v, copy=True) for k, v in g.items()}
    for k in ("x", "y", "tx", "ty"):
        g[k] = g[k] + d
    g["obs"][:, :2] += d
    return g


def _rgg(oracle_mod, x, y, radius):
    """oracle.rgg_csr of the positions moved next to the origin: orc_rgg_csr allocates a cell for every
    radius x radius square between the origin and the farthest agent (1e12 of them at a shift of 1e6).
    The corner c is a whole number below every coordinate, so x - c is exact, and so is every difference
    (x[i] - c) - (x[j] - c) = x[i] - x[j] the rule squares: the same graph."""
    c = max(np.floor(min(x.min(), y.min())) - 10.0, 0.0)
    return oracle_mod.rgg_csr(x - c, y - c, radius)


def _oracle_steps(oracle_mod, g, radius, steps, resense):
    """`steps` oracle steps; resense: the graph of every step's own positions (contract S1), else
    the step-0 graph for all of them (what physics_step does without sense_radius)."""
    cur = {k: g[k] for k in KEYS}
    sing = 0
    rp = col = None
    for s in range(steps):
        if resense or s == 0:
            rp, col = _rgg(oracle_mod, cur["x"], cur["y"], radius)
        o = oracle_mod.physics(g["ids"], g["state"], g["leader"], cur["x"], cur["y"], cur["vx"], cur["vy"],
                               cur["tx"], cur["ty"], cur["has_t"], g["obs"], rp, col, float(g["dt"]), 5.0, 1,
                               use_pow=False)
        sing += o.pop("singular")
        cur = o
    cur["singular"] = sing
    return cur


def _swarm(g, layout="input"):
    from swarm_amd.swarm import Swarm
    s = Swarm(g["ids"], g["x"], g["y"], layout=layout, device="cuda")
    st = lambda a, dt: s._storage(np.ascontiguousarray(a), dt)  # noqa: E731
    s.state = st(g["state"], torch.uint8)
    s.vel = torch.stack([st(g["vx"], torch.float64), st(g["vy"], torch.float64)], 1).contiguous()
    s.target = torch.stack([st(g["tx"], torch.float64), st(g["ty"], torch.float64)], 1).contiguous()
    s.has_target = st(g["has_t"], torch.uint8)
    perm = s.perm.cpu().numpy().astype(np.int64)  # storage k holds input agent perm[k]
    inv = np.empty(len(perm), np.int64)
    inv[perm] = np.arange(len(perm))
    lead = np.asarray(g["leader"], np.int64)[perm]
    li = np.where(lead >= 0, inv[np.maximum(lead, 0)], -1).astype(np.int32)
    return s, torch.as_tensor(li, device="cuda")


def _result(s, r):
    p, v, t = s.to_input_order(s.pos), s.to_input_order(s.vel), s.to_input_order(s.target)
    return dict(x=p[:, 0], y=p[:, 1], vx=v[:, 0], vy=v[:, 1], tx=t[:, 0], ty=t[:, 1],
                has_t=s.to_input_order(s.has_target), singular=r["singular"], steps_done=r.get("steps_done"))


def _gpu_sensed(g, radius, steps, layout="input"):
    s, li = _swarm(g, layout)
    r = s.physics_step(g["obs"], leader_index=li, dt=float(g["dt"]), steps=steps, sense_radius=radius)
    return _result(s, r)


def _assert_bits(got, want, what=""):
    for k in KEYS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{k} {what}")


# ---------------------------------------------------------------- 1. step-by-step parity
@pytest.mark.gpu
@pytest.mark.parametrize("radius", [1.0, 1.5, 2.5])
@pytest.mark.parametrize("n,seed,side", [(2000, 1, 25.0), (5000, 1, 40.0), (3000, 3, 60.0)])
def test_sensed_steps_match_the_resensing_oracle_loop(oracle_mod, n, seed, side, radius):
    g = _shift(_random_case(n, seed, side), 10.0)
    want = _oracle_steps(oracle_mod, g, radius, 4, resense=True)
    frozen = _oracle_steps(oracle_mod, g, radius, 4, resense=False)
    # a build-once implementation cannot pass: the frozen step-0 graph ends elsewhere
    moving = want["has_t"] != 0
    differs = (frozen["x"] != want["x"]) | (frozen["y"] != want["y"])
    assert differs[moving].sum() >= 0.5 * moving.sum(), (int(differs[moving].sum()), int(moving.sum()))
    got = _gpu_sensed(g, radius, 4)
    assert got["steps_done"] == 4
    _assert_bits(got, want)
    assert got["singular"] == 0 and want["singular"] == 0


# ---------------------------------------------------------------- 2. radius boundary, close pairs
def _lattice_case(shift):
    """The lattice of test_gpu_physics_lattice_and_close_pairs_match_oracle: spacing 0.5, so pairs lie
    exactly at distance R = 1.0 (s2 == R * R) and same-row / same-column offsets are exactly 0 (the
    library path); plus 60 near-coincident agents at 3e-4, 1e-9 and 1e-6..1e-3."""
    side = 40
    gx, gy = np.meshgrid(np.arange(side) * 0.5, np.arange(side) * 0.5)
    x, y = gx.ravel().astype(np.float64), gy.ravel().astype(np.float64)
    rng = np.random.default_rng(17)
    pick = rng.choice(x.size, 60, replace=False)
    close = np.concatenate([np.full(20, 3e-4), np.full(20, 1e-9), rng.uniform(1e-6, 1e-3, 20)])
    x = np.concatenate([x, x[pick] + close])
    y = np.concatenate([y, y[pick] + close[::-1]])
    g = _random_case(len(x), 5, 20.0, m_obs=4)
    g["x"], g["y"] = x + shift, y + shift
    g["tx"], g["ty"] = g["x"] + 3.0, g["y"] - 2.0
    g["obs"][:, :2] += shift
    return g


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [10.0, 1.0e6])
def test_sensed_lattice_at_the_radius_and_close_pairs_match_oracle(oracle_mod, shift):
    g = _lattice_case(shift)
    rp, _ = _rgg(oracle_mod, g["x"], g["y"], 1.0)
    if shift == 10.0:  # 0.5 k + 10 is exact: an interior lattice agent senses the 12 others within 1.0
        assert np.diff(rp)[: 40 * 40].max() >= 12  # (4 of them exactly at 1.0)
    want = _oracle_steps(oracle_mod, g, 1.0, 2, resense=True)
    got = _gpu_sensed(g, 1.0, 2)
    _assert_bits(got, want, f"shift={shift}")
    assert got["singular"] == want["singular"]


# ---------------------------------------------------------------- 3. many contributors
@pytest.mark.gpu
def test_sensed_dense_block_merges_all_nine_window_cells_in_index_order(oracle_mod):
    """A 6 x 6 block at spacing 0.3 in a sparse background, R = 2.5: every block agent senses the 35
    others (all but the far corners within the 2.0 personal space).  A unit lattice of 100 agents around
    the block puts at least one agent into every cell (2.0 wide, wherever the grid's origin falls) of
    every block agent's 3 x 3 window, and block and lattice sit at scattered storage indices, so the
    ascending order only comes out of a merge over all nine runs."""
    n = 1500
    g = _random_case(n, 11, 60.0, m_obs=4)
    rng = np.random.default_rng(5)
    pick = rng.permutation(n)
    blk, lat = pick[:36], pick[36:136]
    bx, by = np.meshgrid(np.arange(6) * 0.3, np.arange(6) * 0.3)
    g["x"][blk], g["y"][blk] = 27.3 + bx.ravel(), 31.2 + by.ravel()
    lx, ly = np.meshgrid(23.05 + np.arange(10.0), 26.95 + np.arange(10.0))
    g["x"][lat], g["y"][lat] = lx.ravel(), ly.ravel()
    g["has_t"][blk] = 1
    g["state"][blk], g["leader"][blk] = 3, -1  # the block keeps the random targets: it stays a block
    g = _shift(g, 10.0)
    rp, _ = _rgg(oracle_mod, g["x"], g["y"], 2.5)
    assert np.diff(rp)[blk].min() >= 35
    want = _oracle_steps(oracle_mod, g, 2.5, 2, resense=True)
    got = _gpu_sensed(g, 2.5, 2)
    _assert_bits(got, want)
    assert got["singular"] == 0 and want["singular"] == 0
    # the block's separation terms are really summed: a run that senses nobody ends elsewhere
    none = _gpu_sensed(g, 1e-6, 2)
    assert np.all((none["x"][blk] != got["x"][blk]) | (none["y"][blk] != got["y"][blk]))


# ---------------------------------------------------------------- 4. against the two-call GPU path
def _big_case(n=200_000, seed=4, half=150.0):
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(-half, half, n), rng.uniform(-half, half, n)
    ids = rng.permutation(n).astype(np.int32)
    state = np.where(rng.uniform(size=n) < 0.02, 3, 1).astype(np.uint8)
    leaders = np.nonzero(state == 3)[0]
    leader = np.where((state == 1) & (rng.uniform(size=n) < 0.7), rng.choice(leaders, n), -1).astype(np.int32)
    has_t = (rng.uniform(size=n) < 0.3).astype(np.uint8)
    tx, ty = rng.uniform(-half, half, n), rng.uniform(-half, half, n)
    obs = np.stack([rng.uniform(-half, half, 16), rng.uniform(-half, half, 16), rng.uniform(0.2, 2, 16)], 1)
    return dict(ids=ids, state=state, leader=leader, x=x, y=y, vx=np.zeros(n), vy=np.zeros(n), tx=tx, ty=ty,
                has_t=has_t, obs=obs, dt=np.float64(0.1))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["input", "spatial"])
def test_sensed_run_equals_build_graph_plus_step_on_the_gpu(layout):
    g = _big_case()
    a, li_a = _swarm(g, layout)
    a.build_graph(1.0)
    rp0, col0, rp_keep, col_keep = a.row_ptr, a.col, a.row_ptr.clone(), a.col.clone()
    ra = a.physics_step(g["obs"], leader_index=li_a, steps=3, sense_radius=1.0)
    assert ra["steps_done"] == 3
    assert a.row_ptr is rp0 and a.col is col0
    assert torch.equal(a.row_ptr, rp_keep) and torch.equal(a.col, col_keep)
    b, li_b = _swarm(g, layout)
    sing = 0
    for _ in range(3):
        b.build_graph(1.0)
        sing += b.physics_step(g["obs"], leader_index=li_b, steps=1)["singular"]
    assert ra["singular"] == sing
    got, want = _result(a, ra), _result(b, {"singular": sing})  # through to_input_order
    _assert_bits(got, want, layout)
    moved = (got["x"] != g["x"]) | (got["y"] != g["y"])
    assert moved.sum() >= 0.7 * len(moved)  # followers travel to their formation slots
    for t in ("pos", "vel", "target", "has_target"):
        assert torch.equal(getattr(a, t), getattr(b, t)), t


# ---------------------------------------------------------------- 5. singular
def _singular_case():
    """test_physics.py's _singular_case, shifted: an agent on an obstacle centre, two on each other."""
    g = _random_case(300, 7, 12.0, m_obs=4)
    g["obs"][0, :2] = g["x"][5], g["y"][5]
    g["x"][9], g["y"][9] = g["x"][8], g["y"][8]
    for k in (5, 8, 9):
        g["has_t"][k] = 1
        g["state"][k] = 3
    return _shift(g, 10.0)


@pytest.mark.gpu
def test_sensed_singular_step_matches_oracle_and_later_steps_stay_safe(oracle_mod):
    g = _singular_case()
    want = _oracle_steps(oracle_mod, g, 2.5, 1, resense=True)
    assert want["singular"] >= 3 and not np.isfinite(want["x"][5]) and not np.isfinite(want["x"][8])
    got = _gpu_sensed(g, 2.5, 1)
    assert got["singular"] == want["singular"]
    _assert_bits(got, want)
    more = _gpu_sensed(g, 2.5, 3)  # non-finite agents in steps 2 and 3: the call returns
    assert more["steps_done"] == 3 and more["singular"] >= want["singular"]
    # an agent out of everyone's reach of the non-finite ones still moves as if they were absent
    assert np.isfinite(more["x"][g["has_t"] != 0]).sum() >= 0.9 * (g["has_t"] != 0).sum()


# ---------------------------------------------------------------- 6. too dense
@pytest.mark.gpu
def test_sensed_refuses_co_located_agents_before_scanning():
    from swarm_amd import _lib
    from swarm_amd.swarm import Swarm
    n = 1_200_000
    rng = np.random.default_rng(2)
    x, y = 3.0 + rng.uniform(0, 1e-3, n), -2.0 + rng.uniform(0, 1e-3, n)
    s = Swarm(np.arange(n, dtype=np.int32), x, y, layout="input", device="cuda")
    s.vel = torch.zeros((n, 2), dtype=torch.float64, device="cuda")
    s.target = torch.ones((n, 2), dtype=torch.float64, device="cuda")
    s.has_target = torch.ones(n, dtype=torch.uint8, device="cuda")
    before = s.pos.clone()
    li = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    t0 = time.perf_counter()
    with pytest.raises(_lib.SwarmError) as e:
        s.physics_step(leader_index=li, steps=3, sense_radius=1.0)
    torch.cuda.synchronize()
    assert time.perf_counter() - t0 < 20.0
    assert e.value.code == _lib.ERR_RANGE and "too dense" in str(e.value)
    assert s.last_steps_done == 0
    assert torch.equal(s.pos, before)
    assert not s.vel.any()


# ---------------------------------------------------------------- 7. empty and trivial
@pytest.mark.gpu
def test_sensed_empty_swarm_zero_steps_and_no_targets():
    from swarm_amd.swarm import Swarm
    e = Swarm(np.zeros(0, np.int32), np.zeros(0), np.zeros(0), layout="input", device="cuda")
    r = e.physics_step(leader_index=np.zeros(0, np.int32), steps=2, sense_radius=1.0)
    assert r == {"singular": 0, "steps_done": 2} and e.pos.shape == (0, 2)  # nothing to do: all steps "ran"
    g = _shift(_random_case(500, 9, 10.0), 10.0)
    s, li = _swarm(g)
    before = s.pos.clone()
    r = s.physics_step(g["obs"], leader_index=li, steps=0, sense_radius=1.0)
    assert r == {"singular": 0, "steps_done": 0} and torch.equal(s.pos, before)
    s.has_target.zero_()
    none = torch.full_like(li, -1)
    for steps in (1, 2):  # either parity of the double buffer
        r = s.physics_step(g["obs"], leader_index=none, steps=steps, sense_radius=1.0)
        assert r == {"singular": 0, "steps_done": steps} and torch.equal(s.pos, before)
    assert not s.vel.any()


# ---------------------------------------------------------------- 8. without a GPU
def test_sensed_entry_point_rejects_a_null_ctx_without_gpu():
    from swarm_amd import _lib
    L = _lib.load()
    rc = L.swarm_physics_run_sensed(None, 4, None, None, None, None, None, None, None, 0, None, 1.0, 1, 0.1, 5.0,
                                    None, None, None)
    assert rc == _lib.ERR_ARG
    assert b"ctx is NULL" in L.swarm_last_error()


def test_physics_step_refuses_sensors_with_sense_radius():
    from swarm_amd.swarm import Swarm
    s = Swarm.__new__(Swarm)  # no device needed: the keywords are checked before anything else
    with pytest.raises(ValueError, match="sensors must be None"):
        s.physics_step(sensors=(np.zeros(1, np.int32), np.zeros(0, np.int32)), sense_radius=1.0)
    assert Swarm.physics_step.__kwdefaults__["sense_radius"] is None
