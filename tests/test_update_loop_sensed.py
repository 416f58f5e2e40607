"""The update loop that re-senses its separation neighbours every tick (contract U1-S):
swarm_update_loop_sensed / Swarm.update_loop_sensed(ticks, R).

tests/golden/loop_sensed_*.npz were produced by real SwarmAgent objects whose update_sensors was fed, every
tick, the agents within R of that tick's snapshot (tools/gen_golden_loop_sensed.py).  The CPU model
(tests/loop_sensed_model.py) must reproduce them bit for bit with the reference's libm pow; the GPU must equal
the same model with its own x*x squares bit for bit -- the model run over the GPU's storage order, since the
sensed neighbours are applied in ascending storage index -- and the fixture itself in everything the squares
cannot reach.
"""
import ctypes
import time

import numpy as np
import pytest

from conftest import load_golden
import loop_sensed_model
from loop_model import FSM_KEYS, OUT_KEYS, F

SENSED = ("loop_sensed_n200", "loop_sensed_r12_n250", "loop_sensed_wide_n400")
# what the arithmetic of the squares cannot reach: the FSM's decisions do not depend on positions
EXACT = ("state", "leader", "last_hb", "wait_start", "delay", "has_lpos", "alive")
PER_AGENT = ("ids", "x", "y", "tick_off", "last_hb0", "tx", "ty", "has_t")


# ----------------------------------------------------------------------------- CPU

@pytest.mark.parametrize("name", SENSED)
def test_model_with_pow_equals_the_reference_fixture(oracle_mod, name):
    g = load_golden(name)
    o = loop_sensed_model.run(oracle_mod, g, use_pow=True)
    for k in OUT_KEYS:  # the thirteen arrays
        np.testing.assert_array_equal(o[k], g[k + "_out"], err_msg=k)
    np.testing.assert_array_equal(o["counts"], g["counts"])
    assert o["singular"] == 0


@pytest.mark.parametrize("name", SENSED)
def test_fixtures_tell_resensing_from_a_frozen_graph(oracle_mod, name):
    g = load_golden(name)
    frozen = loop_sensed_model.run(oracle_mod, g, use_pow=True, resense=False)
    differs = (frozen["x"] != g["x_out"]) | (frozen["y"] != g["y_out"])
    assert 2 * differs.sum() >= len(differs), (int(differs.sum()), len(differs))


def test_entry_point_rejects_a_null_ctx_without_gpu():
    from swarm_amd import _lib
    L = _lib.load()
    rc = L.swarm_update_loop_sensed(None, 4, None, None, None, None, None, None, None, None, None, 0, 1, 0.1, 3.0,
                                    0.2, ctypes.c_uint64(0), None, 0, 0.125, None, None, None, 0, None, 2.5, 5.0,
                                    None, 0, None, None, None, None)
    assert rc == _lib.ERR_ARG
    assert b"ctx is NULL" in L.swarm_last_error()


def test_update_loop_sensed_refuses_sensors_without_a_device():
    from swarm_amd.swarm import Swarm
    s = Swarm.__new__(Swarm)  # no device needed: the keywords are checked before anything else
    with pytest.raises(ValueError, match="sensors must be None"):
        s.update_loop_sensed(3, 1.0, sensors=(np.zeros(1, np.int32), np.zeros(0, np.int32)))
    with pytest.raises(ValueError, match="sensors must be None"):
        s.update_loop_sensed(3, sense_radius=1.0, sensors=(np.zeros(1, np.int32), np.zeros(0, np.int32)))
    with pytest.raises(TypeError):
        s.update_loop_sensed(3)  # the radius has no default


# ----------------------------------------------------------------------------- GPU

def _swarm(g, layout="spatial"):
    from swarm_amd.swarm import Swarm
    s = Swarm(g["ids"], g["x"], g["y"], layout=layout, device="cuda")
    s.set_graph(g["row_ptr"], g["col"])
    s.protocol_reset(tick_off=g["tick_off"], last_hb=g["last_hb0"])
    idx = np.flatnonzero(g["has_t"])
    s.set_target(g["tx"][idx], g["ty"][idx], index=idx)
    return s


def _run(s, g, ticks, **kw):
    """update_loop_sensed at the case's radius, or at sense_radius=...; sense_radius=None: update_loop."""
    radius = kw.pop("sense_radius", float(g["sense_radius"]))
    kw.update(obstacles=g["obs"], kill_ticks=g["kill_ticks"], dt=float(g["dt"]), seed=int(g["seed"]),
              max_speed=float(g["max_speed"]))
    return s.update_loop(ticks, **kw) if radius is None else s.update_loop_sensed(ticks, radius, **kw)


def _state(s):
    f = s.fsm
    t = dict(state=s.state, leader=s.leader, last_hb=f["last_hb"], wait_start=f["wait_start"], delay=f["delay"],
             has_lpos=f["has_leader_pos"], lpos=f["leader_pos"], alive=f["alive"], has_t=s.has_target)
    out = {k: s.to_input_order(v) for k, v in t.items()}
    for kx, ky, v in (("x", "y", s.pos), ("vx", "vy", s.vel), ("tx", "ty", s.target), ("px", "py", s.pos_prev)):
        a = s.to_input_order(v)
        out[kx], out[ky] = a[:, 0], a[:, 1]
    return out


def _model_in_storage_order(oracle_mod, s, g, ticks=None, **kw):
    """The model run over s's storage order (agent k of the run is input agent perm[k]; the message graph as s
    holds it), its per-agent results put back into input order."""
    perm = s.perm.cpu().numpy().astype(np.int64)
    q = dict(g)
    for k in PER_AGENT:
        q[k] = np.asarray(g[k])[perm]
    if "fsm0" in g:
        q["fsm0"] = {k: np.asarray(v)[perm] for k, v in g["fsm0"].items()}
    q["row_ptr"], q["col"] = s.row_ptr.cpu().numpy().astype(np.int64), s.col.cpu().numpy()
    o = loop_sensed_model.run(oracle_mod, q, ticks, **kw)
    out = {}
    for k, v in o.items():
        if isinstance(v, np.ndarray) and k != "counts":
            out[k] = np.empty_like(v)
            out[k][perm] = v
        else:
            out[k] = v
    return out


def _assert_equal(got, want, keys=OUT_KEYS):
    for k in keys:  # bit for bit; NaN == NaN (a singular tick leaves non-finite values on both sides)
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


_models = {}


# 1. fixtures
@pytest.mark.gpu
@pytest.mark.parametrize("name", SENSED)
@pytest.mark.parametrize("layout,mode", [("input", "hybrid"), ("spatial", "hybrid"), ("input", "pull"),
                                         ("spatial", "pull")])
def test_gpu_equals_the_model_and_the_reference_fixture(oracle_mod, name, layout, mode):
    g = load_golden(name)
    s = _swarm(g, layout)
    if (name, layout) not in _models:  # computed once per storage order, shared by the modes, left unchanged
        _models[name, layout] = _model_in_storage_order(oracle_mod, s, g)
    want = _models[name, layout]
    r = _run(s, g, int(g["ticks"]), mode=mode)
    got = _state(s)
    _assert_equal(got, want, OUT_KEYS + ("px", "py"))
    np.testing.assert_array_equal(r["counts"], want["counts"])
    assert r["singular"] == want["singular"] == 0
    for k in EXACT:
        np.testing.assert_array_equal(got[k], g[k + "_out"], err_msg=k)
    np.testing.assert_array_equal(r["counts"], g["counts"])
    assert s.fsm_tick == int(g["ticks"]) and s.last_refused_tick == -1


# 2. resume and trace
@pytest.mark.gpu
def test_gpu_chunks_resume_one_run_on_other_grids_and_trace_frames_are_the_runs_positions():
    g = load_golden("loop_sensed_n200")
    one, s = _swarm(g), _swarm(g)
    for q in (one, s):  # a hundred ticks in: elections held, a kill behind, followers on their way
        _run(q, g, 100)
    r1 = _run(one, g, 12, trace_every=6)
    full = _state(one)
    assert r1["trace"].shape == (2, 200, 2)
    parts = [_run(s, g, 1), _run(s, g, 5)]  # each call builds its grid from its own entry bounding box
    np.testing.assert_array_equal(r1["trace"][0].cpu().numpy(), s.pos.cpu().numpy())
    parts.append(_run(s, g, 6))
    np.testing.assert_array_equal(r1["trace"][1].cpu().numpy(), s.pos.cpu().numpy())
    _assert_equal(_state(s), full, OUT_KEYS + ("px", "py"))
    np.testing.assert_array_equal(np.concatenate([p["counts"] for p in parts]), r1["counts"])
    assert s.fsm_tick == one.fsm_tick == 112
    moved = (full["x"] != g["x"]) | (full["y"] != g["y"])
    assert moved.sum() >= 100


def _random_case(n, seed, ticks=12, n_obs=16):
    """test_update_loop.py's random swarm, its coordinates at 10 + ticks x 0.5 or above for the whole run
    (no agent moves more than max_speed * dt = 0.5 a tick): oracle.rgg_csr applies.  The first elections
    start at tick 6, leaders stand by tick 9 and die at the kill of tick 10."""
    from swarm_amd import gen
    rng = np.random.default_rng(seed)
    side = np.sqrt(n * np.pi * 2.5 ** 2 / 20.0)  # degree ~ 20 at radius 2.5
    lo = 10.0 + ticks * 0.5
    x, y = rng.uniform(lo, lo + side, n), rng.uniform(lo, lo + side, n)
    ids = rng.permutation(n).astype(np.int32)
    rp, col = gen.rgg_csr(x, y, 2.5)
    off = rng.integers(0, 40, n).astype(np.int32)
    has_t = (rng.uniform(size=n) < 0.3).astype(np.uint8)
    obs = np.stack([rng.uniform(lo, lo + side, n_obs), rng.uniform(lo, lo + side, n_obs),
                    rng.uniform(0.2, 1.0, n_obs)], 1)
    return dict(ids=ids, x=x, y=y, row_ptr=np.asarray(rp, np.int64), col=np.asarray(col, np.int32), tick_off=off,
                last_hb0=-2.5 - off * 0.1,
                tx=np.where(has_t, rng.uniform(lo, lo + 3.0 * side, n), 0.0),
                ty=np.where(has_t, rng.uniform(lo, lo + 3.0 * side, n), 0.0), has_t=has_t, obs=obs,
                ticks=np.int64(ticks), kill_ticks=np.array([10], np.int64), seed=np.uint64(seed),
                dt=np.float64(0.1), max_speed=np.float64(5.0), sense_radius=np.float64(2.5))


def _radius_graph(s, radius):
    """swarm_build_rgg of s's current storage positions, s's own graph left alone (what build_graph does)."""
    import torch
    from swarm_amd import _lib
    n, L = s.n, _lib.lib()
    rp = torch.empty(n + 1, dtype=torch.int32, device=s.device)
    ne = ctypes.c_int64(0)
    with torch.cuda.device(s.device):
        _lib.check(L.swarm_build_rgg(_lib.ctx(), n, _lib.ptr(s.pos), float(radius), _lib.ptr(rp), None, 0,
                                     ctypes.byref(ne), _lib.stream()))
        col = torch.empty(max(ne.value, 1), dtype=torch.int32, device=s.device)
        _lib.check(L.swarm_build_rgg(_lib.ctx(), n, _lib.ptr(s.pos), float(radius), _lib.ptr(rp), _lib.ptr(col),
                                     col.numel(), ctypes.byref(ne), _lib.stream()))
    return rp, col[: ne.value]


# 3. against the parent's method
@pytest.mark.gpu
def test_gpu_equals_a_radius_graph_then_one_tick_repeated_on_a_twin_swarm():
    import torch
    g = _random_case(20001, 31)
    a, b = _swarm(g), _swarm(g)
    ra = _run(a, g, 12, mode="push")
    counts, sing = [], 0
    for _ in range(12):
        r = _run(b, g, 1, mode="push", sense_radius=None, sensors=_radius_graph(b, 2.5))
        counts.append(r["counts"])
        sing += r["singular"]
    for t in ("pos", "pos_prev", "vel", "target", "has_target", "state", "leader"):
        assert torch.equal(getattr(a, t), getattr(b, t)), t
    for k in a.fsm:
        assert torch.equal(a.fsm[k], b.fsm[k]), k
    np.testing.assert_array_equal(ra["counts"], np.concatenate(counts))
    assert ra["singular"] == sing and a.fsm_tick == b.fsm_tick == 12
    frozen = _swarm(g)  # the graph of tick 0 for all twelve ticks ends elsewhere
    _run(frozen, g, 12, mode="push", sense_radius=None, sensors=_radius_graph(frozen, 2.5))
    assert not torch.equal(frozen.pos, a.pos)


# 4. random swarms against the model
@pytest.mark.gpu
@pytest.mark.parametrize("n", [4099, 20001])  # odd; one and four 4 096-agent chunks + a partial last workgroup
def test_gpu_random_swarm_equals_the_model(oracle_mod, n):
    g = _random_case(n, 17)
    s = _swarm(g)
    want = _model_in_storage_order(oracle_mod, s, g)
    fol = (want["state"] == F) & (want["has_lpos"] == 1) & (want["alive"] == 1)
    assert (want["alive"] == 0).sum() >= 1 and fol.sum() >= 1, ((want["alive"] == 0).sum(), fol.sum())
    assert min(want["x"].min(), want["y"].min()) >= 10.0
    r = _run(s, g, 12)
    _assert_equal(_state(s), want, OUT_KEYS + ("px", "py"))
    np.testing.assert_array_equal(r["counts"], want["counts"])
    assert r["singular"] == want["singular"]


def _plain_case(x, y, seed, n_obs=4):
    """Agents at (x, y), all with targets and no message graph: nobody hears anybody, the FSM idles."""
    rng = np.random.default_rng(seed)
    n = len(x)
    lo, hi = float(min(x.min(), y.min())), float(max(x.max(), y.max()))
    obs = np.stack([rng.uniform(lo, hi, n_obs), rng.uniform(lo, hi, n_obs), rng.uniform(0.2, 1.0, n_obs)], 1)
    return dict(ids=rng.permutation(n).astype(np.int32), x=x, y=y, row_ptr=np.zeros(n + 1, np.int64),
                col=np.zeros(0, np.int32), tick_off=np.zeros(n, np.int32), last_hb0=np.zeros(n),
                tx=x + 3.0, ty=y - 2.0, has_t=np.ones(n, np.uint8), obs=obs, ticks=np.int64(1),
                kill_ticks=np.zeros(0, np.int64), seed=np.uint64(seed), dt=np.float64(0.1),
                max_speed=np.float64(5.0))


# 5. radius boundary
@pytest.mark.gpu
def test_gpu_lattice_pairs_at_exactly_the_radius_are_sensed(oracle_mod):
    gx, gy = np.meshgrid(10.0 + np.arange(40) * 0.5, 10.0 + np.arange(40) * 0.5)  # exact coordinates
    g = _plain_case(gx.ravel(), gy.ravel(), 3)
    g["sense_radius"] = np.float64(1.0)
    rp, col = loop_sensed_model.sense_csr(oracle_mod, g["x"], g["y"], 1.0)
    i = 20 * 40 + 20  # an interior agent senses the 12 others within 1.0, four of them at exactly 1.0
    row = col[rp[i]:rp[i + 1]]
    d2 = (g["x"][row] - g["x"][i]) ** 2 + (g["y"][row] - g["y"][i]) ** 2
    assert len(row) == 12 and (d2 == 1.0).sum() == 4
    for layout in ("input", "spatial"):
        s = _swarm(g, layout)
        want = _model_in_storage_order(oracle_mod, s, g)
        r = _run(s, g, 1)
        _assert_equal(_state(s), want)
        assert r["singular"] == want["singular"] == 0
    open_ball = _swarm(g, "input")  # a rule that drops the pairs at exactly R ends elsewhere
    _run(open_ball, g, 1, sense_radius=1.0 - 1e-12)
    assert not np.array_equal(open_ball.pos.cpu().numpy(), s.to_input_order(s.pos))


# 6. dense block
@pytest.mark.gpu
def test_gpu_dense_block_merges_all_nine_window_cells_in_index_order(oracle_mod):
    """test_physics_sensed.py's block: 6 x 6 agents at spacing 0.3 inside a unit lattice of 100, both at
    scattered storage indices among 1 500 agents, R = 2.5 -- every block agent senses the 35 others and its
    3 x 3 window has an agent in every cell, so the ascending order only comes out of a merge over all nine
    runs.  A third of the agents are FOLLOWERs that hold a leader position and retarget behind it."""
    import torch
    n = 1500
    rng = np.random.default_rng(5)
    x, y = rng.uniform(10.0, 70.0, n), rng.uniform(10.0, 70.0, n)
    pick = rng.permutation(n)
    blk, lat = pick[:36], pick[36:136]
    bx, by = np.meshgrid(np.arange(6) * 0.3, np.arange(6) * 0.3)
    x[blk], y[blk] = 37.3 + bx.ravel(), 41.2 + by.ravel()
    lx, ly = np.meshgrid(33.05 + np.arange(10.0), 36.95 + np.arange(10.0))
    x[lat], y[lat] = lx.ravel(), ly.ravel()
    g = _plain_case(x, y, 11)
    g["sense_radius"], g["ticks"] = np.float64(2.5), np.int64(2)
    has_lpos = (rng.uniform(size=n) < 0.33).astype(np.uint8)
    has_lpos[blk[::2]] = 1
    lpos = np.where(has_lpos[:, None] != 0, rng.uniform(20.0, 60.0, (n, 2)), 0.0).astype(np.float32)
    g["fsm0"] = dict(has_lpos=has_lpos, lpos=lpos)
    rp, _ = loop_sensed_model.sense_csr(oracle_mod, x, y, 2.5)
    assert np.diff(rp)[blk].min() >= 35
    s = _swarm(g, "input")
    s.fsm["has_leader_pos"].copy_(torch.as_tensor(has_lpos))
    s.fsm["leader_pos"].copy_(torch.as_tensor(lpos))
    want = _model_in_storage_order(oracle_mod, s, g)
    assert want["max_row"] >= 35 and want["singular"] == 0
    r = _run(s, g, 2)
    got = _state(s)
    _assert_equal(got, want, OUT_KEYS + ("px", "py"))
    assert r["singular"] == 0
    retargeted = (got["tx"] != g["tx"]) | (got["ty"] != g["ty"])
    np.testing.assert_array_equal(retargeted, has_lpos != 0)
    none = _swarm(g, "input")  # the block's separation terms are really summed: sensing nobody ends elsewhere
    _run(none, g, 2, sense_radius=1e-6)
    far = none.pos.cpu().numpy()
    assert np.all((far[blk, 0] != got["x"][blk]) | (far[blk, 1] != got["y"][blk]))


# 7. message graph untouched
@pytest.mark.gpu
def test_gpu_message_graph_is_untouched_and_a_following_allocate_works(oracle_mod):
    import torch
    from swarm_amd import gen
    from swarm_amd.swarm import Swarm
    d = gen.swarm_inputs(3000, 41, t=60)
    for k in ("x", "y", "tx", "ty"):  # room for the agents' way to their targets
        d[k] = d[k] + 10.0
    s = Swarm(d["ids"], d["x"], d["y"], d["caps"], device="cuda").build_graph(1.0)
    s.allocate(d["tx"], d["ty"], d["treq"])  # builds the cell index of the storage order
    rp0, col0, v0 = s.row_ptr, s.col, (s.row_ptr._version, s.col._version)
    rp_keep, col_keep = s.row_ptr.clone(), s.col.clone()
    s.protocol_reset()
    s.set_target(d["x"] + 4.0, d["y"] - 3.0)
    x0 = s.pos.clone()
    r = s.update_loop_sensed(6, 1.0)
    assert r["singular"] == 0 and not torch.equal(s.pos, x0)
    assert s.row_ptr is rp0 and s.col is col0 and (s.row_ptr._version, s.col._version) == v0
    assert torch.equal(s.row_ptr, rp_keep) and torch.equal(s.col, col_keep)
    assert s._cindex is None and s._pos_prev_key[0] is s.pos
    a = s.allocate(d["tx"], d["ty"], d["treq"])  # the agents moved: allocated from where they are now
    p = s.to_input_order(s.pos)
    want = oracle_mod.allocate(d["ids"], p[:, 0], p[:, 1], d["caps"], d["tx"], d["ty"], d["treq"])
    np.testing.assert_array_equal(a.winner.cpu().numpy(), want["winner"])
    np.testing.assert_array_equal(a.util.cpu().numpy(), want["util"])


# 8. singular tick
@pytest.mark.gpu
def test_gpu_singular_tick_is_counted_and_a_later_chunk_returns(oracle_mod):
    g = _random_case(300, 5, n_obs=2)
    g["ticks"] = np.int64(9)
    g["x"][7], g["y"][7] = g["x"][3], g["y"][3]  # two agents on one point ...
    for i, k in ((3, 40.0), (7, 50.0)):          # ... both with targets, so both compute the zero distance
        g["has_t"][i], g["tx"][i], g["ty"][i] = 1, k, k
    s = _swarm(g, "input")
    want = _model_in_storage_order(oracle_mod, s, g, 3)
    assert want["singular"] >= 2 and not np.isfinite(want["x"][3]) and not np.isfinite(want["x"][7])
    r = _run(s, g, 3)
    assert r["singular"] == want["singular"]
    _assert_equal(_state(s), want)
    later = _model_in_storage_order(oracle_mod, s, g, 9)
    r2 = _run(s, g, 6)  # non-finite agents present: they sense nobody, nobody senses them, the call returns
    _assert_equal(_state(s), later)
    assert r["singular"] + r2["singular"] == later["singular"]
    assert np.isfinite(later["x"]).sum() >= 290


# 9. refusal
@pytest.mark.gpu
def test_gpu_refused_tick_leaves_every_array_as_it_was():
    import torch
    from swarm_amd import _lib
    from swarm_amd.swarm import Swarm
    n = 1_200_000
    rng = np.random.default_rng(2)
    x, y = 3.0 + rng.uniform(0, 1e-3, n), -2.0 + rng.uniform(0, 1e-3, n)
    s = Swarm(np.arange(n, dtype=np.int32), x, y, layout="input", device="cuda")
    s.row_ptr = torch.zeros(n + 1, dtype=torch.int32, device="cuda")  # nobody hears anybody
    s.col = torch.zeros(0, dtype=torch.int32, device="cuda")
    # every agent's failure detector fires at tick 1 (3.05 s of silence): the FSM kernels of all three ticks
    # write the timers and the records, and the discard has something to undo
    s.protocol_reset(last_hb=np.full(n, -2.95))
    s.set_target(np.full(n, 9.0), np.full(n, 9.0))
    s.vel.fill_(0.25)
    s.pos_prev = s.pos + 0.5
    s._pos_prev_key = (s.pos, s.pos._version)
    s.fsm["outbox"][::3] = 1
    keep = dict(pos=s.pos, pos_prev=s.pos_prev, vel=s.vel, target=s.target, has_target=s.has_target,
                state=s.state, leader=s.leader, **s.fsm)
    before = {k: v.clone() for k, v in keep.items()}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with pytest.raises(_lib.SwarmError) as e:
        s.update_loop_sensed(3, 1.0)
    torch.cuda.synchronize()
    assert time.perf_counter() - t0 < 20.0
    assert e.value.code == _lib.ERR_RANGE and "too dense" in str(e.value) and "tick 1" in str(e.value)
    assert s.last_refused_tick == 1 and s.fsm_tick == 0
    for k, v in keep.items():
        assert torch.equal(v, before[k]), k
    assert keep["pos_prev"] is s.pos_prev and keep["pos"] is s.pos
    # the swarm is usable as it stands: the fixed-graph loop runs it, and every failure detector fires
    r = s.update_loop(3)
    assert r["counts"][:, 1].max() == n and s.fsm_tick == 3


# 10. trivial and bad arguments
@pytest.mark.gpu
def test_gpu_empty_swarm_zero_ticks_and_bad_radii():
    import torch
    from swarm_amd import _lib
    from swarm_amd.swarm import Swarm
    e = Swarm(np.zeros(0, np.int32), np.zeros(0), np.zeros(0), layout="input", device="cuda")
    e.set_graph(np.zeros(1, np.int64), np.zeros(0, np.int32))
    r = e.update_loop_sensed(5, 2.5, trace_every=2)
    assert r["counts"].shape == (5, 4) and not r["counts"].any() and r["singular"] == 0
    assert r["trace"].shape == (2, 0, 2) and e.fsm_tick == 5 and e.last_refused_tick == -1
    g = load_golden("loop_sensed_n200")
    s = _swarm(g)
    keep = dict(pos=s.pos, vel=s.vel, target=s.target, has_target=s.has_target, state=s.state, **s.fsm)
    before = {k: v.clone() for k, v in keep.items()}
    r = _run(s, g, 0)
    assert r["counts"].shape == (0, 4) and s.fsm_tick == 0
    for radius in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(_lib.SwarmError, match="sense_radius must be positive and finite") as err:
            _run(s, g, 4, sense_radius=radius)
        assert err.value.code == _lib.ERR_ARG and s.fsm_tick == 0
    s.pos[5, 1] = float("inf")  # non-finite positions at entry: refused before anything is written
    before["pos"] = s.pos.clone()
    with pytest.raises(_lib.SwarmError, match="positions must be finite") as err:
        _run(s, g, 4)
    assert err.value.code == _lib.ERR_ARG and s.fsm_tick == 0
    for k, v in keep.items():
        assert torch.equal(v, before[k]), k
