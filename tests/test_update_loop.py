"""The coupled update loop (contract U1): the reference's update_loop (agent.py:67-81), each tick
_process_logic then _update_physics, for the whole swarm in one call (swarm_update_loop / Swarm.update_loop).

tests/golden/loop_*.npz were produced by real SwarmAgent objects (tools/gen_golden_loop.py).  The CPU model
(tests/loop_model.py, the existing oracle composed per tick) must reproduce them bit for bit with the
reference's libm pow; the GPU must equal the same model with its own x*x squares bit for bit, and the
reference fixture itself in everything that does not depend on the arithmetic.
"""
import ctypes
import functools

import numpy as np
import pytest

from conftest import load_golden
import loop_model
from loop_model import FSM_KEYS, OUT_KEYS, F

LOOP = ("loop_n200", "loop_n250", "loop_wide_n400")
# what the arithmetic of the squares cannot reach: the FSM's decisions do not depend on positions
EXACT = ("state", "leader", "last_hb", "wait_start", "delay", "has_lpos", "alive")


@functools.lru_cache(maxsize=None)
def _model(name, use_pow, hb_lagged=True):
    from oracle import oracle
    return loop_model.run(oracle, load_golden(name), use_pow=use_pow, hb_lagged=hb_lagged)


# ----------------------------------------------------------------------------- CPU

@pytest.mark.parametrize("name", LOOP)
def test_model_with_pow_equals_the_reference_fixture(oracle_mod, name):
    g = load_golden(name)
    o = _model(name, True)
    for k in OUT_KEYS:
        np.testing.assert_array_equal(o[k], g[k + "_out"], err_msg=k)
    np.testing.assert_array_equal(o["counts"], g["counts"])
    assert o["singular"] == 0


@pytest.mark.parametrize("name", LOOP)
def test_fixtures_tell_implementations_apart(oracle_mod, name):
    g = load_golden(name)
    n = len(g["ids"])
    fol = (g["state_out"] == F) & (g["has_lpos_out"] == 1) & (g["alive_out"] == 1)
    assert 2 * fol.sum() >= n                       # the formation half of the loop is what most agents run
    assert (g["alive_out"] == 0).sum() >= 1           # kills happened: frozen bodies, re-election
    moved = (g["x_out"] != g["x"]) | (g["y_out"] != g["y"])
    assert moved.sum() >= 0.9 * n
    # heartbeats that read the sender's CURRENT position (P_{t-1}) instead of the one it packed (P_{t-2})
    wrong = _model(name, True, hb_lagged=False)
    differs = (wrong["lpos"] != g["lpos_out"]).any(1)
    assert 2 * (differs & fol).sum() >= fol.sum(), ((differs & fol).sum(), fol.sum())


def test_entry_point_rejects_a_null_ctx_without_gpu():
    from swarm_amd import _lib
    L = _lib.load()
    rc = L.swarm_update_loop(None, 4, None, None, None, None, None, None, None, None, None, 0, 1, 0.1, 3.0, 0.2,
                             ctypes.c_uint64(0), None, 0, 0.125, None, None, None, 0, None, None, None, 5.0, None,
                             0, None, None, None)
    assert rc == _lib.ERR_ARG
    assert b"ctx is NULL" in L.swarm_last_error()


def test_update_loop_and_set_target_argument_errors_need_no_device():
    from swarm_amd.swarm import Swarm
    s = Swarm.__new__(Swarm)  # no device: the keywords and shapes are checked before anything else
    s.n, s.layout = 5, "input"
    with pytest.raises(ValueError, match="unknown mode"):
        s.update_loop(3, mode="shove")
    with pytest.raises(ValueError, match="ticks must not be negative"):
        s.update_loop(-1)
    with pytest.raises(ValueError, match="trace_every must not be negative"):
        s.update_loop(3, trace_every=-2)
    with pytest.raises(TypeError):
        s.update_loop(3, sense_radius=1.0)  # not offered here: the neighbour lists are fixed for the call
    with pytest.raises(ValueError, match="x: expected 5 values"):
        s.set_target(np.zeros(4), np.zeros(5))
    with pytest.raises(ValueError, match="y: expected 2 values"):
        s.set_target(np.zeros(2), np.zeros(3), index=[0, 1])
    with pytest.raises(ValueError, match="index out of range"):
        s.set_target(1.0, 2.0, index=[0, 5])
    with pytest.raises(ValueError, match="index out of range"):
        s.clear_target(index=[-1])
    with pytest.raises(ValueError, match="1-D array of agent indices"):
        s.set_target(1.0, 2.0, index=[0.5])


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
    return s.update_loop(ticks, obstacles=g["obs"], kill_ticks=g["kill_ticks"], dt=float(g["dt"]),
                         seed=int(g["seed"]), max_speed=float(g["max_speed"]), **kw)


def _state(s):
    f = s.fsm
    t = dict(state=s.state, leader=s.leader, last_hb=f["last_hb"], wait_start=f["wait_start"], delay=f["delay"],
             has_lpos=f["has_leader_pos"], lpos=f["leader_pos"], alive=f["alive"], has_t=s.has_target)
    out = {k: s.to_input_order(v) for k, v in t.items()}
    for kx, ky, v in (("x", "y", s.pos), ("vx", "vy", s.vel), ("tx", "ty", s.target), ("px", "py", s.pos_prev)):
        a = s.to_input_order(v)
        out[kx], out[ky] = a[:, 0], a[:, 1]
    return out


def _assert_equal(got, want, keys=OUT_KEYS):
    for k in keys:  # bit for bit; NaN == NaN (a singular tick leaves non-finite values on both sides)
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


@pytest.mark.gpu
@pytest.mark.parametrize("name", LOOP)
@pytest.mark.parametrize("layout,mode", [("input", "hybrid"), ("spatial", "hybrid"), ("input", "pull"),
                                         ("spatial", "pull")])
def test_gpu_equals_the_model_and_the_reference_fixture(oracle_mod, name, layout, mode):
    g = load_golden(name)
    want = _model(name, False)
    s = _swarm(g, layout)
    r = _run(s, g, int(g["ticks"]), mode=mode)
    got = _state(s)
    _assert_equal(got, want)
    np.testing.assert_array_equal(r["counts"], want["counts"])
    assert r["singular"] == want["singular"] == 0
    for k in EXACT:
        np.testing.assert_array_equal(got[k], g[k + "_out"], err_msg=k)
    np.testing.assert_array_equal(r["counts"], g["counts"])
    np.testing.assert_array_equal(got["px"], want["px"])  # pos_prev = P_{end-1}
    np.testing.assert_array_equal(got["py"], want["py"])


@pytest.mark.gpu
def test_gpu_chunks_resume_one_run_and_trace_frames_are_the_runs_positions():
    g = load_golden("loop_n200")
    assert int(g["ticks"]) == 260
    one = _swarm(g)
    r1 = _run(one, g, 260, trace_every=20)
    full = _state(one)
    s = _swarm(g)  # odd chunks, both buffer parities, resume through pos_prev and the outbox
    parts = [_run(s, g, k) for k in (1, 99, 160)]
    got = _state(s)
    _assert_equal(got, full, OUT_KEYS + ("px", "py"))
    np.testing.assert_array_equal(np.concatenate([p["counts"] for p in parts]), r1["counts"])
    assert r1["trace"].shape == (13, 200, 2)
    for stop in (20, 140, 260):  # frames against separate runs stopped there
        q = _swarm(g)
        _run(q, g, stop)
        np.testing.assert_array_equal(r1["trace"][stop // 20 - 1].cpu().numpy(), q.pos.cpu().numpy())
    assert _run(_swarm(g), g, 19, trace_every=20)["trace"].shape == (0, 200, 2)


def _random_case(n, seed, n_obs=16):
    from swarm_amd import gen
    rng = np.random.default_rng(seed)
    side = np.sqrt(n * np.pi * 2.5 ** 2 / 20.0)  # degree ~ 20 at radius 2.5
    x, y = rng.uniform(10.0, 10.0 + side, n), rng.uniform(10.0, 10.0 + side, n)
    ids = rng.permutation(n).astype(np.int32)
    rp, col = gen.rgg_csr(x, y, 2.5)
    off = rng.integers(0, 40, n).astype(np.int32)
    has_t = (rng.uniform(size=n) < 0.3).astype(np.uint8)
    obs = np.stack([rng.uniform(10.0, 10.0 + side, n_obs), rng.uniform(10.0, 10.0 + side, n_obs),
                    rng.uniform(0.2, 1.0, n_obs)], 1)
    return dict(ids=ids, x=x, y=y, row_ptr=np.asarray(rp, np.int64), col=np.asarray(col, np.int32), tick_off=off,
                last_hb0=-2.5 - off * 0.1,  # the first election starts at tick 6
                tx=np.where(has_t, rng.uniform(0.0, 3.0 * side, n), 0.0),
                ty=np.where(has_t, rng.uniform(0.0, 3.0 * side, n), 0.0), has_t=has_t, obs=obs,
                ticks=np.int64(120), kill_ticks=np.array([60], np.int64), seed=np.uint64(seed), dt=np.float64(0.1),
                max_speed=np.float64(5.0))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4099, 20001])  # odd; one and four 4 096-agent chunks + a partial last workgroup
def test_gpu_random_swarm_equals_the_model(oracle_mod, n):
    g = _random_case(n, 17)
    want = loop_model.run(oracle_mod, g, use_pow=False)
    fol = (want["state"] == F) & (want["has_lpos"] == 1) & (want["alive"] == 1)
    assert (want["alive"] == 0).sum() >= 1 and 2 * fol.sum() >= n, ((want["alive"] == 0).sum(), fol.sum())
    s = _swarm(g)
    r = _run(s, g, 120)
    _assert_equal(_state(s), want, OUT_KEYS + ("px", "py"))
    np.testing.assert_array_equal(r["counts"], want["counts"])
    assert r["singular"] == want["singular"]


@pytest.mark.gpu
def test_gpu_fsm_half_equals_protocol_run_on_a_twin_swarm():
    """The FSM's decisions do not depend on positions: every FSM array but leader_pos, and the counts, after
    update_loop equal protocol_run's on a twin swarm with the same arguments, exactly."""
    n = 100_000
    g = _random_case(n, 23, n_obs=4)
    a, b = _swarm(g), _swarm(g)
    kw = dict(kill_ticks=g["kill_ticks"], seed=23)
    ra = a.update_loop(120, obstacles=g["obs"], **kw)
    cb = b.protocol_run(120, **kw)
    np.testing.assert_array_equal(ra["counts"], cb)
    assert cb[:, 0].max() > 0 and cb[:, 3].sum() > 0
    import torch
    for k in ("last_hb", "wait_start", "delay", "has_leader_pos", "alive", "outbox"):
        assert torch.equal(a.fsm[k], b.fsm[k]), k
    assert torch.equal(a.state, b.state) and torch.equal(a.leader, b.leader)
    assert not torch.equal(a.pos, b.pos) and a.fsm_tick == b.fsm_tick == 120


@pytest.mark.gpu
def test_gpu_sensor_graph_of_its_own_and_push_mode_equal_the_model(oracle_mod):
    """`sensors`: the separation neighbours are not the message graph (here the agents within 1.2 instead of
    2.5, over storage indices: input layout).  Push mode mails every tick."""
    g = _random_case(3001, 29)
    srp, scol = oracle_mod.rgg_csr(g["x"], g["y"], 1.2)
    g["sense_row_ptr"], g["sense_col"] = np.asarray(srp, np.int64), np.asarray(scol, np.int32)
    want = loop_model.run(oracle_mod, g, use_pow=False)
    same_graph = loop_model.run(oracle_mod, {k: v for k, v in g.items() if not k.startswith("sense_")}, use_pow=False)
    assert not np.array_equal(want["x"], same_graph["x"])
    s = _swarm(g, "input")
    r = _run(s, g, 120, sensors=(g["sense_row_ptr"], g["sense_col"]), mode="push")
    _assert_equal(_state(s), want, OUT_KEYS + ("px", "py"))
    np.testing.assert_array_equal(r["counts"], want["counts"])


@pytest.mark.gpu
def test_gpu_pos_prev_follows_self_pos_and_overlapping_buffers_are_refused():
    import torch
    from swarm_amd import _lib
    g = load_golden("loop_n200")
    s = _swarm(g)
    _run(s, g, 30)
    assert not torch.equal(s.pos_prev, s.pos)        # agents are moving: P_29 != P_30
    kept = s.pos_prev.clone()
    _run(s, g, 0)
    assert torch.equal(s.pos_prev, kept)             # self.pos untouched since the last call: kept
    s.pos.mul_(1.0)                                  # anything else wrote self.pos: pos_prev restarts as a copy
    _run(s, g, 0)
    assert torch.equal(s.pos_prev, s.pos)
    state0, tick0 = s.state.clone(), s.fsm_tick
    s.pos_prev = s.pos                               # one buffer for both: refused before anything is launched
    with pytest.raises(_lib.SwarmError, match="must not overlap"):
        _run(s, g, 4)
    assert torch.equal(s.state, state0) and s.fsm_tick == tick0


@pytest.mark.gpu
def test_gpu_singular_tick_is_counted_and_later_chunks_return(oracle_mod):
    g = _random_case(300, 5, n_obs=2)
    g["x"][7], g["y"][7] = g["x"][3], g["y"][3]  # two agents on one point ...
    rp, col = oracle_mod.rgg_csr(g["x"], g["y"], 2.5)
    g["row_ptr"], g["col"] = np.asarray(rp, np.int64), np.asarray(col, np.int32)
    for i, k in ((3, 40.0), (7, 50.0)):          # ... both with targets, so both compute the zero distance
        g["has_t"][i], g["tx"][i], g["ty"][i] = 1, k, k
    want = loop_model.run(oracle_mod, g, 3, use_pow=False)
    assert want["singular"] >= 2 and not np.isfinite(want["x"][3])
    s = _swarm(g)
    r = _run(s, g, 3)
    assert r["singular"] == want["singular"]
    _assert_equal(_state(s), want)
    later = loop_model.run(oracle_mod, g, 30, use_pow=False)
    r2 = _run(s, g, 27)  # non-finite positions present: the call still returns, and equals the model
    _assert_equal(_state(s), later)
    assert r["singular"] + r2["singular"] == later["singular"]


@pytest.mark.gpu
def test_gpu_empty_swarm_zero_ticks_and_nothing_to_chase():
    import torch
    from swarm_amd.swarm import Swarm
    e = Swarm(np.zeros(0, np.int32), np.zeros(0), np.zeros(0), layout="input", device="cuda")
    e.set_graph(np.zeros(1, np.int64), np.zeros(0, np.int32))
    r = e.update_loop(5, trace_every=2)
    assert r["counts"].shape == (5, 4) and not r["counts"].any() and r["singular"] == 0
    assert r["trace"].shape == (2, 0, 2) and e.fsm_tick == 5
    g = load_golden("loop_n200")
    s = _swarm(g)
    before = {k: v.clone() for k, v in (("pos", s.pos), ("target", s.target), ("state", s.state))}
    r = _run(s, g, 0)
    assert r["counts"].shape == (0, 4) and s.fsm_tick == 0
    assert all(torch.equal(before[k], getattr(s, k)) for k in before)
    # no targets and fewer ticks than the first heartbeat (protocol_reset's defaults: the first timeout is
    # at tick 31): nobody has anything to chase
    s = _swarm(g)
    s.protocol_reset()
    s.clear_target()
    x0 = s.pos.clone()
    r = _run(s, g, 25)
    assert not r["counts"].any() and torch.equal(s.pos, x0) and torch.equal(s.pos_prev, x0)
    assert not s.vel.any() and not s.has_target.any()
