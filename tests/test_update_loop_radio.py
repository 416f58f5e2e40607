"""The update loop that re-senses who hears whom every tick (contract U1-R):
swarm_update_loop_radio / Swarm.update_loop_radio(ticks, Rc, Rs).

tests/golden/loop_radio_*.npz were produced by real SwarmAgent objects that received, every tick, the packets
of the agents within Rc of them in the snapshot at the start of the tick, in ascending index, and whose
update_sensors was fed the agents within Rs of the same snapshot (tools/gen_golden_loop_radio.py).  The CPU
model (tests/loop_radio_model.py) must reproduce them bit for bit with the reference's libm pow; the GPU must
equal the same model with its own x*x squares bit for bit -- the model run over the GPU's storage order, since
the heard senders are handled in ascending storage index -- and the fixture itself in everything the squares
cannot reach.
"""
import ctypes
import time

import numpy as np
import pytest

from conftest import load_golden
import loop_radio_model
from loop_model import OUT_KEYS, F, L
from loop_sensed_model import sense_csr
from test_update_loop_sensed import EXACT, PER_AGENT, _assert_equal, _radius_graph, _random_case, _state

RADIO = ("loop_radio_n200", "loop_radio_r12_n250", "loop_radio_wide_n400")
ALL = OUT_KEYS + ("px", "py")


# ----------------------------------------------------------------------------- CPU

@pytest.mark.parametrize("name", RADIO)
def test_model_with_pow_equals_the_reference_fixture(oracle_mod, name):
    g = load_golden(name)
    o = loop_radio_model.run(oracle_mod, g, use_pow=True)
    for k in OUT_KEYS:  # the thirteen arrays
        np.testing.assert_array_equal(o[k], g[k + "_out"], err_msg=k)
    np.testing.assert_array_equal(o["counts"], g["counts"])
    assert o["singular"] == 0 and 30 <= o["max_heard"] <= 35


@pytest.mark.parametrize("name", RADIO)
def test_fixtures_tell_a_resensed_radio_from_a_frozen_graph(oracle_mod, name):
    g = load_golden(name)
    frozen = loop_radio_model.run(oracle_mod, g, use_pow=True, reradio=False)  # U1-S on the tick-0 graph
    differs = frozen["leader"] != g["leader_out"]
    assert 4 * differs.sum() >= len(differs), (int(differs.sum()), len(differs))


def test_entry_point_rejects_a_null_ctx_without_gpu():
    from swarm_amd import _lib
    lib = _lib.load()
    rc = lib.swarm_update_loop_radio(None, 4, None, None, None, None, None, 0, 1, 0.1, 3.0, 0.2, ctypes.c_uint64(0),
                                     None, 0, None, None, None, 0, None, 2.5, 2.5, 5.0, None, 0, None, None, None,
                                     None)
    assert rc == _lib.ERR_ARG
    assert b"ctx is NULL" in lib.swarm_last_error()


def test_update_loop_radio_refuses_bad_radii_without_a_device():
    from swarm_amd.swarm import Swarm
    s = Swarm.__new__(Swarm)  # no device needed: the radii are checked before anything else
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="radio_radius must be positive and finite"):
            s.update_loop_radio(3, bad, 1.0)
        with pytest.raises(ValueError, match="sense_radius must be positive and finite"):
            s.update_loop_radio(3, 2.5, bad)
    with pytest.raises(TypeError):
        s.update_loop_radio(3, 2.5)  # the sensing radius has no default
    with pytest.raises(TypeError):
        s.update_loop_radio(3, 2.5, 1.0, sensors=None)  # no sensors, mode or pull_frac: there is no graph


# ----------------------------------------------------------------------------- GPU

def _swarm(g, layout="spatial", graph=False):
    """A swarm of the case's agents; no neighbour graph unless asked for."""
    import torch
    from swarm_amd.swarm import Swarm
    s = Swarm(g["ids"], g["x"], g["y"], layout=layout, device="cuda")
    if graph:
        s.set_graph(g["row_ptr"], g["col"])
    s.protocol_reset(tick_off=g["tick_off"], last_hb=g["last_hb0"])
    idx = np.flatnonzero(g["has_t"])
    if len(idx):
        s.set_target(g["tx"][idx], g["ty"][idx], index=idx)
    where = dict(state=(s.state, torch.uint8), leader=(s.leader, torch.int32), alive=(s.fsm["alive"], torch.uint8))
    for k, v in g.get("fsm0", {}).items():  # input order -> storage order
        where[k][0].copy_(s._storage(v, where[k][1]))
    return s


def _kw(g):
    return dict(obstacles=g["obs"], kill_ticks=g["kill_ticks"], dt=float(g["dt"]), seed=int(g["seed"]),
                max_speed=float(g["max_speed"]))


def _run(s, g, ticks, **kw):
    return s.update_loop_radio(ticks, float(g["radio_radius"]), float(g["sense_radius"]), **_kw(g), **kw)


def _model(oracle_mod, s, g, ticks=None, plan=None):
    """The model run over s's storage order (agent k of the run is input agent perm[k]; the message graph, where
    a chunk reads one, as s holds it), its per-agent results put back into input order.  plan: the run as
    chunks [(ticks, loop_radio_model.run keywords), ...], each starting where the one before ended."""
    perm = s.perm.cpu().numpy().astype(np.int64)
    q = dict(g)
    for k in PER_AGENT:
        q[k] = np.asarray(g[k])[perm]
    if "fsm0" in g:
        q["fsm0"] = {k: np.asarray(v)[perm] for k, v in g["fsm0"].items()}
    if s.row_ptr is not None:
        q["row_ptr"], q["col"] = s.row_ptr.cpu().numpy().astype(np.int64), s.col.cpu().numpy()
    o, counts, singular = None, [], 0
    for chunk, kw in (plan or [(ticks, {})]):
        o = loop_radio_model.run(oracle_mod, q, chunk, start=o, **kw)
        counts.append(o["counts"])
        singular += o["singular"]
    out = {}
    for k, v in o.items():
        if isinstance(v, np.ndarray) and k != "counts":
            out[k] = np.empty_like(v)
            out[k][perm] = v
        else:
            out[k] = v
    out["counts"], out["singular"] = np.concatenate(counts), singular
    return out


def _case(n, seed, rc, rs, ticks=12, **kw):
    g = _random_case(n, seed, ticks=ticks, **kw)
    g["radio_radius"], g["sense_radius"] = np.float64(rc), np.float64(rs)
    return g


# 1. fixtures
@pytest.mark.gpu
@pytest.mark.parametrize("name", RADIO)
@pytest.mark.parametrize("layout", ["input", "spatial"])
def test_gpu_equals_the_model_and_the_reference_fixture(oracle_mod, name, layout):
    """The reference side of the comparison follows the contract's order: the heard senders are handled in
    ascending STORAGE index, and what a receiver ends with depends on that order.  In layout "input" the storage
    order is the fixture's own, so the GPU must equal the fixture itself in everything the squares cannot
    reach.  In layout "spatial" the agents are stored in another order, and real agents numbered that way end
    elsewhere than the fixture's (measured on the GPU: state differs from the fixture for 32 / 200, 38 / 250
    and 54 / 400 agents while every array equals the x*x model of the storage order bit for bit); there the
    reference is the same run of the reference's own arithmetic -- the model with libm pow, which the CPU test
    above pins to real agents bit for bit -- over the storage order."""
    g = load_golden(name)
    s = _swarm(g, layout)
    want = _model(oracle_mod, s, g)
    r = _run(s, g, int(g["ticks"]))
    got = _state(s)
    _assert_equal(got, want, ALL)
    np.testing.assert_array_equal(r["counts"], want["counts"])
    assert r["singular"] == want["singular"] == 0
    if layout == "input":
        ref, ref_counts = {k: g[k + "_out"] for k in EXACT}, g["counts"]
    else:
        ref = _model(oracle_mod, s, g, plan=[(int(g["ticks"]), dict(use_pow=True))])
        ref_counts = ref["counts"]
    for k in EXACT:  # state, leader, the timers, alive
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    np.testing.assert_array_equal(r["counts"], ref_counts)
    assert s.fsm_tick == int(g["ticks"]) and s.last_refused_tick == -1 and s.row_ptr is None


# 2. against the parent's method
@pytest.mark.gpu
def test_gpu_equals_a_radius_graph_then_one_sensed_tick_repeated_on_a_twin_swarm():
    import torch
    g = _case(20001, 31, 2.5, 1.2)
    a, b = _swarm(g), _swarm(g)
    ra = _run(a, g, 12)
    counts, sing = [], 0
    for _ in range(12):
        b.row_ptr, b.col = _radius_graph(b, 2.5)  # the message graph of this tick's positions
        b._hear = None
        r = b.update_loop_sensed(1, 1.2, **_kw(g))
        counts.append(r["counts"])
        sing += r["singular"]
    for t in ("pos", "pos_prev", "vel", "target", "has_target", "state", "leader"):
        assert torch.equal(getattr(a, t), getattr(b, t)), t
    for k in a.fsm:  # both outbox halves among them
        assert torch.equal(a.fsm[k], b.fsm[k]), k
    np.testing.assert_array_equal(ra["counts"], np.concatenate(counts))
    assert ra["singular"] == sing and a.fsm_tick == b.fsm_tick == 12 and a.row_ptr is None
    assert ra["counts"][:, 2].sum() > 0 and ra["counts"][:, 3].sum() > 0  # acclaims and heartbeats were sent


# 3. random swarms against the model
@pytest.mark.gpu
@pytest.mark.parametrize("n", [4099, 20001])  # odd; one and four 4 096-agent chunks + a partial last workgroup
def test_gpu_random_swarm_equals_the_model(oracle_mod, n):
    g = _case(n, 17, 2.5, 2.5)
    s = _swarm(g)
    want = _model(oracle_mod, s, g, 12)
    fol = (want["state"] == F) & (want["has_lpos"] == 1) & (want["alive"] == 1)
    assert (want["alive"] == 0).sum() >= 1 and fol.sum() >= 1, ((want["alive"] == 0).sum(), fol.sum())
    assert min(want["x"].min(), want["y"].min()) >= 10.0
    r = _run(s, g, 12)
    _assert_equal(_state(s), want, ALL)
    np.testing.assert_array_equal(r["counts"], want["counts"])
    assert r["singular"] == want["singular"]


# 4. the radio radius above, equal to and below the sensing cell
@pytest.mark.gpu
@pytest.mark.parametrize("rc,rs", [(2.5, 1.2), (1.0, 2.5), (0.5, 0.7), (3.0, 3.0)])
def test_gpu_radius_pairs_equal_the_model(oracle_mod, rc, rs):
    g = _case(2000, 23, rc, rs, ticks=30)
    s = _swarm(g)
    want = _model(oracle_mod, s, g, 30)
    r = _run(s, g, 30)
    _assert_equal(_state(s), want, ALL)
    np.testing.assert_array_equal(r["counts"], want["counts"])
    assert r["singular"] == want["singular"]
    assert want["counts"][:, 0].max() >= 1  # leaders stood and were heard or not


def _leaders_case(x, y, ids, seed=1):
    """Agents at (x, y) without targets, every one a LEADER (of itself) in lock step: all heartbeat at tick 10,
    the heartbeats are received at tick 11, judged on positions nobody has left."""
    n = len(x)
    return dict(ids=np.asarray(ids, np.int32), x=np.asarray(x, np.float64), y=np.asarray(y, np.float64),
                tick_off=np.zeros(n, np.int32), last_hb0=np.zeros(n), tx=np.zeros(n), ty=np.zeros(n),
                has_t=np.zeros(n, np.uint8), obs=np.array([[1000.0, 1000.0, 0.5]]), ticks=np.int64(11),
                kill_ticks=np.zeros(0, np.int64), seed=np.uint64(seed), dt=np.float64(0.1),
                max_speed=np.float64(5.0), radio_radius=np.float64(5.0), sense_radius=np.float64(1.0),
                fsm0=dict(state=np.full(n, L, np.uint8), leader=np.asarray(ids, np.int32)))


# 5. exactly at the radius
@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["input", "spatial"])
def test_gpu_a_sender_at_exactly_the_radius_is_heard_and_one_ulp_further_is_not(oracle_mod, layout):
    # an 8 x 8 integer lattice (many pairs at exactly 5: offsets (3, 4), (4, 3), (5, 0), (0, 5)) and two pairs
    # on their own: receiver 64 at (100, 10) with sender 65 at offset (3, 4); receiver 66 at (200, 10) with
    # sender 67 at offset (3, 4 + one ulp of 14).  The senders have the higher IDs, so a LEADER that hears yields.
    lx, ly = np.meshgrid(10.0 + np.arange(8.0), 10.0 + np.arange(8.0))
    x = np.concatenate([lx.ravel(), [100.0, 103.0, 200.0, 203.0]])
    y = np.concatenate([ly.ravel(), [10.0, 14.0, 10.0, np.nextafter(14.0, np.inf)]])
    ids = np.concatenate([np.random.default_rng(4).permutation(64), [100, 200, 101, 201]])
    g = _leaders_case(x, y, ids)
    rp, col = sense_csr(oracle_mod, x, y, 5.0)
    assert list(col[rp[64]:rp[65]]) == [65] and rp[67] == rp[66]  # the rule itself: <= hears, one ulp more does not
    d2 = (x[col[rp[27]:rp[28]]] - x[27]) ** 2 + (y[col[rp[27]:rp[28]]] - y[27]) ** 2
    assert (d2 == 25.0).sum() >= 4
    s = _swarm(g, layout)
    want = _model(oracle_mod, s, g, 11)
    r = _run(s, g, 11)
    got = _state(s)
    _assert_equal(got, want, ALL)
    np.testing.assert_array_equal(r["counts"], want["counts"])
    assert got["state"][64] == F and got["leader"][64] == 200 and got["has_lpos"][64] == 1
    np.testing.assert_array_equal(got["lpos"][64], np.float32([103.0, 14.0]))
    assert got["state"][66] == L and got["leader"][66] == 101 and got["has_lpos"][66] == 0
    assert got["state"][65] == L and got["state"][67] == L  # a lower ID's heartbeat does not unseat a LEADER


# 6. order
@pytest.mark.gpu
def test_gpu_dense_block_hears_its_senders_in_ascending_index_over_all_nine_cells(oracle_mod):
    """300 agents at random in a 7.4 x 7.4 block -- three cells of side 2.5 each way, the indices scattered over
    them -- all LEADERs that heartbeat at tick 10.  Wherever the grid's origin lies, the block straddles two
    cell boundaries each way, so some receivers hear senders in all nine cells of their windows (about a
    hundred each); once a receiver has yielded, every further heartbeat replaces its leader and leader
    position, so the last sender in ascending index decides: only a merge over all nine runs gets it."""
    rng = np.random.default_rng(8)
    n = 300
    x, y = 20.0 + rng.uniform(0.0, 7.4, n), 30.0 + rng.uniform(0.0, 7.4, n)
    g = _leaders_case(x, y, rng.permutation(n), seed=2)
    g["radio_radius"], g["sense_radius"] = np.float64(2.5), np.float64(2.5)
    s = _swarm(g, "input")
    want = _model(oracle_mod, s, g, 11)
    assert want["max_heard"] >= 80
    rp, col = sense_csr(oracle_mod, x, y, 2.5)
    side = 2.5 * (1.0 + 1e-9)
    for ox in np.arange(5) * side / 5:  # any alignment of cells of that side
        for oy in np.arange(5) * side / 5:
            cx, cy = np.floor((x - ox) / side), np.floor((y - oy) / side)
            assert any(len({(cx[j] - cx[i], cy[j] - cy[i]) for j in col[rp[i]:rp[i + 1]]}) == 9 for i in range(n))
    # the same agents numbered backwards (index k <-> n - 1 - k) hear in the opposite order and end elsewhere
    rev = dict(g)
    for k in PER_AGENT:
        rev[k] = np.asarray(g[k])[::-1].copy()
    rev["fsm0"] = {k: v[::-1].copy() for k, v in g["fsm0"].items()}
    back = loop_radio_model.run(oracle_mod, rev, 11)
    assert (back["leader"][::-1] != want["leader"]).sum() >= n // 4
    r = _run(s, g, 11)
    got = _state(s)
    _assert_equal(got, want, ALL)
    np.testing.assert_array_equal(r["counts"], want["counts"])
    assert (got["state"] == F).sum() >= n // 2


# 6b. few heard senders and many
@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["input", "spatial"])
def test_gpu_one_to_seven_heard_senders_are_handled_in_the_same_order(oracle_mod, layout):
    """The tick kernel keeps up to four heard senders in a sorted register list and merges the whole window
    when there are more: clusters of 2 .. 8 LEADERs, 50 apart, every member within range of the others, so
    that the receivers of a cluster hear 1 .. 7 heartbeats at tick 11 -- both sides of that threshold, and
    the threshold itself."""
    rng = np.random.default_rng(12)
    x, y = [], []
    for m in range(1, 8):
        for rep in range(3):  # three clusters of each size
            a, r = rng.uniform(0.0, 2.0 * np.pi, m + 1), rng.uniform(0.0, 1.0, m + 1)
            x.extend(50.0 * m + r * np.cos(a))
            y.extend(50.0 * (rep + 1) + r * np.sin(a))
    n = len(x)
    order = rng.permutation(n)  # a cluster's members at scattered indices
    x, y = np.array(x)[order], np.array(y)[order]
    g = _leaders_case(x, y, rng.permutation(n), seed=3)
    g["radio_radius"] = np.float64(2.5)
    rp, _ = sense_csr(oracle_mod, x, y, 2.5)
    assert sorted(set(np.diff(rp))) == [1, 2, 3, 4, 5, 6, 7]
    s = _swarm(g, layout)
    want = _model(oracle_mod, s, g, 11)
    r = _run(s, g, 11)
    got = _state(s)
    _assert_equal(got, want, ALL)
    np.testing.assert_array_equal(r["counts"], want["counts"])
    assert (got["state"] == F).sum() >= n // 2


# 7. moving out of range
@pytest.mark.gpu
def test_gpu_a_follower_that_leaves_its_leaders_range_times_out_and_leads_itself(oracle_mod):
    g = _leaders_case([10.0, 11.0], [10.0, 10.0], [5, 2])
    g["fsm0"] = dict(state=np.array([L, F], np.uint8), leader=np.array([5, -1], np.int32))
    g["has_t"], g["tx"], g["ty"] = np.array([0, 1], np.uint8), np.array([0.0, 100.0]), np.array([0.0, 10.0])
    g["radio_radius"], g["sense_radius"], g["ticks"] = np.float64(2.5), np.float64(1.0), np.int64(45)
    g["row_ptr"], g["col"] = np.array([0, 1, 2], np.int64), np.array([1, 0], np.int32)  # the graph of tick 0
    s = _swarm(g, "input")
    want = _model(oracle_mod, s, g, 45)
    r = _run(s, g, 45)
    got = _state(s)
    _assert_equal(got, want, ALL)
    np.testing.assert_array_equal(r["counts"], want["counts"])
    # out of range before the first heartbeat (tick 10): silence since 0.0, the failure detector fires, and
    # after its jitter delay the agent acclaims itself -- at the ticks the model gives
    assert got["state"][1] == L and got["leader"][1] == 2 and got["has_lpos"][1] == 0
    waits, leads = np.flatnonzero(r["counts"][:, 1] == 1), np.flatnonzero(r["counts"][:, 0] == 2)
    assert len(waits) and len(leads) and 29 <= waits[0] < leads[0] and r["counts"][leads[0], 2] == 1
    frozen = _swarm(g, "input", graph=True)  # the graph of tick 0 keeps delivering the leader's heartbeats
    frozen.update_loop_sensed(45, 1.0, **_kw(g))
    fz = _state(frozen)
    assert fz["state"][1] == F and fz["leader"][1] == 5 and fz["has_lpos"][1] == 1
    assert got["x"][1] != fz["x"][1]


# 8. resume, chaining and trace
@pytest.mark.gpu
def test_gpu_chunks_resume_one_run_chain_with_update_loop_and_trace_frames_are_the_runs_positions(oracle_mod):
    g = load_golden("loop_radio_n200")
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
    _assert_equal(_state(s), full, ALL)
    np.testing.assert_array_equal(np.concatenate([p["counts"] for p in parts]), r1["counts"])
    assert s.fsm_tick == one.fsm_tick == 112
    # twenty ticks of update_loop on the tick-0 graph (its rows the sensors too), then the radio loop, then the
    # sensed loop on that graph again: one run through fsm, fsm_tick and pos_prev
    c = _swarm(g, graph=True)
    want = _model(oracle_mod, c, g, plan=[(20, dict(reradio=False, resense=False)), (30, {}),
                                          (10, dict(reradio=False))])
    rs = [c.update_loop(20, **_kw(g)), _run(c, g, 30), c.update_loop_sensed(10, float(g["sense_radius"]), **_kw(g))]
    _assert_equal(_state(c), want, ALL)
    np.testing.assert_array_equal(np.concatenate([p["counts"] for p in rs]), want["counts"])
    assert c.fsm_tick == 60 and sum(p["singular"] for p in rs) == want["singular"]


# 9. dead and non-finite agents
@pytest.mark.gpu
def test_gpu_dead_agents_neither_send_nor_receive_but_are_sensed(oracle_mod):
    import torch
    g = _case(300, 9, 2.5, 1.0, n_obs=2)
    rng = np.random.default_rng(9)
    alive = (rng.uniform(size=300) < 0.6).astype(np.uint8)
    # far from the others: dead LEADER 0 half a unit from agent 1, which lives, has a target and hears nobody else
    g["x"][:2], g["y"][:2] = [500.0, 500.5], [500.0, 500.0]
    alive[:2] = [0, 1]
    g["has_t"][1], g["tx"][1], g["ty"][1] = 1, 520.0, 520.0
    state = np.where(rng.uniform(size=300) < 0.5, L, F).astype(np.uint8)
    state[:2] = [L, F]
    g["fsm0"] = dict(state=state, alive=alive, leader=np.where(state == L, g["ids"], -1).astype(np.int32))
    g["tick_off"][:] = 0  # every LEADER's heartbeat is due at tick 10: the dead ones' must not arrive
    g["kill_ticks"] = np.zeros(0, np.int64)
    s = _swarm(g, "input")
    s.pos_prev = s.pos.clone()  # (what the first call starts from anyway)
    before = _state(s)
    want = _model(oracle_mod, s, g, 12)
    r = _run(s, g, 12)
    got = _state(s)
    _assert_equal(got, want, ALL)
    np.testing.assert_array_equal(r["counts"], want["counts"])
    dead = alive == 0
    for k in ALL:  # a dead agent is frozen: FSM, position, motion
        np.testing.assert_array_equal(got[k][dead], before[k][dead], err_msg=k)
    assert got["leader"][1] != g["ids"][0]  # nothing arrived from the dead leader next to it
    far = _swarm(g, "input")  # ... but its body is sensed: with it out of the way agent 1 goes elsewhere
    far.pos[0] += 50.0
    _run(far, g, 12)
    assert not torch.equal(far.pos[1], s.pos[1])


@pytest.mark.gpu
def test_gpu_singular_tick_is_counted_and_a_later_chunk_returns(oracle_mod):
    g = _case(300, 5, 2.5, 2.5, n_obs=2)
    g["x"][7], g["y"][7] = g["x"][3], g["y"][3]  # two agents on one point ...
    for i, k in ((3, 40.0), (7, 50.0)):          # ... both with targets, so both compute the zero distance
        g["has_t"][i], g["tx"][i], g["ty"][i] = 1, k, k
    s = _swarm(g, "input")
    want = _model(oracle_mod, s, g, 3)
    assert want["singular"] >= 2 and not np.isfinite(want["x"][3]) and not np.isfinite(want["x"][7])
    r = _run(s, g, 3)
    assert r["singular"] == want["singular"]
    _assert_equal(_state(s), want, ALL)
    later = _model(oracle_mod, s, g, plan=[(3, {}), (9, {})])
    r2 = _run(s, g, 9)  # non-finite agents present: they hear nobody, nobody hears them, the call returns
    got = _state(s)
    _assert_equal(got, later, ALL)
    np.testing.assert_array_equal(np.concatenate([r["counts"], r2["counts"]]), later["counts"])
    assert r["singular"] + r2["singular"] == later["singular"]
    assert np.isfinite(later["x"]).sum() >= 290


# 10. refusal
@pytest.mark.gpu
def test_gpu_refused_tick_leaves_every_array_as_it_was():
    import torch
    from swarm_amd import _lib
    from swarm_amd.swarm import Swarm
    n = 1_200_000
    rng = np.random.default_rng(2)
    x, y = 3.0 + rng.uniform(0, 1e-3, n), -2.0 + rng.uniform(0, 1e-3, n)
    s = Swarm(np.arange(n, dtype=np.int32), x, y, layout="input", device="cuda")
    # every agent's failure detector fires at tick 1 (3.05 s of silence): the FSM kernels of all three ticks
    # would write the timers and the records, and the discard has something to undo
    s.protocol_reset(last_hb=np.full(n, -2.95))
    s.set_target(np.full(n, 9.0), np.full(n, 9.0))
    s.vel.fill_(0.25)
    s.pos_prev = s.pos + 0.5
    s._pos_prev_key = (s.pos, s.pos._version)
    s.fsm["outbox"][::3] = 1  # senders in flight in both halves: the receive kernel has to be held back
    keep = dict(pos=s.pos, pos_prev=s.pos_prev, vel=s.vel, target=s.target, has_target=s.has_target,
                state=s.state, leader=s.leader, **s.fsm)
    before = {k: v.clone() for k, v in keep.items()}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with pytest.raises(_lib.SwarmError) as e:
        s.update_loop_radio(3, 1.0, 1.0)
    torch.cuda.synchronize()
    assert time.perf_counter() - t0 < 20.0
    assert e.value.code == _lib.ERR_RANGE and "too dense" in str(e.value) and "tick 1" in str(e.value)
    assert s.last_refused_tick == 1 and s.fsm_tick == 0 and s.row_ptr is None
    for k, v in keep.items():
        assert torch.equal(v, before[k]), k
    assert keep["pos_prev"] is s.pos_prev and keep["pos"] is s.pos


# 11. no graph needed; trivial and bad arguments
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
    r = s.update_loop_radio(6, 1.0, 1.0)
    assert r["singular"] == 0 and not torch.equal(s.pos, x0) and r["counts"].shape == (6, 4)
    assert s.row_ptr is rp0 and s.col is col0 and (s.row_ptr._version, s.col._version) == v0
    assert torch.equal(s.row_ptr, rp_keep) and torch.equal(s.col, col_keep)
    assert s._cindex is None and s._pos_prev_key[0] is s.pos
    a = s.allocate(d["tx"], d["ty"], d["treq"])  # the agents moved: allocated from where they are now
    p = s.to_input_order(s.pos)
    want = oracle_mod.allocate(d["ids"], p[:, 0], p[:, 1], d["caps"], d["tx"], d["ty"], d["treq"])
    np.testing.assert_array_equal(a.winner.cpu().numpy(), want["winner"])
    np.testing.assert_array_equal(a.util.cpu().numpy(), want["util"])


@pytest.mark.gpu
def test_gpu_empty_swarm_zero_ticks_and_bad_radii():
    import torch
    from swarm_amd import _lib
    from swarm_amd.swarm import Swarm
    e = Swarm(np.zeros(0, np.int32), np.zeros(0), np.zeros(0), layout="input", device="cuda")
    r = e.update_loop_radio(5, 2.5, 2.5, trace_every=2)
    assert r["counts"].shape == (5, 4) and not r["counts"].any() and r["singular"] == 0
    assert r["trace"].shape == (2, 0, 2) and e.fsm_tick == 5 and e.last_refused_tick == -1
    g = load_golden("loop_radio_n200")
    s = _swarm(g)
    keep = dict(pos=s.pos, vel=s.vel, target=s.target, has_target=s.has_target, state=s.state, **s.fsm)
    before = {k: v.clone() for k, v in keep.items()}
    r = _run(s, g, 0)
    assert r["counts"].shape == (0, 4) and s.fsm_tick == 0
    run = lambda rc, rs: s._update_loop(4, rs, None, None, (), 0.1, 3.0, 0.2, 0, 5.0, "pull", 0.125, 0,  # noqa: E731
                                        radio_radius=rc)  # past the Python check: the entry point's own
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="radio_radius must be positive and finite"):
            s.update_loop_radio(4, bad, 2.5)
        with pytest.raises(_lib.SwarmError, match="radio_radius must be positive and finite") as err:
            run(bad, 2.5)
        assert err.value.code == _lib.ERR_ARG
        with pytest.raises(_lib.SwarmError, match="sense_radius must be positive and finite") as err:
            run(2.5, bad)
        assert err.value.code == _lib.ERR_ARG and s.fsm_tick == 0
    s.pos[5, 1] = float("inf")  # non-finite positions at entry: refused before anything is written
    before["pos"] = s.pos.clone()
    with pytest.raises(_lib.SwarmError, match="positions must be finite") as err:
        _run(s, g, 4)
    assert err.value.code == _lib.ERR_ARG and s.fsm_tick == 0
    for k, v in keep.items():
        assert torch.equal(v, before[k]), k
