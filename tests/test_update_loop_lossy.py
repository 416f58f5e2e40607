"""The radio and task update loops over a lossy channel (contract U1-L):
swarm_update_loop_channel / Swarm.update_loop_radio(..., loss=, loss_seed=) and Swarm.update_loop_tasks(...).

Every comparison is against tests/loop_lossy_model.py with the GPU's x*x squares, run over the GPU's storage
order, bit for bit, in both layouts; in layout "input" also against the fixtures themselves
(tests/golden/loop_lossy_*.npz: real SwarmAgent objects, tools/gen_golden_loop_lossy.py).  The hand-built cases
are test_update_loop_tasks' resting agents in layout "input"; where a case needs particular links dropped, the
test searches loss_seed with the model's rule and says what it looked for.
"""
import ctypes
import time

import numpy as np
import pytest

from conftest import load_golden
import loop_lossy_model
from loop_lossy_model import dropped
from loop_model import OUT_KEYS, F, L
from test_update_loop_sensed import EXACT, PER_AGENT, _assert_equal, _state
from test_update_loop_tasks import ASSIGNED, LOCKED, OPEN, TENTATIVE, _assert_tasks, _hand, _kw, _swarm, _task_state

pytestmark = pytest.mark.gpu

LOSSY = ("loop_lossy_n200", "loop_lossy_wide_n400", "loop_lossy_p1_n200")
ALL = OUT_KEYS + ("px", "py")
W = 2  # ELECTION_WAIT


def _ch(g):
    return dict(loss=float(g["loss"]), loss_seed=int(g["loss_seed"]))


def _run(s, g, ticks, **kw):
    return s.update_loop_tasks(ticks, float(g["radio_radius"]), float(g["sense_radius"]), **_kw(g), **kw)


def _run_radio(s, g, ticks, **kw):
    return s.update_loop_radio(ticks, float(g["radio_radius"]), float(g["sense_radius"]), **_kw(g), **kw)


def _model(oracle_mod, s, g, ticks=None, plan=None, **kw):
    """loop_lossy_model.run over s's storage order, its per-agent results put back into input order."""
    perm = s.perm.cpu().numpy().astype(np.int64)
    q = dict(g)
    for k in PER_AGENT + ("caps",):
        q[k] = np.asarray(g[k])[perm]
    if "fsm0" in g:
        q["fsm0"] = {k: np.asarray(v)[perm] for k, v in g["fsm0"].items()}
    o, per_tick, singular, guard = None, {"counts": [], "task_counts": [], "link_counts": []}, 0, 0
    for chunk in (plan or [ticks]):
        o = loop_lossy_model.run(oracle_mod, q, chunk, start=o, **kw)
        for k in per_tick:
            per_tick[k].append(o[k])
        singular += o["singular"]
        guard += o["guard"]
    out = {}
    for k, v in o.items():
        if k in ("claim_out", "conflict_out"):
            out[k] = np.empty_like(v)
            out[k][:, perm] = v
        elif isinstance(v, np.ndarray) and k not in per_tick:
            out[k] = np.empty_like(v)
            out[k][perm] = v
        else:
            out[k] = v
    out.update({k: np.concatenate(v) for k, v in per_tick.items()}, singular=singular, guard=guard)
    return out


def _check(s, r, want, radio=False):
    """The swarm and the call's per-tick outputs against a model run."""
    _assert_equal(_state(s), want, ALL)
    np.testing.assert_array_equal(r["counts"], want["counts"])
    np.testing.assert_array_equal(r["link_counts"], want["link_counts"])
    assert r["singular"] == want["singular"]
    if not radio:
        _assert_tasks(_task_state(s), want)
        np.testing.assert_array_equal(r["task_counts"], want["task_counts"])
        assert r["guard"] == want["guard"]


def _cat(rs, k):
    return np.concatenate([r[k] for r in rs])


_models = {}


def _fixture_model(oracle_mod, s, name, layout, use_pow=False):
    key = (name, layout, use_pow)
    if key not in _models:  # once per storage order, shared, left unchanged
        _models[key] = _model(oracle_mod, s, load_golden(name), int(load_golden(name)["ticks"]), use_pow=use_pow)
    return _models[key]


# 1. the fixtures: the radio loop or an empty board up to the hand-out, then the board
@pytest.mark.parametrize("first", ["radio loop", "empty board"])
@pytest.mark.parametrize("layout", ["input", "spatial"])
@pytest.mark.parametrize("name", LOSSY)
def test_gpu_equals_the_model_and_the_reference_fixture(oracle_mod, name, layout, first):
    g = load_golden(name)
    s = _swarm(g, layout, board=False)
    head, ticks = int(g["task_tick"]) - 1, int(g["ticks"])
    if first == "radio loop":
        r0 = _run_radio(s, g, head, **_ch(g))
        assert "task_counts" not in r0
        r0["task_counts"] = np.zeros((head, 3), np.int64)
    else:
        s.set_tasks([], [])
        r0 = _run(s, g, head, **_ch(g))
        assert r0["task_counts"].sum() == 0 and r0["guard"] == 0
    assert r0["link_counts"].shape == (head, 2)
    s.set_tasks(g["task_x"], g["task_y"], g["task_req"])
    r1 = _run(s, g, ticks - head, **_ch(g))
    r = {k: _cat((r0, r1), k) for k in ("counts", "task_counts", "link_counts")}
    r.update(singular=r0["singular"] + r1["singular"], guard=r1["guard"])
    want = _fixture_model(oracle_mod, s, name, layout)
    _check(s, r, want)
    assert r["guard"] == 0 and r["singular"] == 0
    got, tk = _state(s), _task_state(s)
    if layout == "input":  # the fixture's own order: real agents, in everything the squares cannot reach
        for k in EXACT:
            np.testing.assert_array_equal(got[k], g[k + "_out"], err_msg=k)
        _assert_tasks(tk, dict(status=g["status_out"], tab_winner=g["tab_winner_out"], tab_util=g["tab_util_out"],
                               claim_out=g["claim_out"], conflict_out=g["conflict_out"]))
        for k in ("counts", "task_counts", "link_counts"):
            np.testing.assert_array_equal(r[k], g[k], err_msg=k)
    else:  # another order: the reference is the pow model over it (pinned to real agents on the CPU)
        ref = _fixture_model(oracle_mod, s, name, layout, use_pow=True)
        for k in EXACT:
            np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
        _assert_tasks(tk, ref)
        for k in ("task_counts", "link_counts"):  # (the walk order decides who leads: not the fixture's counts)
            np.testing.assert_array_equal(r[k], ref[k], err_msg=k)
    assert s.fsm_tick == ticks and s.last_refused_tick == -1 and s.row_ptr is None


# 2. loss = 0: the loss-free entry points, whatever the seed
@pytest.mark.parametrize("loop", ["radio", "tasks"])
def test_gpu_loss_zero_with_a_seed_equals_the_call_without_the_keywords(loop):
    import torch
    g = load_golden("loop_lossy_n200")
    a, b = _swarm(g, "spatial", board=loop == "tasks"), _swarm(g, "spatial", board=loop == "tasks")
    go = _run if loop == "tasks" else _run_radio
    ra, rb = go(a, g, 100, loss=0.0, loss_seed=987654321), go(b, g, 100)
    assert "link_counts" not in ra and set(ra) == set(rb)
    for t in ("pos", "pos_prev", "vel", "target", "has_target", "state", "leader"):
        assert torch.equal(getattr(a, t), getattr(b, t)), t
    for k in a.fsm:
        assert torch.equal(a.fsm[k], b.fsm[k]), k
    np.testing.assert_array_equal(ra["counts"], rb["counts"])
    if loop == "tasks":
        for k in a.tasks:
            if isinstance(a.tasks[k], torch.Tensor):
                assert torch.equal(a.tasks[k], b.tasks[k]), k
        np.testing.assert_array_equal(ra["task_counts"], rb["task_counts"])
        assert ra["task_counts"].sum() > 0


def _rest(s, g):
    st = _state(s)
    np.testing.assert_array_equal(st["x"], g["x"])  # at rest
    np.testing.assert_array_equal(st["y"], g["y"])
    return st


# 3. loss = 1: nobody ever hears anybody
def test_gpu_loss_one_makes_every_agent_the_leader_of_itself(oracle_mod):
    rng = np.random.default_rng(4)
    n = 50
    ids = rng.permutation(n) + 1
    g = _hand(np.stack([5.0 + rng.uniform(0, 1.5, n), 5.0 + rng.uniform(0, 1.5, n)], 1), ids, lead=(0,))
    s = _swarm(g, "input")
    r = _run_radio(s, g, 45, loss=1.0, loss_seed=5)
    st = _rest(s, g)
    # the one initial leader's heartbeats (ticks 10, 20, 30) reach nobody: all time out, wait, elect themselves
    np.testing.assert_array_equal(st["state"], np.full(n, L))
    np.testing.assert_array_equal(st["leader"], ids)
    assert not st["has_lpos"].any() and (st["last_hb"] == 0.0).all()
    lc = r["link_counts"]
    np.testing.assert_array_equal(lc[:, 1], lc[:, 0])
    np.testing.assert_array_equal(lc[[10, 20, 30], 0], [n - 1] * 3)  # one sender, 49 receivers
    assert lc[40, 0] == n * (n - 1) and r["counts"][-1].tolist()[:2] == [n, 0]  # tick 41: everyone's heartbeat
    _check(s, r, _model(oracle_mod, s, g, 45, loss=1.0, loss_seed=5), radio=True)


# 4. three lost heartbeats in a row: the failure detector's margin
def test_gpu_follower_misses_three_heartbeats_times_out_acclaims_and_yields_again(oracle_mod):
    """Agent 3 (index 0, FOLLOWER) and agent 9 (index 1, LEADER, heartbeats at ticks 10, 20, ...) at rest, in
    range, loss 0.5.  Wanted: 9 -> 3 kept at tick 11, dropped at 21, 31 and 41, kept at 51 -- agent 3 then
    times out at tick 41 (41 x 0.1 - 11 x 0.1 > 3.0 in fp64, after a receive that brought nothing), waits,
    elects itself and acclaims; and 3 -> 9 dropped at the tick
    after that acclaim, so that 9 stays LEADER, heartbeats at 50 and agent 3 yields again at tick 51."""
    g = _hand([(0, 0), (1, 0)], [3, 9], lead=(1,))
    seeds = np.arange(1, 20001)
    sd = np.array([[dropped(int(q), t, 9, 3, 0.5) for t in (11, 21, 31, 41, 51)] for q in seeds[:4000]])
    cand = seeds[:4000][(sd == [False, True, True, True, False]).all(1)]
    assert len(cand) >= 10
    s = _swarm(g, "input")
    seq = None
    for q in cand:  # the model decides: the acclaim's tick depends on the jitter
        o, rows = None, []
        for t in range(1, 56):
            o = loop_lossy_model.run(oracle_mod, g, 1, start=o, loss=0.5, loss_seed=int(q))
            rows.append({k: o[k].copy() for k in ("state", "leader", "last_hb", "wait_start", "delay", "link_counts")})
        st3 = [int(r_["state"][0]) for r_ in rows]
        st9 = [int(r_["state"][1]) for r_ in rows]
        if set(st9) == {L} and L in st3[40:50] and st3[50] == F and rows[50]["leader"][0] == 9:
            seq, seed = rows, int(q)
            break
    assert seq is not None, "no seed among the candidates"
    st3 = [int(r_["state"][0]) for r_ in seq]
    assert st3[:40] == [F] * 40 and st3[40] == W and st3[50:] == [F] * 5  # ticks 1..40, 41, 51..55
    first_l = st3.index(L) + 1
    assert first_l in (42, 43, 44) and st3[first_l - 1:50] == [L] * (51 - first_l)
    assert seq[10]["leader"][0] == 9 and seq[39]["last_hb"][0] == 11 * 0.1 and seq[40]["leader"][0] == -1
    assert seq[40]["wait_start"][0] == 41 * 0.1 and 0.0 <= seq[40]["delay"][0] < 0.2
    assert seq[50]["last_hb"][0] == 51 * 0.1 and dropped(seed, first_l + 1, 3, 9, 0.5)
    for t in range(1, 56):  # the GPU, tick by tick
        r = _run_radio(s, g, 1, loss=0.5, loss_seed=seed)
        st = _state(s)
        for k in ("state", "leader", "last_hb", "wait_start", "delay"):
            np.testing.assert_array_equal(st[k], seq[t - 1][k], err_msg="%s at tick %d" % (k, t))
        np.testing.assert_array_equal(r["link_counts"], seq[t - 1]["link_counts"], err_msg="tick %d" % t)
    _rest(s, g)


# 5. the two directions of a pair
def test_gpu_asymmetric_tick_one_leader_hears_the_other_and_yields(oracle_mod):
    """LEADERs A (ID 3) and B (ID 9) in range heartbeat at tick 10.  At tick 11 B -> A is kept and A -> B is
    dropped: A yields to B; B, which heard nothing, stays LEADER.  With the
    verdicts swapped (the same seed search, the other way round) A hears nothing and stays LEADER, and B, the
    higher ID, ignores A's heartbeat: two leaders remain."""
    g = _hand([(0, 0), (1, 0)], [3, 9], lead=(0, 1))
    fwd = next(q for q in range(1, 1000) if not dropped(q, 11, 9, 3, 0.5) and dropped(q, 11, 3, 9, 0.5))
    rev = next(q for q in range(1, 1000) if dropped(q, 11, 9, 3, 0.5) and not dropped(q, 11, 3, 9, 0.5))
    for seed, states, leaders in ((fwd, [F, L], [9, 9]), (rev, [L, L], [3, 9])):
        s = _swarm(g, "input")
        r = _run_radio(s, g, 11, loss=0.5, loss_seed=seed)
        st = _rest(s, g)
        np.testing.assert_array_equal(st["state"], states)
        np.testing.assert_array_equal(st["leader"], leaders)
        np.testing.assert_array_equal(r["link_counts"][10], [2, 1])
        assert r["link_counts"][:10].sum() == 0
        np.testing.assert_array_equal(st["last_hb"], [11 * 0.1 if states[0] == F else 0.0, 0.0])
        _check(s, r, _model(oracle_mod, s, g, 11, loss=0.5, loss_seed=seed), radio=True)


# 6. the conflict pass and the tick kernel reach the same verdict
def test_gpu_heartbeat_and_conflict_of_one_sender_are_dropped_or_heard_together(oracle_mod):
    """LEADER H (ID 99, heartbeats at tick 2) handles claimer C's claim at tick 2 and so sends a HEARTBEAT and a
    TASK_CONFLICT during tick 2.  Bystanders R1 (ID 5) and R2 (ID 6) lack the capability.  The seed keeps
    C -> H at tick 2 and H -> R2 at tick 3 and drops H -> R1 at tick 3: R1 gets neither the liveness proof nor
    the status change, R2 gets both -- the heartbeat is the tick kernel's, the conflict the conflict pass's."""
    g = _hand([(0, 0), (0.5, 0), (0, 0.5), (0.5, 0.5)], [99, 1, 5, 6], lead=(0,), caps=[0, 1, 0, 0],
              tasks=[(0.5, -1.0, 0)], off=[8, 0, 0, 0])
    seed = next(q for q in range(1, 1000) if not dropped(q, 2, 1, 99, 0.5) and dropped(q, 3, 99, 5, 0.5) and
                not dropped(q, 3, 99, 6, 0.5) and not dropped(q, 3, 99, 1, 0.5))
    s = _swarm(g, "input")
    r = _run(s, g, 3, loss=0.5, loss_seed=seed)
    st, tk = _rest(s, g), _task_state(s)
    np.testing.assert_array_equal(r["task_counts"], [[1, 0, 0], [0, 1, 1], [0, 0, 0]])
    np.testing.assert_array_equal(tk["status"][:, 0], [OPEN, ASSIGNED, OPEN, LOCKED])
    np.testing.assert_array_equal(st["leader"], [99, 99, -1, 99])
    np.testing.assert_array_equal(st["last_hb"], [0.0, 3 * 0.1, 0.0, 3 * 0.1])
    np.testing.assert_array_equal(st["has_lpos"], [0, 1, 0, 1])
    np.testing.assert_array_equal(r["link_counts"], [[0, 0], [0, 0], [3, 1]])
    _check(s, r, _model(oracle_mod, s, g, 3, loss=0.5, loss_seed=seed))


# 7. both paths of hear_window with senders dropped
@pytest.mark.parametrize("m", [1, 2, 3, 4, 5, 6, 7])
def test_gpu_one_to_seven_claimers_around_one_leader_with_some_links_dropped(oracle_mod, m):
    """test_update_loop_tasks' ring of m claimers around a LEADER (ID 99, index m): up to four in-range senders
    are handled from the sorted list, five or more by the merge.  The seed drops some of the m claims at tick 2
    and keeps some (m = 1: keeps it at one seed, drops it at another)."""
    ang = 2.0 * np.pi * np.arange(m) / 7.0
    rad = 0.3 * (np.arange(m) + 1.0)
    xy = [(50.0 + r_ * np.cos(a), 50.0 + r_ * np.sin(a)) for r_, a in zip(rad, ang)] + [(50.0, 50.0)]
    g = _hand(xy, list(range(1, m + 1)) + [99], lead=(m,), caps=[1] * m + [0], tasks=[(50.0, 50.0, 0)])
    lost = lambda q: dropped(q, 2, np.arange(1, m + 1), 99, 0.5)  # noqa: E731
    if m == 1:
        seeds = [next(q for q in range(1, 100) if lost(q)[0]), next(q for q in range(1, 100) if not lost(q)[0])]
    else:
        seeds = [next(q for q in range(1, 100) if 0 < lost(q).sum() < m)]
    for seed in seeds:
        kept = int((~lost(seed)).sum())
        s = _swarm(g, "input")
        r = _run(s, g, 3, loss=0.5, loss_seed=seed)
        _rest(s, g)
        want = _model(oracle_mod, s, g, 3, loss=0.5, loss_seed=seed)
        np.testing.assert_array_equal(r["task_counts"][:2], [[m, 0, 0], [0, kept, kept]])  # handled at tick 2
        tk = _task_state(s)
        first = int(np.flatnonzero(~lost(seed))[0]) + 1 if kept else -1
        assert tk["tab_winner"][m, 0] == first  # the nearest claimer that got through holds the entry
        assert (tk["status"][:m, 0] != OPEN).all() and tk["status"][m, 0] == OPEN
        _check(s, r, want)


# 8. an election storm in a dense block
def test_gpu_dense_block_in_an_election_storm_over_all_nine_cells(oracle_mod):
    """test_update_loop_tasks' block of 300 agents over three cells each way, every fifth a LEADER, the rest
    claimers whose failure detectors all fire at tick 1 (240 waiting, dozens of ACCLAIMs at tick 2): ACCLAIMs,
    heartbeats, claims and conflicts from dozens of senders per window, three in ten links dropped."""
    rng = np.random.default_rng(12)
    n = 300
    xy = np.stack([20.0 + rng.uniform(0.0, 7.4, n), 30.0 + rng.uniform(0.0, 7.4, n)], 1)
    tasks = [(20.0 + rng.uniform(0.0, 7.4), 30.0 + rng.uniform(0.0, 7.4), int(rng.integers(-1, 3))) for _ in range(12)]
    g = _hand(xy, rng.permutation(n), lead=tuple(range(0, n, 5)), caps=rng.integers(0, 8, n), tasks=tasks,
              off=rng.integers(0, 10, n))
    g["last_hb0"] = np.full(n, -2.95)
    s = _swarm(g, "input")
    want = _model(oracle_mod, s, g, 6, loss=0.3, loss_seed=31)
    lc, tc = want["link_counts"], want["task_counts"]
    assert want["max_heard"] >= 80 and want["counts"][0, 1] >= 200 and want["counts"][1, 2] >= 40 and lc[:, 0].sum() >= 4000
    assert abs(lc[:, 1].sum() - 0.3 * lc[:, 0].sum()) <= 5.0 * np.sqrt(lc[:, 0].sum() * 0.21)
    assert tc[0, 0] >= 500 and tc[:, 1].sum() >= 300 and tc[:, 2].sum() >= 300
    r = _run(s, g, 6, loss=0.3, loss_seed=31)
    _rest(s, g)
    _check(s, r, want)


# 9. chunks: the rule uses the absolute tick
@pytest.mark.parametrize("chunks", [(1, 1, 1, 1, 3, 8), (2, 2, 2, 9), (3, 12)])
def test_gpu_chunked_run_is_the_same_run(chunks):
    import torch
    g = load_golden("loop_lossy_n200")
    head = int(g["task_tick"]) - 1
    a, b = _swarm(g, "spatial"), _swarm(g, "spatial")
    ra0, rb0 = _run_radio(a, g, head, **_ch(g)), [_run_radio(b, g, c, **_ch(g)) for c in (21, 23)]
    np.testing.assert_array_equal(ra0["link_counts"], _cat(rb0, "link_counts"))
    ra = _run(a, g, sum(chunks), **_ch(g))
    rb = [_run(b, g, c, **_ch(g)) for c in chunks]
    assert ra["task_counts"][0, 0] > 0 and ra["task_counts"][:, 2].sum() > 0 and ra["link_counts"][:, 1].sum() > 0
    for t in ("pos", "pos_prev", "vel", "target", "has_target", "state", "leader"):
        assert torch.equal(getattr(a, t), getattr(b, t)), t
    for k in a.fsm:
        assert torch.equal(a.fsm[k], b.fsm[k]), k
    for k in a.tasks:
        if isinstance(a.tasks[k], torch.Tensor):
            assert torch.equal(a.tasks[k], b.tasks[k]), k
    for k in ("task_counts", "counts", "link_counts"):
        np.testing.assert_array_equal(ra[k], _cat(rb, k), err_msg=k)
    assert ra["guard"] == sum(r["guard"] for r in rb)


def _spy_link_counts(monkeypatch):
    """What swarm_update_loop_channel left in the caller's link_counts buffer, read when the call returns."""
    from swarm_amd import _lib
    lib, seen = _lib.lib(), {}
    real = lib.swarm_update_loop_channel

    def spy(*args):
        rc = real(*args)
        ticks = args[8]
        seen["rc"] = rc
        seen["link_counts"] = np.ctypeslib.as_array(ctypes.cast(args[-1], ctypes.POINTER(ctypes.c_int64)),
                                                    (ticks, 2)).copy()
        return rc
    monkeypatch.setattr(lib, "swarm_update_loop_channel", spy)
    return seen


# 10. the all-or-nothing refusal
def test_gpu_refused_tick_leaves_every_array_as_it_was_and_withholds_the_link_counts(monkeypatch):
    """test_update_loop_radio's too-dense swarm (a window work limit is only reached by a million agents in one
    cell), senders in flight in both outbox halves, loss 0.2."""
    import torch
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
    keep = dict(pos=s.pos, pos_prev=s.pos_prev, vel=s.vel, target=s.target, has_target=s.has_target,
                state=s.state, leader=s.leader, **s.fsm)
    before = {k: v.clone() for k, v in keep.items()}
    seen = _spy_link_counts(monkeypatch)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with pytest.raises(_lib.SwarmError) as e:
        s.update_loop_radio(3, 1.0, 1.0, loss=0.2, loss_seed=4)
    torch.cuda.synchronize()
    assert time.perf_counter() - t0 < 20.0
    assert e.value.code == _lib.ERR_RANGE and "too dense" in str(e.value) and "tick 1" in str(e.value)
    assert s.last_refused_tick == 1 and s.fsm_tick == 0 and s.row_ptr is None
    for k, v in keep.items():
        assert torch.equal(v, before[k]), k
    assert seen["rc"] == _lib.ERR_RANGE and not seen["link_counts"].any()


# 11. bad loss
@pytest.mark.parametrize("bad", [-0.1, 1.5, float("nan")])
def test_gpu_bad_loss_is_refused_and_nothing_is_written(monkeypatch, bad):
    import torch
    from swarm_amd import _lib, swarm as swarm_mod
    g = _hand([(0, 0), (0, 2)], [1, 9], lead=(1,), caps=[1, 0], tasks=[(1, 0, 0)])
    s = _swarm(g, "input")
    keep = dict(pos=s.pos, state=s.state, leader=s.leader, **s.fsm,
                **{k: v for k, v in s.tasks.items() if isinstance(v, torch.Tensor)})
    before = {k: v.clone() for k, v in keep.items()}
    for go in (_run, _run_radio):
        with pytest.raises(ValueError, match="loss must be in"):
            go(s, g, 3, loss=bad)
    # the library's own check: the value passed through as it is
    monkeypatch.setattr(swarm_mod, "_channel", lambda loss, seed: (float(loss), int(seed)))
    seen = _spy_link_counts(monkeypatch)
    for go in (_run, _run_radio):
        with pytest.raises(_lib.SwarmError) as e:
            go(s, g, 3, loss=bad)
        assert e.value.code == _lib.ERR_ARG and "loss must be in [0, 1]" in str(e.value)
        assert seen["rc"] == _lib.ERR_ARG and not seen["link_counts"].any()
    assert s.fsm_tick == 0
    for k, v in keep.items():
        assert torch.equal(v, before[k]), k


# 12. a large random swarm
def test_gpu_random_swarm_of_20001_agents_equals_the_model(oracle_mod):
    from test_update_loop_sensed import _random_case
    g = _random_case(20001, 23, ticks=40)
    rng = np.random.default_rng(5)
    lo, hi = g["x"].min(), g["x"].max()
    g.update(radio_radius=np.float64(2.5), sense_radius=np.float64(2.5), caps=rng.integers(0, 8, 20001).astype(np.uint32),
             task_x=rng.uniform(lo, hi, 24), task_y=rng.uniform(lo, hi, 24),
             task_req=rng.integers(-1, 3, 24).astype(np.int8))
    s = _swarm(g, "spatial")
    want = _model(oracle_mod, s, g, 40, loss=0.2, loss_seed=2024)
    tc, lc = want["task_counts"], want["link_counts"]
    assert tc[:, 0].sum() >= 100 and tc[:, 1].sum() >= 20 and tc[:, 2].sum() >= 20 and want["guard"] == 0
    assert lc[:, 0].sum() >= 10000 and abs(lc[:, 1].sum() - 0.2 * lc[:, 0].sum()) <= 5.0 * np.sqrt(lc[:, 0].sum() * 0.16)
    r = _run(s, g, 40, loss=0.2, loss_seed=2024)
    _check(s, r, want)
    assert r["guard"] == 0
