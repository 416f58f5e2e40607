"""The lossy channel of the radio and task update loops, without a GPU (contract U1-L).

tests/golden/loop_lossy_*.npz were produced by real SwarmAgent objects driven through the task loop with the
one line `if dropped(...): continue` in the delivery (tools/gen_golden_loop_lossy.py, the draw restated on
Python integers).  The CPU model (tests/loop_lossy_model.py, the draw restated in numpy) must reproduce them
bit for bit with the reference's libm pow, must not change in anything discrete with the GPU's x*x squares, and
must be the two loss-free models at loss = 0.  The library's host export swarm_link_dropped -- the header
function the kernels call -- must give the model's verdicts (libswarm loads without a GPU).
"""
import ctypes

import numpy as np
import pytest

from conftest import load_golden
import loop_lossy_model
import loop_radio_model
import loop_tasks_model
from loop_model import OUT_KEYS
from test_update_loop_sensed import _assert_equal

LOSSY = ("loop_lossy_n200", "loop_lossy_wide_n400", "loop_lossy_p1_n200")
ALL = OUT_KEYS + ("px", "py")
TASK_ARRAYS = ("status", "tab_winner", "tab_util", "claim_out", "conflict_out")
DISCRETE = ("state", "leader", "has_lpos", "alive", "has_t")

_pow_models = {}


def _pow_model(oracle_mod, name):
    if name not in _pow_models:  # computed once, shared, left unchanged
        _pow_models[name] = loop_lossy_model.run(oracle_mod, load_golden(name), use_pow=True)
    return _pow_models[name]


@pytest.mark.parametrize("name", LOSSY)
def test_model_with_pow_equals_the_reference_fixture(oracle_mod, name):
    g = load_golden(name)
    o = _pow_model(oracle_mod, name)
    for k in OUT_KEYS:  # the thirteen arrays
        np.testing.assert_array_equal(o[k], g[k + "_out"], err_msg=k)
    np.testing.assert_array_equal(o["counts"], g["counts"])
    for k in ("status", "tab_winner"):
        np.testing.assert_array_equal(o[k], g[k + "_out"], err_msg=k)
    np.testing.assert_array_equal(o["tab_util"].view(np.uint32), g["tab_util_out"].view(np.uint32))
    for k in ("claim_out", "conflict_out", "task_counts", "link_counts"):
        np.testing.assert_array_equal(o[k], g[k], err_msg=k)
    assert o["singular"] == 0 and o["guard"] == 0


def test_fixtures_hold_what_they_were_chosen_for():
    g = load_golden("loop_lossy_n200")
    lc = g["link_counts"]
    assert float(g["loss"]) == 0.3 and int(g["ticks"]) == 120 and int(g["task_tick"]) == 45
    assert sorted(set(g["status_out"].ravel().tolist())) == [0, 1, 2, 3]
    n, p = lc[:, 0].sum(), 0.3  # the drops of the election links are a binomial sample
    assert n > 1000 and abs(lc[:, 1].sum() - n * p) <= 5.0 * np.sqrt(n * p * (1.0 - p))
    assert (lc[:, 1] <= lc[:, 0]).all() and (g["counts"][60:, 0] > g["counts"][59, 0]).any()
    w = load_golden("loop_lossy_wide_n400")
    assert float(w["loss"]) == 0.1 and int(w["ids"].max()) > 255 and int(w["ticks"]) == 120
    assert sorted(set(w["status_out"].ravel().tolist())) == [0, 1, 2, 3]
    p1 = load_golden("loop_lossy_p1_n200")
    al = p1["alive_out"] != 0
    assert float(p1["loss"]) == 1.0 and int(p1["ticks"]) == 60
    np.testing.assert_array_equal(p1["link_counts"][:, 0], p1["link_counts"][:, 1])
    assert p1["link_counts"].sum() > 0 and p1["task_counts"][:, 1:].sum() == 0
    assert (p1["state_out"][al] == 3).all() and (p1["leader_out"][al] == p1["ids"][al]).all()
    assert sorted(set(p1["status_out"].ravel().tolist())) == [0, 1]  # a claim nobody hears stays TENTATIVE


@pytest.mark.parametrize("name", LOSSY)
def test_squares_model_equals_the_pow_model_in_everything_discrete(oracle_mod, name):
    g = load_golden(name)
    a, b = _pow_model(oracle_mod, name), loop_lossy_model.run(oracle_mod, g, use_pow=False)
    for k in TASK_ARRAYS + ("task_counts", "counts", "link_counts") + DISCRETE:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert b["guard"] == 0


def test_loss_zero_equals_the_task_model_and_the_radio_model(oracle_mod):
    g = load_golden("loop_lossy_n200")
    a = loop_lossy_model.run(oracle_mod, g, 80, loss=0.0, loss_seed=77)
    b = loop_tasks_model.run(oracle_mod, g, 80)
    _assert_equal(a, b, ALL + TASK_ARRAYS)
    for k in ("counts", "task_counts"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert a["link_counts"][:, 1].sum() == 0 and a["link_counts"][:, 0].sum() > 0
    assert b["task_counts"].sum() > 0
    r = {k: v for k, v in g.items() if not k.startswith("task_") and k != "caps"}  # no board: the radio loop
    a, b = loop_lossy_model.run(oracle_mod, r, 80, loss=0.0, loss_seed=77), loop_radio_model.run(oracle_mod, r, 80)
    _assert_equal(a, b, ALL)
    np.testing.assert_array_equal(a["counts"], b["counts"])
    assert a["max_heard"] == b["max_heard"] and a["task_counts"].sum() == 0


def test_model_in_chunks_equals_one_run(oracle_mod):
    g = load_golden("loop_lossy_n200")
    one = loop_lossy_model.run(oracle_mod, g, 60)
    o, lc = None, []
    for chunk in (44, 1, 1, 3, 11):
        o = loop_lossy_model.run(oracle_mod, g, chunk, start=o)
        lc.append(o["link_counts"])
    _assert_equal(o, one, ALL + TASK_ARRAYS)
    np.testing.assert_array_equal(np.concatenate(lc), one["link_counts"])


def _tuples(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 1 << 40, n), rng.integers(-(1 << 31), 1 << 31, n).astype(np.int32),
            rng.integers(-(1 << 31), 1 << 31, n).astype(np.int32))


def test_library_rule_equals_the_python_rule():
    from swarm_amd import _lib
    lib = _lib.load()
    t, sid, rid = _tuples(100_000, 1)
    seeds = np.random.default_rng(2).integers(0, 1 << 63, 100_000).astype(np.uint64) * np.uint64(2) + np.uint64(1)
    for loss in (0.3, 0.0, 1.0):
        want = np.array([loop_lossy_model.dropped(int(seeds[0]), t, sid, rid, loss),
                         loop_lossy_model.dropped(0, t, sid, rid, loss)])
        got = np.array([[lib.swarm_link_dropped(ctypes.c_uint64(s), int(a), int(b), int(c), loss)
                         for a, b, c in zip(t, sid, rid)] for s in (int(seeds[0]), 0)], bool)
        np.testing.assert_array_equal(got, want)
        assert loss not in (0.0, 1.0) or (got == bool(loss)).all()
    # a seed of its own per tuple, small ticks and IDs as the loops use them
    t, sid, rid = t[:20_000] % 1000, np.abs(sid[:20_000]) % 512, np.abs(rid[:20_000]) % 512
    want = np.array([loop_lossy_model.dropped(int(s), int(a), int(b), int(c), 0.5)
                     for s, a, b, c in zip(seeds, t, sid, rid)])
    got = np.array([lib.swarm_link_dropped(ctypes.c_uint64(int(s)), int(a), int(b), int(c), 0.5)
                    for s, a, b, c in zip(seeds, t, sid, rid)], bool)
    np.testing.assert_array_equal(got, want)
    assert 0.45 < got.mean() < 0.55


@pytest.mark.parametrize("p", [0.05, 0.2, 0.5])
def test_drop_count_lies_within_the_binomial_bound(p):
    n = 1_000_000
    t, sid, rid = _tuples(n, 3)
    k = int(loop_lossy_model.dropped(12345, t % 100_000, sid, rid, p).sum())
    print("p", p, "dropped", k, "sigma", (k - n * p) / np.sqrt(n * p * (1.0 - p)))
    assert abs(k - n * p) <= 5.0 * np.sqrt(n * p * (1.0 - p))


def test_the_two_directions_of_a_pair_are_decided_independently():
    ids = np.arange(300, dtype=np.int32)
    s, r = np.meshgrid(ids, ids, indexing="ij")
    m = s < r
    n, p, diff, total = int(m.sum()) * 40, 0.5, 0, 0
    for t in range(1, 41):
        a, b = loop_lossy_model.dropped(9, t, s[m], r[m], p), loop_lossy_model.dropped(9, t, r[m], s[m], p)
        diff += int((a != b).sum())
        total += int(a.sum()) + int(b.sum())
    # independent fair verdicts differ on half the pairs; both are binomial bounds
    assert abs(diff - n * 0.5) <= 5.0 * np.sqrt(n * 0.25)
    assert abs(total - 2 * n * p) <= 5.0 * np.sqrt(2 * n * 0.25)


def test_bad_loss_is_refused_without_a_device():
    from swarm_amd import _lib
    from swarm_amd.swarm import Swarm
    lib = _lib.load()
    for bad in (-0.1, 1.5, float("nan")):
        ch = _lib.Channel(bad, 0)
        links = np.full((1, 2), -7, np.int64)
        rc = lib.swarm_update_loop_channel(None, 4, None, None, None, None, None, 0, 1, 0.1, 3.0, 0.2,
                                           ctypes.c_uint64(0), None, 0, None, None, None, 0, None, 2.5, 2.5, 5.0,
                                           None, 0, None, None, None, None, None, None, None, ctypes.byref(ch),
                                           links.ctypes.data_as(ctypes.c_void_p))
        assert rc == _lib.ERR_ARG and b"loss must be in [0, 1]" in lib.swarm_last_error()
        assert (links == -7).all()
        s = Swarm.__new__(Swarm)
        with pytest.raises(ValueError, match="loss must be in"):
            s.update_loop_radio(3, 2.5, 2.5, loss=bad)
        with pytest.raises(ValueError, match="loss must be in"):
            s.update_loop_tasks(3, 2.5, 2.5, loss=bad)
    assert ctypes.sizeof(_lib.Channel) == 16
