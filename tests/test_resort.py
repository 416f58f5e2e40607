"""Restoring the spatial storage order of a moved swarm (contract R1): Swarm.resort() and the three
library calls under it, swarm_resort_plan / swarm_permute_rows / swarm_graph_relabel.

The reference has no storage order (its agents live in a Python list), so the references here are: numpy for the
row permutation and the relabelled graph; a fresh Swarm constructed from the input-order view of the state, which
contract R1 says the resorted swarm equals byte for byte; the CPU models of the update loops, run over storage
order A up to the resort and over storage order B after it; and the election / allocation oracle.
"""
import ctypes

import numpy as np
import pytest

from conftest import load_golden
import loop_lossy_model
import loop_sensed_model
import loop_tasks_model
from loop_model import FSM_KEYS, OUT_KEYS, F, L
from loop_sensed_model import sense_csr
from test_update_loop_sensed import PER_AGENT, _assert_equal, _random_case, _state

ALL = OUT_KEYS + ("px", "py")
MOTION = ("x", "y", "px", "py", "vx", "vy", "tx", "ty", "has_t")


# ----------------------------------------------------------------------------- helpers without a device

def _relabel_np(rp, col, frm):
    """swarm_graph_relabel restated: out row k = in row frm[k], columns through the inverse, row order kept."""
    rp, col, frm = np.asarray(rp, np.int64), np.asarray(col, np.int64), np.asarray(frm, np.int64)
    n = len(frm)
    to = np.empty(n, np.int64)
    to[frm] = np.arange(n)
    deg = np.diff(rp)[frm]
    out = np.zeros(n + 1, np.int64)
    np.cumsum(deg, out=out[1:])
    flat = np.repeat(rp[:-1][frm] - out[:-1], deg) + np.arange(out[-1])
    return out.astype(np.int32), to[col[flat]].astype(np.int32)


def _loop_model(oracle, q, ticks, start=None, resense=True):
    """loop_sensed_model.run (resense) or loop_model.run with the message graph as the sensors (resense=False),
    restated with a `start` state as loop_tasks_model.run has one: the dict this function returned, so that a
    run can go on -- in another storage order, after _reorder_state."""
    ids = np.asarray(q["ids"], np.int32)
    n = len(ids)
    radius = float(q["sense_radius"])
    rp, col = np.asarray(q["row_ptr"], np.int64), np.asarray(q["col"], np.int32)
    dt, ms, seed = float(q["dt"]), float(q["max_speed"]), int(q["seed"])
    if start is None:
        t0 = 0
        x, y = np.array(q["x"], np.float64), np.array(q["y"], np.float64)
        px, py = x.copy(), y.copy()
        vx, vy = np.zeros(n), np.zeros(n)
        tx, ty = np.array(q["tx"], np.float64), np.array(q["ty"], np.float64)
        has_t = np.array(q["has_t"], np.uint8)
        fsm = dict(last_hb=np.array(q["last_hb0"], np.float64))
        fsm.update({k: np.array(v) for k, v in q.get("fsm0", {}).items()})
    else:
        t0 = int(start["tick"])
        x, y, px, py, vx, vy, tx, ty = (np.array(start[k], np.float64) for k in MOTION[:-1])
        has_t = np.array(start["has_t"], np.uint8)
        fsm = {k: np.array(v) for k, v in start["fsm"].items()}
    counts = np.zeros((ticks, 4), np.int64)
    singular = 0
    ids2 = np.concatenate([ids, ids])
    lead_rows = np.arange(n, 2 * n, dtype=np.int32)
    z = np.zeros(n)
    for t in range(t0 + 1, t0 + ticks + 1):
        o = oracle.protocol(ids, px, py, rp, col, q["tick_off"], 1, t0=t - 1, dt=dt, timeout=3.0, jitter=0.2,
                            seed=seed, kill_ticks=q["kill_ticks"], **fsm)
        counts[t - t0 - 1] = o.pop("counts")[0]
        fsm = o
        alive = fsm["alive"] != 0
        follows = alive & (fsm["state"] == F) & (fsm["has_lpos"] != 0)
        lp = fsm["lpos"].astype(np.float64)
        srp, scol = sense_csr(oracle, x, y, radius) if resense else (rp, col)
        ph = oracle.physics(
            ids2, np.concatenate([fsm["state"], np.full(n, L, np.uint8)]),
            np.concatenate([np.where(follows, lead_rows, -1).astype(np.int32), np.full(n, -1, np.int32)]),
            np.concatenate([x, lp[:, 0]]), np.concatenate([y, lp[:, 1]]), np.concatenate([vx, z]),
            np.concatenate([vy, z]), np.concatenate([tx, z]), np.concatenate([ty, z]),
            np.concatenate([np.where(alive, has_t, 0).astype(np.uint8), np.zeros(n, np.uint8)]),
            q["obs"], np.concatenate([srp, np.full(n, srp[-1], np.int64)]), scol, dt=dt, max_speed=ms, steps=1,
            use_pow=False)
        singular += ph["singular"]
        px, py = x, y
        x, y, vx, vy, tx, ty = (ph[k][:n].copy() for k in ("x", "y", "vx", "vy", "tx", "ty"))
        has_t = np.where(alive, ph["has_t"][:n], has_t).astype(np.uint8)
    out = {k: fsm[k] for k in FSM_KEYS}
    out.update(fsm=fsm, x=x, y=y, vx=vx, vy=vy, tx=tx, ty=ty, has_t=has_t, counts=counts, singular=singular, px=px,
               py=py, tick=t0 + ticks)
    return out


def _reorder_state(o, frm):
    """A model result over storage order A as the `start` of a run over order B, row k of B being row frm[k] of A.
    Nothing in it is a storage index (leaders and winners are IDs), so the rows move and that is all."""
    frm = np.asarray(frm, np.int64)
    n = len(frm)
    out = dict(tick=o["tick"])
    for k in MOTION:
        out[k] = np.asarray(o[k])[frm]
    out["fsm"] = {k: (np.concatenate([v[:n][frm], v[n:][frm]]) if k == "outbox" else np.asarray(v)[frm])
                  for k, v in o["fsm"].items()}
    if "tasks" in o:
        out["tasks"] = {k: (v[frm] if isinstance(v, np.ndarray) else [list(v[f]) for f in frm])
                        for k, v in o["tasks"].items()}
    return out


def _case_in_order(g, perm, graph=None):
    """The fixture-style case g with its per-agent inputs in the storage order perm (and the graph given)."""
    q = dict(g)
    for k in PER_AGENT + (("caps",) if "caps" in g else ()):
        q[k] = np.asarray(g[k])[perm]
    if "fsm0" in g:
        q["fsm0"] = {k: np.asarray(v)[perm] for k, v in g["fsm0"].items()}
    if graph is not None:
        q["row_ptr"], q["col"] = np.asarray(graph[0], np.int64), np.asarray(graph[1], np.int32)
    return q


def _agents_to_input(o, perm):
    """A model result's per-agent arrays (the task sets as (2, n)) from storage order perm into input order."""
    out = {}
    for k, v in o.items():
        if k in ("claim_out", "conflict_out"):
            out[k] = np.empty_like(v)
            out[k][:, perm] = v
        elif isinstance(v, np.ndarray) and k not in ("counts", "task_counts", "link_counts"):
            out[k] = np.empty_like(v)
            out[k][perm] = v
        else:
            out[k] = v
    return out


# ----------------------------------------------------------------------------- CPU

def test_exports_and_struct_size():
    from swarm_amd import _lib
    lib = _lib.load()
    for name in ("swarm_permute_rows", "swarm_graph_relabel", "swarm_resort_plan"):
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    with open(_lib.INCLUDE_H) as f:
        text = f.read()
    assert "typedef struct swarm_rows" in text
    assert ctypes.sizeof(_lib.Rows) == 24  # two pointers and an int64: 64 of them fit a kernel's arguments


def test_entry_points_refuse_bad_arguments_without_a_device():
    from swarm_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(8)  # never dereferenced: the arguments below are refused first
    rows = (_lib.Rows * 1)(_lib.Rows(0x10000, 0x20000, 4))

    def refused(rc, text):
        return rc == _lib.ERR_ARG and text in lib.swarm_last_error()
    assert refused(lib.swarm_permute_rows(None, 4, fake, 1, rows, None), b"ctx is NULL")
    assert refused(lib.swarm_permute_rows(fake, 4, fake, 65, rows, None), b"[0, 64]")
    assert refused(lib.swarm_permute_rows(fake, 4, fake, -1, rows, None), b"[0, 64]")
    for rb in (0, 16385):
        bad = (_lib.Rows * 1)(_lib.Rows(0x10000, 0x20000, rb))
        assert refused(lib.swarm_permute_rows(fake, 4, fake, 1, bad, None), b"[1, 16384]")
    assert refused(lib.swarm_permute_rows(fake, 1 << 31, fake, 1, rows, None), b"2^31")
    assert refused(lib.swarm_permute_rows(fake, 4, None, 1, rows, None), b"from is NULL")
    assert refused(lib.swarm_permute_rows(fake, 4, None, 0, None, None), b"from is NULL")
    assert refused(lib.swarm_permute_rows(fake, 4, fake, 1, None, None), b"arrays is NULL")
    null = (_lib.Rows * 1)(_lib.Rows(None, 0x20000, 4))
    assert refused(lib.swarm_permute_rows(fake, 4, fake, 1, null, None), b"NULL src / dst")
    over = (_lib.Rows * 1)(_lib.Rows(0x10000, 0x10008, 4))  # 4 rows of 4 bytes: the last 8 src bytes
    assert refused(lib.swarm_permute_rows(fake, 4, fake, 1, over, None), b"overlaps a src")
    two = (_lib.Rows * 2)(_lib.Rows(0x10000, 0x20000, 4), _lib.Rows(0x30000, 0x2000c, 8))
    assert refused(lib.swarm_permute_rows(fake, 4, fake, 2, two, None), b"another dst")
    onfrom = (_lib.Rows * 1)(_lib.Rows(0x10000, 16, 4))
    assert refused(lib.swarm_permute_rows(fake, 4, fake, 1, onfrom, None), b"overlaps from")
    assert refused(lib.swarm_graph_relabel(None, 4, fake, fake, fake, fake, fake, None), b"ctx is NULL")
    assert refused(lib.swarm_graph_relabel(fake, 1 << 31, fake, fake, fake, fake, fake, None), b"2^31")
    assert refused(lib.swarm_graph_relabel(fake, 4, fake, None, fake, fake, fake, None), b"row_ptr")
    assert refused(lib.swarm_graph_relabel(fake, 4, None, 0x10000, fake, 0x20000, fake, None), b"from is NULL")
    assert refused(lib.swarm_graph_relabel(fake, 4, 0x30000, 0x10000, fake, 0x10008, fake, None), b"overlaps")
    moved = ctypes.c_int64(-7)
    assert refused(lib.swarm_resort_plan(None, 4, fake, fake, 1.0, fake, fake, ctypes.byref(moved), None),
                   b"ctx is NULL")
    assert refused(lib.swarm_resort_plan(fake, 4, fake, fake, 0.0, fake, fake, ctypes.byref(moved), None), b"cell")
    assert refused(lib.swarm_resort_plan(fake, 4, fake, fake, 1.0, fake, fake, None, None), b"moved is NULL")
    assert refused(lib.swarm_resort_plan(fake, 4, None, fake, 1.0, fake, fake, ctypes.byref(moved), None), b"NULL")
    assert refused(lib.swarm_resort_plan(fake, 4, 0x10000, 0x20000, 1.0, 0x20004, 0x30000, ctypes.byref(moved),
                                         None), b"overlaps")
    assert moved.value == -7


def test_resort_refuses_the_input_layout_without_a_device():
    from swarm_amd.swarm import Swarm
    s = Swarm.__new__(Swarm)  # no device needed: the layout is checked before anything else
    s.layout = "input"
    with pytest.raises(ValueError, match="layout='input'"):
        s.resort()


def test_model_with_a_start_state_equals_the_models_it_restates(oracle_mod):
    """_loop_model in chunks is loop_sensed_model.run, and with resense=False a frozen-sensor run."""
    g = load_golden("loop_sensed_n200")
    one = loop_sensed_model.run(oracle_mod, g, 45)
    o = _loop_model(oracle_mod, g, 31)
    o = _loop_model(oracle_mod, g, 14, start=_reorder_state(o, np.arange(200)))
    _assert_equal(o, one, ALL)
    np.testing.assert_array_equal(o["counts"], one["counts"][31:])
    import loop_model
    fixed = loop_model.run(oracle_mod, g, 45)
    o = _loop_model(oracle_mod, g, 45, resense=False)
    _assert_equal(o, fixed, ALL)


def test_relabel_restatement_on_a_hand_graph():
    rp, col = [0, 2, 2, 5], [2, 1, 0, 2, 1]  # row 2 unsorted, with a self loop
    out_rp, out_col = _relabel_np(rp, col, [2, 0, 1])  # new 0 = old 2, new 1 = old 0, new 2 = old 1
    np.testing.assert_array_equal(out_rp, [0, 3, 5, 5])
    np.testing.assert_array_equal(out_col, [1, 0, 2, 0, 2])


# ----------------------------------------------------------------------------- GPU

def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _froms(n):
    rng = np.random.default_rng(n)
    return dict(identity=np.arange(n), reversal=np.arange(n)[::-1], rotation=np.roll(np.arange(n), 1),
                shuffle=rng.permutation(n))


def _permute(n, frm, pairs):
    """swarm_permute_rows over (src address, dst address, row_bytes) triples."""
    from swarm_amd import _lib
    arr = (_lib.Rows * max(len(pairs), 1))(*[_lib.Rows(*p) for p in pairs])
    return _lib.lib().swarm_permute_rows(_lib.ctx(), n, _lib.ptr(frm) if frm is not None else None, len(pairs), arr,
                                         _lib.stream())


def _check_widths(n, frm, widths, offset=0):
    """One call over a random array per width (src and dst `offset` bytes into their buffers); numpy's rows."""
    import torch
    from swarm_amd import _lib
    rng = np.random.default_rng(1000 * n + len(widths))
    src_np = [rng.integers(0, 256, (n, w), dtype=np.uint8) for w in widths]
    src = [torch.zeros(n * w + 16, dtype=torch.uint8, device="cuda") for w in widths]
    dst = [torch.full((n * w + 16,), 0xA5, dtype=torch.uint8, device="cuda") for w in widths]
    for t, a in zip(src, src_np):
        t[offset:offset + a.size] = _dev(a.ravel())
    frm_t = _dev(np.asarray(frm, np.int32))
    rc = _permute(n, frm_t, [(s.data_ptr() + offset, d.data_ptr() + offset, w) for s, d, w in zip(src, dst, widths)])
    assert rc == _lib.OK, _lib.last_error()
    for d, a, w in zip(dst, src_np, widths):
        got = d.cpu().numpy()
        np.testing.assert_array_equal(got[offset:offset + n * w].reshape(n, w), a[np.asarray(frm)], err_msg=str(w))
        assert (got[:offset] == 0xA5).all() and (got[offset + n * w:] == 0xA5).all(), w  # nothing past the rows


# 1. the row permutation against numpy
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097, 100_003])
def test_gpu_permute_rows_equals_numpy(n):
    for name, frm in _froms(n).items():
        # narrow and wide rows mixed in one call: one narrow launch, a 4-byte path (12, 20, 260), a 16-byte one (64)
        _check_widths(n, frm, [1, 2, 4, 8, 16, 12, 20, 64, 260])
        if n <= 4097:
            _check_widths(n, frm, [3, 7, 16, 4], offset=1)  # misaligned bases: the byte path, narrow widths too


@pytest.mark.gpu
def test_gpu_permute_rows_widest_row_and_the_counts():
    import torch
    from swarm_amd import _lib
    for frm in _froms(65).values():
        _check_widths(65, frm, [16384])
    n = 4097
    frm = _froms(n)["shuffle"]
    _check_widths(n, frm, [1 + (k % 5 == 0) * 3 + (k % 7 == 0) * 4 for k in range(64)])  # 64 arrays: 1, 4, 5, 8 wide
    _check_widths(n, frm, [16] * 17)  # more than one batch of the narrow kernel
    assert _permute(n, _dev(frm.astype(np.int32)), []) == _lib.OK  # count 0
    assert _permute(0, None, []) == _lib.OK
    src = torch.zeros(64, dtype=torch.uint8, device="cuda")
    assert _permute(0, None, [(src.data_ptr(), src.data_ptr(), 4)]) == _lib.OK  # n == 0: nothing is looked at


# 2. refusals leave the outputs as they were
@pytest.mark.gpu
@pytest.mark.parametrize("bad", ["duplicate", "n", "minus_one"])
def test_gpu_a_from_that_is_no_permutation_is_refused_and_nothing_is_written(bad):
    import torch
    from swarm_amd import _lib
    n = 4097
    frm = _froms(n)["shuffle"].astype(np.int32)
    frm[77] = dict(duplicate=frm[4000], n=n, minus_one=-1)[bad]
    frm_t = _dev(frm)
    src = [torch.zeros(n * w, dtype=torch.uint8, device="cuda") for w in (4, 20, 3)]
    dst = [torch.full((n * w,), 0xA5, dtype=torch.uint8, device="cuda") for w in (4, 20, 3)]
    rc = _permute(n, frm_t, [(s.data_ptr(), d.data_ptr(), w) for s, d, w in zip(src, dst, (4, 20, 3))])
    assert rc == _lib.ERR_ARG
    assert ("twice" if bad == "duplicate" else "outside [0, n)") in _lib.last_error()
    for d in dst:
        assert bool((d == 0xA5).all())
    rp, col = _dev(np.arange(n + 1, dtype=np.int32)), _dev(np.arange(n, dtype=np.int32))
    rpo = torch.full((n + 1,), -3, dtype=torch.int32, device="cuda")
    colo = torch.full((n,), -3, dtype=torch.int32, device="cuda")
    rc = _lib.lib().swarm_graph_relabel(_lib.ctx(), n, _lib.ptr(frm_t), _lib.ptr(rp), _lib.ptr(col), _lib.ptr(rpo),
                                        _lib.ptr(colo), _lib.stream())
    assert rc == _lib.ERR_ARG and bool((rpo == -3).all()) and bool((colo == -3).all())


@pytest.mark.gpu
@pytest.mark.parametrize("bad", ["n", "minus_one", "row_ptr"])
def test_gpu_relabel_refuses_a_bad_graph_and_writes_nothing(bad):
    import torch
    from swarm_amd import _lib
    n = 1000
    rng = np.random.default_rng(3)
    deg = rng.integers(0, 9, n)
    rp = np.zeros(n + 1, np.int32)
    rp[1:] = np.cumsum(deg)
    col = rng.integers(0, n, rp[-1]).astype(np.int32)
    if bad == "row_ptr":
        rp[500] = rp[499] - 1
    else:
        col[rp[-1] - 1 if bad == "n" else 17] = n if bad == "n" else -1
    frm_t = _dev(rng.permutation(n).astype(np.int32))
    rpo = torch.full((n + 1,), -3, dtype=torch.int32, device="cuda")
    colo = torch.full((int(rp[-1]),), -3, dtype=torch.int32, device="cuda")
    rp_t, col_t = _dev(rp), _dev(col)  # (held: a temporary's memory would be handed to the next tensor)
    rc = _lib.lib().swarm_graph_relabel(_lib.ctx(), n, _lib.ptr(frm_t), _lib.ptr(rp_t), _lib.ptr(col_t),
                                        _lib.ptr(rpo), _lib.ptr(colo), _lib.stream())
    assert rc == _lib.ERR_ARG and ("row_ptr" if bad == "row_ptr" else "column") in _lib.last_error()
    assert bool((rpo == -3).all()) and bool((colo == -3).all())


# 3. the relabelled graph against the numpy restatement
def _relabel_gpu(n, frm, rp, col):
    import torch
    from swarm_amd import _lib
    frm_t, rp_t, col_t = _dev(np.asarray(frm, np.int32)), _dev(np.asarray(rp, np.int32)), _dev(np.asarray(col, np.int32))
    rpo = torch.full((n + 1,), -3, dtype=torch.int32, device="cuda")
    colo = torch.full((len(col),), -3, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib().swarm_graph_relabel(
        _lib.ctx(), n, _lib.ptr(frm_t) if n else None, _lib.ptr(rp_t), _lib.ptr(col_t) if len(col) else None,
        _lib.ptr(rpo), _lib.ptr(colo) if len(col) else None, _lib.stream()))
    return rpo.cpu().numpy(), colo.cpu().numpy()


@pytest.mark.gpu
def test_gpu_relabel_equals_the_numpy_restatement():
    from swarm_amd import gen
    rng = np.random.default_rng(8)
    # a 5 000-agent radius graph
    d = gen.swarm_inputs(5000, 5)
    rp, col = gen.rgg_csr(d["x"], d["y"], 1.0)
    for frm in (rng.permutation(5000), np.arange(5000)[::-1]):
        got = _relabel_gpu(5000, frm, rp, col)
        want = _relabel_np(rp, col, frm)
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])
    # directed, unsorted rows, empty rows (whole 64-row tasks of them too), one row of 300 neighbours
    n = 1000
    deg = rng.integers(0, 12, n)
    deg[rng.uniform(size=n) < 0.3] = 0
    deg[128:260] = 0
    deg[401] = 300
    deg[-1] = 0
    rp = np.zeros(n + 1, np.int64)
    rp[1:] = np.cumsum(deg)
    col = rng.integers(0, n, rp[-1])
    frm = rng.permutation(n)
    got, want = _relabel_gpu(n, frm, rp, col), _relabel_np(rp, col, frm)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    # n = 1 (with a self loop), E = 0, n = 0
    got = _relabel_gpu(1, [0], [0, 2], [0, 0])
    np.testing.assert_array_equal(got[0], [0, 2])
    np.testing.assert_array_equal(got[1], [0, 0])
    got = _relabel_gpu(70, rng.permutation(70), np.zeros(71, np.int64), np.zeros(0, np.int64))
    np.testing.assert_array_equal(got[0], np.zeros(71))
    got = _relabel_gpu(0, [], [0], [])
    np.testing.assert_array_equal(got[0], [0])


# ---- a fresh twin: the Swarm one would construct from the input-order view of another's state

PARITY = {("fsm", "outbox"), ("tasks", "claim_out"), ("tasks", "conflict_out"), ("board", "claim_out"),
          ("board", "conflict_out")}
PER_AGENT_ATTRS = ("ids", "pos", "caps", "leader", "state", "vel", "target", "has_target", "pos_prev", "tick_off")
PER_AGENT_KEYS = dict(fsm=("last_hb", "wait_start", "delay", "leader_pos", "has_leader_pos", "alive", "outbox"),
                      tasks=("status_lo", "status_hi", "tab_winner", "tab_util", "claim_out", "conflict_out"),
                      board=("status", "tab_task", "tab_winner", "tab_util", "claim_out", "conflict_out"))


def _arrays(s):
    """Every per-agent array s holds: {name: (tensor, halves)}."""
    out = {a: (getattr(s, a), 1) for a in PER_AGENT_ATTRS if hasattr(s, a)}
    for d, keys in PER_AGENT_KEYS.items():
        if hasattr(s, d):
            out.update({f"{d}.{k}": (getattr(s, d)[k], 2 if (d, k) in PARITY else 1) for k in keys})
    return out


def _input_view(s):
    """in(A) of every per-agent array, by numpy on the host (the parity halves each on their own)."""
    perm = s.perm.cpu().numpy().astype(np.int64)
    out = {}
    for name, (t, halves) in _arrays(s).items():
        a = t.cpu().numpy()
        v = np.empty_like(a)
        for h in range(halves):
            v[h * s.n:(h + 1) * s.n][perm] = a[h * s.n:(h + 1) * s.n]
        out[name] = v
    return out


def _fresh_twin(s, graph_in=None):
    """A Swarm constructed from the input-order view of s's state; graph_in: the (row_ptr, col) over input indices
    that s.set_graph was given.  The task board's handle is shared (s outlives the twin in these tests)."""
    import torch
    from swarm_amd.swarm import Swarm
    view = _input_view(s)
    t = Swarm(view["ids"], view["pos"][:, 0].copy(), view["pos"][:, 1].copy(), view["caps"].view(np.uint32),
              cell=s.cell, device="cuda")
    perm = t.perm.cpu().numpy().astype(np.int64)

    def stored(name):
        halves = _arrays(s)[name][1]
        a = view[name]
        return _dev(np.concatenate([a[h * s.n:(h + 1) * s.n][perm] for h in range(halves)]))
    for name in ("ids", "pos", "caps"):  # what the constructor stored: the same bytes by the host gather
        assert torch.equal(getattr(t, name), stored(name)), name
    for name in PER_AGENT_ATTRS[3:]:
        if name in view:
            setattr(t, name, stored(name))
    if "pos_prev" in view:
        t._pos_prev_key = (t.pos, t.pos._version)
    for d in PER_AGENT_KEYS:
        if hasattr(s, d):
            q = dict(getattr(s, d))
            q.update({k: stored(f"{d}.{k}") for k in PER_AGENT_KEYS[d]})
            setattr(t, d, q)
    for name in ("fsm_tick", "task_ids", "board_task_ids", "last_board_overflow"):
        if hasattr(s, name):
            setattr(t, name, getattr(s, name))
    if graph_in is not None:
        t.set_graph(*graph_in)
    return t


def _assert_same_swarm(a, b):
    """Array for array, byte for byte (the graph and the hearers included)."""
    import torch
    assert torch.equal(a.perm, b.perm)
    xs, ys = _arrays(a), _arrays(b)
    assert sorted(xs) == sorted(ys)
    for name in xs:
        x, y = xs[name][0], ys[name][0]
        assert x.dtype == y.dtype and x.shape == y.shape, name
        assert torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)), name
    assert (a.row_ptr is None) == (b.row_ptr is None)
    if a.row_ptr is not None:
        assert torch.equal(a.row_ptr, b.row_ptr) and torch.equal(a.col, b.col)
        ha, hb = getattr(a, "_hear", None), getattr(b, "_hear", None)
        assert (ha is None) == (hb is None)
        if ha is not None:
            assert torch.equal(ha[0], hb[0]) and torch.equal(ha[1], hb[1])


def _board_case(n, seed, ticks, T=24, kills=(10,)):
    g = _random_case(n, seed, ticks=ticks)
    rng = np.random.default_rng(seed + 1)
    lo, hi = g["x"].min(), g["x"].max()
    g.update(radio_radius=np.float64(2.5), sense_radius=np.float64(2.5), kill_ticks=np.asarray(kills, np.int64),
             caps=rng.integers(0, 8, n).astype(np.uint32), task_x=rng.uniform(lo, hi, T),
             task_y=rng.uniform(lo, hi, T), task_req=rng.integers(-1, 3, T).astype(np.int8))
    return g


def _kw(g):
    return dict(obstacles=g["obs"], kill_ticks=g["kill_ticks"], dt=float(g["dt"]), seed=int(g["seed"]),
                max_speed=float(g["max_speed"]))


# 4. R1, array for array
@pytest.mark.gpu
def test_gpu_resort_is_the_fresh_swarm_of_the_input_order_state():
    from test_update_loop_tasks import _swarm
    n = 20_000
    g = _board_case(n, 31, ticks=16, T=200)
    rng = np.random.default_rng(4)
    # the message graph: the radius graph with a third of its edges dropped in one direction only, rows shuffled
    rows = np.repeat(np.arange(n), np.diff(g["row_ptr"]))
    keep = (rows < g["col"]) | (rng.uniform(size=len(rows)) < 0.66)
    order = np.lexsort((rng.uniform(size=keep.sum()), rows[keep]))
    col_in = g["col"][keep][order]
    rp_in = np.zeros(n + 1, np.int64)
    rp_in[1:] = np.cumsum(np.bincount(rows[keep], minlength=n))
    s = _swarm(g, "spatial", board=False)
    s.set_graph(rp_in, col_in)
    assert s._hear is not None
    s.set_task_board(g["task_x"], g["task_y"], g["task_req"], status_slots=16, table_slots=16)
    r = s.update_loop_board(12, 2.5, 2.5, **_kw(g))  # elections by tick 9, the kill at tick 10
    assert r["counts"][:, 0].max() > 0 and r["task_counts"][:, 0].sum() > 0
    t64 = np.random.default_rng(6)
    s.set_tasks(t64.uniform(g["x"].min(), g["x"].max(), 64), t64.uniform(g["x"].min(), g["x"].max(), 64),
                t64.integers(-1, 3, 64).astype(np.int8))
    r = s.update_loop_tasks(3, 2.5, 2.5, **_kw(g))
    assert r["task_counts"][:, 0].sum() > 0
    s.update_loop(1, **_kw(g))  # the fixed graph's loop on the directed lists; pos_prev stays valid
    before, perm0, olds = _input_view(s), s.perm.clone(), {k: v[0] for k, v in _arrays(s).items()}
    assert "pos_prev" in before and "board.conflict_out" in before and "tasks.tab_util" in before
    assert (before["tasks.claim_out"] != 0).any() and (before["board.status"] >= 0).any()
    assert (before["tasks.status_lo"] != 0).any() and (before["fsm.alive"] == 0).any()
    s.resort()
    assert s.last_resort_moved > 0 and s.resorts == 1
    assert not bool((s.perm == perm0).all())
    after = _input_view(s)
    assert sorted(after) == sorted(before)
    for k in before:  # in(A) is bit for bit what it was
        np.testing.assert_array_equal(after[k].view(np.uint8), before[k].view(np.uint8), err_msg=k)
    for k, v in _arrays(s).items():  # replaced, never overwritten
        assert v[0] is not olds[k] and v[0].data_ptr() != olds[k].data_ptr(), k
    twin = _fresh_twin(s, (rp_in, col_in))
    _assert_same_swarm(s, twin)
    assert s._pos_prev_key[0] is s.pos and s._cindex is None and s._id_index is None
    # a second resort moves nothing and keeps every tensor
    now = {k: v[0] for k, v in _arrays(s).items()}
    graph = (s.row_ptr, s.col, s.perm)
    s.resort()
    assert s.last_resort_moved == 0 and s.resorts == 1
    assert all(v[0] is now[k] for k, v in _arrays(s).items())
    assert s.row_ptr is graph[0] and s.col is graph[1] and s.perm is graph[2]
    # ... and the loops go on from it exactly as from the twin
    ra, rb = s.update_loop_board(4, 2.5, 2.5, **_kw(g)), twin.update_loop_board(4, 2.5, 2.5, **_kw(g))
    np.testing.assert_array_equal(ra["counts"], rb["counts"])
    _assert_same_swarm(s, twin)


# 5. continuity against the CPU models: order A up to the resort, order B after it
def _orders(s, perm_a):
    """(perm_b, frm): s's storage order after a resort, and the row of order A that each of its rows was."""
    perm_b = s.perm.cpu().numpy().astype(np.int64)
    inv_a = np.empty(s.n, np.int64)
    inv_a[perm_a] = np.arange(s.n)
    return perm_b, inv_a[perm_b]


def _task_case(name):
    g = dict(load_golden(name))
    g["task_tick"] = np.int64(1)  # the board is there from the first tick
    return g


@pytest.mark.gpu
@pytest.mark.parametrize("loop", ["tasks", "board"])
def test_gpu_task_loops_go_on_after_a_resort_as_the_model_does(oracle_mod, loop):
    import test_update_loop_board as tb
    import test_update_loop_tasks as tt
    g = _task_case("loop_board_n200" if loop == "board" else "loop_tasks_n200")
    T, t1, t2 = len(g["task_x"]), 70, 30
    kw = dict(loss=0.2, loss_seed=77) if loop == "board" else {}
    s = tt._swarm(g, "spatial", board=loop == "tasks")
    if loop == "board":
        tb._board(s, g, T, T)
    run = (lambda k: tb._run(s, g, k, **kw)) if loop == "board" else (lambda k: tt._run(s, g, k))
    model = (lambda q, k, st: loop_lossy_model.run(oracle_mod, q, k, start=st, **kw)) if loop == "board" else \
        (lambda q, k, st: loop_tasks_model.run(oracle_mod, q, k, start=st))
    perm_a = s.perm.cpu().numpy().astype(np.int64)
    r1 = run(t1)
    m1 = model(_case_in_order(g, perm_a), t1, None)
    np.testing.assert_array_equal(r1["task_counts"], m1["task_counts"])
    assert m1["task_counts"][-1].sum() > 0 or m1["task_counts"][-2].sum() > 0  # task messages in flight
    s.resort()
    assert s.last_resort_moved > 0
    perm_b, frm = _orders(s, perm_a)
    r2 = run(t2)
    m2 = model(_case_in_order(g, perm_b), t2, _reorder_state(m1, frm))
    assert m2["task_counts"].sum(0).min() > 0 and m2["counts"][:, 2:].sum() > 0  # all of it goes on after the resort
    for k in ("counts", "task_counts") + (("link_counts",) if loop == "board" else ()):
        np.testing.assert_array_equal(r2[k], m2[k], err_msg=k)
    assert r2["guard"] == m2["guard"] and r2["singular"] == m2["singular"] and s.fsm_tick == t1 + t2
    if loop == "board":
        want = tb._to_input(m2, perm_b, T, T)
        _assert_equal(_state(s), want, ALL)
        tb._assert_rows(tb._rows(s), want["rows"])
    else:
        want = _agents_to_input(m2, perm_b)
        _assert_equal(_state(s), want, ALL)
        tt._assert_tasks(tt._task_state(s), want)


@pytest.mark.gpu
@pytest.mark.parametrize("loop", ["sensed", "fixed"])
def test_gpu_graph_loops_go_on_after_a_resort_as_the_model_does(oracle_mod, loop):
    from test_update_loop_sensed import _run, _swarm
    g = load_golden("loop_sensed_n200")
    t1, t2 = 60, 40
    s = _swarm(g)
    radius = {} if loop == "sensed" else dict(sense_radius=None)
    perm_a = s.perm.cpu().numpy().astype(np.int64)
    graph_a = (s.row_ptr.cpu().numpy(), s.col.cpu().numpy())
    inv_a = np.empty(s.n, np.int64)
    inv_a[perm_a] = np.arange(s.n)
    np.testing.assert_array_equal(graph_a[1], _relabel_np(g["row_ptr"], g["col"], perm_a)[1])
    r1 = _run(s, g, t1, **radius)
    m1 = _loop_model(oracle_mod, _case_in_order(g, perm_a, graph_a), t1, resense=loop == "sensed")
    np.testing.assert_array_equal(r1["counts"], m1["counts"])
    s.resort()
    assert s.last_resort_moved > 0
    perm_b, frm = _orders(s, perm_a)
    graph_b = _relabel_np(g["row_ptr"], g["col"], perm_b)  # from the input graph: what set_graph would hold
    np.testing.assert_array_equal(s.row_ptr.cpu().numpy(), graph_b[0])
    np.testing.assert_array_equal(s.col.cpu().numpy(), graph_b[1])
    r2 = _run(s, g, t2, **radius)
    m2 = _loop_model(oracle_mod, _case_in_order(g, perm_b, graph_b), t2, start=_reorder_state(m1, frm),
                     resense=loop == "sensed")
    np.testing.assert_array_equal(r2["counts"], m2["counts"])
    assert r2["singular"] == m2["singular"] == 0 and s.fsm_tick == t1 + t2
    _assert_equal(_state(s), _agents_to_input(m2, perm_b), ALL)
    assert m2["counts"][:, 3].sum() > 0 and (m2["x"] != m1["x"][frm]).sum() >= 50  # heartbeats and motion after it


# 6. twin run: resort in the middle against a rebuild in the middle
@pytest.mark.gpu
def test_gpu_a_run_with_a_resort_equals_the_run_rebuilt_from_its_input_order_state():
    from test_update_loop_tasks import _swarm
    g = _board_case(5001, 23, ticks=60, kills=(10, 50))
    a, b = _swarm(g, "spatial", board=False), _swarm(g, "spatial", board=False)
    for s in (a, b):
        s.set_task_board(g["task_x"], g["task_y"], g["task_req"], status_slots=8, table_slots=8)
    run = lambda s, k: s.update_loop_board(k, 2.5, 2.5, loss=0.1, loss_seed=5, **_kw(g))  # noqa: E731
    ra, rb = run(a, 30), run(b, 30)
    np.testing.assert_array_equal(ra["task_counts"], rb["task_counts"])
    a.resort()
    assert a.last_resort_moved > 0
    c = _fresh_twin(b)
    _assert_same_swarm(a, c)
    ra, rc = run(a, 30), run(c, 30)
    for k in ("counts", "task_counts", "link_counts"):
        np.testing.assert_array_equal(ra[k], rc[k], err_msg=k)
    assert ra["guard"] == rc["guard"] and ra["singular"] == rc["singular"]
    assert ra["task_counts"][:, 0].sum() > 0 and bool((a.fsm["alive"] == 0).any())  # claims go on; a kill behind
    _assert_same_swarm(a, c)
    assert a.fsm_tick == c.fsm_tick == 60


# 7. the headline after motion
@pytest.mark.gpu
def test_gpu_election_and_allocation_after_a_fold_find_their_fast_paths_again(oracle_mod):
    import torch
    from swarm_amd import gen
    from swarm_amd.swarm import Swarm
    d = gen.swarm_inputs(120_000, 11, t=1500)
    s = Swarm(d["ids"], d["x"], d["y"], d["caps"], device="cuda")
    y = s.pos[:, 1]
    s.pos[:, 1] = torch.where(y > d["side"] / 2, d["side"] - y, y)  # in place: the upper half onto the lower
    s.build_graph(1.0)
    assert s.graph_compact() is None  # neighbours up to ~n rows apart: the 16-bit deltas do not fit

    def oracle_elect():
        return oracle_mod.elect(s.row_ptr.cpu().numpy().astype(np.int64), s.col.cpu().numpy(), s.ids.cpu().numpy())
    r0 = s.elect()
    lead, state, rounds, changes = oracle_elect()
    assert r0.compact is False and r0.rounds_exec == rounds
    np.testing.assert_array_equal(r0.changes, changes)
    np.testing.assert_array_equal(r0.leader.cpu().numpy(), lead)
    np.testing.assert_array_equal(r0.state.cpu().numpy(), state)
    lead0, state0 = s.to_input_order(r0.leader), s.to_input_order(r0.state)
    s.resort()
    assert s.last_resort_moved > s.n // 4
    s.build_graph(1.0)
    r1 = s.elect()
    lead, state, rounds, changes = oracle_elect()
    assert r1.compact is True and r1.rounds_exec == rounds == r0.rounds_exec
    np.testing.assert_array_equal(r1.changes, changes)
    np.testing.assert_array_equal(r1.changes, r0.changes)
    np.testing.assert_array_equal(r1.leader.cpu().numpy(), lead)
    np.testing.assert_array_equal(r1.state.cpu().numpy(), state)
    np.testing.assert_array_equal(s.to_input_order(r1.leader), lead0)
    np.testing.assert_array_equal(s.to_input_order(r1.state), state0)
    a = s.allocate(d["tx"], d["ty"], d["treq"])
    assert s._cindex not in (None, False)  # the indexed path
    want = oracle_mod.allocate_binned(s.ids.cpu().numpy(), s.pos[:, 0].cpu().numpy(), s.pos[:, 1].cpu().numpy(),
                                      s.caps.cpu().numpy().view(np.uint32), d["tx"], d["ty"], d["treq"],
                                      use_pow=False)
    for k in ("winner", "nclaim", "nmsg", "won"):
        np.testing.assert_array_equal(getattr(a, k).cpu().numpy(), want[k], err_msg=k)
    np.testing.assert_array_equal(a.util.cpu().numpy(), want["util"])
    assert (want["winner"] >= 0).sum() > 100


# 8. edge cases
@pytest.mark.gpu
def test_gpu_a_nan_position_is_refused_and_nothing_is_replaced():
    import torch
    from swarm_amd import _lib, gen
    from swarm_amd.swarm import Swarm
    d = gen.swarm_inputs(3000, 2)
    s = Swarm(d["ids"], d["x"], d["y"], d["caps"], device="cuda").build_graph(1.0)
    s.protocol_reset()
    s.pos[:, 0] = s.pos[:, 0].flip(0)
    for bad in (float("nan"), float("inf")):
        s.pos[1234, 1] = bad
        held = dict(vars(s))
        fsm = dict(s.fsm)
        pos = s.pos.clone()
        with pytest.raises(_lib.SwarmError) as e:
            s.resort()
        assert e.value.code == _lib.ERR_ARG
        assert vars(s).keys() == held.keys() and all(vars(s)[k] is held[k] for k in held)
        assert all(s.fsm[k] is fsm[k] for k in fsm) and s.resorts == 0
        assert torch.equal(s.pos.view(torch.int64), pos.view(torch.int64))
    s.pos[1234, 1] = 1.0
    assert s.resort().last_resort_moved > 0 and s.resorts == 1


@pytest.mark.gpu
def test_gpu_tiny_and_bare_swarms():
    import torch
    from swarm_amd import gen
    from swarm_amd.swarm import Swarm
    for n in (0, 1):
        s = Swarm(np.arange(n, dtype=np.int32), np.full(n, 2.5), np.full(n, 3.5), device="cuda")
        held = (s.ids, s.pos, s.perm)
        assert s.resort() is s and s.last_resort_moved == 0 and s.resorts == 0
        assert all(x is y for x, y in zip((s.ids, s.pos, s.perm), held))
    # no fsm, no motion, no task state, no graph: ids / pos / caps / leader / state only
    d = gen.swarm_inputs(5000, 9)
    s = Swarm(d["ids"], d["x"], d["y"], d["caps"], device="cuda")
    assert s.resort().last_resort_moved == 0  # a fresh swarm is in its order
    s.leader.copy_(s.ids // 3)
    s.state.copy_((s.ids % 3 + 1).to(torch.uint8))
    s.pos[:, 0] = s.pos[:, 0].flip(0)
    before = _input_view(s)
    assert sorted(before) == ["caps", "ids", "leader", "pos", "state"]
    s.resort()
    assert s.last_resort_moved > 1000 and s.row_ptr is None and not hasattr(s, "pos_prev")
    after = _input_view(s)
    for k in before:
        np.testing.assert_array_equal(after[k].view(np.uint8), before[k].view(np.uint8), err_msg=k)
    _assert_same_swarm(s, _fresh_twin(s))
    # two agents of one cell that swapped rows: the order inside a cell is the input order
    s = Swarm([7, 8, 9], [0.2, 0.4, 5.0], [0.2, 0.4, 5.0], device="cuda")
    s.pos[0, 0], s.pos[2, 0] = 5.1, 0.3  # input agent 0 leaves the cell, agent 2 joins agent 1 in it
    s.pos[0, 1], s.pos[2, 1] = 5.1, 0.3
    s.resort()
    assert s.perm.tolist() == [1, 2, 0] and s.ids.tolist() == [8, 9, 7] and s.last_resort_moved == 3
