"""The start of a sparse round and the launches between rounds (elect.hip): k_sparse_block's flat leading
arguments and late scalar guard, the 256-round stamp clear done inside the round before it, the initial
copies of ids dropped when rounds 1 and 2 are dense, and the fused read-back kernel.  None of it may change a
result: every case compares leaders, states, rounds_exec, converged and every per-round change count with
oracle.elect (agent.py:263-275 under contract E2).

The tunables are read once per process, so each setting runs in a child process (all started together):
the defaults, every lever switched on and every lever switched off at once, and with every lever on rounds
1-2 sparse (SWARM_DENSE_ROUNDS=0 / 1: the guard's t > 2 edge, the copies kept) and 2 048-stamp chunks for
small swarms (SWARM_SMALL_CHUNKS=1)."""
import json
import os
import subprocess
import sys

import pytest

from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

_CHILD = r"""
import ctypes, json, sys
import numpy as np
import torch
sys.path[:0] = [%r, %r]
from swarm_amd import _lib, gen
from swarm_amd.swarm import Swarm
from oracle import oracle
out = {}

def csr(s):
    return s.row_ptr.cpu().numpy().astype(np.int64), s.col.cpu().numpy(), s.ids.cpu().numpy()

def same(r, ref):
    lead, state, rounds, changes = ref
    return bool(r.converged and r.rounds_exec == rounds and np.array_equal(r.changes, changes)
                and np.array_equal(r.leader.cpu().numpy(), lead) and np.array_equal(r.state.cpu().numpy(), state))

def same_cut(r, rp, col, ids, ref, m):
    # a run of m rounds: the oracle's state after m rounds; converged only if the oracle is by then
    if m >= ref[2]:
        return same(r, ref)
    lead_m = oracle.elect(rp, col, ids, max_rounds=m)[0]
    state_m = np.where(lead_m == ids, _lib.LEADER, _lib.FOLLOWER).astype(np.uint8)
    return bool(not r.converged and r.rounds_exec == m and np.array_equal(r.changes, ref[3][:m])
                and np.array_equal(r.leader.cpu().numpy(), lead_m)
                and np.array_equal(r.state.cpu().numpy(), state_m))

# ---- guard: a 30 000-agent deg-16 swarm run to convergence (guarded no-op rounds are launched past the end)
d = gen.swarm_inputs(30_000, 11, deg=16.0, t=200)
s = Swarm(d["ids"], d["x"], d["y"], d["caps"], device="cuda:0").build_graph(1.0)
rp, col, ids = csr(s)
ref = oracle.elect(rp, col, ids)
R = ref[2]
out["guard-full-c16"] = same(s.elect(), ref)
out["guard-full-c32"] = same(s.elect(compact=False), ref)
out["guard-dense-mode"] = same(s.elect(mode="dense"), ref)
for name, m in (("at", R), ("before", R - 1), ("after", R + 1)):
    out["guard-max-" + name] = same_cut(s.elect(max_rounds=m), rp, col, ids, ref, m)
ok = same(s.elect(), ref)
s.allocate(d["tx"], d["ty"], d["treq"])  # other work on the same ctx's scratch between two elections
ok = ok and same(s.elect(), ref)
ok = ok and same(s.elect(), ref)
out["guard-three-elections"] = ok
# ---- rounds 1-2: max_rounds 1, 2, 3 (the result's buffer parity with and without the initial copies)
for m in (1, 2, 3):
    out["early-max-%%d" %% m] = (same_cut(s.elect(max_rounds=m), rp, col, ids, ref, m)
                               and same_cut(s.elect(max_rounds=m, mode="dense"), rp, col, ids, ref, m))
out["early-then-full"] = same(s.elect(), ref)
# ids and leader the same buffer, through the C ABI (the copies are kept for such a call).  The state output
# of an aliased call compares leader with the overwritten ids, so only leaders and counts are checked.
buf = s.ids.clone()
state = torch.empty(s.n, dtype=torch.uint8, device=buf.device)
rounds = ctypes.c_int32(0)
changes = np.zeros(1 << 12, np.int64)
rc = _lib.check(_lib.lib().swarm_elect(_lib.ctx(), s.n, _lib.ptr(s.row_ptr), _lib.ptr(s.col), _lib.ptr(buf),
                                       _lib.ptr(buf), _lib.ptr(state), len(changes), _lib.ELECT_FRONTIER,
                                       ctypes.byref(rounds), changes.ctypes.data_as(ctypes.c_void_p), None,
                                       _lib.stream()))
torch.cuda.synchronize()
out["early-ids-alias-leader"] = bool(rc == _lib.OK and rounds.value == R
                                     and np.array_equal(changes[:R], ref[3])
                                     and np.array_equal(buf.cpu().numpy(), ref[0]))

# ---- clears: a path of 1 100 agents takes 1 100 rounds, across the clear points 257/258 ... 1025/1026
def path(ids):
    n = len(ids)
    rp = np.concatenate([[0], np.cumsum([1] + [2] * (n - 2) + [1])]).astype(np.int64)
    col = np.concatenate([[1]] + [[i - 1, i + 1] for i in range(1, n - 1)] + [[n - 2]]).astype(np.int32)
    s = Swarm(ids, np.arange(float(n)), np.zeros(n), layout="input", device="cuda:0").set_graph(rp, col)
    return s, rp, col, oracle.elect(rp, col, ids)

asc = np.arange(1100, dtype=np.int32)
sp, prp, pcol, pref = path(asc)
out["clears-rounds"] = int(pref[2])
out["clears-path-ascending"] = same(sp.elect(), pref)
out["clears-cut-257"] = same_cut(sp.elect(max_rounds=257), prp, pcol, asc, pref, 257)
out["clears-cut-then-full"] = same(sp.elect(), pref)
rnd = np.random.default_rng(12).permutation(1100).astype(np.int32)
sp, prp, pcol, pref = path(rnd)
out["clears-path-random"] = same(sp.elect(), pref)

# ---- sizes: deg 3 (isolated agents, chains), 16-bit and int32 columns
for n in (1, 64, 65, 2048, 2049, 4097):
    dd = gen.swarm_inputs(n, 977 + n, deg=3.0)
    ss = Swarm(dd["ids"], dd["x"], dd["y"], device="cuda:0").build_graph(1.0)
    rr = oracle.elect(*csr(ss))
    for compact in (True, False):
        out["size-%%d-%%s" %% (n, "c16" if compact else "c32")] = same(ss.elect(compact=compact), rr)
print(json.dumps(out))
"""

_LEVERS = ("SWARM_GUARD_LATE", "SWARM_CLEAR_INLINE", "SWARM_SKIP_INIT_COPY", "SWARM_FUSED_READBACK")
_ON, _OFF = {k: "1" for k in _LEVERS}, {k: "0" for k in _LEVERS}
_RUNS = {"default": {}, "levers-on": _ON, "levers-off": _OFF,
         "dense-rounds-0": dict(_ON, SWARM_DENSE_ROUNDS="0"), "dense-rounds-1": dict(_ON, SWARM_DENSE_ROUNDS="1"),
         "large-chunks": dict(_ON, SWARM_SMALL_CHUNKS="1")}
_CASES = (["guard-full-c16", "guard-full-c32", "guard-dense-mode", "guard-max-at", "guard-max-before",
           "guard-max-after", "guard-three-elections", "early-max-1", "early-max-2", "early-max-3",
           "early-then-full", "early-ids-alias-leader", "clears-path-ascending", "clears-cut-257",
           "clears-cut-then-full", "clears-path-random"]
          + ["size-%d-%s" % (n, c) for n in (1, 64, 65, 2048, 2049, 4097) for c in ("c16", "c32")])


@pytest.fixture(scope="module")
def runs():
    procs = {k: subprocess.Popen([sys.executable, "-c", _CHILD % (PKG, ROOT)], env=dict(os.environ, **env),
                                 stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT)
             for k, env in _RUNS.items()}
    res = {}
    for k, p in procs.items():
        try:
            so, se = p.communicate(timeout=240)
        except subprocess.TimeoutExpired:
            for q in procs.values():
                q.kill()
            raise
        assert p.returncode == 0, (k, se[-3000:])
        res[k] = json.loads(so.strip().splitlines()[-1])
    return res


@pytest.mark.parametrize("case", _CASES)
@pytest.mark.parametrize("run", list(_RUNS))
def test_exact_against_oracle(runs, run, case):
    assert runs[run][case] is True, (run, case, runs[run])


def test_path_crosses_every_clear_point(runs):
    """The ascending path must still be changing at round 1 026, or the clear cases above test nothing."""
    for run in _RUNS:
        assert runs[run]["clears-rounds"] >= 1100, (run, runs[run]["clears-rounds"])
