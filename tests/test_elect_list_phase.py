"""The list phase of a sparse round (elect.hip, k_sparse_block): marked lanes from one shift per stamp word and
a scalar past-the-end test (SWARM_LIST_FAST), empty waves that skip the scan (SWARM_LIST_VOTE), list slices
reserved by one LDS add per wave behind one barrier (SWARM_LIST_ATOMIC), and the counter flush that skips quiet
waves (SWARM_FLUSH_VOTE) or adds per wave (SWARM_FLUSH_WAVE).  None of it may change a result: every case
compares leaders, states, rounds_exec, converged and every per-round change count with oracle.elect
(agent.py:263-275 under contract E2).  The listed sets are the same whatever the levers, so active_total and
edges_total of a case must be EQUAL between the all-on and the all-off run.

The tunables are read once per process, so each setting runs in a child process, six in all, started together:
the defaults, every new lever on and every new lever off over the main cases (512-stamp chunks at these
sizes); the list-overflow cases (SWARM_SPARSE_BLOCKS=2, SWARM_DENSE_ROUNDS=1: round 1 changes ~94 % of a
30 000-agent swarm, so each of the two workgroups lists ~15 000 agents in round 2, past the 4 096 entries of
the list, over more chunks than it preloads at once) with every lever on and with every lever off; and one
workgroup (SWARM_SPARSE_BLOCKS=1) with every lever on, 2 048-stamp chunks (SWARM_SMALL_CHUNKS=1) and the
stamp clear done inside the round (SWARM_CLEAR_INLINE=1) over the overflow cases and the paths."""
import json
import os
import subprocess
import sys

import pytest

from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

_PATHS = (1, 2, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4097)

_CHILD = r"""
import json, sys
import numpy as np
sys.path[:0] = [%r, %r]
from swarm_amd import _lib, gen
from swarm_amd.swarm import Swarm
from oracle import oracle
sections = sys.argv[1].split(",")
out = {}

def csr(s):
    return s.row_ptr.cpu().numpy().astype(np.int64), s.col.cpu().numpy(), s.ids.cpu().numpy()

def same(r, ref):
    lead, state, rounds, changes = ref
    return bool(r.converged and r.rounds_exec == rounds and np.array_equal(r.changes, changes)
                and np.array_equal(r.leader.cpu().numpy(), lead) and np.array_equal(r.state.cpu().numpy(), state))

def same_cut(r, rp, col, ids, ref, m):
    lead_m = oracle.elect(rp, col, ids, max_rounds=m)[0]
    state_m = np.where(lead_m == ids, _lib.LEADER, _lib.FOLLOWER).astype(np.uint8)
    return bool(not r.converged and r.rounds_exec == m and np.array_equal(r.changes, ref[3][:m])
                and np.array_equal(r.leader.cpu().numpy(), lead_m)
                and np.array_equal(r.state.cpu().numpy(), state_m))

def put(name, r, ok):
    out[name] = {"ok": bool(ok), "active": int(r.active_total), "edges": int(r.edges_total),
                 "rounds": int(r.rounds_exec), "chg1": int(r.changes[0]) if len(r.changes) else 0}

# paths with ascending IDs: agent i hears i - 1 and i + 1; the top ID walks down one agent per round, so a
# round marks one or two agents and every wave but one is empty, for n - 1 rounds
def path(n):
    ids = np.arange(n, dtype=np.int32)
    s = Swarm(ids, np.arange(float(n)), np.zeros(n), layout="input", device="cuda:0")
    if n == 1:  # one agent that hears nobody
        rp, col = np.zeros(2, np.int64), np.zeros(0, np.int32)
        s.build_graph(0.5)
    else:
        rp = np.concatenate([[0], np.cumsum([1] + [2] * (n - 2) + [1])]).astype(np.int64)
        col = np.concatenate([[1]] + [[i - 1, i + 1] for i in range(1, n - 1)] + [[n - 2]]).astype(np.int32)
        s.set_graph(rp, col)
    r = s.elect()
    put("path-%%d" %% n, r, same(r, oracle.elect(rp, col, ids)))

if "paths" in sections:
    for n in %r:
        path(n)
    path(700)  # 699 rounds: across the 256-round stamp clear at 257/258 and 513/514

def geo(n, seed, deg, cuts):
    d = gen.swarm_inputs(n, seed, deg=deg)
    s = Swarm(d["ids"], d["x"], d["y"], device="cuda:0").build_graph(1.0)
    rp, col, ids = csr(s)
    ref = oracle.elect(rp, col, ids)
    if cuts:  # cut runs leave stamps behind; the full runs follow them on the same swarm
        for m in (8, 9, 10, 11, ref[2] - 3):
            r = s.elect(max_rounds=m)
            put("geo-%%d-cut-%%s" %% (n, m if m < 12 else "R-3"), r, same_cut(r, rp, col, ids, ref, m))
    for compact in (True, False):
        r = s.elect(compact=compact)
        put("geo-%%d-%%s" %% (n, "c16" if compact else "c32"), r, same(r, ref))

if "geo" in sections:
    geo(50_000, 13, 3.0, False)   # deg 3: rows of length 0, chains; past-the-end masks of the interleaved layout
    geo(30_000, 11, 16.0, True)
    geo(65_537, 12, 16.0, False)
if "overflow" in sections:
    geo(30_000, 11, 16.0, False)
print(json.dumps(out))
""" % (PKG, ROOT, _PATHS)

_LEVERS = ("SWARM_LIST_FAST", "SWARM_LIST_VOTE", "SWARM_LIST_ATOMIC", "SWARM_FLUSH_VOTE", "SWARM_FLUSH_WAVE")
_ON, _OFF = {k: "1" for k in _LEVERS}, {k: "0" for k in _LEVERS}
_TWO = {"SWARM_SPARSE_BLOCKS": "2", "SWARM_DENSE_ROUNDS": "1"}
# name -> (environment, sections)
_RUNS = {"default": ({}, "paths,geo"), "levers-on": (_ON, "paths,geo"), "levers-off": (_OFF, "paths,geo"),
         "overflow-on": (dict(_ON, **_TWO), "overflow"), "overflow-off": (dict(_OFF, **_TWO), "overflow"),
         "one-workgroup-on": (dict(_ON, SWARM_SPARSE_BLOCKS="1", SWARM_DENSE_ROUNDS="1", SWARM_SMALL_CHUNKS="1",
                                   SWARM_CLEAR_INLINE="1"), "overflow,paths")}
_PATH_CASES = ["path-%d" % n for n in _PATHS + (700,)]
_GEO_CASES = (["geo-50000-c16", "geo-50000-c32"] + ["geo-30000-cut-%s" % m for m in (8, 9, 10, 11, "R-3")]
              + ["geo-30000-c16", "geo-30000-c32", "geo-65537-c16", "geo-65537-c32"])
_OVER_CASES = ["geo-30000-c16", "geo-30000-c32"]
_SECTION_CASES = {"paths": _PATH_CASES, "geo": _GEO_CASES, "overflow": _OVER_CASES}
_PAIRS = [(run, case) for run, (_, sections) in _RUNS.items() for sec in sections.split(",")
          for case in _SECTION_CASES[sec]]


@pytest.fixture(scope="module")
def runs():
    procs = {k: subprocess.Popen([sys.executable, "-c", _CHILD, sections], env=dict(os.environ, **env),
                                 stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT)
             for k, (env, sections) in _RUNS.items()}
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


@pytest.mark.parametrize("run,case", _PAIRS)
def test_exact_against_oracle(runs, run, case):
    assert runs[run][case]["ok"] is True, (run, case, runs[run][case])


@pytest.mark.parametrize("on,off,case", [("levers-on", "levers-off", c) for c in _PATH_CASES + _GEO_CASES]
                         + [("overflow-on", "overflow-off", c) for c in _OVER_CASES]
                         + [("overflow-on", "one-workgroup-on", c) for c in _OVER_CASES])
def test_same_listed_sets(runs, on, off, case):
    """The agents and edges a run gathers do not depend on the levers, the grid or the chunk size."""
    a, b = runs[on][case], runs[off][case]
    assert (a["active"], a["edges"]) == (b["active"], b["edges"]), (on, off, case, a, b)


def test_paths_are_long_and_the_lists_overflow(runs):
    """A path must change for n - 1 rounds (so that 699 rounds cross the clear points and 4 096 rounds have one
    wave at work), and round 2 of the overflow cases must list more than the list holds (every riser of round
    1 marks itself), or the cases test nothing."""
    for run, (_, sections) in _RUNS.items():
        if "paths" in sections:
            assert runs[run]["path-700"]["rounds"] >= 699 and runs[run]["path-4097"]["rounds"] >= 4096, run
    for run in ("overflow-on", "overflow-off", "one-workgroup-on"):
        assert runs[run]["geo-30000-c16"]["chg1"] > 2 * 4096, (run, runs[run]["geo-30000-c16"])
