#!/usr/bin/env python3
"""Measure the update loop that re-senses its separation neighbours every tick (Swarm.update_loop_sensed,
contract U1-S) at the C3 swarm with the f2 row's schedule (200 ticks, kills at 80 / 150),
against what it replaces and what it costs on top of.  bench.py is not involved.

Legs (ms per tick, wall clock ended on a synchronise; per leg one warm-up run, then --reps timed runs, the
legs taking turns run by run so that drift hits them alike):
  a  update_loop_sensed(ticks, R): one call;
  b  the way to the same result without it: per tick, swarm_build_rgg of the current positions at R, then
     update_loop(1, sensors=that graph) -- a graph build, the FSM's pack / unpack and a host wait per tick;
  c  update_loop(ticks) on the fixed graph: what sensing costs on top of;
  d  update_loop(ticks) and protocol_run(ticks), the two calls whose host loop (run_ticks) the sensed loop
     shares: run it once on this tree and once with --pkg pointing at the parent commit's built package,
     under different --label, and compare.
Legs a and b end in the same state; the tool asserts that their position checksums agree.
Results are merged into --out under --label.

Usage:  python tools/bench_loop_sensed.py [--agents N] [--radius R] [--legs a,b,c,d] [--label NAME]
                                          [--pkg DIR] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=10_000_000)
    ap.add_argument("--deg", type=float, default=16.0)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--radius", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--legs", default="a,b,c,d")
    ap.add_argument("--label", default="this_commit")
    ap.add_argument("--pkg", default=os.path.join(ROOT, "distributed-swarm-algorithm_amd"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_loop_sensed", "update_loop_sensed.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.pkg))
    import torch
    from swarm_amd import _lib, gen
    from swarm_amd.swarm import Swarm

    legs = [k for k in "abcd" if k in a.legs.split(",")]
    dev = torch.device("cuda", 0)
    d = gen.swarm_inputs(a.agents, a.seed, deg=a.deg, t=1)
    sw = Swarm(d["ids"], d["x"], d["y"], d["caps"], device=dev).build_graph(1.0)
    n, e, ticks, R = sw.n, sw.n_edges, a.ticks, a.radius
    print(f"[bench_loop_sensed] {a.label}: n={n} E={e} R={R} legs={legs}", file=sys.stderr, flush=True)
    g = np.random.default_rng(a.seed + 3)
    side = float(sw.pos[:, 0].max())
    obs = np.stack([g.uniform(0, side, 16), g.uniform(0, side, 16), g.uniform(0.2, 1.5, 16)], 1)
    off = (np.arange(n, dtype=np.int64) * 7919 % 40).astype(np.int32)
    has_t = torch.as_tensor(g.uniform(size=n) < 0.3, device=dev)
    tgt = torch.as_tensor(g.uniform(0, side, (n, 2)), device=dev)
    pos0 = sw.pos.clone()
    kills = (80, 150)

    def reset():
        """The same start for every run: positions, FSM, velocity, 30 % of the agents with a target."""
        sw.pos.copy_(pos0)
        sw.protocol_reset(tick_off=off, last_hb=-(off * 0.1))
        sw.vel = torch.zeros((n, 2), dtype=torch.float64, device=dev)
        sw.target = torch.where(has_t[:, None], tgt, torch.zeros_like(tgt)).contiguous()
        sw.has_target = has_t.to(torch.uint8).contiguous()
        torch.cuda.synchronize()

    def radius_graph():
        """swarm_build_rgg of the current positions, the message graph left alone."""
        L = _lib.lib()
        rp = torch.empty(n + 1, dtype=torch.int32, device=dev)
        ne = ctypes.c_int64(0)
        _lib.check(L.swarm_build_rgg(_lib.ctx(), n, _lib.ptr(sw.pos), R, _lib.ptr(rp), None, 0, ctypes.byref(ne),
                                     _lib.stream()))
        col = torch.empty(max(ne.value, 1), dtype=torch.int32, device=dev)
        _lib.check(L.swarm_build_rgg(_lib.ctx(), n, _lib.ptr(sw.pos), R, _lib.ptr(rp), _lib.ptr(col), col.numel(),
                                     ctypes.byref(ne), _lib.stream()))
        return rp, col[: ne.value]

    def per_tick():
        for _ in range(ticks):
            sw.update_loop(1, obstacles=obs, kill_ticks=kills, seed=5, sensors=radius_graph())

    runs = {
        "a_update_loop_sensed": lambda: sw.update_loop_sensed(ticks, R, obstacles=obs, kill_ticks=kills, seed=5),
        "b_rgg_then_update_loop_1_per_tick": per_tick,
        "c_update_loop_fixed_graph": lambda: sw.update_loop(ticks, obstacles=obs, kill_ticks=kills, seed=5),
        "d_update_loop": lambda: sw.update_loop(ticks, obstacles=obs, kill_ticks=kills, seed=5),
        "d_protocol_run": lambda: sw.protocol_run(ticks, kill_ticks=kills, seed=5),
    }
    names = [k for k in runs if k[0] in legs]
    res = {"agents": n, "edges": e, "ticks": ticks, "kill_ticks": list(kills), "sense_radius": R,
           "libswarm": _lib.version(),
           "unit": "ms per tick, wall clock ended on a synchronise, after one warm-up run of the leg; "
                   "the legs take turns run by run"}
    times = {k: [] for k in names}
    sums = {}
    for rep in range(a.reps + 1):  # the first round is the warm-up
        for k in names:
            reset()
            t0 = time.perf_counter()
            runs[k]()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / ticks
            print(f"[bench_loop_sensed] {k} {'warm-up' if rep == 0 else rep}: {ms:.4f} ms per tick",
                  file=sys.stderr, flush=True)
            if rep:
                times[k].append(ms)
            sums[k] = [float(sw.pos[:, 0].sum()), float(sw.pos[:, 1].sum())]
    res.update(times)
    res["pos_checksum"] = sums
    ka, kb = "a_update_loop_sensed", "b_rgg_then_update_loop_1_per_tick"
    if ka in sums and kb in sums:
        assert sums[ka] == sums[kb], ("legs a and b ended in different states", sums[ka], sums[kb])
    out = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            out = json.load(f)
    out[a.label] = res
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps({a.label: res}))


if __name__ == "__main__":
    main()
