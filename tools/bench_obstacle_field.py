#!/usr/bin/env python3
"""Measure update_loop_radio with many obstacles as a flat list and as an obstacle field (contract O1,
DESIGN 4j) on tools/bench_loop_radio.py's setup: the C3 swarm, 30 % of the agents with a target,
Rc = Rs = 1.0.  bench.py is not involved.

For every m of --m (obstacles uniform over the arena, r in U(0.2, --r-max), default 2, fixed seed) two legs:
  flat   the m obstacles as a list (k_physics_loop_sensed: every moving agent walks all m through LDS);
  field  Swarm.obstacle_field of the same list (k_physics_loop_sensed_field: its own cell's list).
ms per tick, wall clock ended on a synchronise; per leg one warm-up run, then --reps timed runs, the legs of
a pair taking turns run by run.  200 ticks at m <= 16, 20 ticks above (--ticks-small / --ticks-large).  Both
legs of a pair must end on equal position and leader checksums.  Also recorded: the field's host build time,
its pairs and longest list, and (--build-only-m) the build time of larger lists that are not run.
Results are merged into --out under --label.

Usage:  python tools/bench_obstacle_field.py [--agents N] [--m 16,1024,16384] [--label NAME] [--out FILE]
"""
from __future__ import annotations

import argparse
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
    ap.add_argument("--m", default="16,1024,16384")
    ap.add_argument("--build-only-m", default="1000000")
    ap.add_argument("--r-max", type=float, default=2.0)
    ap.add_argument("--ticks-small", type=int, default=200)
    ap.add_argument("--ticks-large", type=int, default=20)
    ap.add_argument("--radio-radius", type=float, default=1.0)
    ap.add_argument("--sense-radius", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--legs", default="flat,field")
    ap.add_argument("--label", default="this_commit")
    ap.add_argument("--pkg", default=os.path.join(ROOT, "distributed-swarm-algorithm_amd"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_obstacle_field", "obstacle_field.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.pkg))
    import torch
    from swarm_amd import _lib, gen
    from swarm_amd.swarm import Swarm

    dev = torch.device("cuda", 0)
    d = gen.swarm_inputs(a.agents, a.seed, deg=a.deg, t=1)
    sw = Swarm(d["ids"], d["x"], d["y"], d["caps"], device=dev)
    n, rc, rs = sw.n, a.radio_radius, a.sense_radius
    g = np.random.default_rng(a.seed + 3)
    side = float(sw.pos[:, 0].max())
    off = (np.arange(n, dtype=np.int64) * 7919 % 40).astype(np.int32)
    has_t = torch.as_tensor(g.uniform(size=n) < 0.3, device=dev)
    tgt = torch.as_tensor(g.uniform(0, side, (n, 2)), device=dev)
    pos0 = sw.pos.clone()
    legs = [k for k in ("flat", "field") if k in a.legs.split(",")]
    print(f"[bench_obstacle_field] {a.label}: n={n} side={side:.1f} Rc={rc} Rs={rs} m={a.m} legs={legs}",
          file=sys.stderr, flush=True)

    def obstacles(m):
        q = np.random.default_rng(a.seed + 11 + m)
        return np.stack([q.uniform(0, side, m), q.uniform(0, side, m), q.uniform(0.2, a.r_max, m)], 1)

    def reset():
        """The same start for every run: positions, FSM, velocity, 30 % of the agents with a target."""
        sw.pos.copy_(pos0)
        sw.protocol_reset(tick_off=off, last_hb=-(off * 0.1))
        sw.vel = torch.zeros((n, 2), dtype=torch.float64, device=dev)
        sw.target = torch.where(has_t[:, None], tgt, torch.zeros_like(tgt)).contiguous()
        sw.has_target = has_t.to(torch.uint8).contiguous()
        torch.cuda.synchronize()

    def build(obs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f = sw.obstacle_field(obs)
        ms = (time.perf_counter() - t0) * 1e3
        return f, {"build_ms_host_wall": ms, **{k: f.info[k] for k in ("live", "ncx", "ncy", "cell", "pairs", "longest")}}

    res = {"agents": n, "arena_side": side, "r_max": a.r_max, "radio_radius": rc, "sense_radius": rs, "libswarm": _lib.version(),
           "unit": "ms per tick, wall clock ended on a synchronise, after one warm-up run of the leg; the two "
                   "legs of an m take turns run by run", "m": {}}
    for m in [int(v) for v in a.m.split(",") if v]:
        obs = obstacles(m)
        ticks = a.ticks_small if m <= 16 else a.ticks_large
        kills = tuple(t for t in (80, 150) if t <= ticks)
        field, info = build(obs)
        given = {"flat": torch.as_tensor(obs, device=dev), "field": field}
        times = {k: [] for k in legs}
        sums, leaders, sing = {}, {}, {}
        for rep in range(a.reps + 1):  # the first round is the warm-up
            for k in legs:
                reset()
                t0 = time.perf_counter()
                r = sw.update_loop_radio(ticks, rc, rs, obstacles=given[k], kill_ticks=kills, seed=5)
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) * 1e3 / ticks
                print(f"[bench_obstacle_field] m={m} {k} {'warm-up' if rep == 0 else rep}: {ms:.4f} ms per tick",
                      file=sys.stderr, flush=True)
                if rep:
                    times[k].append(ms)
                sums[k] = [float(sw.pos[:, 0].sum()), float(sw.pos[:, 1].sum())]
                leaders[k] = int(sw.leader.to(torch.int64).sum())
                sing[k] = int(r["singular"])
        if len(legs) == 2:
            assert sums["flat"] == sums["field"] and leaders["flat"] == leaders["field"] and \
                sing["flat"] == sing["field"], ("the legs ended differently", m, sums, leaders, sing)
        e = {"ticks": ticks, "kill_ticks": list(kills), "field": info, "ms_per_tick": times, "pos_checksum": sums,
             "leader_checksum": leaders, "singular": sing}
        if len(legs) == 2:
            e["field_slowest_over_flat_fastest"] = max(times["field"]) / min(times["flat"])
            e["field_slowest_below_flat_fastest"] = max(times["field"]) < min(times["flat"])
        res["m"][str(m)] = e
        field.close()
    for m in [int(v) for v in a.build_only_m.split(",") if v]:
        field, info = build(obstacles(m))
        res.setdefault("build_only", {})[str(m)] = info
        field.close()
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
