#!/usr/bin/env python3
"""Measure the update loop that re-senses who hears whom every tick (Swarm.update_loop_radio, contract U1-R)
at the C3 swarm with the f2 row's schedule (200 ticks, kills at 80 / 150), against what it replaces and what
it costs on top of.  bench.py is not involved.

Legs (ms per tick, wall clock ended on a synchronise; per leg one warm-up run, then --reps timed runs, the
legs taking turns run by run so that drift hits them alike):
  a  update_loop_radio(ticks, Rc, Rs): one call;
  b  the way to the same result without it: per tick, swarm_build_rgg of the current positions at Rc set as
     the message graph, then update_loop_sensed(1, Rs) -- a graph build, the FSM's pack / unpack, a grid and
     two host waits per tick;
  c  update_loop_sensed(ticks, Rs) on the fixed message graph: what re-sensing the radio costs on top of;
  d  update_loop_sensed(ticks, Rs), update_loop(ticks) and protocol_run(ticks), the calls whose host loop
     (run_ticks) the radio loop shares: run it once on this tree and once with --pkg pointing at the parent
     commit's built package, under different --label, and compare.
Legs a and b end in the same state; the tool asserts that their position and leader checksums agree.
Results are merged into --out under --label.

Usage:  python tools/bench_loop_radio.py [--agents N] [--radio-radius Rc] [--sense-radius Rs]
                                         [--legs a,b,c,d] [--label NAME] [--pkg DIR] [--out FILE]
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
    ap.add_argument("--radio-radius", type=float, default=1.0)
    ap.add_argument("--sense-radius", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--legs", default="a,b,c,d")
    ap.add_argument("--label", default="this_commit")
    ap.add_argument("--pkg", default=os.path.join(ROOT, "distributed-swarm-algorithm_amd"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_loop_radio", "update_loop_radio.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.pkg))
    import torch
    from swarm_amd import _lib, gen
    from swarm_amd.swarm import Swarm

    legs = [k for k in "abcd" if k in a.legs.split(",")]
    dev = torch.device("cuda", 0)
    d = gen.swarm_inputs(a.agents, a.seed, deg=a.deg, t=1)
    sw = Swarm(d["ids"], d["x"], d["y"], d["caps"], device=dev).build_graph(1.0)
    n, e, ticks, rc, rs = sw.n, sw.n_edges, a.ticks, a.radio_radius, a.sense_radius
    graph0 = (sw.row_ptr, sw.col)
    print(f"[bench_loop_radio] {a.label}: n={n} E={e} Rc={rc} Rs={rs} legs={legs}", file=sys.stderr, flush=True)
    g = np.random.default_rng(a.seed + 3)
    side = float(sw.pos[:, 0].max())
    obs = np.stack([g.uniform(0, side, 16), g.uniform(0, side, 16), g.uniform(0.2, 1.5, 16)], 1)
    off = (np.arange(n, dtype=np.int64) * 7919 % 40).astype(np.int32)
    has_t = torch.as_tensor(g.uniform(size=n) < 0.3, device=dev)
    tgt = torch.as_tensor(g.uniform(0, side, (n, 2)), device=dev)
    pos0 = sw.pos.clone()
    kills = (80, 150)

    def reset():
        """The same start for every run: positions, message graph, FSM, velocity, 30 % of the agents with a
        target."""
        sw.pos.copy_(pos0)
        sw.row_ptr, sw.col = graph0
        sw._hear = None
        sw.protocol_reset(tick_off=off, last_hb=-(off * 0.1))
        sw.vel = torch.zeros((n, 2), dtype=torch.float64, device=dev)
        sw.target = torch.where(has_t[:, None], tgt, torch.zeros_like(tgt)).contiguous()
        sw.has_target = has_t.to(torch.uint8).contiguous()
        torch.cuda.synchronize()

    def radius_graph():
        """swarm_build_rgg of the current positions at Rc."""
        L = _lib.lib()
        rp = torch.empty(n + 1, dtype=torch.int32, device=dev)
        ne = ctypes.c_int64(0)
        _lib.check(L.swarm_build_rgg(_lib.ctx(), n, _lib.ptr(sw.pos), rc, _lib.ptr(rp), None, 0, ctypes.byref(ne),
                                     _lib.stream()))
        col = torch.empty(max(ne.value, 1), dtype=torch.int32, device=dev)
        _lib.check(L.swarm_build_rgg(_lib.ctx(), n, _lib.ptr(sw.pos), rc, _lib.ptr(rp), _lib.ptr(col), col.numel(),
                                     ctypes.byref(ne), _lib.stream()))
        return rp, col[: ne.value]

    def per_tick():
        for _ in range(ticks):
            sw.row_ptr, sw.col = radius_graph()
            sw._hear = None
            sw.update_loop_sensed(1, rs, obstacles=obs, kill_ticks=kills, seed=5)

    kw = dict(obstacles=obs, kill_ticks=kills, seed=5)
    runs = {
        "a_update_loop_radio": lambda: sw.update_loop_radio(ticks, rc, rs, **kw),
        "b_rgg_then_update_loop_sensed_1_per_tick": per_tick,
        "c_update_loop_sensed_fixed_graph": lambda: sw.update_loop_sensed(ticks, rs, **kw),
        "d_update_loop_sensed": lambda: sw.update_loop_sensed(ticks, rs, **kw),
        "d_update_loop": lambda: sw.update_loop(ticks, **kw),
        "d_protocol_run": lambda: sw.protocol_run(ticks, kill_ticks=kills, seed=5),
    }
    names = [k for k in runs if k[0] in legs]
    res = {"agents": n, "edges": e, "ticks": ticks, "kill_ticks": list(kills), "radio_radius": rc,
           "sense_radius": rs, "libswarm": _lib.version(),
           "unit": "ms per tick, wall clock ended on a synchronise, after one warm-up run of the leg; "
                   "the legs take turns run by run"}
    times = {k: [] for k in names}
    sums, leaders = {}, {}
    for rep in range(a.reps + 1):  # the first round is the warm-up
        for k in names:
            reset()
            t0 = time.perf_counter()
            r = runs[k]()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / ticks
            print(f"[bench_loop_radio] {k} {'warm-up' if rep == 0 else rep}: {ms:.4f} ms per tick",
                  file=sys.stderr, flush=True)
            if rep:
                times[k].append(ms)
            sums[k] = [float(sw.pos[:, 0].sum()), float(sw.pos[:, 1].sum())]
            leaders[k] = int(sw.leader.to(torch.int64).sum())
            if isinstance(r, dict):  # the loops' counts: alive LEADERs / heartbeat senders per tick
                c = r["counts"]
                res[k + "_leaders_every_20_ticks"] = c[::20, 0].tolist()
                res[k + "_sender_ticks"] = {"acclaims_max": int(c[:, 2].max()), "heartbeats_max": int(c[:, 3].max()),
                                            "ticks_without_a_sender": int(((c[:, 2] + c[:, 3]) == 0).sum())}
    res.update(times)
    res["pos_checksum"], res["leader_checksum"] = sums, leaders
    ka, kb = "a_update_loop_radio", "b_rgg_then_update_loop_sensed_1_per_tick"
    if ka in sums and kb in sums:
        assert sums[ka] == sums[kb], ("legs a and b ended in different positions", sums[ka], sums[kb])
        assert leaders[ka] == leaders[kb], ("legs a and b ended with different leaders", leaders[ka], leaders[kb])
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
