"""A/B timing of physics steps that re-sense their neighbours every step, on the C3 swarm with the
bench's f1 setup (bench.py: elected leaders, 16 obstacles) -- one JSON line per run:
  b  ms per step of build_graph(R) + physics_step(steps=1) in a Python loop (works on any build)
  c  ms per step of physics_step(sense_radius=R, steps=K), one C call (swarm_physics_run_sensed)
Both run the same 2 warm-up steps and K >= 10 timed steps from the same start, so their position
checksums must agree (the two paths are bit-identical).  HIP events around the timed steps.
Usage: timeout 600 python tools/physics_sensed_ab.py {b|c} [N] [--root DIR] [--steps K] [--radius R]
--root: the checkout whose package and libswarm.so to time (default: this one), e.g. the parent commit's
for b."""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=["b", "c"])
ap.add_argument("n", nargs="?", type=int, default=10_000_000)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--radius", type=float, default=1.0)
ap.add_argument("--seed", type=int, default=2024)
args = ap.parse_args()
assert args.steps >= 10, "at least 10 timed steps"
sys.path.insert(0, os.path.join(args.root, "distributed-swarm-algorithm_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from swarm_amd import _lib, gen  # noqa: E402
from swarm_amd.swarm import Swarm  # noqa: E402

dev = "cuda:0"
d = gen.swarm_inputs(args.n, args.seed, deg=16)
sw = Swarm(d["ids"], d["x"], d["y"], d["caps"], device=dev).build_graph(1.0)
sw.elect(max_rounds=1 << 16)
g = np.random.default_rng(args.seed + 3)
side = float(sw.pos[:, 0].max())
obs = np.stack([g.uniform(0, side, 16), g.uniform(0, side, 16), g.uniform(0.2, 1.5, 16)], 1)
li = sw.leader_index()
R = args.radius


def window_stats():
    """Per scanning agent (one with a target after the first step: the followers): candidates in its
    3 x 3 window of cells of side min(R, 2) (1 + 1e-9), and sensed neighbours (the graph's degree)."""
    cell = min(R, 2.0) * (1.0 + 1e-9)
    p = sw.pos
    c = torch.floor((p - p.min(0).values) / cell).long()
    ncx, ncy = int(c[:, 0].max()) + 1, int(c[:, 1].max()) + 1
    occ = torch.bincount(c[:, 1] * ncx + c[:, 0], minlength=ncx * ncy).view(ncy, ncx)
    pad = torch.nn.functional.pad(occ, (1, 1, 1, 1))
    win = sum(pad[a:a + ncy, b:b + ncx] for a in range(3) for b in range(3))
    scan = li >= 0
    cand = win.reshape(-1)[(c[:, 1] * ncx + c[:, 0])[scan]].double().mean().item()
    deg = (sw.row_ptr[1:] - sw.row_ptr[:-1])[scan].double().mean().item()
    return {"scanning_agents": int(scan.sum()), "window_candidates_per_scanning_agent": cand,
            "sensed_per_scanning_agent": deg}


stats = window_stats() if R == 1.0 else {}


def run(steps):
    if args.mode == "c":
        return sw.physics_step(obs, leader_index=li, steps=steps, sense_radius=R)
    for _ in range(steps):
        sw.build_graph(R)
        sw.physics_step(obs, leader_index=li, steps=1)


run(2)
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
run(args.steps)
e1.record()
torch.cuda.synchronize()
ms = e0.elapsed_time(e1)
pos = sw.pos
print(json.dumps({"tool": "physics_sensed_ab", "mode": args.mode, "agents": sw.n, "radius": R,
                  "timed_steps": args.steps, "ms_per_step": ms / args.steps,
                  "pos_checksum": [float(pos[:, 0].sum()), float(pos[:, 1].sum())],
                  "finite": bool(torch.isfinite(pos).all()), "lib": _lib.version(), **stats}), flush=True)
