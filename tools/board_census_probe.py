#!/usr/bin/env python3
"""Measure the task census (Swarm.board_census / Swarm.task_census, contract U1-C) against the route a user had
before it: the same ten arrays from torch.bincount / scatter_reduce over the flattened rows.  bench.py is not
involved.

Legs (ms per call, wall clock ended on a synchronise; two warm-up calls of each route, then --reps timed calls, the
two routes of a leg taking turns call by call; min - median - max are reported, and the two routes' arrays are
checked equal at full size):
  a  tools/bench_loop_board.py's leg b: the C3 swarm, C3's own 10 000 tasks, 16 / 16 slots (doubled while the run
     is refused), 200 ticks of update_loop_board; then board_census() against torch;
  b  the same with holders=True: the sorted (task, ID) pairs against torch.nonzero + a sort;
  d  leg a again after Swarm.resort(): 200 ticks have carried three agents in ten towards targets up to 100 units
     away, so a workgroup's range of agents no longer sees only the few tasks of one neighbourhood; the number of
     distinct (range of 2442 agents, task) pairs among the status entries is reported for both orders;
  c  a contention corner: the 64-task board of set_tasks at the same agents, every agent LOCKED on eight or so
     random tasks (every task at more than 10^5 agents), one agent in 64 holding a claim table; task_census()
     against torch over task_status() and the dense tables.
The bytes a census has to read (every status and table-task slot once, winner and utility where a slot holds an
entry, an ID per holder; for c the two status words and every winner) over its median time are reported as a
fraction of the 6.29 TB/s the chip copies at.  --census-only skips the torch route (for a kernel trace).

Usage:  python tools/board_census_probe.py [--agents N] [--legs a,b,c] [--reps R] [--census-only] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("tentative", "locked", "assigned", "tables", "holder_lo", "holder_hi", "winner_lo", "winner_hi",
          "best_winner", "best_util")
COPY_RATE = 6.29e12  # bytes per second, the measured copy rate of the chip


def torch_census(torch, T, ids, status_task, status_code, status_agent, tab_task, tab_winner, tab_util):
    """The ten arrays from flat entry lists (device tensors): the route without the census kernels.  The
    utilities the loops store are positive and finite, so their int32 bits order as the floats do."""
    dev = ids.device
    out = {}
    for name, code in (("tentative", 1), ("locked", 2), ("assigned", 3)):
        out[name] = torch.bincount(status_task[status_code == code], minlength=T).to(torch.int32)
    held = status_code == 3
    ht, hid = status_task[held], ids[status_agent[held]].long()
    big = torch.full((T,), 1 << 40, dtype=torch.int64, device=dev)
    lo = big.scatter_reduce(0, ht, hid, "amin")
    out["holder_lo"] = torch.where(lo == 1 << 40, -1, lo).to(torch.int32)
    out["holder_hi"] = torch.full((T,), -1, dtype=torch.int64, device=dev).scatter_reduce(0, ht, hid, "amax") \
        .to(torch.int32)
    out["tables"] = torch.bincount(tab_task, minlength=T).to(torch.int32)
    w = tab_winner.long()
    lo = big.scatter_reduce(0, tab_task, w, "amin")
    out["winner_lo"] = torch.where(lo == 1 << 40, -1, lo).to(torch.int32)
    out["winner_hi"] = torch.full((T,), -1, dtype=torch.int64, device=dev).scatter_reduce(0, tab_task, w, "amax") \
        .to(torch.int32)
    key = (tab_util.view(torch.int32).long() << 32) | (0xFFFFFFFF - w)
    best = torch.full((T,), -1, dtype=torch.int64, device=dev).scatter_reduce(0, tab_task, key, "amax")
    has = best >= 0
    out["best_winner"] = torch.where(has, 0xFFFFFFFF - (best & 0xFFFFFFFF), -1).to(torch.int32)
    out["best_util"] = torch.where(has, best >> 32, 0).to(torch.int32).view(torch.float32)
    pairs = torch.stack([ht, hid], 1)
    order = torch.argsort(ht * (1 << 31) + hid)
    return out, pairs[order].to(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=10_000_000)
    ap.add_argument("--deg", type=float, default=16.0)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--tasks", type=int, default=10_000)
    ap.add_argument("--slots", type=int, default=16)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--legs", default="a,b,d,c")
    ap.add_argument("--census-only", action="store_true")
    ap.add_argument("--label", default="this_commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27_board_census", "board_census.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "distributed-swarm-algorithm_amd"))
    import torch
    from swarm_amd import _lib, gen
    from swarm_amd.swarm import Swarm

    legs = [k for k in "abdc" if k in a.legs.split(",")]
    dev = torch.device("cuda", 0)
    d = gen.swarm_inputs(a.agents, a.seed, deg=a.deg, t=a.tasks)
    sw = Swarm(d["ids"], d["x"], d["y"], d["caps"], device=dev)
    n, T = sw.n, a.tasks
    print(f"[board_census_probe] n={n} T={T} legs={legs}", file=sys.stderr, flush=True)
    res = {"agents": n, "libswarm": _lib.version(), "reps": a.reps,
           "unit": "ms per call, wall clock ended on a synchronise, after two warm-up calls of each route; the two "
                   "routes of a leg take turns call by call; [min, median, max]"}

    def race(name, routes, nbytes):
        """routes: {label: callable}; timed in turns.  Returns each route's last result."""
        times, last = {k: [] for k in routes}, {}
        for rep in range(a.reps + 2):
            for k, f in routes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                last[k] = f()
                torch.cuda.synchronize()
                if rep >= 2:
                    times[k].append((time.perf_counter() - t0) * 1e3)
        out = {k: [float(np.min(v)), float(np.median(v)), float(np.max(v))] for k, v in times.items()}
        out["bytes_the_census_must_read"] = int(nbytes)
        out["census_fraction_of_copy_rate"] = nbytes / (out["census"][1] * 1e-3) / COPY_RATE
        res[name] = out
        print(f"[board_census_probe] {name}: {json.dumps(out)}", file=sys.stderr, flush=True)
        return last

    def same(c, t, what):
        for k in FIELDS:
            assert torch.equal(c[k].view(torch.int32), t[k].view(torch.int32)), (what, k)

    if "a" in legs or "b" in legs or "d" in legs:
        g = np.random.default_rng(a.seed + 3)  # (tools/bench_loop_board.py's draws, in its order)
        side = float(sw.pos[:, 0].max())
        obs = np.stack([g.uniform(0, side, 16), g.uniform(0, side, 16), g.uniform(0.2, 1.5, 16)], 1)
        off = (np.arange(n, dtype=np.int64) * 7919 % 40).astype(np.int32)
        has_t = torch.as_tensor(g.uniform(size=n) < 0.3, device=dev)
        tgt = torch.as_tensor(g.uniform(0, side, (n, 2)), device=dev)
        pos0, slots = sw.pos.clone(), [a.slots, a.slots]
        while True:
            sw.pos.copy_(pos0)
            sw.protocol_reset(tick_off=off, last_hb=-(off * 0.1))
            sw.vel = torch.zeros((n, 2), dtype=torch.float64, device=dev)
            sw.target = torch.where(has_t[:, None], tgt, torch.zeros_like(tgt)).contiguous()
            sw.has_target = has_t.to(torch.uint8).contiguous()
            sw.set_task_board(d["tx"], d["ty"], d["treq"], status_slots=slots[0], table_slots=slots[1])
            try:
                r = sw.update_loop_board(a.ticks, 1.0, 1.0, obstacles=obs, kill_ticks=(80, 150), seed=5)
                break
            except _lib.SwarmError as err:
                if err.code != _lib.ERR_RANGE or sw.last_board_overflow is None:
                    raise
                slots[0 if sw.last_board_overflow[0] == "status" else 1] *= 2
        b = sw.board
        entries = int((b["status"] >= 0).sum()), int((b["tab_task"] >= 0).sum())
        tc = r["task_counts"]
        res["board"] = {"tasks": T, "ticks": a.ticks, "status_slots": b["Ks"], "table_slots": b["Kt"],
                        "status_entries": entries[0], "table_entries": entries[1],
                        "claims_sent": int(tc[:, 0].sum()), "claims_handled_by_a_leader": int(tc[:, 1].sum())}

        def torch_board():
            st, tt = b["status"].flatten(), b["tab_task"].flatten()
            at = torch.nonzero(st >= 0).squeeze(1)
            e = st[at]
            m = tt >= 0
            return torch_census(torch, T, sw.ids, (e >> 2).long(), e & 3, at // b["Ks"], tt[m].long(),
                                b["tab_winner"].flatten()[m], b["tab_util"].flatten()[m])

        c = sw.board_census()
        res["board"].update(tasks_with_a_holder=int((c["assigned"] > 0).sum()),
                            tasks_with_two_or_more_holders=int((c["assigned"] >= 2).sum()),
                            most_holders_of_one_task=int(c["assigned"].max()),
                            tasks_whose_tables_name_different_winners=int((c["winner_lo"] != c["winner_hi"]).sum()),
                            most_agents_locked_on_one_task=int(c["locked"].max()))
        nbytes = 4 * n * (b["Ks"] + b["Kt"]) + 8 * entries[1] + 4 * int(c["assigned"].sum())
        if "a" in legs:
            routes = {"census": lambda: sw.board_census()}
            if not a.census_only:
                routes["torch"] = lambda: torch_board()[0]
            last = race("a_board_census", routes, nbytes)
            if not a.census_only:
                same(last["census"], last["torch"], "a")
        if "b" in legs:
            routes = {"census": lambda: sw.board_census(holders=True)}
            if not a.census_only:
                routes["torch"] = torch_board
            last = race("b_board_census_with_holders", routes, nbytes + 8 * int(c["assigned"].sum()))
            res["b_board_census_with_holders"]["holder_pairs"] = int(last["census"]["holders"].shape[0])
            if not a.census_only:
                same(last["census"], last["torch"][0], "b")
                assert torch.equal(last["census"]["holders"], last["torch"][1]), "holders"
        def ranges():
            """Distinct (range of agents, task) pairs among the status entries: what a workgroup's LDS table has
            to hold, and the global atomics its flush costs at the least."""
            per = max(128, -(-n // 4096))
            st = b["status"]
            at = torch.nonzero(st.flatten() >= 0).squeeze(1)
            return int(torch.unique((at // (b["Ks"] * per)) * T + (st.flatten()[at] >> 2)).numel())
        res["board"]["distinct_range_task_pairs"] = ranges()
        if "d" in legs:
            sw.resort()
            b = sw.board
            res["board"]["rows_moved_by_resort"] = int(sw.last_resort_moved)
            res["board"]["distinct_range_task_pairs_after_resort"] = ranges()
            routes = {"census": lambda: sw.board_census()}
            if not a.census_only:
                routes["torch"] = lambda: torch_board()[0]
            last = race("d_board_census_after_resort", routes, nbytes)
            same(last["census"], c, "d: the census changed with the storage order")
            if not a.census_only:
                same(last["census"], last["torch"], "d")
        sw.board["finalizer"]()
        del sw.board

    if "c" in legs:
        g = torch.Generator(device=dev).manual_seed(a.seed)
        sw.set_tasks(np.linspace(0.0, 1.0, 64), np.zeros(64))
        tk = sw.tasks
        def words(p):
            bits, w = torch.rand((n, 64), device=dev, generator=g) < p, torch.zeros(n, dtype=torch.int64, device=dev)
            for k in range(64):
                w |= bits[:, k].long() << k
            return w
        tk["status_hi"].copy_(words(1 / 8))  # LOCKED, or ASSIGNED where the low bit is set as well
        tk["status_lo"].copy_(words(1 / 64))
        lead = torch.arange(0, n, 64, device=dev)
        m = torch.rand((lead.numel(), 64), device=dev, generator=g) < 1 / 8
        tk["tab_winner"][lead] = torch.where(m, sw.ids[torch.randint(0, n, m.shape, device=dev, generator=g)], -1)
        tk["tab_util"][lead] = torch.where(m, 20.0 + 80.0 * torch.rand(m.shape, device=dev, generator=g), 0.0) \
            .to(torch.float32)
        c = sw.task_census()
        res["tasks64"] = {"least_agents_locked_on_one_task": int(c["locked"].min()),
                          "table_entries": int(c["tables"].sum()), "holder_pairs": int(c["assigned"].sum())}
        assert res["tasks64"]["least_agents_locked_on_one_task"] >= 100_000 or n < 10_000_000

        def torch_tasks():
            at = torch.nonzero(sw.task_status()).long()
            w = tk["tab_winner"]
            m = w >= 0
            tt = torch.nonzero(m)[:, 1]
            code = ((tk["status_lo"][at[:, 0]] >> at[:, 1]) & 1) | (((tk["status_hi"][at[:, 0]] >> at[:, 1]) & 1) << 1)
            return torch_census(torch, 64, sw.ids, at[:, 1], code, at[:, 0], tt, w[m], tk["tab_util"][m])[0]

        routes = {"census": lambda: sw.task_census()}
        if not a.census_only:
            routes["torch"] = torch_tasks
        last = race("c_task_census_every_task_hot", routes, n * (16 + 4 * 64) + 4 * res["tasks64"]["table_entries"])
        if not a.census_only:
            same(last["census"], last["torch"], "c")

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
