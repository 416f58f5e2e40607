#!/usr/bin/env python3
"""Measure Swarm.resort() (contract R1) and what it buys after motion, on tools/bench_loop_board.py's
setup: the C3 swarm, its own 10 000 tasks on a board of --slots status / table slots, kills at 80 / 150,
Rc = Rs = 1.0.  bench.py is not involved.

Legs (wall clock ended on a synchronise; per leg one warm-up run, then --reps timed runs (--reps-b for leg b), the
variants of a leg taking turns run by run so that drift hits them alike; min / median / max are reported):
  a  the cost of resort() after --ticks ticks of update_loop_board (full fsm + board state): the whole call, and
     its row permutation alone (swarm_permute_rows over the same arrays with the call's own `from`) against the
     same permutation by torch indexing, one column at a time as swarm.take_rows does it; both again for a random
     permutation, the worst case (a 1-byte row gather pulls a whole line); the plan and the relabelling of the
     entry radius graph on their own.  Bytes moved = 2 n sum(row_bytes) + 4 n, as a fraction of --hbm-peak;
  b  the election after motion, from leg a's end state: (i) build_graph(1.0) + elect() as the swarm stands,
     (ii) resort() + build_graph + elect(), (iii) a fresh Swarm of the same input-order positions + build_graph +
     elect().  Leaders, rounds and per-round changes must be equal in all three in input order; (ii) and (iii)
     run on byte-identical arrays, so each one's election median must lie inside the other's min-max span;
  c  the loop after motion: ms per tick of ticks 1-50, 151-200 and 201-250 in a run without a resort and in a
     twin with resort() after tick 200 (the rows doubled first until 250 ticks fit).
Results are merged into --out under --label.

Usage:  python tools/bench_resort.py [--agents N] [--legs a,b,c] [--label NAME] [--out FILE]
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


def spread(v):
    return {"min": float(np.min(v)), "median": float(np.median(v)), "max": float(np.max(v)), "runs": [float(x) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=10_000_000)
    ap.add_argument("--deg", type=float, default=16.0)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--tasks", type=int, default=10_000)
    ap.add_argument("--slots", type=int, default=16)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--reps-b", type=int, default=9, help="timed runs of leg b's variants (an election is short)")
    ap.add_argument("--legs", default="a,b,c")
    ap.add_argument("--hbm-peak", type=float, default=8.0e12, help="bytes per second the fractions are taken of")
    ap.add_argument("--label", default="this_commit")
    ap.add_argument("--pkg", default=os.path.join(ROOT, "distributed-swarm-algorithm_amd"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_resort", "resort.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.pkg))
    import torch
    from swarm_amd import _lib, gen
    from swarm_amd.swarm import Swarm

    legs = [k for k in "abc" if k in a.legs.split(",")]
    dev = torch.device("cuda", 0)
    d = gen.swarm_inputs(a.agents, a.seed, deg=a.deg, t=a.tasks)
    sw = Swarm(d["ids"], d["x"], d["y"], d["caps"], device=dev).build_graph(1.0)
    n, ticks, rc, rs = sw.n, a.ticks, 1.0, 1.0
    graph0, perm0 = (sw.row_ptr, sw.col), sw.perm
    base = {k: getattr(sw, k) for k in ("ids", "caps")}
    log = lambda *m: print("[bench_resort]", *m, file=sys.stderr, flush=True)  # noqa: E731
    log(f"{a.label}: n={n} E={sw.n_edges} T={a.tasks} slots={a.slots} legs={legs}")
    g = np.random.default_rng(a.seed + 3)  # (bench_loop_tasks.py's draws, in its order)
    side = float(sw.pos[:, 0].max())
    obs = np.stack([g.uniform(0, side, 16), g.uniform(0, side, 16), g.uniform(0.2, 1.5, 16)], 1)
    off = (np.arange(n, dtype=np.int64) * 7919 % 40).astype(np.int32)
    has_t = torch.as_tensor(g.uniform(size=n) < 0.3, device=dev)
    tgt = torch.as_tensor(g.uniform(0, side, (n, 2)), device=dev)
    pos0 = sw.pos.clone()
    slots = [a.slots, a.slots]
    kw = dict(obstacles=obs, kill_ticks=(80, 150), seed=5)
    sync = torch.cuda.synchronize

    def reset():
        """The same start for every run, in the entry storage order, without a neighbour graph (the board loop
        senses its own)."""
        sw.perm = perm0
        sw.ids, sw.caps = base["ids"], base["caps"]
        sw.pos = pos0.clone()
        sw.leader = torch.empty(n, dtype=torch.int32, device=dev)
        sw.state = torch.empty(n, dtype=torch.uint8, device=dev)
        sw.row_ptr = sw.col = sw._hear = None
        sw._cindex = sw._id_index = sw._pos_prev_key = None
        sw.protocol_reset(tick_off=off, last_hb=-(off * 0.1))
        sw.vel = torch.zeros((n, 2), dtype=torch.float64, device=dev)
        sw.target = torch.where(has_t[:, None], tgt, torch.zeros_like(tgt)).contiguous()
        sw.has_target = has_t.to(torch.uint8).contiguous()
        sw.set_task_board(d["tx"], d["ty"], d["treq"], status_slots=slots[0], table_slots=slots[1])
        sync()

    def loop(k):
        return sw.update_loop_board(k, rc, rs, **kw)

    def moved_state(k):
        """reset() + k ticks, the rows doubled and the run repeated while it is refused."""
        while True:
            reset()
            try:
                loop(k)
                sync()
                return
            except _lib.SwarmError as err:
                if err.code != _lib.ERR_RANGE or sw.last_board_overflow is None:
                    raise
                slots[0 if sw.last_board_overflow[0] == "status" else 1] *= 2
                log(f"rows full at tick {sw.last_refused_tick}, now {slots}")

    def capture():
        """The swarm's state by reference: resort() replaces tensors and never writes into one."""
        return dict(vars(sw)), dict(sw.fsm), dict(sw.board)

    def restore(snap):
        for k in [k for k in vars(sw) if k not in snap[0]]:
            delattr(sw, k)
        vars(sw).update(snap[0])
        sw.fsm, sw.board = dict(snap[1]), dict(snap[2])

    res = {"agents": n, "ticks": ticks, "tasks": a.tasks, "libswarm": _lib.version(), "hbm_peak_bytes_per_s": a.hbm_peak,
           "unit": "ms, wall clock ended on a synchronise, after one warm-up run; variants take turns run by run"}
    L = _lib.lib()

    def save():
        """Merges what is measured so far into --out (after every leg: a later leg's failure loses nothing)."""
        out = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                out = json.load(f)
        out.setdefault(a.label, {}).update(res)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)

    def timed(fn):
        sync()
        t0 = time.perf_counter()
        r = fn()
        sync()
        return (time.perf_counter() - t0) * 1e3, r

    if "a" in legs or "b" in legs:
        moved_state(ticks)
        snap = capture()
        res["slots"] = list(slots)
        travelled = (sw.to_input_order(sw.pos) - np.stack([d["x"], d["y"]], 1))
        res["max_distance_travelled"] = float(np.sqrt((travelled ** 2).sum(1)).max())

    if "a" in legs:
        arrays = [x for x in sw._resort_arrays() if x[1].numel()]
        row_bytes = [(t.element_size() * (t.numel() // (h * n)), h) for _p, t, h in arrays]
        total_rb = sum(rb * h for rb, h in row_bytes)
        nbytes = 2 * n * total_rb + 4 * n
        frm = torch.empty(n, dtype=torch.int32, device=dev)
        pout = torch.empty(n, dtype=torch.int32, device=dev)
        moved = ctypes.c_int64(0)

        def plan(to_from=None, to_perm=None):
            restore(snap)  # (the whole call before it in the round has left the swarm resorted)
            _lib.check(L.swarm_resort_plan(_lib.ctx(), n, _lib.ptr(sw.pos), _lib.ptr(sw.perm), sw.cell,
                                           _lib.ptr(frm if to_from is None else to_from),
                                           _lib.ptr(pout if to_perm is None else to_perm), ctypes.byref(moved),
                                           _lib.stream()))
        plan()
        rows_moved = int(moved.value)
        assert rows_moved > 0, "the run moved no agent out of its row"
        spare = (torch.empty_like(frm), torch.empty_like(pout))  # the timed plans write here: frm stays the run's
        rnd = torch.randperm(n, device=dev).to(torch.int32)
        outs = [torch.empty_like(t) for _p, t, _h in arrays]
        descs = []
        for (_p, t, h), o, (rb, _h) in zip(arrays, outs, row_bytes):
            descs += [_lib.Rows(t.data_ptr() + k * n * rb, o.data_ptr() + k * n * rb, rb) for k in range(h)]
        carr = (_lib.Rows * len(descs))(*descs)

        def native(idx):
            _lib.check(L.swarm_permute_rows(_lib.ctx(), n, _lib.ptr(idx), len(descs), carr, _lib.stream()))

        def by_torch(idx):
            """The same rows by torch indexing, one column at a time (swarm.take_rows: a row gather of an (N, 2)
            float64 tensor is wrong above 2^26 rows on this build)."""
            i64, out = idx.long(), []
            for _p, t, h in arrays:
                parts = []
                for k in range(h):
                    v = t[k * n:(k + 1) * n]
                    parts.append(v[i64] if v.dim() == 1 else
                                 torch.stack([v[:, j].contiguous()[i64] for j in range(v.shape[1])], 1))
                out.append(torch.cat(parts) if h > 1 else parts[0].contiguous())
            return out

        def whole():
            restore(snap)
            return sw.resort()

        def relabel():
            rp, cl = torch.empty_like(graph0[0]), torch.empty_like(graph0[1])
            _lib.check(L.swarm_graph_relabel(_lib.ctx(), n, _lib.ptr(frm), _lib.ptr(graph0[0]), _lib.ptr(graph0[1]),
                                             _lib.ptr(rp), _lib.ptr(cl), _lib.stream()))
        variants = {"resort_whole_call": whole, "plan": lambda: plan(*spare), "permute_native": lambda: native(frm),
                    "permute_torch": lambda: by_torch(frm), "permute_native_random": lambda: native(rnd),
                    "permute_torch_random": lambda: by_torch(rnd), "relabel_entry_graph": relabel}
        times = {k: [] for k in variants}
        for rep in range(a.reps + 1):
            for k, fn in variants.items():
                ms, _ = timed(fn)
                log(f"a {k} {'warm-up' if rep == 0 else rep}: {ms:.3f} ms")
                if rep:
                    times[k].append(ms)
        assert torch.equal(spare[0], frm) and int((frm != torch.arange(n, device=dev)).sum()) == rows_moved
        got = by_torch(frm)
        native(frm)
        sync()
        assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(outs, got))
        leg = {k: spread(v) for k, v in times.items()}
        leg.update(arrays=len(arrays), descriptors=len(descs), sum_row_bytes=total_rb, bytes_moved=nbytes,
                   rows_moved=rows_moved, edges_relabelled=int(graph0[1].numel()),
                   row_bytes=sorted(rb for rb, h in row_bytes for _ in range(h)))
        for k in ("permute_native", "permute_torch", "permute_native_random", "permute_torch_random"):
            leg[k]["fraction_of_hbm_peak"] = nbytes / (leg[k]["median"] * 1e-3) / a.hbm_peak
        res["a"] = leg
        del outs, got
        restore(snap)
        save()

    if "b" in legs:
        pos_in = sw.to_input_order(sw.pos)
        ids_in, caps_in = sw.to_input_order(sw.ids), sw.to_input_order(sw.caps).view(np.uint32)

        def elect_here(s):
            s.leader, s.state = s.leader.clone(), s.state.clone()  # elect() writes them in place
            t_graph, _ = timed(lambda: s.build_graph(1.0))
            c16 = s.graph_compact()  # (built outside the election's clock, as a first elect() would cache it)
            t_elect, r = timed(s.elect)
            return dict(graph_ms=t_graph, elect_ms=t_elect, compact=bool(r.compact), c16=c16 is not None,
                        rounds=int(r.rounds_exec), changes=r.changes.copy(), leader=s.to_input_order(r.leader),
                        edges=s.n_edges)

        def as_it_stands():
            restore(snap)
            return elect_here(sw)

        def resorted():
            restore(snap)
            t_resort, _ = timed(sw.resort)
            return dict(elect_here(sw), resort_ms=t_resort)

        def fresh():
            s = Swarm(ids_in, pos_in[:, 0].copy(), pos_in[:, 1].copy(), caps_in, device=dev)
            return elect_here(s)
        variants = {"i_no_resort": as_it_stands, "ii_resort": resorted, "iii_fresh_swarm": fresh}
        runs = {k: [] for k in variants}
        for rep in range(a.reps_b + 1):
            for k, fn in variants.items():
                r = fn()
                log(f"b {k} {'warm-up' if rep == 0 else rep}: graph {r['graph_ms']:.2f} ms, elect {r['elect_ms']:.2f} ms, "
                    f"compact={r['compact']}, rounds={r['rounds']}")
                if rep:
                    runs[k].append(r)
        ref = runs["iii_fresh_swarm"][0]
        for k, v in runs.items():
            for r in v:
                assert r["rounds"] == ref["rounds"] and np.array_equal(r["changes"], ref["changes"]) and \
                    np.array_equal(r["leader"], ref["leader"]) and r["edges"] == ref["edges"], k
        leg = {k: dict(elect_ms=spread([r["elect_ms"] for r in v]), build_graph_ms=spread([r["graph_ms"] for r in v]),
                       compact=v[0]["compact"], rounds=v[0]["rounds"], edges=v[0]["edges"]) for k, v in runs.items()}
        leg["ii_resort"]["resort_ms"] = spread([r["resort_ms"] for r in runs["ii_resort"]])
        e2, e3 = leg["ii_resort"]["elect_ms"], leg["iii_fresh_swarm"]["elect_ms"]
        leg["bound_ii_iii_medians_inside_each_others_span"] = bool(
            e3["min"] <= e2["median"] <= e3["max"] and e2["min"] <= e3["median"] <= e2["max"])
        leg["results_equal_in_input_order"] = True
        res["b"] = leg
        restore(snap)
        save()

    if "c" in legs:
        spans = ("ticks_1_50", "ticks_151_200", "ticks_201_250")
        times = {v: {k: [] for k in spans} for v in ("no_resort", "resort_after_200")}
        sums = {}
        moved_state(ticks + 50)  # rows that last the 50 ticks more (every run of the leg then uses the same)
        for rep in range(a.reps + 1):
            for v in times:
                reset()
                t = [timed(lambda: loop(50))[0] / 50]
                loop(100)
                t.append(timed(lambda: loop(50))[0] / 50)
                if v == "resort_after_200":
                    sw.resort()
                t.append(timed(lambda: loop(50))[0] / 50)
                log(f"c {v} {'warm-up' if rep == 0 else rep}: " + ", ".join(f"{x:.3f}" for x in t) + " ms per tick")
                if rep:
                    for k, x in zip(spans, t):
                        times[v][k].append(x)
                pin = sw.to_input_order(sw.pos)
                sums[v] = [float(pin[:, 0].sum()), float(pin[:, 1].sum()), int(sw.to_input_order(sw.leader).sum())]
        res["c"] = {v: {k: spread(x) for k, x in t.items()} for v, t in times.items()}
        res["c"]["unit"] = "ms per tick"
        res["c"]["slots"] = list(slots)
        res["c"]["end_state_checksums_input_order"] = sums

    save()
    print(json.dumps({a.label: res}))
    if "b" in res:
        assert res["b"]["bound_ii_iii_medians_inside_each_others_span"], "leg b: (ii) and (iii) differ"


if __name__ == "__main__":
    main()
