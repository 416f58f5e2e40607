#!/usr/bin/env python3
"""Generate tests/golden/loop_sensed_*.npz by driving REAL reference agents through the update loop with
their sensors refreshed every tick (build container only; the helpers are tools/gen_golden_loop.py's).

Contract U1-S: gen_golden_loop.ref_loop -- the lock-step loop of contract U1 -- with
update_sensors fed, every tick, the agents within sense_radius of the tick's snapshot (dx*dx + dy*dy <= R*R
on the snapshot's doubles), in ascending index, dead ones included.  The message graph is the radius-2.5
graph of the tick-0 positions for the whole run.  Only data is written: the inputs (loop_*'s keys plus
sense_radius), every final per-agent array and the per-tick counts.  tests/golden/index.json is not touched.

Usage:  python tools/gen_golden_loop_sensed.py [--only NAME ...]
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as gg  # noqa: E402
import gen_golden_loop as ggl  # noqa: E402

SENSED_CASES = {
    # loop_n200's inputs and kills, sensed at the message radius: cells of side 2 (min(R, 2))
    "loop_sensed_n200": dict(ggl.LOOP_CASES["loop_n200"], sense_radius=2.5),
    # a sensing radius below the personal space: cells of side R
    "loop_sensed_r12_n250": dict(ggl.LOOP_CASES["loop_n250"], sense_radius=1.2),
    # IDs > 255: the wide codec path
    "loop_sensed_wide_n400": dict(ggl.LOOP_CASES["loop_wide_n400"], sense_radius=2.5),
}


def sensed_rows(radius):
    """snapshot -> per agent, the indices within `radius` of it (itself excluded), ascending."""
    def rows(snap):
        p = np.asarray(snap, np.float64)
        dx, dy = p[:, 0][:, None] - p[:, 0][None, :], p[:, 1][:, None] - p[:, 1][None, :]
        near = dx * dx + dy * dy <= radius * radius
        np.fill_diagonal(near, False)
        rows.longest = max(rows.longest, int(near.sum(1).max()))
        return [np.flatnonzero(r) for r in near]
    rows.longest = 0
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=None)
    args = ap.parse_args()
    mod = gg.load_reference()
    for name, c in SENSED_CASES.items():
        if args.only is not None and name not in args.only:
            continue
        t0 = time.time()
        inp = ggl.make_loop_inputs(c)
        inp["sense_radius"] = np.float64(c["sense_radius"])
        rows = sensed_rows(float(c["sense_radius"]))
        out = ggl.ref_loop(mod, inp, sensed=rows)
        arrays = dict(inp)
        arrays.update(out)
        np.savez_compressed(os.path.join(gg.OUT, name + ".npz"), **arrays)
        fol = (out["state_out"] == 1) & (out["has_lpos_out"] == 1) & (out["alive_out"] == 1)
        print(name, "R", c["sense_radius"], "followers with leader_pos", int(fol.sum()), "dead",
              int((out["alive_out"] == 0).sum()), "longest sensed row", rows.longest, "extent x %.0f y %.0f" %
              (np.ptp(out["x_out"]), np.ptp(out["y_out"])), "%.1fs" % (time.time() - t0))


if __name__ == "__main__":
    main()
