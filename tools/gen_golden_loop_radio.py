#!/usr/bin/env python3
"""Generate tests/golden/loop_radio_*.npz by driving REAL reference agents through the update loop with both
their sensors and their radio neighbours refreshed every tick (build container only; the helpers are
tools/gen_golden_loop.py's and tools/gen_golden_loop_sensed.py's).

Contract U1-R: gen_golden_loop.ref_loop -- the lock-step loop of contract U1 -- with, every tick,
the packets of the previous tick delivered from the agents within radio_radius of the receiver in the snapshot
at the start of the tick (dx*dx + dy*dy <= Rc*Rc on the snapshot's doubles, ascending index), and
update_sensors fed the agents within sense_radius of the same snapshot, as U1-S.  There is no message graph:
the inputs' row_ptr / col (the radius-2.5 graph of the tick-0 positions, kept so that the frozen-graph run can
be told from this one) are not read.  Only data is written: the inputs (loop_sensed_*'s keys plus
radio_radius), every final per-agent array and the per-tick counts.  tests/golden/index.json is not touched.

Usage:  python tools/gen_golden_loop_radio.py [--only NAME ...]
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
import gen_golden_loop_sensed as ggs  # noqa: E402

RADIO_RADIUS = 2.5
RADIO_CASES = {
    # loop_n200's inputs and kills, heard and sensed at 2.5
    "loop_radio_n200": dict(ggl.LOOP_CASES["loop_n200"], sense_radius=2.5),
    # a sensing radius below the personal space and below the radio radius
    "loop_radio_r12_n250": dict(ggl.LOOP_CASES["loop_n250"], sense_radius=1.2),
    # IDs > 255: the wide codec path
    "loop_radio_wide_n400": dict(ggl.LOOP_CASES["loop_wide_n400"], sense_radius=2.5),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=None)
    args = ap.parse_args()
    mod = gg.load_reference()
    for name, c in RADIO_CASES.items():
        if args.only is not None and name not in args.only:
            continue
        t0 = time.time()
        inp = ggl.make_loop_inputs(c)
        inp["sense_radius"] = np.float64(c["sense_radius"])
        inp["radio_radius"] = np.float64(RADIO_RADIUS)
        sensed, heard = ggs.sensed_rows(float(c["sense_radius"])), ggs.sensed_rows(RADIO_RADIUS)
        out = ggl.ref_loop(mod, inp, sensed=sensed, heard=heard)
        arrays = dict(inp)
        arrays.update(out)
        np.savez_compressed(os.path.join(gg.OUT, name + ".npz"), **arrays)
        fol = (out["state_out"] == 1) & (out["has_lpos_out"] == 1) & (out["alive_out"] == 1)
        print(name, "Rs", c["sense_radius"], "followers with leader_pos", int(fol.sum()), "dead",
              int((out["alive_out"] == 0).sum()), "leaders at the end", int(out["counts"][-1, 0]),
              "longest radio row", heard.longest, "longest sensed row", sensed.longest, "extent x %.0f y %.0f" %
              (np.ptp(out["x_out"]), np.ptp(out["y_out"])), "%.1fs" % (time.time() - t0))


if __name__ == "__main__":
    main()
