"""Per-workgroup clocks of single sparse rounds, from the SWARM_PHASES build (`make -C csrc phases`).
Usage: python tools/phase_probe.py LIBNAME [N] [ROUNDS]   (LIBNAME under swarm_amd/, e.g. libswarm_phases.so;
ROUNDS one round or a comma list, default 300,600,1000,1300)

Runs swarm_elect(FRONTIER) at N agents cut at max_rounds = ROUND, so that ROUND is the last round launched,
and reads that round's per-workgroup clocks (g_phase, 100 MHz): start, end, stamps in (the marked lanes of the
first chunk group known), listed (the list complete), gathered.  Three elections per round; per election the
median over workgroups of stamps-in minus start and of end minus start, and the median and the slowest
workgroup of "list built - stamps in" and of "end - gathered" (the counter flush), in microseconds."""
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, "distributed-swarm-algorithm_amd")
import torch  # noqa: E402
from swarm_amd import _lib  # noqa: E402

L = _lib.load(os.path.join(_lib.HERE, sys.argv[1]))
from swarm_amd import gen  # noqa: E402
from swarm_amd.swarm import Swarm  # noqa: E402

n = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
rounds = [int(r) for r in (sys.argv[3] if len(sys.argv) > 3 else "300,600,1000,1300").split(",")]
d = gen.swarm_inputs(n, 2026, t=0)
sw = Swarm(d["ids"], d["x"], d["y"], d["caps"], device="cuda:0").build_graph(1.0)
L.swarm_debug_phases.argtypes = [ctypes.c_void_p, ctypes.c_int]
L.swarm_debug_phases.restype = ctypes.c_int
for rnd in rounds:
    for _ in range(3):
        r = sw.elect(max_rounds=rnd)
        torch.cuda.synchronize()
        assert r.rounds_exec == rnd and not r.converged, (r.rounds_exec, r.converged)
        ph = np.zeros(2048 * 8, np.uint64)
        _lib.check(L.swarm_debug_phases(ph.ctypes.data_as(ctypes.c_void_p), len(ph)))
        ph = ph.reshape(-1, 8).astype(np.int64)
        ph = ph[(ph[:, 0] > 0) & (ph[:, 4] > 0)]
        us = lambda a, b: (ph[:, a] - ph[:, b]) / 100.0  # noqa: E731
        lst, fl = us(5, 4), us(1, 6)
        print(f"{sys.argv[1]}: n={n} round {rnd}: over {len(ph)} workgroups: stamps-in - start median "
              f"{np.median(us(4, 0)):.2f} us, end - start median {np.median(us(1, 0)):.2f} us, list built - stamps "
              f"in median {np.median(lst):.2f} slowest {lst.max():.2f} us, end - gathered median "
              f"{np.median(fl):.2f} slowest {fl.max():.2f} us, list built - start median {np.median(us(5, 0)):.2f} "
              f"slowest {us(5, 0).max():.2f} us")
