"""Start-of-round clocks of one sparse round, from the SWARM_PHASES build (`make -C csrc phases`).
Usage: python tools/phase_probe.py LIBNAME [N] [ROUND]   (LIBNAME under swarm_amd/, e.g. libswarm_phases.so)

Runs swarm_elect(FRONTIER) at N agents cut at max_rounds = ROUND, so that ROUND is the last round launched,
and reads that round's per-workgroup clocks (g_phase, 100 MHz): start, end, stamps in, listed, gathered.
Prints the median over workgroups of stamps-in minus start and of end minus start, in microseconds."""
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
rnd = int(sys.argv[3]) if len(sys.argv) > 3 else 1000
d = gen.swarm_inputs(n, 2026, t=0)
sw = Swarm(d["ids"], d["x"], d["y"], d["caps"], device="cuda:0").build_graph(1.0)
L.swarm_debug_phases.argtypes = [ctypes.c_void_p, ctypes.c_int]
L.swarm_debug_phases.restype = ctypes.c_int
res = []
for _ in range(3):
    r = sw.elect(max_rounds=rnd)
    torch.cuda.synchronize()
    assert r.rounds_exec == rnd and not r.converged, (r.rounds_exec, r.converged)
    ph = np.zeros(2048 * 8, np.uint64)
    _lib.check(L.swarm_debug_phases(ph.ctypes.data_as(ctypes.c_void_p), len(ph)))
    ph = ph.reshape(-1, 8).astype(np.int64)
    ph = ph[(ph[:, 0] > 0) & (ph[:, 4] > 0)]
    res.append((np.median(ph[:, 4] - ph[:, 0]) / 100.0, np.median(ph[:, 1] - ph[:, 0]) / 100.0, len(ph)))
for a, b, k in res:
    print(f"{sys.argv[1]}: n={n} round {rnd}: median over {k} workgroups: stamps-in - start {a:.2f} us, "
          f"end - start {b:.2f} us")
