"""Summary of a rocprofv3 --kernel-trace --stats run of the bench for the sparse election rounds, in the form
of profiles/r13_round_start/round_ranges.txt.
Usage: python tools/round_ranges.py DIR [DENSE_ROUNDS] [ROUNDS_EXEC]   (DIR: rocprofv3's -d output directory)

Prints the five largest rows of the kernel stats, then from the kernel trace the k_sparse_block dispatches in
launch order, cut into elections of equal length: the median duration of the no-op rounds launched past
convergence (rounds ROUNDS_EXEC + 1 ...), the median of rounds 907 ... ROUNDS_EXEC, and the sparse kernel time
per election.  Dispatch i of an election is round DENSE_ROUNDS + 1 + i."""
import csv
import glob
import os
import sys

import numpy as np

d = sys.argv[1]
dense = int(sys.argv[2]) if len(sys.argv) > 2 else 9
rexec = int(sys.argv[3]) if len(sys.argv) > 3 else 1364


def find(suffix):
    hits = sorted(glob.glob(os.path.join(d, "**", "*" + suffix), recursive=True))
    assert hits, f"no *{suffix} under {d}"
    return hits[0]


rows = list(csv.DictReader(open(find("kernel_stats.csv"))))
for r in sorted(rows, key=lambda r: -int(r["TotalDurationNs"]))[:5]:
    print(f"  {r['Name'][:70]}: calls {r['Calls']} avg {float(r['AverageNs']):.0f} ns total "
          f"{int(r['TotalDurationNs']) / 1e6:.3f} ms")
tr = [r for r in csv.DictReader(open(find("kernel_trace.csv"))) if "k_sparse_block" in r["Kernel_Name"]]
tr.sort(key=lambda r: int(r["Start_Timestamp"]))
dur = np.array([int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in tr], np.int64)
# an election's sparse dispatches: the dense kernels between them cut the trace into elections
dn = sorted(int(r["Start_Timestamp"]) for r in csv.DictReader(open(find("kernel_trace.csv")))
            if "k_elect_dense" in r["Kernel_Name"])
elections = max(1, len(dn) // dense) if dense else 1
per = len(dur) // elections
print(f"  k_sparse_block dispatches {len(dur)} = {elections} elections x {per} (+{len(dur) - elections * per})")
e = dur[:elections * per].reshape(elections, per)
first = dense + 1  # round of dispatch 0
noop = e[:, rexec + 1 - first:]
tail = e[:, 907 - first:rexec + 1 - first]
print(f"  no-op rounds {rexec + 1}-{first + per - 1}: median {np.median(noop):.0f} ns; rounds 907-{rexec} median "
      f"{np.median(tail):.0f} ns; sparse kernel time per election {e.sum() / elections / 1e6:.3f} ms")
