"""Sparse election launches of a rocprofv3 --kernel-trace --stats run of the bench, split by round range, for
elections with or without pair rounds ("pair rounds").
Usage: python tools/pair_ranges.py DIR [DENSE_ROUNDS] [ROUNDS_EXEC]   (DIR: rocprofv3's -d output directory)

A k_sparse_block dispatch covers one round, or two when it is the pair instantiation (its last template
argument has bit 32 set: <..., 38u>); dispatch i of an election starts at the round behind the one the dispatch
before it ended at, the first at DENSE_ROUNDS + 1.  Per range of first rounds (the issue's: 10-99, 100-399,
400-906, 907-ROUNDS_EXEC, and the launches past convergence) it prints launches, total, median and slowest per
election, then the pair launches' count, median and slowest and the sparse kernel time per election."""
import csv
import glob
import os
import re
import sys

import numpy as np

d = sys.argv[1]
dense = int(sys.argv[2]) if len(sys.argv) > 2 else 9
rexec = int(sys.argv[3]) if len(sys.argv) > 3 else 1364


def find(suffix):
    hits = sorted(glob.glob(os.path.join(d, "**", "*" + suffix), recursive=True))
    assert hits, f"no *{suffix} under {d}"
    return hits[0]


rows = sorted(csv.DictReader(open(find("kernel_trace.csv"))), key=lambda r: int(r["Start_Timestamp"]))
elections, cur, seen_dense = [], None, 0
for r in rows:
    name = r["Kernel_Name"]
    if "k_elect_dense" in name:
        if seen_dense % dense == 0:
            cur = []
            elections.append(cur)
        seen_dense += 1
    elif "k_sparse_block" in name and cur is not None:
        m = re.search(r"(\d+)u?>", name)
        lf = int(m.group(1)) if m else 0
        cur.append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), 2 if lf & 32 else 1))
ranges = [(dense + 1, 99), (100, 399), (400, 906), (907, rexec), (rexec + 1, 1 << 30)]
tot = {k: [] for k in ranges}
pairs, per_election, launches = [], [], []
for e in elections:
    t = dense + 1
    acc = {k: [] for k in ranges}
    for dur, nr in e:
        for k in ranges:
            if k[0] <= t <= k[1]:
                acc[k].append(dur)
        if nr == 2:
            pairs.append(dur)
        t += nr
    for k in ranges:
        tot[k].append(acc[k])
    per_election.append(sum(x for x, _ in e))
    launches.append(len(e))
print(f"  elections {len(elections)}, sparse launches per election {sorted(set(launches))}, sparse kernel time per "
      f"election {np.mean(per_election) / 1e6:.3f} ms")
for k in ranges:
    a = [x for e in tot[k] for x in e]
    if not a:
        continue
    name = f"rounds {k[0]}-{k[1]}" if k[1] < (1 << 30) else f"past convergence (from round {k[0]})"
    print(f"  {name}: launches {len(a) / len(elections):.0f} per election, {np.sum(a) / len(elections) / 1e6:.3f} ms "
          f"per election, median {np.median(a):.0f} ns, slowest {np.max(a)} ns")
if pairs:
    print(f"  pair launches: {len(pairs) / len(elections):.0f} per election, median {np.median(pairs):.0f} ns, slowest "
          f"{np.max(pairs)} ns")
