"""The task census (contract U1-C) in plain numpy, from its definition: dense (n, T) status / winner /
utility arrays, the agents' IDs and a byte mask in, the ten per-task arrays and the sorted holder pairs out.  One
loop over the tasks, one pass over a task's column each; it shares nothing with the kernels."""
import numpy as np

TENTATIVE, LOCKED, ASSIGNED = 1, 2, 3
FIELDS = ("tentative", "locked", "assigned", "tables", "holder_lo", "holder_hi", "winner_lo", "winner_hi",
          "best_winner", "best_util")


def util_image(u):
    """The order-preserving integer image of f32 bits: negative values (sign bit set) are complemented, the
    others get the sign bit -- ascending as the floats ascend, defined for any bytes."""
    b = np.asarray(u, np.float32).view(np.uint32).astype(np.uint64)
    return np.where(b & 0x80000000, b ^ 0xFFFFFFFF, b | 0x80000000)


def census(status, winner, util, ids, mask=None, entry=None):
    """status (n, T) codes 0..3; winner (n, T) int32 and util (n, T) float32, the dense claim tables; entry (n, T)
    bool, where a table holds an entry (default: winner >= 0); ids (n,) int32; mask (n,) bytes or None.  Returns
    a dict of the ten arrays plus "holders", the (task, ID) pairs with status ASSIGNED sorted by (task, ID)."""
    status, winner = np.asarray(status), np.asarray(winner, np.int32)
    util, ids = np.asarray(util, np.float32), np.asarray(ids, np.int32)
    n, T = status.shape
    counted = np.ones(n, bool) if mask is None else np.asarray(mask) != 0
    entry = winner >= 0 if entry is None else np.asarray(entry, bool)
    out = {k: np.zeros(T, np.int32) if k in FIELDS[:4] else np.full(T, -1, np.int32) for k in FIELDS[:9]}
    out["best_util"] = np.zeros(T, np.float32)
    holders = []
    for k in range(T):
        col = status[:, k]
        for name, code in (("tentative", TENTATIVE), ("locked", LOCKED), ("assigned", ASSIGNED)):
            out[name][k] = np.count_nonzero(counted & (col == code))
        held = ids[counted & (col == ASSIGNED)]
        if held.size:
            # the lows are minima of the IDs as unsigned words, the highs maxima as signed ones
            out["holder_lo"][k] = held.view(np.uint32).min().astype(np.uint32).view(np.int32)
            out["holder_hi"][k] = max(held.max(), -1)
            holders += [(k, int(i)) for i in held]
        rows = np.flatnonzero(counted & entry[:, k])
        out["tables"][k] = rows.size
        if rows.size:
            w, u = winner[rows, k], util[rows, k]
            out["winner_lo"][k] = w.view(np.uint32).min().astype(np.uint32).view(np.int32)
            out["winner_hi"][k] = max(w.max(), -1)
            img = util_image(u)
            top = img == img.max()
            best = int(np.argmin(np.where(top, w.view(np.uint32).astype(np.int64), 1 << 40)))
            out["best_winner"][k], out["best_util"][k] = w[best], u[best]
    out["holders"] = np.array(sorted(holders), np.int32).reshape(-1, 2)
    return out


def summary(c):
    """The figures of the issue's table for one census: tasks with a holder, with two or more, the most holders
    of one task, tasks whose tables name different winners."""
    return (int((c["assigned"] > 0).sum()), int((c["assigned"] >= 2).sum()), int(c["assigned"].max()),
            int((c["winner_lo"] != c["winner_hi"]).sum()))
