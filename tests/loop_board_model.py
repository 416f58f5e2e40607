"""Dense <-> sparse converters for the board update loop (contract U1-B) -- TESTS ONLY.

The CPU models (loop_tasks_model, loop_lossy_model) keep every agent's task state dense: status (n x T codes),
tab_winner / tab_util (n x T), and the sends of the last two ticks as lists of (task, payload) per agent
(`tasks` in their result).  swarm_update_loop_board keeps it in sparse canonical rows.  Nothing here models
anything: these only move the same state between the two layouts.
"""
import numpy as np


def sparse_status(status, Ks):
    """(n, T) codes -> (n, Ks) int32 rows of task << 2 | code, ascending by task, -1 behind the last entry."""
    status = np.asarray(status)
    n = status.shape[0]
    out = np.full((n, Ks), -1, np.int32)
    for i in range(n):
        k = np.flatnonzero(status[i])
        if len(k) > Ks:
            raise ValueError(f"agent {i} holds {len(k)} statuses, the rows {Ks}")
        out[i, :len(k)] = (k.astype(np.int64) << 2 | status[i, k]).astype(np.int32)
    return out


def dense_status(rows, T):
    rows = np.asarray(rows)
    out = np.zeros((rows.shape[0], T), np.uint8)
    i, s = np.nonzero(rows >= 0)
    out[i, rows[i, s] >> 2] = rows[i, s] & 3
    return out


def sparse_tables(tab_winner, tab_util, Kt):
    """Dense tables (-1 = no entry) -> (task, winner, utility) rows of Kt slots; an empty slot is (-1, -1, 0)."""
    tab_winner, tab_util = np.asarray(tab_winner), np.asarray(tab_util, np.float32)
    n = tab_winner.shape[0]
    tt, tw = np.full((n, Kt), -1, np.int32), np.full((n, Kt), -1, np.int32)
    tu = np.zeros((n, Kt), np.float32)
    for i in range(n):
        k = np.flatnonzero(tab_winner[i] >= 0)
        if len(k) > Kt:
            raise ValueError(f"agent {i} holds {len(k)} table entries, the rows {Kt}")
        tt[i, :len(k)], tw[i, :len(k)], tu[i, :len(k)] = k, tab_winner[i, k], tab_util[i, k]
    return tt, tw, tu


def dense_tables(tab_task, tab_winner, tab_util, T):
    tab_task = np.asarray(tab_task)
    n = tab_task.shape[0]
    w, u = np.full((n, T), -1, np.int32), np.zeros((n, T), np.float32)
    i, s = np.nonzero(tab_task >= 0)
    w[i, tab_task[i, s]] = np.asarray(tab_winner)[i, s]
    u[i, tab_task[i, s]] = np.asarray(tab_util)[i, s]
    return w, u


def sparse_sets(lists, K):
    """Per-agent lists of tasks (or of (task, payload) messages) -> (n, K) int32 rows: the distinct tasks
    ascending, -1 behind the last."""
    out = np.full((len(lists), K), -1, np.int32)
    for i, msgs in enumerate(lists):
        k = sorted({int(m[0]) if isinstance(m, (tuple, list)) else int(m) for m in msgs})
        if len(k) > K:
            raise ValueError(f"agent {i} sent on {len(k)} tasks, the rows hold {K}")
        out[i, :len(k)] = k
    return out


def set_lists(rows):
    """Rows of task indices -> per-agent sorted lists."""
    return [[int(k) for k in r if k >= 0] for r in np.asarray(rows)]


def out_rows(model, Ks, Kt):
    """The model's sends of its last two ticks as claim_out / conflict_out, (2, n, K) by tick parity."""
    tk, end = model["tasks"], int(model["tick"])
    n = len(tk["claims"])
    cl, cf = np.full((2, n, Ks), -1, np.int32), np.full((2, n, Kt), -1, np.int32)
    for tick, c, f in ((end - 1, tk["claims_prev"], tk["conflicts_prev"]), (end, tk["claims"], tk["conflicts"])):
        cl[tick & 1], cf[tick & 1] = sparse_sets(c, Ks), sparse_sets(f, Kt)
    return cl, cf


def sparse_state(model, Ks, Kt):
    """Everything swarm_board_state holds, from a model result."""
    tt, tw, tu = sparse_tables(model["tab_winner"], model["tab_util"], Kt)
    cl, cf = out_rows(model, Ks, Kt)
    return dict(status=sparse_status(model["status"], Ks), tab_task=tt, tab_winner=tw, tab_util=tu, claim_out=cl,
                conflict_out=cf)


def peak_slots(model):
    """(status entries, table entries) the fullest agent holds at the end of the model's run."""
    return int((np.asarray(model["status"]) != 0).sum(1).max(initial=0)), \
        int((np.asarray(model["tab_winner"]) >= 0).sum(1).max(initial=0))
