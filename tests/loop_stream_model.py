"""CPU model of task boards that reuse the slots of closed tasks (contract U1-P) -- TESTS ONLY.

A thin driver over the unchanged loop_lifetimes_model.drive(..., start=), in segments, with *places* between them.
A place, after tick `last` has run, gives slot k a new task: a position, a velocity, a requirement and a window
that opens after `last`.  Two forms of the same run:

  (a) slot form (drive_slots): the board has T columns.  A place rewrites column k's cur / lag / V / window /
      requirement and, unless keep_tables, clears column k of the model's claim tables (the purge).  Before it
      writes, the driver checks what the quiet rule promises: the slot was absent at ticks last and last - 1, no
      agent holds a status about it, and no claim or conflict sent at tick `last` names it.
  (b) virtual form (drive_virtual): one column per *life*, every life a plain U1-A window fixed from the start --
      the reference's dict, whose arrivals get fresh keys.  The driver only sets a life's cur / lag at the tick
      it is placed (an absent column's position is never read).  Nothing is purged, nothing rewritten.

The lives 0 .. T - 1 are the tasks the board is created with (slot k holds life k); a place names the life each
slot takes.  to_slots() maps a virtual result through the slot map; contract U1-P.4 says it equals the slot form.

init:   dict(pos (T, 2), vel (T, 2), req (T,), open (T,), close (T,))
places: list of dict(tick (the last tick run before the place), slot (m,), life (m,), pos (m, 2), vel (m, 2),
        req (m,), open (m,), close (m,)), ascending by tick.
"""
import numpy as np

import loop_board_model as lbm
import loop_lifetimes_model as llm

FOREVER = llm.FOREVER


def eligible(open_tick, close_tick, last):
    """The quiet rule: absent at ticks last and last - 1 (comparisons only, as csrc/task_place.h)."""
    lo, hi = np.asarray(open_tick, np.int64), np.asarray(close_tick, np.int64)
    return (hi < last) | (lo > last) | (lo == hi)


def case_from_fixture(g):
    """(init, places, T) of a tools/gen_golden_task_stream.py fixture: its arrays are per life (task_x, task_y,
    task_req, task_vx, task_vy, open_tick, close_tick, life_slot, life_place); lives 0 .. T - 1 are the first
    tenants of slots 0 .. T - 1, the others were placed after tick life_place."""
    T = int(g["slots"])
    per_life = dict(pos=np.stack([g["task_x"], g["task_y"]], 1), vel=np.stack([g["task_vx"], g["task_vy"]], 1),
                    req=np.asarray(g["task_req"], np.int64), open=np.asarray(g["open_tick"], np.int64),
                    close=np.asarray(g["close_tick"], np.int64))
    slot, place = np.asarray(g["life_slot"], np.int64), np.asarray(g["life_place"], np.int64)
    assert (slot[:T] == np.arange(T)).all() and (place[:T] < 0).all() and (place[T:] >= 0).all()
    init = {k: v[:T].copy() for k, v in per_life.items()}
    places = []
    for t in np.unique(place[T:]):
        i = np.flatnonzero(place == t)
        places.append(dict(tick=int(t), slot=slot[i], life=i, **{k: v[i] for k, v in per_life.items()}))
    return init, places, T


def _segments(places, first, ticks):
    """(ticks to run, the places after them) up to the absolute tick `ticks` (later places are not reached)."""
    now, out = 0, []
    for e in places:
        t = int(e["tick"])
        if t > ticks:
            break
        assert first < t and t >= now, "a place comes after a tick run on the board, in order"
        out.append((t - now, e))
        now = t
    out.append((ticks - now, None))
    return out


def _drive(oracle_mod, q, segs, first, state, apply, kw):
    d = None
    for seg, e in segs:
        if d is None:
            d = llm.drive(oracle_mod, q, state["cur0"], state["V"], state["open"], state["close"], seg - first,
                          first=first, **kw)
        elif seg:
            d = llm.drive(oracle_mod, q, None, state["V"], state["open"], state["close"], seg, start=d, **kw)
        if e is not None:
            apply(d, e)
    return d


def drive_slots(oracle_mod, q, init, places, ticks, *, first=0, keep_tables=False, **kw):
    """Form (a) -> loop_lifetimes_model.drive's dict plus `purged` (table entries removed, per place), `stale`
    ((place, slot, agent, winner) of every table entry found about a slot being placed) and the board's final
    `open` / `close` / `req` / `V` / `life` (the life in each slot)."""
    T = len(init["open"])
    req = np.array(init["req"], np.int64)
    q = dict(q, task_x=np.array(init["pos"][:, 0]), task_y=np.array(init["pos"][:, 1]), task_req=req)
    st = dict(cur0=np.array(init["pos"], np.float64), V=np.array(init["vel"], np.float64),
              open=np.array(init["open"], np.int64), close=np.array(init["close"], np.int64))
    life = np.arange(T, dtype=np.int64)
    purged, stale = [], []

    def apply(d, e):
        last, k = int(e["tick"]), np.asarray(e["slot"], np.int64)
        tk = d["o"]["tasks"]
        assert int(d["o"]["tick"]) == last and len(np.unique(k)) == len(k)
        assert eligible(st["open"][k], st["close"][k], last).all(), "a slot that is not eligible"
        assert (np.asarray(e["open"]) > last).all() and (np.asarray(e["open"]) <= np.asarray(e["close"])).all()
        # what the quiet rule promises: no status, and nothing sent at tick `last`, about the slot
        assert (tk["status"][:, k] == 0).all()
        sent = {int(msg[0]) for key in ("claims", "conflicts") for row in tk[key] for msg in row}
        assert not sent & set(k.tolist()), "a message in flight names a placed slot"
        held = tk["tab_winner"][:, k] >= 0
        for a, j in zip(*np.nonzero(held)):
            stale.append((len(purged), int(k[j]), int(a), int(tk["tab_winner"][a, k[j]])))
        if keep_tables:
            purged.append(0)
        else:
            purged.append(int(held.sum()))
            tk["tab_winner"][:, k] = -1
            tk["tab_util"][:, k] = 0
        d["cur"][k] = d["lag"][k] = np.asarray(e["pos"], np.float64)
        st["V"][k] = e["vel"]
        req[k] = e["req"]
        st["open"][k], st["close"][k] = e["open"], e["close"]
        life[k] = e["life"]

    d = _drive(oracle_mod, q, _segments(places, first, ticks), first, st, apply, kw)
    d.update(purged=purged, stale=stale, open=st["open"], close=st["close"], req=req, V=st["V"], life=life)
    return d


def virtual_board(init, places):
    """The board with one index per life: dict(pos, vel, req, open, close, slot) over all lives."""
    T = len(init["open"])
    L = T + sum(len(e["slot"]) for e in places)
    b = dict(pos=np.zeros((L, 2)), vel=np.zeros((L, 2)), req=np.full(L, -1, np.int64), open=np.zeros(L, np.int64),
             close=np.zeros(L, np.int64), slot=np.full(L, -1, np.int64))
    for key in ("pos", "vel", "req", "open", "close"):
        b[key][:T] = init[key]
    b["slot"][:T] = np.arange(T)
    for e in places:
        i = np.asarray(e["life"], np.int64)
        assert (b["slot"][i] < 0).all() and (i >= T).all(), "every arrival is a fresh life"
        for key in ("pos", "vel", "req", "open", "close", "slot"):
            b[key][i] = e[key]
    assert (b["slot"] >= 0).all()
    return b


def drive_virtual(oracle_mod, q, init, places, ticks, *, first=0, **kw):
    """Form (b) -> loop_lifetimes_model.drive's dict plus `board` (virtual_board)."""
    b = virtual_board(init, places)
    q = dict(q, task_x=np.array(b["pos"][:, 0]), task_y=np.array(b["pos"][:, 1]), task_req=b["req"])
    st = dict(cur0=b["pos"].copy(), V=b["vel"], open=b["open"], close=b["close"])

    def apply(d, e):
        i = np.asarray(e["life"], np.int64)
        d["cur"][i] = d["lag"][i] = np.asarray(e["pos"], np.float64)

    d = _drive(oracle_mod, q, _segments(places, first, ticks), first, st, apply, kw)
    d["board"] = b
    return d


def to_slots(v, life):
    """A virtual result as the slot form sees it: the columns of the lives now in the slots (`life`, drive_slots'),
    the message records renamed life -> slot (a life has one slot, and two lives of a slot are never named by one
    tick's records).  -> dict(status, tab_winner, tab_util, cur, lag, claims, conflicts, claims_prev,
    conflicts_prev)."""
    o, slot = v["o"], v["board"]["slot"]
    tk = o["tasks"]
    out = dict(status=o["status"][:, life], tab_winner=o["tab_winner"][:, life], tab_util=o["tab_util"][:, life],
               cur=v["cur"][life], lag=v["lag"][life])
    for key in ("claims", "conflicts", "claims_prev", "conflicts_prev"):
        out[key] = [sorted({int(slot[int(msg[0])]) for msg in row}) for row in tk[key]]
    return out


def slot_view(d):
    """The slot form's result in to_slots' shape."""
    o = d["o"]
    tk = o["tasks"]
    out = dict(status=o["status"], tab_winner=o["tab_winner"], tab_util=o["tab_util"], cur=d["cur"], lag=d["lag"])
    for key in ("claims", "conflicts", "claims_prev", "conflicts_prev"):
        out[key] = [sorted({int(msg[0]) for msg in row}) for row in tk[key]]
    return out


def assert_same(a, b):
    """Two views equal bit for bit."""
    for key in ("status", "tab_winner", "cur", "lag"):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    np.testing.assert_array_equal(np.asarray(a["tab_util"], np.float32).view(np.uint32),
                                  np.asarray(b["tab_util"], np.float32).view(np.uint32), err_msg="tab_util")
    for key in ("claims", "conflicts", "claims_prev", "conflicts_prev"):
        assert a[key] == b[key], key


def assert_same_counts(a, b):
    """The per-tick counts of two drives."""
    for key in ("counts", "task_counts", "link_counts"):
        if a["acc"][key] or b["acc"][key]:
            np.testing.assert_array_equal(np.concatenate(a["acc"][key]), np.concatenate(b["acc"][key]), err_msg=key)
    assert a["acc"]["guard"] == b["acc"]["guard"] and a["acc"]["singular"] == b["acc"]["singular"]


def peaks(d):
    """(status entries, table entries) of the fullest agent over the run."""
    p = np.asarray(d["acc"]["peaks"])
    return int(p[:, 0].max()), int(p[:, 1].max())


__all__ = ["FOREVER", "eligible", "drive_slots", "drive_virtual", "virtual_board", "to_slots", "slot_view",
           "assert_same", "assert_same_counts", "peaks", "lbm"]
