"""Adversarial auction instances (plain numpy, no HIP) and the auction's defining properties.

Every family returns ``(args, kw)``: ``args = (ids, x, y, caps, tx, ty, treq)`` and the keyword
arguments (``eps``, ``claim_thr``, ``u_scale``, ``max_rounds``) both ``oracle.auction`` and
``Swarm.auction`` take.  IDs are a seeded permutation (spread out, never ``arange``), so storage
order, ID order and task order all differ.  tests/test_auction_edges.py says what each family pins.
"""
import itertools

import numpy as np

ALL_CAPS = np.uint32(0xF)
# list lengths around the pass boundaries of group_bid<64,4> (256 per pass) and group_bid<16,8> (128)
ISLAND_LENGTHS = (1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1025)


def _ids(n, seed):
    return (np.random.default_rng(seed).permutation(n) * 7 + 3).astype(np.int32)


def _treq(t, seed):
    return np.random.default_rng(seed).integers(-1, 4, t).astype(np.int8)


def price_war(n, t, eps=0.1, seed=101, **kw):
    """All agents at one point with every capability, all tasks at one other point 0.5 away: one
    value, so every best/second tie goes to the lowest task index, every bid tie to the lowest ID,
    and every increment is eps alone.  n > t: a standing crowd of n - t bidders."""
    ids = _ids(n, seed)
    x, y = np.full(n, 3.0), np.full(n, 4.0)
    caps = np.full(n, ALL_CAPS, np.uint32)
    tx, ty = np.full(t, 3.5), np.full(t, 4.0)
    return (ids, x, y, caps, tx, ty, _treq(t, seed + 1)), dict(eps=eps, **kw)


def scarce_agents(n=12, t=96, eps=0.1, seed=103):
    """price_war with t > n: the agents take tasks 0 .. n-1 one round at a time (all bid on the
    lowest free index, the lowest ID wins); no task is ever bid on twice, every price is eps."""
    assert t > n
    return price_war(n, t, eps=eps, seed=seed)


def islands(lengths=ISLAND_LENGTHS, seed=107):
    """Islands 10 apart on a line, claim radius 4 (claim_thr 20), 3 co-located agents each; every
    length L of `lengths` twice: once with its L tasks co-located (equal values: ties by task index
    across lanes and passes) and once at L distinct distances.  Task indices are shuffled, so an
    island's tasks are neither contiguous nor in list order.  Plus 4 agents with no task in reach.
    Returns the per-agent intended list length and co-location flag in kw["_meta"]."""
    rng = np.random.default_rng(seed)
    ax, ay, tx, ty, want, colo = [], [], [], [], [], []
    j = 0
    for L in lengths:
        for same in (True, False):
            cx = 10.0 * j
            ax += [cx] * 3
            ay += [0.0] * 3
            want += [L] * 3
            colo += [same] * 3
            if same:
                tx += [cx + 1.0] * L
                ty += [0.0] * L
            else:
                d = 0.5 + 3.0 * np.arange(L) / L          # distinct, all inside the radius
                th = 2.399963229728653 * np.arange(L)     # golden angle: spread over the disc
                tx += list(cx + d * np.cos(th))
                ty += list(d * np.sin(th))
            j += 1
    for cx, cy in ((-10.0, 0.0), (10.0 * j, 0.0), (5.0, 30.0), (15.0, -30.0)):  # nothing in reach
        ax.append(cx)
        ay.append(cy)
        want.append(0)
        colo.append(False)
    n, t = len(ax), len(tx)
    tp = rng.permutation(t)
    ap = rng.permutation(n)
    tx, ty = np.asarray(tx)[tp], np.asarray(ty)[tp]
    meta = dict(want=np.asarray(want)[ap], colocated=np.asarray(colo)[ap])
    args = (_ids(n, seed + 1), np.asarray(ax)[ap], np.asarray(ay)[ap], np.full(n, ALL_CAPS, np.uint32), tx, ty,
            _treq(t, seed + 2))
    return args, dict(eps=0.1, _meta=meta)


def clusters(k=8, agents=20, tasks=6, eps=0.1, seed=109):
    """k clusters (4 per row, pitch 5) of `agents` nearly co-located agents (scatter 0.005) contesting
    `tasks` tasks scattered 0.3 around them, capabilities mixed and requirements in {-1, 0..3}:
    hundreds of rounds of contested price rises over uneven, capability-dependent lists."""
    rng = np.random.default_rng(seed)
    cx = 5.0 * (np.arange(k) % 4)
    cy = 5.0 * (np.arange(k) // 4)
    x = np.repeat(cx, agents) + rng.normal(0, 0.005, k * agents)
    y = np.repeat(cy, agents) + rng.normal(0, 0.005, k * agents)
    tx = np.repeat(cx, tasks) + rng.normal(0, 0.3, k * tasks)
    ty = np.repeat(cy, tasks) + rng.normal(0, 0.3, k * tasks)
    caps = rng.integers(1, 16, k * agents).astype(np.uint32)
    ap, tp = rng.permutation(k * agents), rng.permutation(k * tasks)
    return (_ids(k * agents, seed + 1), x[ap], y[ap], caps[ap], tx[tp], ty[tp], _treq(k * tasks, seed + 2)[tp]), \
        dict(eps=eps)


def lattice(side=20, transposed=False, seed=113):
    """Agents on a side x side lattice of pitch 0.5, tasks on the (side/2)^2 sub-lattice of pitch 1
    offset by 0.25: symmetric distances, many equal values between distinct positions.
    transposed: the roles swapped (t > n)."""
    rng = np.random.default_rng(seed)
    g = np.arange(side) * 0.5
    fx, fy = [v.ravel() for v in np.meshgrid(g, g)]
    h = 0.25 + np.arange(side // 2) * 1.0
    cx, cy = [v.ravel() for v in np.meshgrid(h, h)]
    if transposed:
        fx, fy, cx, cy = cx, cy, fx, fy
    ap, tp = rng.permutation(len(fx)), rng.permutation(len(cx))
    n, t = len(fx), len(cx)
    return (_ids(n, seed + 1), fx[ap], fy[ap], np.full(n, ALL_CAPS, np.uint32), cx[tp], cy[tp],
            np.full(t, -1, np.int8)), dict(eps=0.1)


def wide_reach(n=200, t=3000, claim_thr=5.0, u_scale=100.0, seed=127):
    """Uniform agents and tasks in a 10 x 10 box under a claim radius of 19: every agent's list
    holds every task (one grid cell, n * t pairs)."""
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(0, 10, n), rng.uniform(0, 10, n)
    tx, ty = rng.uniform(0, 10, t), rng.uniform(0, 10, t)
    return (_ids(n, seed + 1), x, y, np.full(n, ALL_CAPS, np.uint32), tx, ty, _treq(t, seed + 2)), \
        dict(eps=0.1, claim_thr=claim_thr, u_scale=u_scale)


def no_reach(claim_thr=100.0, n=40, t=24, seed=131):
    """claim_thr >= u_scale: claim radius <= 0, no admissible pair; one round, everyone drops out."""
    rng = np.random.default_rng(seed)
    return (_ids(n, seed + 1), rng.uniform(0, 3, n), rng.uniform(0, 3, n), np.full(n, ALL_CAPS, np.uint32),
            rng.uniform(0, 3, t), rng.uniform(0, 3, t), _treq(t, seed + 2)), \
        dict(eps=0.1, claim_thr=claim_thr, u_scale=100.0)


def absorbed_eps(n=96, t=12, max_rounds=3000, standing=False):
    """eps = 1e-6, cut at max_rounds; nothing converges.
    standing=False: price_war(n, t).  Every bid is the price plus eps alone, so the prices crawl
    up from 0 by 1e-6 a round and stay far below the point (32) where f32 would absorb eps; only
    the nets absorb the prices (value - price == value while price < ulp(value)/2).
    standing=True: task 0 is worth 80 (0.25 away), tasks 1 .. t-1 are worth 40 (1.5 away).  Round
    1 bids 0 + (80 - 40) + eps == 40 in f32 on task 0; from then on task 0 nets 40, ties with
    every other task and wins the tie by index, and every bid is 40 + 0 + eps == 40: the price
    stands, the key's ID half alone decides, and ownership ping-pongs between the two lowest IDs."""
    args, kw = price_war(n, t, eps=1e-6, max_rounds=max_rounds)
    if standing:
        tx = args[4].copy()
        tx[0], tx[1:] = 3.25, 4.5
        args = args[:4] + (tx,) + args[5:]
    return args, kw


def split(case):
    """(args, public keyword arguments) of a family's return value."""
    args, kw = case
    return args, {k: v for k, v in kw.items() if not k.startswith("_")}


def values(oracle, args, claim_thr=20.0, u_scale=100.0, **_):
    """(n, t) f32 values of the admissible pairs (U > claim_thr), 0 elsewhere, and the mask."""
    ids, x, y, caps, tx, ty, treq = args
    n, t = len(ids), len(tx)
    U = oracle.utility(np.repeat(x, t), np.repeat(y, t), np.repeat(np.asarray(caps, np.uint32), t), np.tile(tx, n),
                       np.tile(ty, n), np.tile(treq, n), use_pow=False, u_scale=u_scale).reshape(n, t)
    adm = U > claim_thr
    return np.where(adm, U.astype(np.float32), np.float32(0)), adm


def total_value(V, assigned):
    a = np.nonzero(assigned >= 0)[0]
    return float(V[a, assigned[a]].astype(np.float64).sum())


def brute_force_optimum(V):
    """Best total value over every injective map of the smaller side into the larger (an
    inadmissible pair is worth 0: the same as staying unassigned)."""
    W = V.astype(np.float64)
    if W.shape[0] > W.shape[1]:
        W = W.T
    rows = np.arange(W.shape[0])
    return max(W[rows, list(p)].sum() for p in itertools.permutations(range(W.shape[1]), W.shape[0]))


def check_slackness(V, adm, res, eps, slack=1e-4):
    """eps-complementary slackness of every assigned agent against the full value matrix (the
    slack check_properties uses), and only admissible pairs assigned."""
    price, assigned = res["price"], res["assigned"]
    for a in np.nonzero(assigned >= 0)[0]:
        assert adm[a, assigned[a]]
        net = np.where(adm[a], V[a] - price, -np.inf)
        assert V[a, assigned[a]] - price[assigned[a]] >= max(net.max(), 0.0) - eps - slack


def _check_properties(d, res, eps=0.1, thr=20.0):
    """Matching consistency, prices, and eps-complementary slackness at termination."""
    from oracle import oracle
    owner, price, assigned = res["owner"], res["price"], res["assigned"]
    n, t = len(d["ids"]), len(d["tx"])
    for k in range(t):
        if owner[k] >= 0:
            assert assigned[owner[k]] == k
    for a in range(n):
        if assigned[a] >= 0:
            assert owner[assigned[a]] == a
    assert (price >= 0).all()
    assert ((price > 0) == (owner >= 0)).all()  # a task's price rises exactly when it is taken
    # eps-CS: an assigned agent's net value is within eps of its best alternative (incl. 0)
    rng = np.random.default_rng(0)
    for a in rng.choice(n, size=min(n, 50), replace=False):
        if assigned[a] < 0:
            continue
        U = oracle.utility(np.full(t, d["x"][a]), np.full(t, d["y"][a]), np.full(t, d["caps"][a], np.uint32),
                           d["tx"], d["ty"], d["treq"], use_pow=False)
        adm = U > thr
        net = np.where(adm, U.astype(np.float32) - price, -np.inf)
        mine = np.float32(U[assigned[a]]) - price[assigned[a]]
        assert mine >= max(net.max(), 0.0) - eps - 1e-4
