"""The auction on adversarial instances (tests/auction_cases.py), on every round path.

The auction has no reference counterpart: what it computes is pinned by oracle.auction, bit for
bit.  The uniform inputs of test_auction.py have essentially no exact ties, smoothly falling
bidder counts and lists of a few hundred entries; the families here are what the kernels'
stated invariants are about:

  price_war      one value: every best/second tie by task index, every bid tie by ID, eps-only
                 increments, a standing crowd of n - t bidders for thousands of rounds (batches
                 of 256, the counter ring recycled); n - t = 16 / 17 at the tail's wave / 16-lane
                 group switch and n - t = 2048 at the tail's list capacity
  scarce_agents  t > n: n rounds, one uncontested task a round, eps-only prices
  islands        list lengths at the pass boundaries of group_bid<64,4> and group_bid<16,8>, with
                 equal values (ties across lanes and passes) and with distinct ones; agents
                 with empty lists
  clusters       hundreds of contested rounds over capability-dependent lists; eps 0.1 and 0.01
  lattice        symmetric distances: equal values between distinct positions; and transposed
  wide_reach     claim radius 19 (claim_thr 5, or u_scale 1000 / claim_thr 50): one grid cell,
                 every list 3000 long; and transposed
  no_reach       claim_thr >= u_scale: the radius <= 0 branch, no grid, one round
  absorbed_eps   eps = 1e-6 cut at 3000 rounds; standing=True: bids that equal the price they
                 were made at, ownership decided by the key's ID half alone

CPU tests: oracle.auction against the pure-Python restatement and against the auction's defining
properties (and the optimum), and each family proves from oracle.utility that it is what its name
says.  GPU tests: Swarm.auction / ShardedSwarm.auction bit-exact against oracle.auction.
"""
import functools
import threading

import numpy as np
import pytest

import auction_cases as C
from auction_cases import _check_properties

# ----------------------------------------------------------------------------- the instances
FULL = {
    "price_war_96x12": lambda: C.price_war(96, 12),
    "price_war_28x12": lambda: C.price_war(28, 12),      # 16 standing bidders: a wave per bidder
    "price_war_29x12": lambda: C.price_war(29, 12),      # 17: 16-lane groups
    "price_war_2060x12": lambda: C.price_war(2060, 12),  # 2048: the tail's list capacity
    "price_war_96x12_eps1": lambda: C.price_war(96, 12, eps=1.0),
    "scarce_agents_12x96": lambda: C.scarce_agents(12, 96),
    "islands": lambda: C.islands(),
    "clusters_eps0.1": lambda: C.clusters(eps=0.1),
    "clusters_eps0.01": lambda: C.clusters(eps=0.01),
    "lattice": lambda: C.lattice(),
    "lattice_transposed": lambda: C.lattice(transposed=True),
    "wide_reach_200x3000": lambda: C.wide_reach(200, 3000),
    "wide_reach_3000x200": lambda: C.wide_reach(3000, 200),
    "wide_reach_u_scale1000": lambda: C.wide_reach(200, 3000, claim_thr=50.0, u_scale=1000.0),
    "no_reach_thr_eq_scale": lambda: C.no_reach(100.0),
    "no_reach_thr_gt_scale": lambda: C.no_reach(150.0),
    "absorbed_eps": lambda: C.absorbed_eps(),
    "absorbed_eps_standing": lambda: C.absorbed_eps(standing=True),
}
# sizes at which the Python restatement takes a few seconds at most
SMALL = {
    "price_war": lambda: C.price_war(40, 6, eps=0.5),
    "scarce_agents": lambda: C.scarce_agents(6, 20),
    "islands": lambda: C.islands(lengths=(1, 2, 3, 5)),
    "clusters_eps0.1": lambda: C.clusters(k=3, agents=8, tasks=3),
    "clusters_eps0.01": lambda: C.clusters(k=3, agents=8, tasks=3, eps=0.01),
    "lattice": lambda: C.lattice(side=6),
    "lattice_transposed": lambda: C.lattice(side=6, transposed=True),
    "wide_reach": lambda: C.wide_reach(20, 300),
    "wide_reach_transposed": lambda: C.wide_reach(300, 20),
    "wide_reach_u_scale1000": lambda: C.wide_reach(20, 300, claim_thr=50.0, u_scale=1000.0),
    "no_reach_thr_eq_scale": lambda: C.no_reach(100.0),
    "no_reach_thr_gt_scale": lambda: C.no_reach(150.0),
    "absorbed_eps": lambda: C.absorbed_eps(40, 6, max_rounds=300),
    "absorbed_eps_standing": lambda: C.absorbed_eps(40, 6, max_rounds=300, standing=True),
}
# no more than 8 agents or tasks: the optimum by brute force over the permutations
TINY = {
    "price_war": lambda: C.price_war(8, 5, eps=0.5),
    "scarce_agents": lambda: C.scarce_agents(5, 8),
    "clusters": lambda: C.clusters(k=1, agents=8, tasks=4),
    "wide_reach": lambda: C.wide_reach(7, 8),
    "wide_reach_transposed": lambda: C.wide_reach(8, 7),
    "no_reach": lambda: C.no_reach(100.0, n=6, t=5),
}
NEVER_CONVERGES = ("absorbed_eps", "absorbed_eps_standing")


@functools.lru_cache(maxsize=None)
def _full(name):
    return FULL[name]()


@functools.lru_cache(maxsize=None)
def _want(name, max_rounds=None):
    """oracle.auction of a full-size instance, computed once and shared (never modified)."""
    from oracle import oracle
    args, kw = C.split(_full(name))
    if max_rounds is not None:
        kw["max_rounds"] = max_rounds
    return oracle.auction(*args, **kw)


def _as_dict(args):
    return dict(zip(("ids", "x", "y", "caps", "tx", "ty", "treq"), args))


def _check_all_properties(oracle, args, kw, res):
    """Matching consistency, price > 0 iff owned and eps-complementary slackness (the moved
    _check_properties where its fixed u_scale of 100 applies; every agent against the full value
    matrix, with the same slack, under any u_scale).  Returns the values for the optimum checks."""
    V, adm = C.values(oracle, args, **kw)
    if kw.get("u_scale", 100.0) == 100.0:
        _check_properties(_as_dict(args), res, eps=kw["eps"], thr=kw.get("claim_thr", 20.0))
    else:
        owner, assigned = res["owner"], res["assigned"]
        assert all(assigned[owner[k]] == k for k in np.nonzero(owner >= 0)[0])
        assert all(owner[assigned[a]] == a for a in np.nonzero(assigned >= 0)[0])
        assert ((res["price"] > 0) == (owner >= 0)).all()
    C.check_slackness(V, adm, res, kw["eps"])
    return V


def _assert_near_optimum(V, res, eps, optimum):
    """Bertsekas' bound: an auction that ends in eps-complementary slackness is within eps per
    assigned agent of the optimum (plus _check_properties' 1e-4 of f32 slack per agent)."""
    got = C.total_value(V, res["assigned"])
    assert got <= optimum + 1e-6
    assert optimum - got <= int((res["assigned"] >= 0).sum()) * (eps + 1e-4), (optimum, got)


# ----------------------------------------------------------------------------- CPU: the oracle itself
@pytest.mark.parametrize("name", sorted(SMALL))
def test_oracle_c_matches_python_restatement(oracle_mod, name):
    args, kw = C.split(SMALL[name]())
    a = oracle_mod.auction(*args, **kw)
    b = oracle_mod.auction_py(*args, **kw)
    for k in ("owner", "price", "assigned", "bidders"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    if name in NEVER_CONVERGES:
        # cut at max_rounds: the C oracle reports -1, the restatement the rounds it ran
        assert a["rounds"] == -1 and b["rounds"] == kw["max_rounds"] == len(a["bidders"])
        # No property or value check: both describe the END of an auction.  Cut mid-way, agents
        # that were just outbid hold nothing, and (standing) the price of 40 on task 0 leaves
        # every bidder indifferent for ever; there is no terminal state to be near-optimal.
        return
    assert a["rounds"] == b["rounds"] == len(a["bidders"]) >= 1
    _check_all_properties(oracle_mod, args, kw, a)


@pytest.mark.parametrize("name", sorted(TINY))
def test_oracle_value_against_brute_force(oracle_mod, name):
    args, kw = C.split(TINY[name]())
    assert min(len(args[0]), len(args[4])) <= 8
    r = oracle_mod.auction(*args, **kw)
    V = _check_all_properties(oracle_mod, args, kw, r)
    _assert_near_optimum(V, r, kw["eps"], C.brute_force_optimum(V))


@pytest.mark.parametrize("name", [k for k in sorted(FULL) if k not in NEVER_CONVERGES])
def test_oracle_value_against_linear_sum_assignment(oracle_mod, name):
    """Full size.  clusters, lattice and islands are the ones whose optimum is not obvious; the
    others come along at no cost (price_war: any min(n, t) pairs; no_reach: 0)."""
    opt = pytest.importorskip("scipy.optimize")
    args, kw = C.split(_full(name))
    r = _want(name)
    assert r["rounds"] >= 1
    V = _check_all_properties(oracle_mod, args, kw, r)
    rows, cols = opt.linear_sum_assignment(V.astype(np.float64), maximize=True)
    _assert_near_optimum(V, r, kw["eps"], float(V.astype(np.float64)[rows, cols].sum()))


# ----------------------------------------------------------------------------- CPU: each family is what it says
def _best_second(V, adm):
    """Per agent: admissible count, best value, second-best value (-inf if none) at price 0."""
    W = np.where(adm, V, -np.inf)
    s = np.sort(W, axis=1)
    return adm.sum(1), s[:, -1], (s[:, -2] if W.shape[1] > 1 else np.full(len(W), -np.inf))


@pytest.mark.parametrize("name", ["price_war_96x12", "price_war_28x12", "price_war_29x12", "price_war_2060x12",
                                  "price_war_96x12_eps1", "scarce_agents_12x96"])
def test_family_price_war_has_one_value(oracle_mod, name):
    args, kw = C.split(_full(name))
    V, adm = C.values(oracle_mod, args, **kw)
    n, t = V.shape
    assert adm.all() and len(np.unique(V.view(np.uint32))) == 1
    ids = args[0]
    assert len(set(ids.tolist())) == n and not np.array_equal(ids, np.sort(ids))  # a permutation, not arange
    r = _want(name)
    eps = np.float32(kw["eps"])
    if n > t:  # rounds 1 .. t take the tasks in index order, then n - t agents bid every round
        np.testing.assert_array_equal(r["bidders"][:t], n - np.arange(t))
        assert (r["bidders"][t:] == n - t).all() and r["rounds"] > 50 * t
        assert (np.abs(r["price"] - V[0, 0]) <= 2 * eps).all()  # every task bid up to the value: all drop out
    else:      # one task a round, lowest free index, lowest ID first; never contested again
        np.testing.assert_array_equal(r["bidders"], n - np.arange(n))
        np.testing.assert_array_equal(r["price"], np.where(np.arange(t) < n, eps, np.float32(0)))
        np.testing.assert_array_equal(ids[r["owner"][:n]][0], ids.min())


def test_family_price_war_standing_bidders_sit_on_the_tail_boundaries():
    """16 / 17 standing bidders: k_auc_tail's wave-per-bidder / 16-lane-group switch (16 waves);
    2048: its list capacity."""
    for name, standing in (("price_war_28x12", 16), ("price_war_29x12", 17), ("price_war_2060x12", 2048)):
        assert _want(name)["bidders"][-1] == standing == _want(name)["bidders"][12]


def test_family_islands_list_lengths_and_ties(oracle_mod):
    args, kw = _full("islands")
    meta = kw["_meta"]
    V, adm = C.values(oracle_mod, args)
    cnt, best, second = _best_second(V, adm)
    np.testing.assert_array_equal(cnt, meta["want"])
    assert set(meta["want"].tolist()) == set(C.ISLAND_LENGTHS) | {0}
    for L in C.ISLAND_LENGTHS:  # every length in both forms, three agents each
        assert ((meta["want"] == L) & meta["colocated"]).sum() == 3 == ((meta["want"] == L) & ~meta["colocated"]).sum()
    many = meta["want"] >= 2
    assert (best[many & meta["colocated"]] == second[many & meta["colocated"]]).all()
    assert (best[many & ~meta["colocated"]] > second[many & ~meta["colocated"]]).all()
    for a in np.nonzero(many & meta["colocated"])[0]:   # one value over the whole list ...
        assert len(np.unique(V[a][adm[a]])) == 1
    for a in np.nonzero(many & ~meta["colocated"])[0]:  # ... or no two equal
        assert len(np.unique(V[a][adm[a]])) == cnt[a]
    # an island's tasks are not contiguous in task index (the shuffle): ties by index cross the list
    a = np.nonzero(meta["colocated"] & (meta["want"] == 1025))[0][0]
    k = np.nonzero(adm[a])[0]
    assert k.max() - k.min() > 2 * 1025


def test_family_lattice_ties(oracle_mod):
    """Transposed: every agent sits in the middle of four tasks, a four-way tie for the best.
    As stated: the best (0.25, 0.25 away) is unique, the second best ties two-way between
    (0.25, 0.75) and (0.75, 0.25) for every agent off the border."""
    args, kw = C.split(_full("lattice_transposed"))
    V, adm = C.values(oracle_mod, args)
    _, best, _ = _best_second(V, adm)
    assert V.shape == (100, 400) and ((V == best[:, None]).sum(1) == 4).all()
    args, kw = C.split(_full("lattice"))
    V, adm = C.values(oracle_mod, args)
    _, best, second = _best_second(V, adm)
    assert V.shape == (400, 100) and (best > second).all()
    # 18 x 18 agents have a task 0.75 away on both axes; the 4 corners have none on either and tie
    # between (0.25, 1.25) and (1.25, 0.25); the other border agents have one second best
    assert ((V == second[:, None]).sum(1) >= 2).sum() == 18 * 18 + 4
    assert _want("lattice")["rounds"] > 1                     # contested: the tied seconds become bests


def test_family_clusters_is_mixed_and_long(oracle_mod):
    args, kw = C.split(_full("clusters_eps0.1"))
    assert set(args[6].tolist()) == {-1, 0, 1, 2, 3} and len(set(args[3].tolist())) > 8
    V, adm = C.values(oracle_mod, args)
    assert 0 < adm.sum() < adm.size // 4 and len(set(adm.sum(1).tolist())) > 3  # uneven lists
    # both reach the first 256-round batch (rounds 249-504), eps 0.01 past the cut in its middle
    assert _want("clusters_eps0.1")["rounds"] > 249 and _want("clusters_eps0.01")["rounds"] > 377


@pytest.mark.parametrize("name", ["wide_reach_200x3000", "wide_reach_3000x200", "wide_reach_u_scale1000"])
def test_family_wide_reach_lists_hold_every_task(oracle_mod, name):
    args, kw = C.split(_full(name))
    assert kw["u_scale"] / kw["claim_thr"] - 1.0 == 19.0
    assert _want(name)["n_pairs"] == 600000 == len(args[0]) * len(args[4])


@pytest.mark.parametrize("name", ["no_reach_thr_eq_scale", "no_reach_thr_gt_scale"])
def test_family_no_reach_has_no_pair(oracle_mod, name):
    args, kw = C.split(_full(name))
    assert kw["u_scale"] / kw["claim_thr"] - 1.0 <= 0.0
    r = _want(name)
    assert r["n_pairs"] == 0 and r["rounds"] == 1 and r["bidders"].tolist() == [len(args[0])]
    assert (r["assigned"] == -1).all() and (r["owner"] == -1).all() and (r["price"] == 0).all()


def test_family_absorbed_eps(oracle_mod):
    """standing: the final price absorbs eps (price + eps == price in f32), the owner changes
    every round at that price, the two lowest IDs alternate.  As stated in price_war form, eps is
    never absorbed by a price within 3000 rounds -- the prices only reach 3000 eps / t -- so that
    form is pinned as what it is: an eps-only crawl that the cut ends."""
    eps = np.float32(1e-6)
    args, kw = C.split(_full("absorbed_eps_standing"))
    r = _want("absorbed_eps_standing")
    assert r["rounds"] == -1 and len(r["bidders"]) == kw["max_rounds"] == 3000
    p = r["price"][r["price"] > 0]
    assert len(p) == 1 and r["price"][0] == np.float32(40.0)
    assert (np.float32(p) + eps == np.float32(p)).all()
    assert (r["bidders"][1:] == len(args[0]) - 1).all()
    lowest = np.sort(args[0])[:2]
    owners = [int(args[0][_want("absorbed_eps_standing", m)["owner"][0]]) for m in (2997, 2998, 2999)] + \
        [int(args[0][r["owner"][0]])]
    assert owners == [int(lowest[1 - m % 2]) for m in (2997, 2998, 2999, 3000)]  # odd rounds: the lowest ID
    for m in (2998, 2999):
        np.testing.assert_array_equal(_want("absorbed_eps_standing", m)["price"], r["price"])
    args, kw = C.split(_full("absorbed_eps"))
    r = _want("absorbed_eps")
    assert r["rounds"] == -1 and (np.diff(r["bidders"]) <= 0).all() and r["bidders"][-1] == len(args[0]) - 12
    assert (r["price"] > 0).all() and r["price"].max() <= 3000 * eps
    v = np.float32(C.values(oracle_mod, args)[0][0, 0])
    assert v - eps == v  # the nets absorb a price of eps: the early rounds all tie at the full value


# ----------------------------------------------------------------------------- GPU
PATHS = {  # (SWARM_AUCTION_FUSED, SWARM_AUCTION_TAIL); None: unset, the defaults (8192, 32)
    "list": ("0", "0"),
    "fused": ("1000000000", "0"),
    "tail2048": ("0", "2048"),
    "fused_tail32": ("1000000000", "32"),
    "default": (None, None),
}


def _set_path(monkeypatch, fused, tail):
    for k, v in (("SWARM_AUCTION_FUSED", fused), ("SWARM_AUCTION_TAIL", tail)):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)


def _expected_tail_rounds(bidders, n, tail, rounds_run):
    """Rounds the one-workgroup tail runs under the host's schedule: batches of 8, 16, ... 256
    rounds, the bidder count read back after each, the tail taking over once the last count read
    (n before round 1) is <= the threshold."""
    tail = 32 if tail is None else min(int(tail), 2048)
    r, batch, last = 1, 8, n
    while r <= rounds_run:
        if last <= tail:
            return rounds_run - r + 1
        rend = r + batch - 1
        if rend > rounds_run:
            return 0  # converged (or cut) inside a multi-workgroup batch
        last = int(bidders[rend - 1])
        r, batch = rend + 1, min(2 * batch, 256)
    return 0


def _assert_exact(s, r, want, kw, tail):
    """Swarm.auction's result r against oracle.auction's, bit for bit."""
    converged = want["rounds"] >= 0
    rounds = want["rounds"] if converged else kw["max_rounds"]
    assert r.converged == converged and r.rounds_exec == rounds == len(want["bidders"])
    np.testing.assert_array_equal(r.bidders, want["bidders"])
    np.testing.assert_array_equal(r.price.cpu().numpy().view(np.uint32), want["price"].view(np.uint32))
    perm = s.perm.cpu().numpy()
    own = r.owner.cpu().numpy()
    np.testing.assert_array_equal(np.where(own >= 0, perm[np.maximum(own, 0)], -1), want["owner"])
    np.testing.assert_array_equal(s.to_input_order(r.assigned), want["assigned"])
    assert r.stats["n_pairs"] == want["n_pairs"] and r.stats["bids_total"] == int(want["bidders"].sum())
    assert r.stats["tail_rounds"] == _expected_tail_rounds(want["bidders"], s.n, tail, rounds)


def _swarm(args):
    from swarm_amd.swarm import Swarm
    return Swarm(*args[:4], device="cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", list(FULL))
def test_gpu_auction_edges_match_oracle(oracle_mod, monkeypatch, name, path):
    fused, tail = PATHS[path]
    _set_path(monkeypatch, fused, tail)
    args, kw = C.split(_full(name))
    want = _want(name)
    s = _swarm(args)
    r = s.auction(*args[4:], **kw)
    _assert_exact(s, r, want, kw, tail)
    if tail == "0":
        assert r.stats["tail_rounds"] == 0
    elif tail == "2048":
        assert r.stats["tail_rounds"] > 0  # from round 1, or (n > 2048) once 2048 or fewer bid
    elif name in ("price_war_28x12", "price_war_29x12", "islands", "clusters_eps0.1", "wide_reach_3000x200"):
        assert r.stats["tail_rounds"] > 0  # threshold 32: these end in a long tail of few bidders
    if name == "price_war_96x12" and path == "fused":
        # fused rounds from round 9 on, batches of up to 256 rounds: the 512-slot counter ring is
        # recycled 14 times; every round's count is in the comparison above
        assert r.rounds_exec > 7000 and r.stats["rounds_launched"] > 13 * 512


@pytest.mark.gpu
@pytest.mark.parametrize("fused,tail,first_tail_round", [("0", "90", 9), ("1000000000", "90", 9),
                                                         ("1000000000", "88", 25), ("0", "88", 25)])
def test_gpu_auction_hand_over_mid_decline(oracle_mod, monkeypatch, fused, tail, first_tail_round):
    """price_war (96, 12): the bidders decline 96, 95, ... 84.  Threshold 90: the first batch (rounds
    1-8, list-driven under either setting) ends at 89, the tail starts at round 9 after
    k_auc_clear_keys.  Threshold 88: the second batch (rounds 9-24) ends at 84 and hands over at
    round 25 -- after fused rounds through fused_flush (a resolve-only round, every key buffer
    zeroed), after list rounds through k_auc_clear_keys."""
    _set_path(monkeypatch, fused, tail)
    args, kw = C.split(_full("price_war_96x12"))
    want = _want("price_war_96x12")
    s = _swarm(args)
    r = s.auction(*args[4:], **kw)
    _assert_exact(s, r, want, kw, tail)
    assert r.stats["tail_rounds"] == want["rounds"] - first_tail_round + 1


def _cuts(rounds):
    """The batch boundaries 8, 8+16, 8+16+32 and the round after each; the middle of the first
    256-round batch (rounds 249-504) or of a later one; the last round but one."""
    mid = 633 if rounds > 761 else 377
    assert 57 < mid < rounds - 1
    return (1, 2, 8, 9, 24, 25, 56, 57, mid, rounds - 1)


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", ["price_war_96x12", "clusters_eps0.01"])
def test_gpu_auction_cut_at_max_rounds(oracle_mod, monkeypatch, name, path):
    """max_rounds = m: the oracle's state after exactly m rounds, not converged."""
    fused, tail = PATHS[path]
    _set_path(monkeypatch, fused, tail)
    args, kw = C.split(_full(name))
    full = _want(name)
    s = _swarm(args)
    for m in _cuts(full["rounds"]):
        want = _want(name, m)
        assert want["rounds"] == -1
        np.testing.assert_array_equal(want["bidders"], full["bidders"][:m])
        kwm = dict(kw, max_rounds=m)
        r = s.auction(*args[4:], **kwm)
        assert not r.converged and r.rounds_exec == m, m
        _assert_exact(s, r, want, kwm, tail)


def _sharded(args, kw, parts, check_every=32):
    """ShardedSwarm.auction of the agent subsets `parts` (index arrays), one thread per shard on
    one GPU, tasks replicated; returns each shard's result and its agents' IDs."""
    import torch
    from shard_doubles import ThreadHalo
    from swarm_amd.dist import ShardedSwarm
    ids, x, y, caps = args[:4]
    world = len(parts)
    hub = ThreadHalo(world)
    outs, errs = {}, []

    def run(rank):
        try:
            torch.cuda.set_device(0)
            p = parts[rank]
            # one strip far taller than the swarm: no ghosts (the auction exchanges keys, not agents)
            sh = ShardedSwarm(ids[p], x[p], y[p], caps[p], (-1e6, 1e6), device="cuda:0", halo=hub.member(rank))
            r = sh.auction(*args[4:], check_every=check_every, **kw)
            torch.cuda.synchronize()
            outs[rank] = dict(r=r, ids=sh.ids.cpu().numpy(), owner=r.owner_id.cpu().numpy(),
                              price=r.price.cpu().numpy(), assigned=r.assigned.cpu().numpy())
        except Exception as e:  # surfaced below
            errs.append(e)
            hub.barrier.abort()

    th = [threading.Thread(target=run, args=(k,)) for k in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    assert not errs, errs
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["price_war_96x12", "clusters_eps0.1"])
def test_gpu_sharded_auction_edges_two_shards_on_one_gpu(oracle_mod, name):
    """The all-agents rounds of swarm_auction_begin / _bid / _resolve: agents split by ID parity, so
    every contested task has bidders on both shards and every ID tie is settled by the MAX
    reduce; against oracle.auction over the union."""
    args, kw = C.split(_full(name))
    ids = args[0]
    parts = [np.nonzero(ids % 2 == k)[0] for k in (0, 1)]
    assert all(len(p) > len(ids) // 4 for p in parts)
    want = _want(name)
    assert want["rounds"] > 200
    outs = _sharded(args, kw, parts)
    owner_id = np.where(want["owner"] >= 0, ids[np.maximum(want["owner"], 0)], -1)
    by_id = dict(zip(ids.tolist(), want["assigned"].tolist()))
    for k in (0, 1):
        o = outs[k]
        assert o["r"].converged and o["r"].rounds_exec == want["rounds"]
        np.testing.assert_array_equal(o["r"].bidders, want["bidders"])
        np.testing.assert_array_equal(o["owner"], owner_id)
        np.testing.assert_array_equal(o["price"].view(np.uint32), want["price"].view(np.uint32))
        assert sorted(o["ids"].tolist()) == sorted(ids[parts[k]].tolist())
        assert all(by_id[int(i)] == int(a) for i, a in zip(o["ids"], o["assigned"]))


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [dict(eps=0.0), dict(eps=-0.1), dict(eps=float("nan")), dict(eps=float("inf")),
                                 dict(claim_thr=0.0), dict(claim_thr=-20.0), dict(u_scale=0.0),
                                 dict(u_scale=-100.0), dict(max_rounds=0)],
                         ids=lambda b: "_".join(f"{k}={v}" for k, v in b.items()))
def test_gpu_auction_argument_checks(oracle_mod, bad):
    """SWARM_ERR_ARG, and a following valid call on the same context is exact."""
    from swarm_amd import _lib
    args, kw = C.split(_full("clusters_eps0.1"))
    s = _swarm(args)
    with pytest.raises(_lib.SwarmError) as e:
        s.auction(*args[4:], **dict(kw, **bad))
    assert e.value.code == _lib.ERR_ARG
    _assert_exact(s, s.auction(*args[4:], **kw), _want("clusters_eps0.1"), kw, None)
