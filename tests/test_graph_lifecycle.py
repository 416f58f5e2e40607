"""A Swarm that outlives its neighbour graph: elections after the graph (or the IDs) were replaced.

Between elections the Swarm keeps structures derived from the graph -- the 16-bit columns (graph_compact),
the int64 copy of row_ptr (elect(wide=True)) -- and from the IDs (id_index).  Each must be rebuilt when the
tensor it was derived from is replaced, also when the replacement lies at the SAME address with the SAME
version counter (the caching allocator hands a freed block to the next tensor of that size, and a new
tensor starts at version 0): an election on the old neighbour lists raises nothing and names wrong leaders.

Every election here is compared with the oracle on the graph the Swarm holds at that moment (reference
semantics agent.py:263-275): leaders, states, rounds_exec and every per-round change count, bit for bit.

The graph pairs are built so that stale state can only give wrong answers, never an index outside the arrays:
  P1  circulants i +- {1, 3} (A), i +- {1, 2} (B), i +- {2, 4} (C): row_ptr = 4 i for all three, so a stale
      column buffer decodes, in every row, neighbours of that same row of another circulant (all in [0, n));
      every 16-bit delta lies in [-4032, 4095].  C splits into the even and the odd agents, A is connected.
  P2  two separate band graphs over the first and the second half of the agents, half-widths (1, 3) for A and
      (3, 1) for C: the same edge count, other offsets.  A stale offset array is A's: every offset <= E, so
      every int32 column read is a valid agent.  (New 16-bit columns decoded at old offsets could leave
      [0, n): the int32-column elections are asserted first.)
"""
import gc
import weakref

import numpy as np
import pytest

N = 4096
VARIANTS = [(mode, compact) for mode in ("frontier", "dense") for compact in (True, False)]


def circulant(n, offs):
    """i +- offs (mod n), rows ascending: (row_ptr, col), row_ptr = 2 len(offs) i."""
    d = np.array([s * o for o in offs for s in (1, -1)], np.int64)
    col = np.sort((np.arange(n, dtype=np.int64)[:, None] + d) % n, axis=1)
    assert (np.diff(col, axis=1) > 0).all()  # 2 len(offs) distinct neighbours in every row
    return np.arange(n + 1, dtype=np.int64) * len(d), col.reshape(-1).astype(np.int32)


def band_halves(n, w_first, w_second):
    """Agents [0, n/2) and [n/2, n) as two separate band graphs (i hears j of its half with 0 < |i - j| <= w),
    rows ascending."""
    h = n // 2
    rows = []
    for lo, hi, w in ((0, h, w_first), (h, n, w_second)):
        i = np.arange(lo, hi, dtype=np.int64)[:, None]
        j = i + np.array([d for d in range(-w, w + 1) if d], np.int64)
        rows += [r[(r >= lo) & (r < hi)] for r in j]
    rp = np.zeros(n + 1, np.int64)
    rp[1:] = np.cumsum([len(r) for r in rows])
    return rp, np.concatenate(rows).astype(np.int32)


def drop_one_direction(rp, col, share, seed):
    """The graph without the entry `j in row i` of a seeded share of the edges i < j (row j keeps i)."""
    n = len(rp) - 1
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    keep = ~((src < col) & (np.random.default_rng(seed).random(len(col)) < share))
    out = np.zeros(n + 1, np.int64)
    out[1:] = np.cumsum(np.bincount(src[keep], minlength=n))
    return out, col[keep]


def in_range(rp, col, n):
    return rp[0] == 0 and rp[-1] == len(col) and (np.diff(rp) >= 0).all() and col.min() >= 0 and col.max() < n


@pytest.fixture(scope="module")
def cases(oracle_mod):
    """IDs, the graphs and the oracle's election on each, computed once (read-only)."""
    ids = np.random.default_rng(4096).permutation(4 * N)[:N].astype(np.int32)
    graphs = {"A": circulant(N, (1, 3)), "B": circulant(N, (1, 2)), "C": circulant(N, (2, 4)),
              "A2": band_halves(N, 1, 3), "C2": band_halves(N, 3, 1)}
    graphs["D"] = drop_one_direction(*graphs["A"], 0.25, 7)
    want = {}
    for k, (rp, col) in graphs.items():
        assert in_range(rp, col, N), k
        want[k] = oracle_mod.elect(rp, col, ids)
        # the frontier restatement agrees (hear = the transpose; the symmetric graphs are their own)
        fr = oracle_mod.elect_frontier(rp, col, ids, hear=oracle_mod.transpose_csr(rp, col) if k == "D" else None)
        assert fr[2] == want[k][2] > 1, k
        for a, b in zip(fr[:2] + fr[3:], want[k][:2] + want[k][3:]):
            np.testing.assert_array_equal(a, b)
    for arrs in list(graphs.values()) + list(want.values()) + [(ids,)]:
        for a in arrs:
            if isinstance(a, np.ndarray):
                a.flags.writeable = False
    return {"ids": ids, "graphs": graphs, "want": want}


def assert_p1(cases):
    """P1's precondition: same offsets, same edge count, other columns, deltas that fit 16 bits, and elections
    that differ in the leaders and in the per-round changes."""
    g, w = cases["graphs"], cases["want"]
    for k in "ABC":
        np.testing.assert_array_equal(g[k][0], 4 * np.arange(N + 1))
        delta = g[k][1].astype(np.int64) - (np.repeat(np.arange(N), 4) & ~63)
        assert -4032 <= delta.min() and delta.max() <= 4095
    assert not np.array_equal(g["A"][1], g["C"][1]) and not np.array_equal(g["B"][1], g["C"][1])
    for k in "AB":
        assert (w[k][0] != w["C"][0]).sum() > N // 8, k
        assert not np.array_equal(w[k][3], w["C"][3]), k


def assert_p2(cases):
    """P2's precondition: same edge count, other offsets, elections that differ in rounds_exec and in the
    per-round changes -- and A's offsets over C's columns stay inside the arrays."""
    (rpa, cola), (rpc, colc) = cases["graphs"]["A2"], cases["graphs"]["C2"]
    wa, wc = cases["want"]["A2"], cases["want"]["C2"]
    assert len(cola) == len(colc) == 16370 and not np.array_equal(rpa, rpc)
    assert in_range(rpa, colc, N)
    assert wa[2] != wc[2] and not np.array_equal(wa[3], wc[3])


def check(r, want, what):
    lead, state, rounds, changes = want
    assert r.converged and r.rounds_exec == rounds, (what, r.rounds_exec, rounds)
    np.testing.assert_array_equal(r.changes, changes, err_msg=str(what))
    np.testing.assert_array_equal(r.leader.cpu().numpy(), lead, err_msg=str(what))
    np.testing.assert_array_equal(r.state.cpu().numpy(), state, err_msg=str(what))


@pytest.fixture(scope="module")
def sw():
    import swarm_amd.swarm as swm
    from swarm_amd import _lib
    _lib.load()
    return swm


def new_swarm(sw, cases):
    return sw.Swarm(cases["ids"], np.arange(float(N)), np.zeros(N), layout="input", device="cuda")


def put_at_same_address(s, rp, col):
    """Another graph's contents in the memory of s.row_ptr / s.col, under NEW tensor objects whose version
    counters equal the old ones: what the caching allocator does when it hands a freed graph's blocks to the
    next one, made certain.  (A write through a .data alias leaves the tensor's own counter alone, and a .data
    alias is a new object with a counter of its own, starting at 0.)"""
    import torch
    for name, new in (("row_ptr", rp), ("col", col)):
        old = getattr(s, name)
        assert old.numel() == len(new)
        ver = old._version
        old.data.copy_(torch.as_tensor(np.array(new, np.int32), device=old.device))
        alias = old.data
        assert alias is not old and alias.data_ptr() == old.data_ptr() and alias._version == old._version == ver
        setattr(s, name, alias)
    s._hear = None
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_columns_replaced_at_the_same_address(cases, sw):
    """Test 1: graph C in graph A's memory (same addresses, versions, n, edge count, offsets) after A's
    elections filled every cache: every variant must elect on C's columns."""
    assert_p1(cases)
    s = new_swarm(sw, cases).set_graph(*cases["graphs"]["A"])
    for mode, compact in VARIANTS:
        r = s.elect(mode=mode, compact=compact)
        assert r.compact == compact
        check(r, cases["want"]["A"], ("A", mode, compact))
    c_before = s.graph_compact()
    assert c_before is not None
    put_at_same_address(s, *cases["graphs"]["C"])
    for mode, compact in VARIANTS:
        r = s.elect(mode=mode, compact=compact)
        assert r.compact == compact
        check(r, cases["want"]["C"], ("C", mode, compact))
    assert s.graph_compact() is not None and s.graph_compact() is not c_before


@pytest.mark.gpu
def test_offsets_replaced_at_the_same_address(cases, sw):
    """Test 2: the same for the int64 copy of row_ptr (elect(wide=True)); P2's C in A's memory.  The int32
    columns first: with stale offsets they read valid agents, the 16-bit ones might not."""
    assert_p2(cases)
    s = new_swarm(sw, cases).set_graph(*cases["graphs"]["A2"])
    for mode, compact in (("frontier", False), ("dense", False), ("frontier", True)):  # fills both caches
        check(s.elect(mode=mode, compact=compact, wide=True), cases["want"]["A2"], ("A2", mode, compact))
    rp64_before = s._rp64
    assert s.graph_compact() is not None
    put_at_same_address(s, *cases["graphs"]["C2"])
    for mode in ("frontier", "dense"):
        r = s.elect(mode=mode, compact=False, wide=True)
        assert r.wide and not r.compact
        check(r, cases["want"]["C2"], ("C2", mode, False))
    assert s._rp64 is not rp64_before
    np.testing.assert_array_equal(s._rp64[1].cpu().numpy(), cases["graphs"]["C2"][0])
    # only now the 16-bit columns at those offsets
    for mode in ("frontier", "dense"):
        r = s.elect(mode=mode, wide=True)
        assert r.wide and r.compact == (mode == "frontier")
        check(r, cases["want"]["C2"], ("C2", mode, True))


@pytest.mark.gpu
def test_graph_replaced_twice_between_elections(cases, sw):
    """Test 3: the allocator's route as a caller meets it -- A elected, B set and never elected, C set: C's
    tensors may get A's freed blocks back.  Skips (after its asserts) when they did not: the run then says
    nothing about reuse, which test_columns_replaced_at_the_same_address makes certain."""
    assert_p1(cases)
    s = new_swarm(sw, cases).set_graph(*cases["graphs"]["A"])
    ptr_a = (s.row_ptr.data_ptr(), s.col.data_ptr())
    for mode, compact in VARIANTS:
        check(s.elect(mode=mode, compact=compact), cases["want"]["A"], ("A", mode, compact))
    s.set_graph(*cases["graphs"]["B"])
    s.set_graph(*cases["graphs"]["C"])
    ptr_c = (s.row_ptr.data_ptr(), s.col.data_ptr())
    for mode, compact in VARIANTS:
        check(s.elect(mode=mode, compact=compact), cases["want"]["C"], ("C", mode, compact))
    if ptr_c != ptr_a:
        pytest.skip(f"the allocator did not hand A's blocks to C: (row_ptr, col) at {ptr_a} then {ptr_c}")


@pytest.mark.gpu
def test_symmetric_directed_symmetric(cases, sw):
    """Test 4: a directed graph of another edge count between two symmetric ones: the 16-bit columns are set
    aside for it and rebuilt after it."""
    assert_p1(cases)
    g, w = cases["graphs"], cases["want"]
    # (D stays connected, so its leaders are A's: its rounds and per-round changes tell them apart)
    assert len(g["D"][1]) < len(g["A"][1]) and w["D"][2] not in (w["A"][2], w["C"][2])
    assert not np.array_equal(w["D"][3][:8], w["A"][3][:8]) and not np.array_equal(w["D"][3][:8], w["C"][3][:8])
    s = new_swarm(sw, cases)
    for k, compact in (("A", True), ("D", False), ("C", True)):
        s.set_graph(*g[k])
        assert (s._hear is not None) == (k == "D")
        for mode in ("frontier", "dense"):
            r = s.elect(mode=mode)
            assert r.compact == compact, (k, mode)
            check(r, w[k], (k, mode))


@pytest.mark.gpu
def test_caches_still_cache(cases, sw):
    """Test 5: elections on an unchanged graph keep the 16-bit columns and the int64 offsets they have."""
    s = new_swarm(sw, cases).set_graph(*cases["graphs"]["A"])
    check(s.elect(), cases["want"]["A"], "first")
    c16 = s.graph_compact()
    check(s.elect(wide=True), cases["want"]["A"], "wide")
    rp64 = s._rp64
    assert c16 is not None and rp64 is not None
    check(s.elect(), cases["want"]["A"], "again")
    check(s.elect(wide=True), cases["want"]["A"], "wide again")
    assert s.graph_compact() is c16 and s._rp64 is rp64 and s._rp64[1] is rp64[1]


@pytest.mark.gpu
def test_replaced_graph_is_not_kept_alive(cases, sw):
    """Test 6: the caches must not pin the graph they were built from (at C5 scale col alone is 6.4 GB)."""
    s = new_swarm(sw, cases).set_graph(*cases["graphs"]["A"])
    for mode, compact in VARIANTS:
        check(s.elect(mode=mode, compact=compact), cases["want"]["A"], ("A", mode, compact))
    check(s.elect(wide=True), cases["want"]["A"], "wide")
    refs = (weakref.ref(s.row_ptr), weakref.ref(s.col))
    s.set_graph(*cases["graphs"]["B"])
    gc.collect()
    assert refs[0]() is None and refs[1]() is None
    check(s.elect(), cases["want"]["B"], "B")


@pytest.mark.gpu
def test_ids_replaced(cases, sw):
    """Test 7: id_index() after self.ids was replaced by a tensor of the same IDs in another order, at the
    same version: leader_index() must look the IDs up in the new order.  (Every agent is a FOLLOWER before an
    election, so every row is looked up.)"""
    import torch
    ids = cases["ids"]
    rng = np.random.default_rng(77)
    leader = rng.choice(ids, N).astype(np.int32)
    absent = np.setdiff1d(np.arange(4 * N), ids)
    leader[:5] = [absent[0], absent[-1], 4 * N + 2000, -1, ids.max()]

    def lookup(order):
        table = {int(v): i for i, v in enumerate(order)}
        return np.array([table.get(int(v), -1) for v in leader], np.int32)

    ids2 = ids[rng.permutation(N)]
    assert (lookup(ids) != lookup(ids2)).sum() > N // 2
    s = new_swarm(sw, cases)
    lead_t = torch.as_tensor(leader, device="cuda")
    np.testing.assert_array_equal(s.leader_index(lead_t).cpu().numpy(), lookup(ids))
    table = s.id_index()
    assert table is not None and s.id_index() is table  # built once for unchanged IDs
    old = s.ids
    s.ids = torch.as_tensor(ids2, device="cuda")
    assert s.ids is not old and s.ids._version == old._version
    np.testing.assert_array_equal(s.leader_index(lead_t).cpu().numpy(), lookup(ids2))
    assert s.id_index() is not table
    # ... and after a write in place
    s.ids.copy_(torch.as_tensor(ids.copy(), device="cuda"))
    np.testing.assert_array_equal(s.leader_index(lead_t).cpu().numpy(), lookup(ids))


def test_same_tensor_helper():
    """The caches' key comparison (swarm._same_tensor over swarm._tensor_rec), on CPU tensors."""
    import torch
    from swarm_amd.swarm import _same_tensor, _tensor_rec
    t = torch.arange(8, dtype=torch.int32)
    rec = _tensor_rec(t)
    assert _same_tensor(rec, t)
    assert not _same_tensor(None, t) and not _same_tensor(rec, None)
    # another object over the same memory at the same version
    alias = t.data
    assert alias is not t and alias.data_ptr() == t.data_ptr() and alias._version == t._version
    assert not _same_tensor(rec, alias)
    # a write through the alias leaves t's counter alone (what the GPU tests rely on)
    alias.add_(1)
    assert _same_tensor(rec, t) and int(t[0]) == 1
    # an in-place write
    t.add_(1)
    assert not _same_tensor(rec, t)
    assert _same_tensor(_tensor_rec(t), t)
    # the recorded tensor is gone: a dead record matches nothing, whatever lies at its address now
    rec = _tensor_rec(t)
    ptr = t.data_ptr()
    del t, alias
    gc.collect()
    assert rec[0]() is None
    for _ in range(4):
        u = torch.arange(8, dtype=torch.int32)
        assert not _same_tensor(rec, u), u.data_ptr() == ptr
