"""swarm_build_rgg against a brute-force reference at the edges of its input domain.

Every other GPU test takes its graph from build_graph(1.0) over uniform positions in [0, side) and checks
the kernel downstream against the oracle run over the GPU's own graph: a wrong graph is invisible to
them, and the two references the builder itself is compared with (oracle.rgg_csr, gen.rgg_csr) are cell
lists of the kernel's own design.  Here the reference is tests/rgg_brute.py -- all pairs, no cells -- over
rgg_brute.CASES: radii from 1e-3 to 1e3, negative and far-away coordinates, pairs at exactly the radius,
one-row grids, co-located agents, cells grown by the cell cap, and rows that need sorting on both sides of
the in-kernel / hipCUB switch (graph.hip, `max_win <= kInKernelSort`; tests/test_rgg_brute.py checks on the
CPU that the inputs sit on the side they claim, since no output shows which path ran).  Then the spatial
layout over three of the cases, the C ABI's two-pass contract, and the refusals: a position that is not
finite, and finite positions whose extent is not (they made the parent's grid shaping loop for ever;
tests/test_grid_shape.py proves on the CPU that it ends now).  No reference counterpart (agent.py has no
graph: its transport is a stub, agent.py:191-194).
"""
import ctypes
import time

import numpy as np
import pytest

import rgg_brute as rb

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sw():
    import swarm_amd.swarm as swm
    from swarm_amd import _lib
    _lib.load()
    return swm


@pytest.fixture(scope="module")
def brute():
    memo = {}

    def get(name):
        if name not in memo:
            c = rb.BY_NAME[name]
            rp, col = rb.rgg_brute(c.x, c.y, c.r)
            rp.setflags(write=False)
            col.setflags(write=False)
            memo[name] = (rp, col)
        return memo[name]
    return get


def _ids(n, seed=77):
    return np.random.default_rng(seed).permutation(n).astype(np.int32)


@pytest.mark.parametrize("name", [c.name for c in rb.CASES])
def test_build_graph_equals_brute_force(sw, brute, name):
    c = rb.BY_NAME[name]
    s = sw.Swarm(_ids(c.n), c.x, c.y, layout="input", device="cuda").build_graph(c.r)
    rp, col = s.row_ptr.cpu().numpy(), s.col.cpu().numpy()
    want_rp, want_col = brute(name)
    np.testing.assert_array_equal(rp, want_rp)
    np.testing.assert_array_equal(col, want_col)
    assert s.n_edges == want_rp[-1]


@pytest.mark.parametrize("name", [c.name for c in rb.CASES])
def test_build_graph_is_a_radius_graph(sw, name):
    """Needs no reference: rows strictly ascending, no self-loop, symmetric, row_ptr[0] == 0, and the edges
    the case fixes by construction."""
    c = rb.BY_NAME[name]
    s = sw.Swarm(_ids(c.n), c.x, c.y, layout="input", device="cuda").build_graph(c.r)
    rp, col = s.row_ptr.cpu().numpy(), s.col.cpu().numpy()
    rb.check_structure(rp, col, c.n)
    c.check_known(rp.astype(np.int64), col)


@pytest.mark.parametrize("name", ["shift_wholly_negative", "lattice_r0.5", "sparse_box_64"])
def test_spatial_layout_graph_and_election(sw, brute, oracle_mod, name):
    """The default layout stores agents in cell order (swarm_cell_order over the same binning): the graph
    relabelled to input indices is the brute-force graph, and the election over it is the oracle's."""
    c = rb.BY_NAME[name]
    ids = _ids(c.n, 5)
    s = sw.Swarm(ids, c.x, c.y, device="cuda").build_graph(c.r)
    assert s.layout == "spatial"
    perm = s.perm.cpu().numpy().astype(np.int64)
    assert np.array_equal(np.sort(perm), np.arange(c.n))
    assert not np.array_equal(perm, np.arange(c.n))  # the layout did reorder
    rp, col = s.row_ptr.cpu().numpy().astype(np.int64), s.col.cpu().numpy()
    rb.check_structure(rp, col, c.n)
    # storage row k is input agent perm[k]; its neighbours perm[col], sorted
    deg = np.diff(rp)
    src_in, dst_in = np.repeat(perm, deg), perm[col]
    o = np.lexsort((dst_in, src_in))
    got_rp = np.zeros(c.n + 1, np.int64)
    got_rp[1:] = np.cumsum(np.bincount(src_in, minlength=c.n))
    want_rp, want_col = brute(name)
    np.testing.assert_array_equal(got_rp, want_rp)
    np.testing.assert_array_equal(dst_in[o].astype(np.int32), want_col)
    r = s.elect()
    lead, state, rounds, changes = oracle_mod.elect(want_rp, want_col, ids)
    assert r.rounds_exec == rounds
    np.testing.assert_array_equal(r.changes, changes)
    np.testing.assert_array_equal(s.to_input_order(r.leader), lead)
    np.testing.assert_array_equal(s.to_input_order(r.state), state)


# ------------------------------------------------------------------ the C ABI, through _lib directly

def _rgg(pos, radius, row_ptr, col, cap):
    """One swarm_build_rgg call -> (return code, n_edges)."""
    import torch
    from swarm_amd import _lib
    ne = ctypes.c_int64(-1)
    n = 0 if pos is None else pos.shape[0]
    with torch.cuda.device(row_ptr.device):
        rc = _lib.lib().swarm_build_rgg(_lib.ctx(), n, _lib.ptr(pos) if n else None, float(radius),
                                        _lib.ptr(row_ptr), _lib.ptr(col) if col is not None else None, cap,
                                        ctypes.byref(ne), _lib.stream())
        torch.cuda.synchronize()
    return rc, ne.value


def _pos(x, y):
    import torch
    return torch.as_tensor(np.stack([x, y], 1), dtype=torch.float64, device="cuda").contiguous()


def test_two_pass_contract(sw, brute):
    import torch
    from swarm_amd import _lib
    c = rb.BY_NAME["radius_1"]
    want_rp, want_col = brute(c.name)
    e = int(want_rp[-1])
    pos = _pos(c.x, c.y)
    row_ptr = torch.full((c.n + 1,), -9, dtype=torch.int32, device="cuda")
    # the counting pass alone: n_edges and a complete row_ptr
    assert _rgg(pos, c.r, row_ptr, None, 0) == (_lib.OK, e)
    np.testing.assert_array_equal(row_ptr.cpu().numpy(), want_rp)
    # one slot short: refused, and nothing written to col
    col = torch.full((e + 8,), -7, dtype=torch.int32, device="cuda")
    rc, _ = _rgg(pos, c.r, row_ptr, col, e - 1)
    assert rc == _lib.ERR_ARG and "col_capacity" in _lib.last_error()
    assert bool((col == -7).all())
    np.testing.assert_array_equal(row_ptr.cpu().numpy(), want_rp)
    # exactly n_edges: succeeds, and writes no further than that
    assert _rgg(pos, c.r, row_ptr, col, e) == (_lib.OK, e)
    np.testing.assert_array_equal(col[:e].cpu().numpy(), want_col)
    assert bool((col[e:] == -7).all())


def test_no_agents(sw):
    import torch
    from swarm_amd import _lib
    row_ptr = torch.full((1,), -9, dtype=torch.int32, device="cuda")
    assert _rgg(None, 1.0, row_ptr, None, 0) == (_lib.OK, 0)
    assert row_ptr.cpu().tolist() == [0]
    s = sw.Swarm(np.zeros(0, np.int32), np.zeros(0), np.zeros(0), layout="input", device="cuda").build_graph(1.0)
    assert s.row_ptr.cpu().tolist() == [0] and s.n_edges == 0


@pytest.mark.parametrize("radius", [0.0, -1.0, float("nan"), float("inf"), float("-inf")])
def test_bad_radius_is_refused(sw, radius):
    import torch
    from swarm_amd import _lib
    pos = _pos(np.array([0.0, 0.5]), np.array([0.0, 0.0]))
    row_ptr = torch.full((3,), -9, dtype=torch.int32, device="cuda")
    rc, _ = _rgg(pos, radius, row_ptr, None, 0)
    assert rc == _lib.ERR_ARG and "radius" in _lib.last_error()
    assert row_ptr.cpu().tolist() == [-9, -9, -9]


def _cell_order(pos, cell=1.0):
    import torch
    from swarm_amd import _lib
    n = pos.shape[0]
    perm = torch.full((n,), -9, dtype=torch.int32, device="cuda")
    with torch.cuda.device(pos.device):
        rc = _lib.lib().swarm_cell_order(_lib.ctx(), n, _lib.ptr(pos), float(cell), _lib.ptr(perm), _lib.stream())
        torch.cuda.synchronize()
    return rc, perm.cpu().numpy()


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
@pytest.mark.parametrize("axis", [0, 1])
def test_position_that_is_not_finite_is_refused(sw, bad, axis):
    """An infinite coordinate shows in the bounding box; a NaN does not (fmin / fmax return the other
    operand), so the builder and the cell order fold the box with k_bbox_partial<true>, which counts a NaN as
    +inf.  Before that a NaN position built a graph (SWARM_OK) in which the agent had no edges."""
    import torch
    from swarm_amd import _lib
    g = np.random.default_rng(3)
    xy = g.uniform(0, 10, (300, 2))
    xy[137, axis] = bad
    pos = _pos(xy[:, 0], xy[:, 1])
    row_ptr = torch.full((301,), -9, dtype=torch.int32, device="cuda")
    rc, _ = _rgg(pos, 1.0, row_ptr, None, 0)
    assert rc == _lib.ERR_ARG and "positions must be finite" in _lib.last_error()
    rc, perm = _cell_order(pos)
    assert rc == _lib.ERR_ARG and "positions must be finite" in _lib.last_error()
    assert (perm == -9).all()


@pytest.mark.parametrize("axis", [0, 1])
def test_extent_that_is_not_finite_is_refused_promptly(sw, axis):
    """Two agents at -1e308 and +1e308: finite positions, but max - min is inf.  The grid shaping grew its
    cell to inf and then compared NaN for ever; now SWARM_ERR_ARG before the loop."""
    import torch
    from swarm_amd import _lib
    xy = np.zeros((2, 2))
    xy[:, axis] = (-1e308, 1e308)
    pos = _pos(xy[:, 0], xy[:, 1])
    row_ptr = torch.full((3,), -9, dtype=torch.int32, device="cuda")
    t0 = time.time()
    rc, _ = _rgg(pos, 1.0, row_ptr, None, 0)
    assert rc == _lib.ERR_ARG and "finite extent" in _lib.last_error()
    rc, perm = _cell_order(pos)
    assert rc == _lib.ERR_ARG and "finite extent" in _lib.last_error()
    assert time.time() - t0 < 10.0
    assert row_ptr.cpu().tolist() == [-9, -9, -9] and (perm == -9).all()
    with pytest.raises(_lib.SwarmError, match="finite extent") as e:
        sw.Swarm(np.arange(2, dtype=np.int32), xy[:, 0], xy[:, 1], device="cuda")
    assert e.value.code == _lib.ERR_ARG
    # the largest extent a double holds still builds
    xy[:, axis] = (-8.9e307, 8.9e307)
    s = sw.Swarm(np.arange(2, dtype=np.int32), xy[:, 0], xy[:, 1], device="cuda").build_graph(1.0)
    assert s.n_edges == 0 and s.row_ptr.cpu().tolist() == [0, 0, 0]
