"""The three radius-graph references agree (CPU): tests/rgg_brute.py (all pairs, no cells), oracle.rgg_csr
and gen.rgg_csr (cell lists indexed from floor(x / r) >= 0, the kernel's own design).

The larger GPU tests compare swarm_build_rgg with the two cell-list references; this pins those to a
reference that shares nothing with them, on every input of rgg_brute.CASES that they can take:
  * gen.rgg_csr  -- every case without a negative coordinate (its cell keys are sparse);
  * oracle.rgg_csr -- those of them whose dense cell table, (floor(max x / r) + 3) * (floor(max y / r) + 3)
    cells indexed from the origin, has at most 2^24 cells (128 MiB of offsets).  The others need from
    0.8 GB (the 1e4 x 1e4 box) to 8e18 cells (coordinates of 1e9) of a table it cannot allocate.
No reference counterpart (agent.py has no graph).
"""
import numpy as np
import pytest

import rgg_brute as rb

ORACLE_TABLE_LIMIT = float(1 << 24)
NON_NEG = [c.name for c in rb.CASES if c.non_negative]
ORACLE_OK = [n for n in NON_NEG if rb.BY_NAME[n].dense_table_cells() <= ORACLE_TABLE_LIMIT]


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


def test_case_matrix_is_what_it_claims():
    assert len(rb.CASES) == 34 and max(c.n for c in rb.CASES) <= 4096
    assert len(NON_NEG) == 31 and len(ORACLE_OK) == 25
    for c in rb.CASES:
        assert np.isfinite(c.x).all() and np.isfinite(c.y).all() and c.x.dtype == c.y.dtype == np.float64
    b = rb.BY_NAME
    assert b["shift_wholly_negative"].x.max() < 0 and b["shift_wholly_negative"].y.max() < 0
    s = b["shift_straddles_origin"]
    assert s.x.min() < 0 < s.x.max() and s.y.min() < 0 < s.y.max()
    assert b["sparse_box_64"].n == 64 and b["one_point_200"].n == 200 and b["duplicates_40x6"].n == 240


@pytest.mark.parametrize("name", [c.name for c in rb.CASES])
def test_brute_force_is_a_radius_graph(brute, name):
    c = rb.BY_NAME[name]
    rp, col = brute(name)
    assert rp.dtype == np.int64 and col.dtype == np.int32
    rb.check_structure(rp, col, c.n)
    c.check_known(rp, col)


def test_brute_force_against_a_double_loop():
    """The vectorised all-pairs table against the definition written as two loops, over a chunk boundary."""
    g = np.random.default_rng(9)
    x, y = g.uniform(-3, 3, 70), g.uniform(-3, 3, 70)
    rp, col = rb.rgg_brute(x, y, 0.9, chunk=32)
    want = [[j for j in range(70) if j != i and (x[i] - x[j]) * (x[i] - x[j]) + (y[i] - y[j]) * (y[i] - y[j])
             <= 0.9 * 0.9] for i in range(70)]
    assert rp.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
    assert col.tolist() == [j for w in want for j in w]
    assert rb.rgg_brute(np.zeros(0), np.zeros(0), 1.0)[0].tolist() == [0]


@pytest.mark.parametrize("name", ["lattice_r0.1", "lattice_r_third"])
def test_inexact_lattices_discriminate(brute, name):
    """Spacing k * r for a radius that is no dyadic number: the computed differences fall on both sides of r,
    so a builder that compares with < or in another precision cannot pass by luck."""
    c = rb.BY_NAME[name]
    (m,) = c.mixed_axis
    rp, _ = brute(name)
    ix, iy = np.rint(c.x / c.r).astype(int), np.rint(c.y / c.r).astype(int)
    interior = (ix > 0) & (ix < m - 1) & (iy > 0) & (iy < m - 1)
    deg = np.diff(rp)[interior]
    assert 0 < (deg == 4).mean() < 0.25 and (deg < 4).any(), np.bincount(deg)


def _max_window(c):
    """The largest 3 x 3 cell window of swarm_build_rgg's grid for a case whose cells are not grown: cells of
    side r * (1 + 1e-9) from the bounding box's minimum."""
    cell = c.r * (1.0 + 1e-9)
    cx = np.floor((c.x - c.x.min()) / cell).astype(int)
    cy = np.floor((c.y - c.y.min()) / cell).astype(int)
    assert (cx.max() + 1) * (cy.max() + 1) <= 4 * c.n + 1024, "the cell cap would grow these cells"
    occ = np.zeros((cy.max() + 3, cx.max() + 3), int)
    np.add.at(occ, (cy + 1, cx + 1), 1)
    win = sum(occ[1 + dy:occ.shape[0] - 1 + dy, 1 + dx:occ.shape[1] - 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1))
    return int(win[occ[1:-1, 1:-1] > 0].max())


@pytest.mark.parametrize("name,in_kernel", [("sort_in_kernel_50", True), ("sort_hipcub_120", False),
                                            ("sort_window_64", True), ("sort_window_65", False)])
def test_sort_cases_sit_on_their_side_of_the_switch(brute, name, in_kernel):
    """swarm_build_rgg sorts rows in the kernel iff the largest window holds <= 64 agents (graph.hip,
    `max_win <= kInKernelSort`); the tests cannot see which path ran, so the inputs are checked against the
    rule here.  Each has rows that arrive unsorted: some row's neighbours do not ascend in cell order."""
    c = rb.BY_NAME[name]
    w = _max_window(c)
    assert (w <= 64) == in_kernel, w
    if name.startswith("sort_window"):
        assert w == c.n - 6
    assert np.diff(brute(name)[0]).max() >= 20


@pytest.mark.parametrize("name", NON_NEG)
def test_gen_rgg_csr_equals_brute_force(brute, name):
    from swarm_amd import gen
    c = rb.BY_NAME[name]
    rp, col = gen.rgg_csr(c.x, c.y, c.r)
    np.testing.assert_array_equal(rp, brute(name)[0])
    np.testing.assert_array_equal(col, brute(name)[1])


@pytest.mark.parametrize("name", ORACLE_OK)
def test_oracle_rgg_csr_equals_brute_force(brute, oracle_mod, name):
    c = rb.BY_NAME[name]
    rp, col = oracle_mod.rgg_csr(c.x, c.y, c.r)
    np.testing.assert_array_equal(rp, brute(name)[0])
    np.testing.assert_array_equal(col, brute(name)[1])
