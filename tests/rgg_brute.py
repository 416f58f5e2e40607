"""A brute-force radius graph and the inputs at which a cell-list builder goes wrong.

rgg_brute is the reference of tests/test_graph_edges.py: plain numpy over ALL pairs -- no cells, no floor,
no origin -- so it is right for any finite coordinates, where oracle.rgg_csr and gen.rgg_csr are cell lists
of the same design as the kernel (cells from floor(x / r) >= 0) and would share a bug in "within r =>
adjacent cells".  tests/test_rgg_brute.py pins the three to each other where all three apply.

cases() is the input matrix: radii, translations, pairs at exactly the radius, degenerate shapes, cells
grown by the cell cap, and both row-sort paths of swarm_build_rgg.  No reference counterpart (agent.py has
no graph: its transport is a stub, agent.py:191-194).
"""
from dataclasses import dataclass, field

import numpy as np


def rgg_brute(x, y, radius, chunk=256):
    """Edge i~j iff i != j and dx*dx + dy*dy <= r*r in float64, dx = x[i] - x[j], dy = y[i] - y[j], the two
    products rounded separately (numpy has no FMA here; the library is built with -ffp-contract=off).  Rows
    ascending.  -> (row_ptr int64, col int32).  `chunk` rows of the n x n table at a time."""
    x = np.ascontiguousarray(x, np.float64)
    y = np.ascontiguousarray(y, np.float64)
    n = len(x)
    r2 = np.float64(radius) * np.float64(radius)
    row_ptr = np.zeros(n + 1, np.int64)
    cols = []
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        dx = x[lo:hi, None] - x[None, :]
        dy = y[lo:hi, None] - y[None, :]
        near = dx * dx + dy * dy <= r2
        near[np.arange(hi - lo), np.arange(lo, hi)] = False
        ii, jj = np.nonzero(near)  # row-major: rows in order, columns ascending within a row
        row_ptr[lo + 1:hi + 1] = np.bincount(ii, minlength=hi - lo)
        cols.append(jj.astype(np.int32))
    np.cumsum(row_ptr, out=row_ptr)
    return row_ptr, (np.concatenate(cols) if cols else np.zeros(0, np.int32))


def has_edge(rp, col, i, j):
    return bool(np.any(col[rp[i]:rp[i + 1]] == j))


def check_structure(rp, col, n):
    """What a radius graph is, whatever the positions: a failure names the kind of wrong."""
    rp = np.asarray(rp, np.int64)
    col = np.asarray(col, np.int64)
    assert len(rp) == n + 1 and rp[0] == 0, "row_ptr[0] != 0"
    deg = np.diff(rp)
    assert (deg >= 0).all() and rp[-1] == len(col), "row_ptr does not ascend to the edge count"
    assert ((col >= 0) & (col < n)).all(), "column out of range"
    src = np.repeat(np.arange(n, dtype=np.int64), deg)
    assert (src != col).all(), "self-loop"
    inner = np.ones(len(col), bool)
    inner[rp[:-1][deg > 0]] = False  # the first entry of each row has no predecessor in its row
    assert (np.diff(col)[inner[1:]] > 0).all(), "a row is not strictly ascending"
    fwd, bwd = src * n + col, col * n + src
    assert np.array_equal(fwd, np.sort(bwd)), "(i, j) present without (j, i)"


@dataclass
class Case:
    name: str
    x: np.ndarray
    y: np.ndarray
    r: float
    edges: list = field(default_factory=list)       # pairs that are edges by construction
    non_edges: list = field(default_factory=list)   # pairs that are not
    degree: dict = field(default_factory=dict)      # agent -> degree known by construction
    mixed_axis: tuple = ()                          # (m,) lattice whose axis neighbours must fall on both sides

    @property
    def n(self):
        return len(self.x)

    @property
    def non_negative(self):
        return bool(self.n == 0 or (self.x.min() >= 0 and self.y.min() >= 0))

    def dense_table_cells(self):
        """Cells of the table orc_rgg_csr allocates: floor(max / r) + 3 a side, indexed from the origin."""
        return (np.floor(self.x.max() / self.r) + 3.0) * (np.floor(self.y.max() / self.r) + 3.0)

    def check_known(self, rp, col):
        """The edges this case fixes by construction (exact arithmetic: dyadic or integer coordinates)."""
        for i, j in self.edges:
            assert has_edge(rp, col, i, j) and has_edge(rp, col, j, i), (self.name, "missing edge", i, j)
        for i, j in self.non_edges:
            assert not has_edge(rp, col, i, j) and not has_edge(rp, col, j, i), (self.name, "false edge", i, j)
        for i, d in self.degree.items():
            assert rp[i + 1] - rp[i] == d, (self.name, "degree", i, int(rp[i + 1] - rp[i]), d)


def _uniform(rng, n, r, deg=8.0):
    side = np.sqrt(n * np.pi * r * r / deg)
    return rng.uniform(0, side, n), rng.uniform(0, side, n), side


def _lattice(name, m, r, shift, rng, known):
    """m x m points k * r (+ shift), agent indices permuted."""
    k = rng.permutation(m * m)
    ix, iy = k % m, k // m
    x, y = ix * r + shift, iy * r + shift
    c = Case(name, x, y, r)
    at = {(int(a), int(b)): i for i, (a, b) in enumerate(zip(ix, iy))}
    if known:  # spacing exactly r: axis neighbours are edges, diagonals (r * sqrt 2) are not, interior degree 4
        for (a, b), i in at.items():
            if a + 1 < m:
                c.edges.append((i, at[a + 1, b]))
            if b + 1 < m:
                c.edges.append((i, at[a, b + 1]))
            if a + 1 < m and b + 1 < m:
                c.non_edges.append((i, at[a + 1, b + 1]))
                c.non_edges.append((at[a + 1, b], at[a, b + 1]))
            if 0 < a < m - 1 and 0 < b < m - 1:
                c.degree[i] = 4
    else:
        c.mixed_axis = (m,)
    return c


def _cluster_with_singletons(name, rng, n_cluster, box, r=1.0):
    """n_cluster agents uniform in a box x box square at (15r, 15r) and six singletons > 3 cells from it and
    from each other, indices permuted.  swarm_build_rgg sorts its rows in the kernel when the largest 3 x 3
    cell window holds at most 64 agents and with hipCUB's segmented sort otherwise (the rule at
    graph.hip:89, `max_win <= kInKernelSort`); the window that covers the cluster decides."""
    sx = np.array([0.0, 30.0, 0.0, 30.0, 5.0, 25.0]) * r   # 31 x 31 cells of side r: below the cell cap
    sy = np.array([0.0, 0.0, 30.0, 30.0, 25.0, 5.0]) * r
    x = np.concatenate([15.0 * r + rng.uniform(0, box, n_cluster), sx])
    y = np.concatenate([15.0 * r + rng.uniform(0, box, n_cluster), sy])
    p = rng.permutation(len(x))
    c = Case(name, x[p], y[p], r)
    inv = np.argsort(p)
    c.degree = {int(inv[n_cluster + k]): 0 for k in range(len(sx))}
    return c


def cases():
    out = []
    # ---- radii: uniform, mean degree ~8 (the box scales with r)
    for k, r in enumerate((0.05, 1.0 / 3.0, 1.0, 2.5, 1e-3, 1e3)):
        rng = np.random.default_rng(100 + k)
        x, y, _ = _uniform(rng, 1500, r)
        out.append(Case(f"radius_{r:.4g}", x, y, r))
    # ---- translations of one cloud at r = 1
    rng = np.random.default_rng(200)
    x, y, side = _uniform(rng, 2000, 1.0)
    for name, sx, sy in (("shift_wholly_negative", -side, -side), ("shift_straddles_origin", -side / 2, -side / 2),
                         ("shift_1e6_mixed_signs", 1e6, -1e6), ("shift_1e9", 1e9, 1e9)):
        out.append(Case(name, x + sx, y + sy, 1.0))
    # ---- exactly at the radius
    rng = np.random.default_rng(300)
    for r in (1.0, 0.5, 0.25):
        out.append(_lattice(f"lattice_r{r}", 20, r, 0.0, rng, True))
        out.append(_lattice(f"lattice_r{r}_shift_1e6", 20, r, 1e6, rng, True))
    out.append(_lattice("lattice_r0.1", 30, 0.1, 0.0, rng, False))
    out.append(_lattice("lattice_r_third", 30, 1.0 / 3.0, 0.0, rng, False))
    # integer 3-4-5 triangles at r = 5: squared distance exactly 25.  Per base b (40 apart): b, b + (3, 4),
    # b + (5, 0), b + (0, 5), b + (4, -3), b + (5, 1) [26: no edge to b], b + (6, 8) [100: no edge to b]
    offs = np.array([(0, 0), (3, 4), (5, 0), (0, 5), (4, -3), (5, 1), (6, 8)], np.float64)
    bases = np.array([(10 + 40 * i, 10 + 40 * j) for i in range(5) for j in range(4)], np.float64)
    pts = (bases[:, None, :] + offs[None, :, :]).reshape(-1, 2)
    c = Case("triangles_3_4_5", pts[:, 0].copy(), pts[:, 1].copy(), 5.0)
    for b in range(len(bases)):
        o = b * len(offs)
        c.edges += [(o, o + 1), (o, o + 2), (o, o + 3), (o, o + 4), (o + 1, o + 6)]
        c.non_edges += [(o, o + 5), (o, o + 6), (o + 3, o + 2)]
    out.append(c)
    # one ulp either side of r = 1.0 (differences from the origin are exact)
    up, down = np.nextafter(1.0, 2.0), np.nextafter(1.0, 0.0)
    c = Case("nextafter_r1", np.array([0.0, 1.0, 0.0, down, 0.0, up]), np.array([0.0, 0.0, up, 0.0, down, 0.0]), 1.0)
    c.edges = [(0, 1), (0, 3), (0, 4)]
    c.non_edges = [(0, 2), (0, 5)]
    out.append(c)
    # ---- degenerate shapes
    out.append(Case("n1", np.array([2.5]), np.array([7.25]), 1.0, degree={0: 0}))
    out.append(Case("n2_colocated", np.array([5.0, 5.0]), np.array([5.0, 5.0]), 1.0, edges=[(0, 1)]))
    out.append(Case("n2_at_radius", np.array([3.0, 4.0]), np.array([4.0, 4.0]), 1.0, edges=[(0, 1)]))
    out.append(Case("n2_apart", np.array([0.0, 3.0]), np.array([0.0, 0.0]), 1.0, non_edges=[(0, 1)]))
    rng = np.random.default_rng(400)
    out.append(Case("line_horizontal", rng.uniform(0, 100, 300), np.full(300, 7.0), 1.0))   # one grid row
    out.append(Case("line_vertical", np.full(300, 7.0), rng.uniform(0, 100, 300), 1.0))     # one grid column
    out.append(Case("one_point_200", np.full(200, 3.5), np.full(200, 2.25), 1.0, degree={i: 199 for i in range(200)}))
    px, py = rng.uniform(0, 4, 40), rng.uniform(0, 4, 40)
    p = rng.permutation(240)
    out.append(Case("duplicates_40x6", np.repeat(px, 6)[p], np.repeat(py, 6)[p], 1.0))
    # ---- cells grown by the cell cap (4n + 1024)
    # 64 agents over 1e4 x 1e4: at most 1280 cells, so cells of 2^8.5 ~ 362 (28 x 28); 10 pairs within r
    rng = np.random.default_rng(500)
    ax, ay = rng.uniform(0, 1e4, 54), rng.uniform(0, 1e4, 54)
    ax[:2], ay[:2] = (0.0, 1e4), (0.0, 1e4)  # the box's corners
    th = rng.uniform(0, 2 * np.pi, 10)
    x = np.concatenate([ax, ax[2:12] + 0.6 * np.cos(th)])
    y = np.concatenate([ay, ay[2:12] + 0.6 * np.sin(th)])
    x, y = np.clip(x, 0, 1e4), np.clip(y, 0, 1e4)
    out.append(Case("sparse_box_64", x, y, 1.0, edges=[(2 + k, 54 + k) for k in range(10)]))
    # two clusters 1e12 apart: two occupied cells of ~5e8 a side
    x = np.concatenate([rng.uniform(0, 5, 100), 1e12 + rng.uniform(0, 5, 100)])
    y = rng.uniform(0, 5, 200)
    out.append(Case("clusters_1e12_apart", x, y, 1.0))
    # ---- both row-sort paths with work to do (the candidates arrive cell by cell, not by index)
    rng = np.random.default_rng(600)
    out.append(_cluster_with_singletons("sort_in_kernel_50", rng, 50, 2.5))     # largest window <= 56
    out.append(_cluster_with_singletons("sort_hipcub_120", rng, 120, 2.5))      # the centre cell's window: 120
    out.append(_cluster_with_singletons("sort_window_64", rng, 64, 0.3))        # exactly 64: the in-kernel sort
    out.append(_cluster_with_singletons("sort_window_65", rng, 65, 0.3))        # exactly 65: hipCUB
    return out


CASES = cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
