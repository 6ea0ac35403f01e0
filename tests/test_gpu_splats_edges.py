"""The splat mesh index (csrc/e3d_splats.hip) at the edges of its pruning bound, against references that prune nothing:
distances bit for bit and ids exactly against splat_ref.mesh_min_sq (every query against every triangle); flags, radii and
corners against splat_ref.splats(cull=False).  No assertion has a tolerance.  Where an output may be NaN the NaN-ness is
compared first and the bits elsewhere (an invalid operation gives 0xffc00000 on x86 and 0x7fc00000 on the GPU)."""
import functools

import numpy as np
import pytest

import splat_ref as sr

pytestmark = pytest.mark.gpu

F = np.float32
REGULAR_SIN2 = 1.0 / 65536.0           # kRegularSin2: the tree takes a triangle whose angle at a has sin^2 >= this (f64)
UP = np.array([[0, 0, 1]], F)


def _u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _assert_same_f32(got, ref, what):
    got = np.ascontiguousarray(got, F); ref = np.ascontiguousarray(ref, F)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    gn, rn = np.isnan(got), np.isnan(ref)
    assert np.array_equal(gn, rn), (what + ": NaN-ness differs", np.argwhere(gn != rn)[:10])
    bad = (_u32(got) != _u32(ref)) & ~gn
    assert not bad.any(), (what + " differ", np.argwhere(bad)[:10], got[bad][:5], ref[bad][:5])


def _check_min(e3d, P, V, T, max_sq=np.inf):
    """e3d_mesh_squared_distance against the full brute force: same bits, same ids"""
    P = np.ascontiguousarray(P, F)
    d, i = e3d.mesh_squared_distance(P, V, T, max_sq)
    with np.errstate(all="ignore"):
        rd, ri = sr.mesh_min_sq(P, V, T, max_sq)
    assert not np.isnan(d).any()
    bad = _u32(d) != _u32(rd)
    assert not bad.any(), ("distances differ", max_sq, np.nonzero(bad)[0][:10], d[bad][:5], rd[bad][:5], P[bad][:5])
    bad = i != ri
    assert not bad.any(), ("ids differ", max_sq, np.nonzero(bad)[0][:10], i[bad][:5], ri[bad][:5], d[bad][:5])
    return d, i


def _check_splats(e3d, xyz, nrm, V, T, thr, max_splat=np.inf):
    """e3d_create_splats against the reference without culling: flags, radii, corners, faces"""
    gv, gf, ga, gr = e3d.create_splats(xyz, nrm, V, T, thr, max_splat)
    with np.errstate(all="ignore"):
        rv, rf, ra, rr = sr.splats(xyz, nrm, V, T, thr, max_splat, cull=False)
    assert np.array_equal(ga, ra), ("flags differ", thr, max_splat, np.nonzero(ga != ra)[0][:10])
    _assert_same_f32(gr, rr, "radii")
    _assert_same_f32(gv, rv, "splat vertices")
    assert np.array_equal(gf, rf) and gv.shape == (4 * int(ga.sum()), 3)
    return ga, gr, gv


def _sin2_at_a(tri):
    """(f64 sin^2 of the angle at a, two vertices equal, all finite) of (m, 3, 3) f32 triangles: k_tri_keys' formula"""
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    with np.errstate(all="ignore"):
        u = b.astype(np.float64) - a.astype(np.float64)
        w = c.astype(np.float64) - a.astype(np.float64)
        n = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)
        nn = n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2]
        uu = u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1] + u[:, 2] * u[:, 2]
        ww = w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1] + w[:, 2] * w[:, 2]
        s2 = nn / (uu * ww)
        in_tree_by_angle = nn >= REGULAR_SIN2 * uu * ww
    equal = (a == b).all(1) | (a == c).all(1) | (b == c).all(1)
    finite = np.isfinite(tri).all((1, 2))
    return s2, in_tree_by_angle, equal, finite


def _in_tree(tri):
    _, by_angle, equal, finite = _sin2_at_a(tri)
    return finite & (equal | by_angle)


def _soup_mesh(tri):
    tri = np.ascontiguousarray(tri, F).reshape(-1, 3, 3)
    return tri.reshape(-1, 3), np.arange(3 * tri.shape[0], dtype=np.uint32).reshape(-1, 3)


def _generic(rng, t, lo=0.0, hi=1.0, size=0.05):
    a = rng.uniform(lo, hi, (t, 3))
    tri = np.stack([a, a + rng.normal(0, size, (t, 3)), a + rng.normal(0, size, (t, 3))], 1).astype(F)
    assert _in_tree(tri).all()
    return tri


OUT_OF_TREE = np.array([[[0.5, 0.5, 0.5], [np.nan, 0.6, 0.5], [0.5, 0.6, 0.6]],                 # a NaN vertex
                        [[0.25, 0.25, 0.25], [0.5, 0.5, 0.5], [0.75, 0.75, 0.75]],             # collinear, exactly
                        [[0.2, 0.7, 0.3], [0.7, 0.7, 0.3], [0.7, 0.7005, 0.3]]], F)            # sin^2 = 1e-6 < 2^-16


def _flat_grid(n, h, z=0.0, x0=0.0, y0=0.0):
    """n x n cells of size h in the plane z: ((n+1)^2 vertices, 2 n^2 triangles (i, i+1, i+nu), (i+1, i+nu+1, i+nu))"""
    nu = n + 1
    ys, xs = np.meshgrid(y0 + h * np.arange(nu), x0 + h * np.arange(nu), indexing="ij")
    V = np.stack([xs, ys, np.full_like(xs, z)], -1).reshape(-1, 3).astype(F)
    idx = (np.arange(n)[:, None] * nu + np.arange(n)[None, :]).reshape(-1)
    T = np.stack([np.stack([idx, idx + 1, idx + nu], -1), np.stack([idx + 1, idx + nu + 1, idx + nu], -1)], 1).reshape(-1, 3)
    return V, T.astype(np.uint32)


# ---- 1. tree shapes -------------------------------------------------------------------------------------------------
def _shape_case(t, k):
    rng = np.random.default_rng(1000 + 7 * t + k)
    tri = _generic(rng, t)
    if k:
        assert not _in_tree(OUT_OF_TREE).any()
        pos = [0, (t + k) // 2, t + k - 1]                            # interleaved by id: first, middle, last
        parts = list(tri)
        for p, o in zip(pos, OUT_OF_TREE):
            parts.insert(p, o)
        tri = np.stack(parts) if parts else tri
    V, T = _soup_mesh(tri)
    d = rng.normal(size=(120, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    far = 0.5 + d * 10.0 ** rng.uniform(1, 3.5, (120, 1))            # 10 .. 3000 box lengths away
    far[100:] = rng.choice([-1.0, 1.0], (20, 3)) * rng.uniform(0.5, 1.0, (20, 3)) * 1.0e6      # coordinates of 10^6 against a unit mesh
    far[110:, 1:] = rng.uniform(0, 1, (10, 2))                                                  # ... and along one axis only
    P = np.concatenate([rng.uniform(-0.2, 1.2, (380, 3)), far]).astype(F)
    return V, T, P


@pytest.mark.parametrize("k", [0, 3])
@pytest.mark.parametrize("t", [0, 1, 3, 4, 5, 8, 9, 1023, 1024, 1025, 4096, 4097])
def test_tree_shapes(e3d, t, k):
    """P = 1 (the root is a leaf), a leaf count one past a power of two (half the leaves empty), the scanned list with and
    without a tree, an empty mesh"""
    V, T, P = _shape_case(t, k)
    assert V.shape == (3 * (t + k), 3) and T.shape == (t + k, 3)
    d, i = _check_min(e3d, P, V, T)
    if t == 0 and k == 0:
        assert np.isinf(d).all() and (i == -1).all()
    else:
        assert np.isfinite(d).all() and (i >= 0).all()
    d, i = _check_min(e3d, P, V, T, 0.003)
    assert np.isinf(d[380:]).all() and (i[380:] == -1).all()
    if t >= 1023:
        assert np.isfinite(d).sum() > 50 and np.isinf(d[:380]).sum() > 50


def test_empty_mesh_flags_every_live_point(e3d):
    rng = np.random.default_rng(5)
    xyz = rng.uniform(0, 1, (60, 3)).astype(F)
    nrm = np.tile(UP, (60, 1))
    nrm[7, 1] = np.nan
    xyz[9, 2] = np.inf
    ga, gr, gv = _check_splats(e3d, xyz, nrm, np.zeros((0, 3), F), np.zeros((0, 3), np.uint32), 0.02)
    live = np.ones(60, bool); live[[7, 9]] = False
    assert np.array_equal(ga, live) and np.isnan(gr[~live]).all() and gv.shape == (4 * 58, 3)


# ---- 2. equal minima in different subtrees --------------------------------------------------------------------------
def _grid_queries(V, n):
    nu = n + 1
    idx = (np.arange(n)[:, None] * nu + np.arange(n)[None, :]).reshape(-1)
    mid = [(V[idx] + V[idx + 1]) * F(0.5), (V[idx] + V[idx + nu]) * F(0.5), (V[idx + 1] + V[idx + nu]) * F(0.5)]
    return np.concatenate([V] + mid).astype(F)


def test_ties_on_a_grid_lowest_id_wins(e3d):
    """all coordinates dyadic: queries on every vertex and edge midpoint have up to six triangles at distance exactly 0, and
    the same queries 1/4 above the grid have them at exactly 1/16"""
    n = 16
    V, T = _flat_grid(n, 0.125)
    Q = _grid_queries(V, n)
    nv = V.shape[0]
    lowest = np.array([np.nonzero((T == v).any(1))[0].min() for v in range(nv)])       # lowest id among a vertex's triangles
    for lift, value in ((0.0, 0.0), (0.25, 0.0625)):
        d, i = _check_min(e3d, Q + np.array([0, 0, lift], F), V, T)
        assert (d == F(value)).all()
        assert np.array_equal(i[:nv], lowest)
    # the list appended to itself in shuffled order: twins have distant ids, the lower twin wins
    rng = np.random.default_rng(11)
    nt = T.shape[0]
    p1, p2 = rng.permutation(nt), rng.permutation(nt)
    T2 = np.concatenate([T[p1], T[p2]])
    d, i = _check_min(e3d, Q, V, T2)
    assert (d == 0).all() and (i < nt).all()
    inv1 = np.empty(nt, np.int64); inv1[p1] = np.arange(nt)
    assert np.array_equal(i[:nv], np.array([inv1[np.nonzero((T == v).any(1))[0]].min() for v in range(nv)]))
    d, i = _check_min(e3d, Q + np.array([0, 0, 0.25], F), V, T2, 0.0625)
    assert (d == F(0.0625)).all() and (i < nt).all()


@pytest.mark.parametrize("first", [1.0, -1.0])
def test_ties_between_two_sheets(e3d, first):
    """two copies of a grid at z = +1 and z = -1, queries at z = 0 above the vertices and the cell centres: the equal minima sit
    in different halves of the tree, the sheet with the lower ids wins whichever half it is"""
    n = 12
    Va, T = _flat_grid(n, 0.25, first)
    Vb, _ = _flat_grid(n, 0.25, -first)
    V = np.concatenate([Va, Vb]); TT = np.concatenate([T, T + Va.shape[0]]).astype(np.uint32)
    nu = n + 1
    idx = (np.arange(n)[:, None] * nu + np.arange(n)[None, :]).reshape(-1)
    Q = np.concatenate([Va, (Va[idx + 1] + Va[idx + nu]) * F(0.5)]).astype(F)
    Q[:, 2] = 0
    for max_sq in (np.inf, 1.0):
        d, i = _check_min(e3d, Q, V, TT, max_sq)
        assert (d == 1).all() and (i < T.shape[0]).all()


# ---- 3. max_sq at the value -----------------------------------------------------------------------------------------
def test_bound_at_the_minimum_and_one_ulp_below(e3d):
    V, T, P = _shape_case(1025, 3)
    P = P[:120]
    with np.errstate(all="ignore"):
        rd, ri = sr.mesh_min_sq(P, V, T)
    picks = np.nonzero(rd > 0)[0][::5][:20]
    assert picks.size == 20
    for j in picks:
        d, i = _check_min(e3d, P, V, T, rd[j])
        assert d[j] == rd[j] and i[j] == ri[j]
        below = np.nextafter(rd[j], F(0))
        assert below < rd[j]
        d, i = _check_min(e3d, P, V, T, below)
        assert np.isinf(d[j]) and i[j] == -1
        assert np.array_equal(np.isfinite(d), rd <= below)


def test_bound_zero_and_negative(e3d):
    V, T, P = _shape_case(1025, 3)
    tri = V.reshape(-1, 3, 3)
    Q = np.concatenate([tri[np.isfinite(tri).all((1, 2))].reshape(-1, 3)[::13], P[:100]])       # exactly on vertices, and elsewhere
    nq = Q.shape[0] - 100
    d, i = _check_min(e3d, Q, V, T, 0.0)
    assert (d[:nq] == 0).all() and (i[:nq] >= 0).all() and np.isinf(d[nq:]).all()
    for max_sq in (-1.0, -np.inf):
        d, i = _check_min(e3d, Q, V, T, max_sq)
        assert np.isinf(d).all() and (i == -1).all()


# ---- 3b. queries that need the margin delta ----------------------------------------------------------------------------
def _bare_gap(p, lo, hi):
    """node_lower_bound with delta = 0 (f32, the kernel's order): the squared box gap times (1 - 2^-20)"""
    g = [np.maximum(np.maximum(lo[:, k] - p[:, k], p[:, k] - hi[:, k]), F(0)) for k in range(3)]
    return ((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]) * (F(1) - F(1) / F(1048576))


@functools.lru_cache(maxsize=None)
def _near_pairs():
    """(queries, triangles) tens of ulps from a vertex or an edge of an ordinary tree triangle, split by the restatement into
    those whose computed value lies below the bare gap of the triangle's own box (only delta keeps the prune right) and the rest"""
    rng = np.random.default_rng(606)
    p, a, b, c = sr.near_feature_pairs(rng, 300_000)
    tri = np.stack([a, b, c], 1)
    s2, _, equal, _ = _sin2_at_a(tri)
    keep = ~equal & (s2 > 0.01)
    p, tri = p[keep], tri[keep]
    with np.errstate(all="ignore"):
        value = sr.ericson_sq(p, tri[:, 0], tri[:, 1], tri[:, 2])
    need = _bare_gap(p, tri.min(1), tri.max(1)) > value
    assert need.sum() >= 80
    return p[need], tri[need], p[~need][:300], tri[~need][:300]


def test_queries_tens_of_ulps_from_one_triangle_need_delta(e3d):
    """P = 1, the root is the triangle's own box: with kMarginScale = 0 the root would be pruned at max_sq = the query's value
    and the call would return +inf / -1"""
    P, tri, _, _ = _near_pairs()
    rng = np.random.default_rng(607)
    for j in range(12):
        V, T = _soup_mesh(tri[j:j + 1])
        d = rng.normal(size=(40, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
        Q = np.concatenate([P[j:j + 1], P[j] + 10.0 ** rng.uniform(-7, -4, (40, 1)) * np.abs(tri[j]).max() * d]).astype(F)
        d0, i0 = _check_min(e3d, Q, V, T)
        assert np.isfinite(d0).all() and (i0 == 0).all()
        d1, i1 = _check_min(e3d, Q, V, T, d0[0])
        assert d1[0] == d0[0] and i1[0] == 0
        assert np.array_equal(np.isfinite(d1), d0 <= d0[0])


def test_queries_tens_of_ulps_from_a_soup_need_delta(e3d):
    """the same pairs in one soup: the winner's leaf holds three more triangles, and max_sq sits at each query's own minimum"""
    Pn, trin, Po, trio = _near_pairs()
    rng = np.random.default_rng(608)
    order = rng.permutation(80 + 300)
    tri = np.concatenate([trin[:80], trio])[order]
    Q = np.concatenate([Pn[:80], Po])[order]
    V, T = _soup_mesh(tri)
    d0, i0 = _check_min(e3d, Q, V, T)
    assert np.isfinite(d0).all()
    needy = np.nonzero(order < 80)[0]
    assert (i0[needy] == needy).mean() > 0.9                              # mostly the near triangle is the winner
    for j in needy[:24]:
        d1, i1 = _check_min(e3d, Q, V, T, d0[j])
        assert d1[j] == d0[j] and i1[j] == i0[j]


# ---- 4. shapes and ranges the margin argument leans on --------------------------------------------------------------
LATTICE = 2.0 ** -10        # vertices on this lattice inside [0, 9): the offset by 4096 is exact in f32


def _lattice_triangles(rng, want, lo2, hi2):
    """triangles on the lattice whose angle at a has f64 sin^2 in [lo2, hi2): a long edge n1 d, the other n2 d + e"""
    out = []
    have = 0
    while have < want:
        m = 20000
        d = rng.integers(-3, 4, (m, 3)); e = rng.integers(-2, 3, (m, 3))
        ab = rng.integers(40, 160, (m, 1)) * d
        ac = rng.integers(40, 160, (m, 1)) * d + e
        a = rng.integers(512, 8 * 1024, (m, 3))
        tri = (np.stack([a, a + ab, a + ac], 1) * LATTICE).astype(F)
        s2, _, equal, _ = _sin2_at_a(tri)
        keep = ~equal & (s2 >= lo2) & (s2 < hi2)
        out.append(tri[keep]); have += int(keep.sum())
    return np.concatenate(out)[:want]


def _sliver_scene():
    rng = np.random.default_rng(77)
    tree = _lattice_triangles(rng, 500, REGULAR_SIN2, 2 * REGULAR_SIN2)          # just on the tree side
    below = _lattice_triangles(rng, 100, REGULAR_SIN2 / 4, REGULAR_SIN2)          # just on the list side
    a = rng.integers(512, 8 * 1024, (400, 1, 3))
    generic = ((a + rng.integers(-200, 201, (400, 3, 3))) * LATTICE).astype(F)
    generic = generic[_sin2_at_a(generic)[0] > 0.01]
    tri = np.concatenate([tree, below, generic])
    side = np.concatenate([np.ones(len(tree), bool), np.zeros(len(below), bool), np.ones(len(generic), bool)])
    order = rng.permutation(len(tri))
    tri, side = tri[order], side[order]
    A = tree[:, 0].astype(np.float64); AB = tree[:, 1] - A; AC = tree[:, 2] - A
    N = np.cross(AB, AC); N /= np.linalg.norm(N, axis=1, keepdims=True)
    ext = 9.0
    j = rng.integers(0, len(tree), 800)
    groups = [
        # beyond the sharp ends, a little to the side
        A[j[:150]] - 10.0 ** rng.uniform(-3, 0.3, (150, 1)) * 0.5 * (AB + AC)[j[:150]] + rng.normal(0, 1e-3, (150, 1)) * np.cross(N, AB)[j[:150]],
        # in the plane
        A[j[150:300]] + rng.uniform(-0.5, 1.5, (150, 1)) * AB[j[150:300]] + rng.uniform(-0.5, 1.5, (150, 1)) * AC[j[150:300]],
        # 10^2 and 10^3 mesh extents away along the normals
        A[j[300:400]] + rng.choice([-1.0, 1.0], (100, 1)) * 100 * ext * N[j[300:400]],
        A[j[400:500]] + rng.choice([-1.0, 1.0], (100, 1)) * 1000 * ext * N[j[400:500]],
        # coordinates of 10^6
        rng.choice([-1.0, 1.0], (60, 3)) * rng.uniform(0.3, 1.0, (60, 3)) * 1.0e6,
        # inside the mesh's box, and just above the slivers
        rng.uniform(0, 9, (150, 3)),
        A[j[500:650]] + rng.uniform(0, 1, (150, 1)) * AB[j[500:650]] * rng.uniform(0, 1, (150, 1)) + 10.0 ** rng.uniform(-5, -1, (150, 1)) * N[j[500:650]],
    ]
    return tri, side, np.concatenate(groups).astype(F)


@pytest.mark.parametrize("offset", [0.0, 4096.0])
def test_slivers_at_the_tree_threshold(e3d, offset):
    tri, side, P = _sliver_scene()
    tri = (tri + F(offset)).astype(F); P = (P + F(offset)).astype(F)
    s2, by_angle, equal, finite = _sin2_at_a(tri)
    assert finite.all() and not equal.any()
    assert np.array_equal(by_angle, side)                               # the side each triangle falls on, by k_tri_keys' formula
    assert ((s2 >= REGULAR_SIN2) & (s2 < 2 * REGULAR_SIN2)).sum() == 500 and ((s2 < REGULAR_SIN2) & (s2 >= REGULAR_SIN2 / 4)).sum() == 100
    V, T = _soup_mesh(tri)
    for max_sq in (np.inf, 0.01, 2.0e12):
        d, _ = _check_min(e3d, P, V, T, max_sq)
        assert np.isfinite(d).sum() > 100


def test_tiny_triangles_in_a_wide_mesh(e3d):
    """triangles of 10^-4 in a mesh that spans 10^3: half of them where 10^-4 is far above an ulp, half where it is a few ulps
    (rounding leaves some with equal or collinear vertices)"""
    rng = np.random.default_rng(31)
    a = np.concatenate([rng.uniform(0, 2, (500, 3)), rng.uniform(0, 1000, (500, 3))])
    tri = np.stack([a, a + rng.normal(0, 1e-4, (1000, 3)), a + rng.normal(0, 1e-4, (1000, 3))], 1).astype(F)
    kinds = _in_tree(tri)
    assert kinds.sum() > 600 and (~kinds).any() and _sin2_at_a(tri)[2].any()      # in the tree, in the list, two equal vertices
    V, T = _soup_mesh(tri[rng.permutation(1000)])
    j = rng.integers(0, 1000, 600)
    P = np.concatenate([a[j] + rng.normal(0, 3e-4, (600, 3)), a[j[:100]] + rng.normal(0, 1e-5, (100, 3)), rng.uniform(0, 1000, (100, 3)),
                        rng.uniform(0, 2, (100, 3))]).astype(F)
    for max_sq in (np.inf, 1.0e-6):
        d, _ = _check_min(e3d, P, V, T, max_sq)
    assert np.isfinite(d).sum() > 100 and np.isinf(d).sum() > 100


def test_infinite_vertices_in_the_mesh_box(e3d):
    """a mesh of unit scale in y and z that spans x in [0, 1000], plus a triangle with a +inf x and one with a -inf y: the box
    is infinite on two sides, the index takes its magnitude from the finite sides only"""
    rng = np.random.default_rng(41)
    a = np.stack([rng.uniform(0, 1000, 600), rng.uniform(0, 1, 600), rng.uniform(0, 1, 600)], 1)
    a[:40, 0] = rng.uniform(0, 3, 40); a[40:80, 0] = rng.uniform(997, 1000, 40)
    tri = np.stack([a, a + rng.normal(0, 0.3, (600, 3)), a + rng.normal(0, 0.3, (600, 3))], 1).astype(F)
    tri[:, :, 0] = np.clip(tri[:, :, 0], 0, 1000); tri[:, :, 1:] = np.clip(tri[:, :, 1:], 0, 1)
    tri = tri[_in_tree(tri)]
    bad = np.array([[[500, 0.5, 0.5], [np.inf, 0.5, 0.6], [500, 0.6, 0.5]], [[2, 0.2, 0.2], [2.1, -np.inf, 0.2], [2, 0.2, 0.3]]], F)
    tri = np.concatenate([tri[:100], bad[:1], tri[100:], bad[1:]])
    V, T = _soup_mesh(tri)
    fin = V[np.isfinite(V).all(1)]
    assert fin[:, 0].max() > 990 and np.abs(fin[:, 1:]).max() <= 1
    q = lambda x0, x1, m: np.stack([rng.uniform(x0, x1, m), rng.uniform(-0.5, 1.5, m), rng.uniform(-0.5, 1.5, m)], 1)
    P = np.concatenate([q(-2, 3, 200), q(997, 1002, 200), q(3, 997, 200)]).astype(F)
    for max_sq in (np.inf, 4.0):
        d, _ = _check_min(e3d, P, V, T, max_sq)
        assert np.isfinite(d).sum() > 100


# ---- 5. any-hit at equality -----------------------------------------------------------------------------------------
GRID_N, GRID_H = 16, 0.25           # the flat mesh of the splat tests: [0, 4]^2 at z = 0, dyadic


def _lattice_cloud(z, m=10, start=1.03125, step=0.1875):
    """m x m points well inside the grid's border (dyadic coordinates: the splat radius is exactly `step`), one more with a
    NaN normal and one non-finite point"""
    ys, xs = np.meshgrid(start + step * np.arange(m), start + step * np.arange(m), indexing="ij")
    xyz = np.stack([xs, ys, np.full_like(xs, z)], -1).reshape(-1, 3).astype(F)
    xyz = np.concatenate([xyz, np.array([[0.5, 0.5, z], [np.nan, 2.0, z]], F)])
    xyz[:, 2] = F(z); xyz[-1, 0] = np.nan
    nrm = np.tile(UP, (xyz.shape[0], 1))
    nrm[-2] = [0, np.nan, 1]
    live = np.ones(xyz.shape[0], bool); live[-2:] = False
    return xyz, nrm, live


@pytest.mark.parametrize("t", [0.02, 0.03125])
def test_any_hit_threshold_exactly_at_the_distance(e3d, t):
    V, T = _flat_grid(GRID_N, GRID_H)
    t = F(t)
    xyz, nrm, live = _lattice_cloud(t)
    ga, gr, _ = _check_splats(e3d, xyz, nrm, V, T, t)
    assert not ga.any()                                                 # `<=`: a point at the threshold is within
    assert gr[live].min() == F(0.1875) and gr[live].max() == F(0.375)    # (inner points, the lattice's corners)
    up = np.nextafter(t, F(np.inf))
    assert F(up) * F(up) > t * t
    xyz, nrm, live = _lattice_cloud(up)
    ga, _, _ = _check_splats(e3d, xyz, nrm, V, T, t)
    assert np.array_equal(ga, live)                                     # one ulp above: every live point is splatted


def test_any_hit_threshold_zero_inf_nan(e3d):
    V, T = _flat_grid(GRID_N, GRID_H)
    # points exactly on the mesh: the interior grid vertices (every corner of their splats is a grid vertex too) ...
    inner = (V[:, 0] >= 0.75) & (V[:, 0] <= 3.25) & (V[:, 1] >= 0.75) & (V[:, 1] <= 3.25)
    xyz = V[inner]
    ga, _, _ = _check_splats(e3d, xyz, np.tile(UP, (xyz.shape[0], 1)), V, T, 0.0)
    assert not ga.any()                                                 # every value is exactly 0
    # ... and points whose projection is not a grid vertex
    xyz, nrm, live = _lattice_cloud(0.0, start=1.03, step=0.19)
    gb, _, _ = _check_splats(e3d, xyz, nrm, V, T, 0.0)
    assert gb[live].any() and not gb[live].all()                        # the computed face point is the query, or an ulp off
    for thr in (np.inf, np.nan):
        xyz, nrm, live = _lattice_cloud(0.5)
        ga, _, gv = _check_splats(e3d, xyz, nrm, V, T, thr)
        assert not ga.any() and gv.shape == (0, 3)


# ---- 6. frame selector and radius cap -------------------------------------------------------------------------------
def _frame_normals():
    e = F(1e-5)
    return np.array([[0, 0, 1], [0, 0, -1], [e, 0, 1], [np.nextafter(e, F(1)), 0, 1], [np.nextafter(e, F(0)), 0, 1], [0, e, 1],
                     [0, np.nextafter(e, F(1)), 1], [-e, 0, -1], [0, 3, 4], [0, 0, 0], [1, 0, 0], [0.6, 0, 0.8]], F)


@pytest.mark.parametrize("z", [0.3, 0.01])
def test_frames_and_radius_cap(e3d, z):
    """both unitOrthogonal branches and their boundary, an unnormalised and a zero normal; z = 0.3: every point is far, every
    frame reaches the output; z = 0.01: the centre is within, the corners of the frame decide"""
    V, T = _flat_grid(GRID_N, GRID_H)
    xyz, _, live = _lattice_cloud(z, m=12, start=0.96875, step=0.1875)
    N = _frame_normals()
    _, first = sr.unit_orthogonal(N)
    assert first[[3, 6, 8, 10, 11]].all() and not first[[0, 1, 2, 4, 5, 7, 9]].any()
    nrm = N[np.arange(xyz.shape[0]) % N.shape[0]]
    nrm[-2] = [0, np.nan, 1]
    with np.errstate(all="ignore"):
        r0 = np.nanmin(sr.splat_radius(xyz))                            # the inner points' radius (the border's is larger)
    assert r0 == F(0.1875)
    seen = set()
    for max_splat in (0.1, r0, np.inf, 0.0):
        ga, gr, gv = _check_splats(e3d, xyz, nrm, V, T, 0.02, max_splat)
        assert (gr[live] <= F(max_splat)).all() and gr[live].min() == min(F(max_splat), r0)
        seen.update(ga[live].tolist())
        if z == 0.3:
            assert np.array_equal(ga, live)
        elif max_splat == 0.0:                                          # radius 0: the corners are the centre, which is within
            assert np.array_equal(ga, live & ~nrm.any(1))               # (the zero normal's corners are 0 * NaN: not finite)
    assert seen == {True} if z == 0.3 else seen == {True, False}


def test_corners_overflow(e3d):
    """a point whose fifth neighbour is farther than sqrt(FLT_MAX): its radius is +inf (or the cap), its corners are not finite
    -- it is splatted although its centre is within the threshold"""
    V, T = _flat_grid(GRID_N, GRID_H)
    ys, xs = np.meshgrid(1.0e16 * np.arange(3), 3.0e19 + 1.0e16 * np.arange(3), indexing="ij")
    xyz = np.concatenate([np.array([[2.03, 2.03, 0.01]]), np.stack([xs, ys, np.zeros_like(xs)], -1).reshape(-1, 3)]).astype(F)
    nrm = np.tile(UP, (10, 1))
    ga, gr, gv = _check_splats(e3d, xyz, nrm, V, T, 0.02)
    assert ga.all() and np.isinf(gr[0]) and np.isfinite(gr[1:]).all()
    assert not np.isfinite(gv[:4]).all(1).any()
    # without its corners the near point is within: with max_splat = 0 it is the only one not splatted
    ga, _, _ = _check_splats(e3d, xyz, nrm, V, T, 0.02, 0.0)
    assert not ga[0] and ga[1:].all()
    ga, gr, gv = _check_splats(e3d, xyz, nrm, V, T, 0.02, 3.0e38)
    assert ga.all() and gr[0] == F(3.0e38)


# ---- 7. the C ABI directly ------------------------------------------------------------------------------------------
CANARY = 0xDEADBEEF


def _abi_case():
    V, T = _flat_grid(GRID_N, GRID_H)
    rng = np.random.default_rng(3)
    xyz, nrm, live = _lattice_cloud(0.01, m=12, start=0.96875, step=0.1875)
    xyz[:100, 2] = rng.choice([0.01, 0.3], 100).astype(F)              # about half are splatted
    nrm[:100] = _frame_normals()[rng.integers(0, 12, 100)]
    return xyz, nrm, V, T


def _raw_splats(L, xyz_p, nrm_p, n, V_p, nv, T, capacity, out_words):
    """e3d_create_splats into a uint32 buffer filled with the canary; out_words None: a null output"""
    buf = None if out_words is None else np.full(out_words, CANARY, np.uint32)
    flag = np.full(n + 8, 0xAB, np.uint8); rad = np.full(n + 8, CANARY, np.uint32)
    m = L.e3d_create_splats(xyz_p, nrm_p, n, V_p, nv, T.ctypes.data, T.shape[0], 0.02, float("inf"), None if buf is None else buf.ctypes.data,
                            capacity, flag.ctypes.data, rad.ctypes.data, None)
    assert (flag[n:] == 0xAB).all() and (rad[n:] == CANARY).all()
    return m, buf, flag[:n].copy(), rad[:n].copy()


def test_capacity_below_the_count(e3d):
    L = e3d.lib()
    xyz, nrm, V, T = _abi_case()
    n = xyz.shape[0]
    gv, _, ga, gr = e3d.create_splats(xyz, nrm, V, T, 0.02)
    count = int(ga.sum())
    assert 10 < count < n - 10
    full = np.ascontiguousarray(gv, F).view(np.uint32).reshape(-1)
    assert full.size == 12 * count
    for capacity in (0, 1, count - 1, count, count + 3):
        m, buf, flag, rad = _raw_splats(L, xyz.ctypes.data, nrm.ctypes.data, n, V.ctypes.data, V.shape[0], T, capacity, 12 * (count + 3) + 64)
        assert m == count                                               # the full count, whatever fits
        w = 12 * min(capacity, count)
        assert np.array_equal(buf[:w], full[:w])
        assert (buf[w:] == CANARY).all()
        assert np.array_equal(flag.astype(bool), ga) and np.array_equal(rad, _u32(gr))
    # capacity > 0 with a null output is refused; capacity 0 with a null output only counts
    m, _, _, _ = _raw_splats(L, xyz.ctypes.data, nrm.ctypes.data, n, V.ctypes.data, V.shape[0], T, 5, None)
    assert m < 0 and b"capacity" in L.e3d_last_error()
    m, _, flag, _ = _raw_splats(L, xyz.ctypes.data, nrm.ctypes.data, n, V.ctypes.data, V.shape[0], T, 0, None)
    assert m == count and np.array_equal(flag.astype(bool), ga)


def test_device_pointer_inputs(e3d):
    import torch
    L = e3d.lib()
    xyz, nrm, V, T = _abi_case()
    n = xyz.shape[0]
    gv, _, ga, gr = e3d.create_splats(xyz, nrm, V, T, 0.02)
    count = int(ga.sum())
    dx, dn, dv = (torch.from_numpy(a.copy()).cuda() for a in (xyz, nrm, V))
    torch.cuda.synchronize()
    words = 12 * count + 64
    runs = [_raw_splats(L, dx.data_ptr(), dn.data_ptr(), n, dv.data_ptr(), V.shape[0], T, count, words) for _ in range(2)]
    torch.cuda.synchronize()
    for m, buf, flag, rad in runs:
        assert m == count
        assert np.array_equal(buf[:12 * count], np.ascontiguousarray(gv, F).view(np.uint32).reshape(-1)) and (buf[12 * count:] == CANARY).all()
        assert np.array_equal(flag.astype(bool), ga) and np.array_equal(rad, _u32(gr))
    assert runs[0][1].tobytes() == runs[1][1].tobytes() and runs[0][3].tobytes() == runs[1][3].tobytes()
    for dev, host in ((dx, xyz), (dn, nrm), (dv, V)):                     # the inputs are unchanged
        assert dev.cpu().numpy().tobytes() == host.tobytes()
    # the binding with device tensors
    gv2, _, ga2, gr2 = e3d.create_splats(dx, dn, dv, T, 0.02)
    assert gv2.tobytes() == gv.tobytes() and np.array_equal(ga2, ga) and gr2.tobytes() == gr.tobytes()

    # e3d_mesh_squared_distance: queries and vertices on the device
    Vs, Ts, P = _shape_case(1025, 3)
    hd, hi = _check_min(e3d, P, Vs, Ts, 0.003)
    dq, dvs = torch.from_numpy(P.copy()).cuda(), torch.from_numpy(Vs.copy()).cuda()
    torch.cuda.synchronize()
    outs = []
    for _ in range(2):
        d = np.full(P.shape[0] + 8, CANARY, np.uint32); ids = np.full(P.shape[0] + 8, -7, np.int32)
        r = L.e3d_mesh_squared_distance(dq.data_ptr(), P.shape[0], dvs.data_ptr(), Vs.shape[0], Ts.ctypes.data, Ts.shape[0], 0.003,
                                        d.ctypes.data, ids.ctypes.data)
        assert r == 0
        assert (d[P.shape[0]:] == CANARY).all() and (ids[P.shape[0]:] == -7).all()
        outs.append((d, ids))
        assert np.array_equal(d[:P.shape[0]], _u32(hd)) and np.array_equal(ids[:P.shape[0]], hi)
    assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1].tobytes() == outs[1][1].tobytes()
    assert dq.cpu().numpy().tobytes() == P.tobytes()
    assert np.array_equal(np.isnan(dvs.cpu().numpy()), np.isnan(Vs)) and dvs.cpu().numpy().tobytes() == Vs.tobytes()
    d2, i2 = e3d.mesh_squared_distance(dq, dvs, Ts, 0.003)
    assert d2.tobytes() == hd.tobytes() and np.array_equal(i2, hi)
    # no ids wanted: a null closest_triangle
    d = np.zeros(P.shape[0], F)
    assert L.e3d_mesh_squared_distance(dq.data_ptr(), P.shape[0], dvs.data_ptr(), Vs.shape[0], Ts.ctypes.data, Ts.shape[0], 0.003,
                                       d.ctypes.data, None) == 0
    assert d.tobytes() == hd.tobytes()
