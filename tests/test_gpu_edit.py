"""The PointCloudEdit kernels (lasso, beyond-plane, pick, stable compaction) against tests/edit_ref.py.  Every comparison is
exact: flags with array_equal, pick distances as bits, coordinates as bits."""
import numpy as np
import pytest

import edit_ref as er

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 1000, 100_003, 3_000_000]
VIEWS = [(64, 48), (1280, 960)]


def lib_view(e3d, v):
    T = np.eye(4, dtype=np.float32)
    T[:3] = v.T
    return e3d.edit_view(v.width, v.height, T, float(v.min_depth), float(v.max_depth))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


_CLOUDS = {}


def random_case(n, width, height):
    """A cloud that fills the view and its surroundings, a pose with scale != 1, NaN / inf sprinkled in; made once per (n, view)."""
    key = (n, width, height)
    if key not in _CLOUDS:
        rng = np.random.RandomState(1000 + n % 9973 + width)
        z = rng.uniform(0.05, 130.0, n)
        cam = np.stack([rng.uniform(-0.8, 0.8, n) * z * width / height, rng.uniform(-0.8, 0.8, n) * z, z], 1)
        A = rng.normal(size=(3, 3))
        R, _ = np.linalg.qr(A)
        if np.linalg.det(R) < 0:
            R[:, 0] = -R[:, 0]
        s = rng.uniform(0.5, 2.0)
        t = rng.uniform(-1.0, 1.0, 3)
        xyz = (((cam - t) @ R) / s).astype(np.float32)
        if n >= 64:
            bad = rng.choice(n, 6, replace=False)
            xyz[bad[0], 0] = np.nan; xyz[bad[1], 2] = np.nan; xyz[bad[2], 1] = np.inf; xyz[bad[3], 2] = -np.inf
            xyz[bad[4]] = np.nan; xyz[bad[5], 2] = np.inf
        T = np.concatenate([s * R, t[:, None]], 1).astype(np.float32)
        _CLOUDS[key] = (xyz, er.make_view(width, height, T))
    return _CLOUDS[key]


def random_polygon(rng, width, height):
    m = rng.randint(3, 41)
    return np.stack([rng.uniform(-0.2 * width, 1.2 * width, m), rng.uniform(-0.2 * height, 1.2 * height, m)], 1)


# ---- lasso: ties --------------------------------------------------------------------------------------------------------------------
TIE_W, TIE_H = 48, 64
TIE_POLYGONS = {
    "triangle": [(4, 4), (44, 4), (4, 44)],
    "concave": [(2, 2), (46, 2), (46, 62), (24, 40), (2, 62)],
    "bow_tie": [(4, 4), (44, 44), (44, 4), (4, 44)],
    "horizontal_edges": [(8, 8), (40, 8), (40, 24), (30, 24), (30, 40), (40, 40), (40, 56), (8, 56)],
    "partly_outside": [(-20, 10), (30, 10), (60, 40), (30, 70), (-20, 70)],
}


def tie_cloud():
    """Identity pose, fx = fy = 64: x = k z / 64, y = m z / 64 at z in {1, 2, 4} has the exact pixel (k + 24, m + 32).  z = 1 and
    z = 4 are the two ends of the depth range; some points lie just outside it, behind the camera, or are NaN / inf."""
    k, m, z = np.meshgrid(np.arange(-30, 31), np.arange(-36, 37), np.array([1.0, 2.0, 4.0]), indexing="ij")
    k, m, z = k.ravel().astype(np.float32), m.ravel().astype(np.float32), z.ravel().astype(np.float32)
    xyz = np.stack([k * z / 64, m * z / 64, z], 1).astype(np.float32)
    one, four = np.float32(1), np.float32(4)
    extra = np.array([[0, 0, np.nextafter(one, np.float32(0))], [0, 0, np.nextafter(four, np.float32(9))], [0, 0, -1], [0.1, 0.1, -2], [0, 0, 0],
                      [np.nan, 0, 2], [0, np.nan, 2], [0, 0, np.nan], [np.inf, 0, 2], [0, -np.inf, 2], [0, 0, np.inf], [0, 0, -np.inf]], np.float32)
    rng = np.random.RandomState(5)
    xyz = np.vstack([xyz, extra])
    return xyz[rng.permutation(len(xyz))], er.make_view(TIE_W, TIE_H, None, 1.0, 4.0)


@pytest.mark.parametrize("name", sorted(TIE_POLYGONS))
def test_lasso_ties(e3d, name):
    xyz, view = tie_cloud()
    polygon = TIE_POLYGONS[name]
    in_range, px, py, _ = er.project(view, xyz)
    assert np.array_equal(px[in_range], np.round(px[in_range])) and np.array_equal(py[in_range], np.round(py[in_range]))
    on = in_range & er.points_on_boundary(px, py, polygon)
    assert on.sum() >= 0.01 * len(xyz), on.sum()                  # the ties are really there
    ref = er.lasso(view, xyz, polygon)
    assert 0 < ref[on].sum() < on.sum()                            # and the rule splits them
    E = e3d.PointCloudEdit(xyz)
    assert E.lasso(lib_view(e3d, view), polygon) == ref.sum()
    assert np.array_equal(E.selection(), ref)


# ---- lasso: random clouds, poses, polygons; the three modes -------------------------------------------------------------------------
@pytest.mark.parametrize("width, height", VIEWS)
@pytest.mark.parametrize("n", SIZES)
def test_lasso_random(e3d, n, width, height):
    xyz, view = random_case(n, width, height)
    rng = np.random.RandomState(n % 1000 + height)
    V = lib_view(e3d, view)
    E = e3d.PointCloudEdit(xyz)
    assert len(E) == n and E.selection_count() == 0
    ref = np.zeros(n, bool)
    for mode in ("replace", "add", "remove", "replace"):
        polygon = random_polygon(rng, width, height)
        ref = er.lasso(view, xyz, polygon, mode, ref)
        assert E.lasso(V, polygon, mode) == ref.sum() == E.selection_count()
        assert np.array_equal(E.selection(), ref), mode
    if n >= 1000:
        assert 0 < ref.sum() < n


def test_lasso_polygon_sizes(e3d):
    xyz, view = random_case(1000, 64, 48)
    V = lib_view(e3d, view)
    E = e3d.PointCloudEdit(xyz)
    before = np.arange(1000) % 3 == 0
    assert E.set_selection(before) == before.sum()
    for small in ([], [(0, 0)], [(0, 0), (64, 48)]):
        assert E.lasso(V, np.array(small, np.float64).reshape(-1, 2), "replace") == before.sum()
        assert np.array_equal(E.selection(), before)              # fewer than 3 vertices: the selection stays
    a = np.linspace(0, 2 * np.pi, 1024, endpoint=False)
    star = np.stack([32 + (20 + 10 * np.cos(9 * a)) * np.cos(a), 24 + (15 + 8 * np.cos(9 * a)) * np.sin(a)], 1)
    ref = er.lasso(view, xyz, star)
    assert E.lasso(V, star) == ref.sum() and ref.sum() > 0
    assert np.array_equal(E.selection(), ref)
    with pytest.raises(e3d.E3DError):
        E.lasso(V, np.vstack([star, star[:1]]))                   # 1025 vertices
    assert np.array_equal(E.selection(), ref)
    with pytest.raises(e3d.E3DError):
        E.lasso(V, star, 3)


def test_lasso_depth_gate(e3d):
    """Per pixel column one kind of depth value; points at z = 100 and z = 50, where 0.99f * z is exactly 99 and 49.5."""
    W, H = 8, 8
    view = er.make_view(W, H, None, 1.0, 200.0)
    assert np.float32(0.99) * np.float32(100) == np.float32(99) and np.float32(0.99) * np.float32(50) == np.float32(49.5)
    pts = []
    for z in (100.0, 50.0):
        for px in range(-1, W + 1):                               # one column beyond each border: clamped to the image
            for py in range(-1, H + 1):
                pts.append([(px - 4) * z / 8, (py - 4) * z / 8, z])
    xyz = np.array(pts, np.float32)
    in_range, px, py, _ = er.project(view, xyz)
    assert in_range.all() and np.array_equal(px, np.round(px)) and px.min() == -1 and px.max() == W
    whole = [(-3, -3), (W + 3, -3), (W + 3, H + 3), (-3, H + 3)]
    V = lib_view(e3d, view)
    E = e3d.PointCloudEdit(xyz)
    seen = set()
    for scale in (100.0, 50.0):
        column = np.array([0.99 * scale - 0.25, 0.99 * scale, 0.99 * scale + 0.25, np.inf, np.nan, -np.inf, 1e-3, 1e6], np.float32)
        assert column[1] == np.float32(0.99) * np.float32(scale)
        depth = np.tile(column, (H, 1))
        ref = er.lasso(view, xyz, whole, depth=depth)
        seen.add(tuple(ref[(xyz[:, 2] == scale) & (py == 3) & (px >= 0) & (px < W)].tolist()))
        assert E.lasso(V, whole, "replace", depth) == ref.sum()
        assert np.array_equal(E.selection(), ref)
    assert seen == {(False, True, True, True, True, True, False, True)}      # below / equal / above / +inf / NaN / -inf / near / far
    assert E.lasso(V, whole) == len(xyz)                          # without the image every point is taken


# ---- beyond-plane ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width, height", VIEWS)
@pytest.mark.parametrize("n", SIZES)
def test_beyond_plane_random(e3d, n, width, height):
    xyz, view = random_case(n, width, height)
    V = lib_view(e3d, view)
    E = e3d.PointCloudEdit(xyz)
    finite = xyz[np.isfinite(xyz).all(1)]
    centre = finite.mean(0) if len(finite) else np.zeros(3, np.float32)
    pts = np.array([centre, centre + [1, 0.2, 0], centre + [0.1, 1, 0.3]], np.float32)
    for camera in ([0, 0, 1000], [0, 0, -1000]):                  # the camera on either side
        for limit in (False, True):
            ref = er.beyond_plane(view, xyz, pts, camera, limit)
            assert E.beyond_plane(V, pts, camera, limit) == ref.sum() == E.selection_count()
            assert np.array_equal(E.selection(), ref), (camera, limit)
    if n >= 1000:
        a = er.beyond_plane(view, xyz, pts, [0, 0, 1000])
        b = er.beyond_plane(view, xyz, pts, [0, 0, -1000])
        assert a.sum() > 0 and b.sum() > 0 and not (a & b).any()


def test_beyond_plane_ties_and_borders(e3d):
    """Identity pose, H = 64: exact pixels.  The plane z = 2 holds a third of the points (distance exactly 0: not selected); points on
    the window's right and bottom borders (pixel == width, pixel == height) are not visible, those on the left and top ones are."""
    xyz, view = tie_cloud()
    V = lib_view(e3d, view)
    E = e3d.PointCloudEdit(xyz)
    pts = np.array([[0, 0, 2], [1, 0, 2], [0, 1, 2]], np.float32)
    in_range, px, py, _ = er.project(view, xyz)
    for camera, side in (([0, 0, 0], xyz[:, 2] > 2), ([0, 0, 9], xyz[:, 2] < 2)):
        ref = er.beyond_plane(view, xyz, pts, camera)
        assert np.array_equal(ref, side)                          # z == 2 and NaN are on neither side
        assert E.beyond_plane(V, pts, camera) == ref.sum()
        assert np.array_equal(E.selection(), ref)
        vis = er.beyond_plane(view, xyz, pts, camera, True)
        inside = in_range & (px >= 0) & (px < TIE_W) & (py >= 0) & (py < TIE_H)
        assert np.array_equal(vis, side & inside)
        assert (side & in_range & (px == TIE_W)).any() and (side & in_range & (py == TIE_H)).any() and (vis & (px == 0)).any() and (vis & (py == 0)).any()
        assert E.beyond_plane(V, pts, camera, True) == vis.sum()
        assert np.array_equal(E.selection(), vis)
    for line in ([[0, 0, 0], [1, 1, 1], [2, 2, 2]], [[1, 2, 3], [1, 2, 3], [4, 5, 6]]):
        with pytest.raises(e3d.E3DError):
            E.beyond_plane(V, np.array(line, np.float32), [0, 0, 0])
    assert np.array_equal(E.selection(), vis)                      # an error leaves the selection


# ---- pick -----------------------------------------------------------------------------------------------------------------------------
def test_pick_ties(e3d):
    xyz, view = tie_cloud()
    clicks = [(24, 32), (0, 0), (47.5, 63.5), (10.25, 20.75), (-100, 5), (24, 1000), (30, 30), (12.5, 12.5)]       # eight at once
    idx, dist = er.pick(view, xyz, clicks)
    in_range, px, py, _ = er.project(view, xyz)
    assert (in_range & (px == 24) & (py == 32)).sum() == 3 and dist[0] == 0          # three depths share the pixel
    assert idx[0] == np.flatnonzero(in_range & (px == 24) & (py == 32)).min()        # the lowest index wins
    g_idx, g_dist = e3d.PointCloudEdit(xyz).pick(lib_view(e3d, view), clicks)
    assert np.array_equal(g_idx, idx)
    assert np.array_equal(bits(g_dist), bits(dist))


@pytest.mark.parametrize("width, height", VIEWS)
@pytest.mark.parametrize("n", SIZES)
def test_pick_random(e3d, n, width, height):
    xyz, view = random_case(n, width, height)
    rng = np.random.RandomState(n % 777 + width)
    clicks = np.stack([rng.randint(0, width, 8), rng.randint(0, height, 8)], 1).astype(np.float64)
    clicks[5:] += rng.uniform(-3, 3, (3, 2))
    E = e3d.PointCloudEdit(xyz)
    for m in (8, 1):
        idx, dist = er.pick(view, xyz, clicks[:m])
        g_idx, g_dist = E.pick(lib_view(e3d, view), clicks[:m])
        assert np.array_equal(g_idx, idx)
        assert np.array_equal(bits(g_dist), bits(dist))
    if n >= 1000:
        assert (idx >= 0).all()
    # no point in range: -1 and +inf
    far = er.make_view(width, height, np.vstack([view.T, [0, 0, 0, 1]]), 1e6, 2e6)
    g_idx, g_dist = E.pick(lib_view(e3d, far), clicks)
    assert (g_idx == -1).all() and np.isposinf(g_dist).all()
    assert np.array_equal(er.pick(far, xyz, clicks)[0], g_idx)
    with pytest.raises(e3d.E3DError):
        E.pick(lib_view(e3d, view), np.zeros((9, 2)))


# ---- compaction -----------------------------------------------------------------------------------------------------------------------
def _pattern(name, n):
    f = np.zeros(n, bool)
    if name == "full":
        f[:] = True
    elif name == "alternating":
        f[::2] = True
    elif name == "run":                                           # one run over every block boundary, a few points free at either end
        f[min(3, n):max(n - 3, 0)] = True
    elif name == "sparse":
        f[np.random.RandomState(n % 100).rand(n) < 0.07] = True
    return f


@pytest.mark.parametrize("pattern", ["empty", "full", "alternating", "run", "sparse"])
@pytest.mark.parametrize("n", SIZES)
def test_compaction(e3d, n, pattern):
    xyz, _ = random_case(n, 64, 48)
    flags = _pattern(pattern, n)
    E = e3d.PointCloudEdit(xyz)
    assert E.set_selection(flags.astype(np.uint8) * 255) == flags.sum() == E.selection_count()       # any non-zero byte selects
    assert np.array_equal(E.selection(), flags)
    moved = E.extract_selected()
    assert moved.shape == (flags.sum(), 3) and np.array_equal(bits(moved), bits(xyz[flags]))
    assert len(E) == n and np.array_equal(E.selection(), flags)   # extracting changes nothing
    assert E.delete_selected() == n - flags.sum() == len(E)
    assert E.selection_count() == 0 and not E.selection().any()
    assert np.array_equal(bits(E.points()), bits(xyz[~flags]))
    # the handle goes on working on the smaller cloud
    if len(E):
        again = np.arange(len(E)) % 5 == 1
        E.set_selection(again)
        assert E.delete_selected() == (~again).sum()
        assert np.array_equal(bits(E.points()), bits(xyz[~flags][~again]))
