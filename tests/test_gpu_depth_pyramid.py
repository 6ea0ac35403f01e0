"""e3d_reg_set_depth_map_level0: one full-resolution depth map goes in, the library sanitises it and builds the depth pyramid on the
device.  The header defines the arithmetic so that it can be restated in numpy bit for bit:

  level 0      valid iff finite and > 0, everything else becomes +0.0f;
  level l + 1  (float)(0.25 * ((((double)a + b) + c) + d)) over the 2 x 2 block, source coordinates clamped to the last row / column;
  strict       a block with a 0 gives +0.0f.

Every comparison here is np.array_equal on the bit patterns (so -0 and +0 differ).  The level sizes come from the camera pyramid
(int(0.5 w + 0.5)); the sizes cover widths that are no multiple of 4 (the pixel-by-pixel path), odd sizes at several levels in a row
and a single-pixel tail."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

AVERAGE, STRICT = 0, 1
SIZES = [(2, 2, 2), (3, 3, 2), (5, 4, 3), (64, 48, 3), (66, 50, 3), (127, 95, 4), (640, 480, 4), (1031, 517, 5)]
FLT_MAX = np.finfo(np.float32).max
DENORMAL = np.float32(1e-42)            # a positive subnormal f32: valid, to be kept


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _sanitise(d):
    d = np.ascontiguousarray(d, np.float32)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(d) & (d > 0)
    return np.where(ok, d, np.float32(0)).astype(np.float32)


def _down(p, w1, h1, mode):
    h, w = p.shape
    y0 = 2 * np.arange(h1); y1 = np.minimum(y0 + 1, h - 1)
    x0 = 2 * np.arange(w1); x1 = np.minimum(x0 + 1, w - 1)
    q = p.astype(np.float64)
    a, b, c, d = q[np.ix_(y0, x0)], q[np.ix_(y0, x1)], q[np.ix_(y1, x0)], q[np.ix_(y1, x1)]
    out = (0.25 * (((a + b) + c) + d)).astype(np.float32)
    if mode == STRICT:
        out[(a == 0) | (b == 0) | (c == 0) | (d == 0)] = np.float32(0)
    return out


def _pyramid(depth, sizes, mode):
    """sizes: [(w, h)] per level, from the camera pyramid.  Chained through f32 level by level."""
    levels = [_sanitise(depth)]
    for w1, h1 in sizes[1:]:
        levels.append(_down(levels[-1], w1, h1, mode))
    return levels


def _problem(e3d, w, h, n_levels):
    P = e3d.RegProblem(e3d.default_reg_params(image_scale_count=n_levels))
    P.set_intrinsics(0, w, h, np.array([0.9 * w, 0.9 * w, 0.5 * w - 0.5, 0.5 * h - 0.5], np.float32), 0, n_levels)
    sizes = [P.intrinsics_level(0, l)[:2] for l in range(n_levels)]
    P.set_image(0, 0, [np.zeros((sh, sw), np.uint8) for sw, sh in sizes])          # the depth maps do not look at the pixels
    assert sizes[0] == (w, h) and all(sizes[l + 1] == ((sizes[l][0] + 1) // 2, (sizes[l][1] + 1) // 2) for l in range(n_levels - 1))
    return P, sizes


def _random_depth(w, h, seed):
    rng = np.random.RandomState(seed)
    d = rng.uniform(0.3, 40.0, (h, w)).astype(np.float32)
    bad = np.array([0.0, -0.0, -1.0, np.nan, np.inf, -np.inf], np.float32)
    m = rng.uniform(size=(h, w)) < 0.05
    d[m] = bad[rng.randint(0, len(bad), int(m.sum()))]
    flat, at = d.reshape(-1), rng.permutation(w * h)
    flat[at[0]] = FLT_MAX
    flat[at[1]] = DENORMAL
    if w * h >= 16:                  # and every invalid value at least once
        flat[at[2:2 + len(bad)]] = bad
    return d


def _check(P, sizes, depth, mode):
    P.set_depth_map_level0(0, depth, mode)
    got = P.get_depth_maps(0)
    want = _pyramid(depth, sizes, mode)
    assert len(got) == len(want) == len(sizes)
    for l, (g, e) in enumerate(zip(got, want)):
        assert g.shape == e.shape == (sizes[l][1], sizes[l][0])
        assert np.array_equal(_bits(g), _bits(e)), (l, int((_bits(g) != _bits(e)).sum()))
    return got


@pytest.mark.parametrize("mode", [AVERAGE, STRICT])
@pytest.mark.parametrize("w,h,n_levels", SIZES)
def test_depth_pyramid_equals_numpy_restatement(e3d, w, h, n_levels, mode):
    P, sizes = _problem(e3d, w, h, n_levels)
    depth = _random_depth(w, h, seed=w * 7 + h)
    got = _check(P, sizes, depth, mode)
    # the valid extremes survive level 0 untouched, the invalid values are +0
    assert FLT_MAX in got[0] and (got[0] == DENORMAL).any()
    with np.errstate(invalid="ignore"):
        invalid = ~(np.isfinite(depth) & (depth > 0))
    assert not _bits(got[0])[invalid].any() and np.array_equal(_bits(got[0])[~invalid], _bits(depth)[~invalid])
    # a rectangular hole that touches the right and bottom borders (the clamped last row / column replicate it)
    hole = np.random.RandomState(5).uniform(1.0, 9.0, (h, w)).astype(np.float32)
    hole[h // 2:, w // 3:] = np.inf
    got = _check(P, sizes, hole, mode)
    assert not got[0][h // 2:, w // 3:].any() and got[0][:h // 2].all()
    if mode == STRICT:
        assert all(g[-1, -1] == 0 for g in got)                                   # the hole keeps its corner at every level
    else:
        assert got[1][-1, 0] > 0                                                  # the column left of the hole keeps a mean
    # nothing valid at all
    got = _check(P, sizes, np.full((h, w), -np.inf, np.float32), mode)
    assert all(not _bits(g).any() for g in got)


@pytest.mark.parametrize("w,h,n_levels", SIZES)
def test_hole_modes_agree_without_holes(e3d, w, h, n_levels):
    P, sizes = _problem(e3d, w, h, n_levels)
    depth = np.random.RandomState(w + h).uniform(0.5, 30.0, (h, w)).astype(np.float32)
    a = _check(P, sizes, depth, AVERAGE)
    b = _check(P, sizes, depth, STRICT)
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))
    assert np.array_equal(_bits(a[0]), _bits(depth))
    # the default of the binding is the strict mode
    P.set_depth_map_level0(0, depth)
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(P.get_depth_maps(0), b))


def test_depth_residuals_equal_those_of_a_caller_built_pyramid(e3d):
    """An all-valid map on even sizes: depth_accumulate and depth_cost after set_depth_map_level0 equal those after set_depth_maps
    with the numpy pyramid exactly -- both paths hold the same buffers and run the same kernels."""
    from reg_util import make_multi_image_scene, plane_depth_pyramid
    M = make_multi_image_scene(n_points=5000, n_images=2, seed=31, perturb=0.004)          # 240 x 180, 3 levels
    sizes = [(240, 180), (120, 90), (60, 45)]

    def build():
        P = e3d.RegProblem(e3d.default_reg_params(image_scale_count=M["n_levels"], point_neighbor_count=M["K"], depth_residuals_weight=1.0))
        P.set_intrinsics(0, M["width"], M["height"], M["params"], 0, M["n_levels"])
        P.set_point_scale(0, M["pts"], M["point_radius"], M["nbr"], M["fixed_desc"])
        P.set_splat_points(M["pts"])
        for i, im in enumerate(M["images"]):
            P.set_image(i, 0, im["pyr"]); P.set_image_pose(i, im["q_init"], im["t_init"])
        return P

    A, B = build(), build()
    for i, im in enumerate(M["images"]):
        level0 = plane_depth_pyramid(M, im)[0]
        assert np.isfinite(level0).all() and (level0 > 0).all()
        A.set_depth_map_level0(i, level0, STRICT if i else AVERAGE)
        B.set_depth_maps(i, _pyramid(level0, sizes, AVERAGE))
        for g, e in zip(A.get_depth_maps(i), B.get_depth_maps(i)):          # get_depth_maps reads back either route
            assert np.array_equal(_bits(g), _bits(e))
    A.update_observations(1); B.update_observations(1)
    for i in range(2):
        Ha, ba, sa, ca = A.depth_accumulate(i, 0)
        Hb, bb, sb, cb = B.depth_accumulate(i, 0)
        assert ca == cb and ca > 1000 and sa == sb and np.array_equal(Ha, Hb) and np.array_equal(ba, bb)
        assert A.depth_cost(i, 0) == B.depth_cost(i, 0)


def test_depth_map_level0_errors(e3d):
    P, sizes = _problem(e3d, 66, 50, 3)
    depth = np.ones((50, 66), np.float32)
    with pytest.raises(e3d.E3DError, match="no depth maps"):
        P.get_depth_maps(0)                                              # get before set
    with pytest.raises(e3d.E3DError, match="image 7 not set"):
        P.set_depth_map_level0(7, depth)                                 # unknown image
    with pytest.raises(e3d.E3DError, match="image 7 not set"):
        P.get_depth_maps(7)
    for mode in (-1, 2):
        with pytest.raises(e3d.E3DError, match="hole mode"):
            P.set_depth_map_level0(0, depth, mode)
    with pytest.raises(e3d.E3DError):
        P.set_depth_map_level0(0, np.ones((50, 64), np.float32))         # not the camera's size
    lib = e3d.lib()
    assert lib.e3d_reg_set_depth_map_level0(P._h, 0, None, STRICT) < 0 and lib.e3d_reg_set_depth_map_level0(None, 0, depth.ctypes.data, STRICT) < 0
    P.set_depth_map_level0(0, depth)
    assert [m.shape for m in P.get_depth_maps(0)] == [(50, 66), (25, 33), (13, 17)]
    for level in (-1, 3):
        with pytest.raises(e3d.E3DError, match="level"):
            P.get_depth_map(0, level)
    out = np.zeros(4, np.float32)
    assert lib.e3d_reg_get_depth_map(P._h, 0, 0, None) < 0 and lib.e3d_reg_get_depth_map(None, 0, 0, out.ctypes.data) < 0
    P.set_depth_maps(0, None)                                            # removing them is the existing call's
    with pytest.raises(e3d.E3DError, match="no depth maps"):
        P.get_depth_maps(0)
