"""GPU parity tests of the multi-resolution point cloud construction against the CPU oracle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mr():
    from oracle import multires
    multires.lib()
    return multires


def _scan_like(n, seed, spacing=0.004):
    """points on two walls in scan-line order (structured input: long greedy dependency chains) + noise"""
    rng = np.random.RandomState(seed)
    side = int(np.sqrt(n / 2))
    u, v = np.meshgrid(np.arange(side) * spacing, np.arange(side) * spacing, indexing="ij")
    a = np.stack([u.ravel(), v.ravel(), np.zeros(side * side)], 1)
    b = np.stack([np.zeros(side * side), u.ravel(), v.ravel() + 0.3], 1)
    P = np.concatenate([a, b]) + rng.normal(0, spacing * 0.15, (2 * side * side, 3))
    return P.astype(np.float32)


@pytest.mark.parametrize("n,dist,scans", [(20000, 0.009, 1), (60000, 0.013, 3), (3000, 0.5, 2)])
def test_merge_close_points_matches_oracle(e3d, mr, n, dist, scans):
    rng = np.random.RandomState(n)
    P = _scan_like(n, n)
    col = rng.uniform(0, 255, len(P)).astype(np.float32)
    sidx = rng.randint(0, scans, len(P)).astype(np.uint8)
    mxr = rng.uniform(0.001, 0.1, len(P)).astype(np.float32)
    g = e3d.merge_close_points(dist, scans, P, col, sidx, mxr)
    o = mr.merge_close_points(dist, scans, P, col, sidx, mxr)
    assert len(g[0]) == len(o[0]) and len(g[0]) < len(P)                       # the same centres, in the same order
    assert np.array_equal(g[2], o[2])                                          # majority scan incl. the tie rule
    assert np.array_equal(g[3].view(np.uint32), o[3].view(np.uint32))          # max of max_radius: exact
    assert np.abs(g[0] - o[0]).max() <= 1e-5 * max(1.0, np.abs(P).max())       # f32 means, different summation order
    assert np.abs(g[1] - o[1]).max() <= 1e-3


def test_merge_close_points_edge_cases(e3d, mr):
    P = np.array([[0, 0, 0]], np.float32)
    g = e3d.merge_close_points(0.1, 1, P, np.array([7], np.float32), np.array([0], np.uint8), np.array([0.5], np.float32))
    assert len(g[0]) == 1 and np.array_equal(g[0][0], P[0]) and g[1][0] == 7 and g[3][0] == 0.5
    # duplicates and a strict radius: points exactly merge_distance apart are NOT merged
    P = np.array([[0, 0, 0], [0, 0, 0], [0.5, 0, 0], [1.0, 0, 0]], np.float32)
    args = (np.arange(4, dtype=np.float32), np.zeros(4, np.uint8), np.ones(4, np.float32))
    g = e3d.merge_close_points(0.5, 1, P, *args); o = mr.merge_close_points(0.5, 1, P, *args)
    assert len(g[0]) == len(o[0]) == 3 and np.allclose(g[0], o[0])
    with pytest.raises(e3d.E3DError):
        e3d.merge_close_points(0.0, 1, P, *args)
    with pytest.raises(e3d.E3DError):
        e3d.merge_close_points(0.1, 99, P, *args)


@pytest.mark.parametrize("model", [0, 1, 2, 3, 4, 10, 11, 12])
def test_point_radius_minmax_matches_oracle(e3d, mr, model):
    from reg_util import make_multi_image_scene
    M = make_multi_image_scene(n_points=8000, n_images=3, seed=21, model=model)
    G = e3d.RegProblem(e3d.default_reg_params(image_scale_count=M["n_levels"], point_neighbor_count=M["K"]))
    G.set_intrinsics(0, M["width"], M["height"], M["params"], 0, M["n_levels"], camera_type=model)
    G.set_splat_points(M["pts"])
    images = {}
    for i, im in enumerate(M["images"]):
        G.set_image(i, 0, im["pyr"]); G.set_image_pose(i, im["q_true"], im["t_true"])
        images[i] = dict(intr=0, pyr=im["pyr"], masks=None, q=im["q_true"], t=im["t_true"])
    intr = {0: dict(w=M["width"], h=M["height"], params=M["params"], min=0, n=M["n_levels"], model=model)}
    # some points far outside every frustum stay unobserved
    pts = np.concatenate([M["pts"], np.array([[50, 3, 0], [0, -5, 0]], np.float32)])
    gmn, gmx = G.point_radius_minmax(pts)
    omn, omx = mr.point_radius_minmax(pts, images, intr, M["pts"], M["n_levels"])
    seen_o = np.isfinite(omn)
    assert np.array_equal(np.isfinite(gmn), seen_o) and seen_o[:-2].sum() > 4000 and not seen_o[-2:].any()
    assert np.array_equal(np.isfinite(gmx), np.isfinite(omx))
    tol = 1e-6                      # every model: shared elementary functions (include/e3d_libm.h)
    assert np.abs(gmn[seen_o] - omn[seen_o]).max() <= tol * omn[seen_o].max()
    assert np.abs(gmx[seen_o] - omx[seen_o]).max() <= tol * omx[seen_o].max()
    # sanity of the magnitude: half a pixel at depth z and focal length f is about z / (2 f)
    assert 0.5 * 2.5 / 210 / 2 < np.median(gmn[seen_o]) < 2 * 3.5 / 210 / 2


# ---- MergeClosePoints against the brute-force restatement (tests/multires_ref.py) ---------------------------------------------------
# tests/test_multires_host.py shows on the CPU that these inputs tell a closed radius, another tie rule and another absorption rule
# apart, and that the restatement equals the oracle bit for bit on each of them.
def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def _check_against_restatement(e3d, name, exact):
    """Always exact: the number of outputs, out_scan, out_max_radius (a wrong or reordered centre shows in them and in the means).
    Means: bit for bit where the f32 sums are exact, else within g(m) max|x_j| (g(c) max|col_j|) of the f64 mean -- derived in
    multires_ref.gamma, not measured."""
    import multires_ref as ref
    R = ref.reference(name)
    g = e3d.merge_close_points(*ref.case(name))
    assert [len(a) for a in g] == [len(R["m"])] * 4 and g[0].shape == (len(R["m"]), 3)
    assert np.array_equal(g[2], R["scan"])
    assert np.array_equal(_bits(g[3]), _bits(R["mxr"]))
    rp, rc = ref.mean_deviation_ratios(g[0], g[1], R)
    print("%s: %d centres, m <= %d, deviation / bound: position %.3g, colour %.3g" % (name, len(R["m"]), R["m"].max() if len(R["m"]) else 0, rp, rc))
    assert rp <= 1.0 and rc <= 1.0
    if exact:
        assert np.array_equal(_bits(g[0]), _bits(R["xyz"])) and np.array_equal(_bits(g[1]), _bits(R["col"]))
    return g, R


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 255, 256, 257, 1000])
def test_merge_sizes_at_wave_and_block_boundaries(e3d, n):
    g, R = _check_against_restatement(e3d, "size_%d" % n, exact=False)
    if n == 0:
        assert g[0].shape == (0, 3) and g[1].shape == g[2].shape == g[3].shape == (0,)
    if n >= 63:
        assert 1 < len(g[0]) < n


@pytest.mark.parametrize("name", ["lattice", "lattice_m64", "lattice_p4096"])
def test_merge_lattice_exact(e3d, name):
    """pairs at exactly the merge distance, duplicates, integer colours; also in negative coordinates and 4096 away from the origin"""
    g, R = _check_against_restatement(e3d, name, exact=True)
    assert R["m"].max() <= 32                  # the sums stay exact


@pytest.mark.parametrize("C", [1, 32, 33, 64, 65, 1024, 1025])
def test_merge_hash_table_size_edges(e3d, C):
    """exactly C occupied grid cells, a pair to merge in each (tests/test_multires_host.py proves it of the input): the table is the
    smallest power of two >= 64 and >= 2 C, and at these C twice the count meets and crosses one, the 64-slot floor included"""
    g, R = _check_against_restatement(e3d, "cells_%d" % C, exact=True)
    assert len(g[0]) == C and (R["m"] == 2).all()


def test_merge_lattice_far_from_the_origin(e3d):
    """the same sites around (2^17, -2^17, 2^17 - 3): the cell size is dominated by 16 FLT_EPSILON * magnitude, the sums round"""
    import multires_ref as ref
    g, R = _check_against_restatement(e3d, "lattice_far", exact=False)
    assert np.array_equal(g[2], ref.reference("lattice")["scan"]) and len(g[0]) == len(ref.reference("lattice")["m"])


@pytest.mark.parametrize("order", ["increasing", "decreasing", "shuffled"])
def test_merge_chain(e3d, order):
    """a line on which every decision waits for the one before it"""
    import multires_ref as ref
    g, R = _check_against_restatement(e3d, "chain_" + order, exact=True)
    if order == "increasing":                  # closed form: the even positions, the ends aside each the mean of three points
        P = ref.case("chain_increasing")[2]
        assert len(g[0]) == ref.CHAIN_N // 2 and np.array_equal(g[0][1:], P[2::2]) and np.array_equal(g[0][0], (P[0] + P[1]) / 2)


def test_merge_dense_neighbourhoods(e3d):
    """more than kMergeList lower-index neighbours, the deciding centre in the own wave and in other blocks"""
    g, R = _check_against_restatement(e3d, "dense", exact=False)
    assert R["m"].max() > 300


def test_merge_sixteen_scans(e3d):
    g, R = _check_against_restatement(e3d, "scans16", exact=False)
    assert len(set(g[2].tolist())) == 16
    g, R = _check_against_restatement(e3d, "scans16_all15", exact=False)
    assert (g[2] == 15).all()


def test_merge_twice_same_bytes(e3d):
    import multires_ref as ref
    for name in ("size_1000", "dense", "scans16"):
        a = e3d.merge_close_points(*ref.case(name)); b = e3d.merge_close_points(*ref.case(name))
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _good_70():
    import multires_ref as ref
    dist, scans, P, col, sidx, mxr = ref.case("size_1000")
    return dist, scans, P[:70].copy(), col[:70].copy(), sidx[:70].copy(), mxr[:70].copy()


def _refused_then_good(e3d, bad_args, good_args, good_bytes):
    with pytest.raises(e3d.E3DError):
        e3d.merge_close_points(*bad_args)
    assert [a.tobytes() for a in e3d.merge_close_points(*good_args)] == good_bytes


def test_merge_refuses_non_finite_coordinates(e3d):
    """the reference defines none of these; a NaN point would become a centre without neighbours, an infinite one collapses the grid"""
    good = _good_70()
    good_bytes = [a.tobytes() for a in e3d.merge_close_points(*good)]
    for value in (np.nan, np.inf, -np.inf):
        for axis in range(3):
            for index in (0, 37, 69):
                P = good[2].copy(); P[index, axis] = value
                _refused_then_good(e3d, (good[0], good[1], P) + good[3:], good, good_bytes)


def test_merge_refuses_scan_indices_beyond_num_scans(e3d):
    good = _good_70()
    good_bytes = [a.tobytes() for a in e3d.merge_close_points(*good)]
    for value in (good[1], 255):
        for index in (0, 37, 69):
            sidx = good[4].copy(); sidx[index] = value
            _refused_then_good(e3d, good[:4] + (sidx,) + good[5:], good, good_bytes)
    sidx = np.full(70, 255, np.uint8)            # a whole neighbourhood without a valid scan
    _refused_then_good(e3d, good[:4] + (sidx,) + good[5:], good, good_bytes)


def test_merge_refuses_bad_merge_distance(e3d):
    good = _good_70()
    good_bytes = [a.tobytes() for a in e3d.merge_close_points(*good)]
    for dist in (np.nan, np.inf, -np.inf, -0.05):
        _refused_then_good(e3d, (dist,) + good[1:], good, good_bytes)


# ---- point_radius_minmax at small sizes and on a handle without images ----------------------------------------------------------------
@pytest.fixture(scope="module")
def pinhole_scene(e3d):
    from reg_util import make_multi_image_scene
    M = make_multi_image_scene(n_points=8000, n_images=3, seed=21, model=0)
    G = e3d.RegProblem(e3d.default_reg_params(image_scale_count=M["n_levels"], point_neighbor_count=M["K"]))
    G.set_intrinsics(0, M["width"], M["height"], M["params"], 0, M["n_levels"], camera_type=0)
    G.set_splat_points(M["pts"])
    images = {}
    for i, im in enumerate(M["images"]):
        G.set_image(i, 0, im["pyr"]); G.set_image_pose(i, im["q_true"], im["t_true"])
        images[i] = dict(intr=0, pyr=im["pyr"], masks=None, q=im["q_true"], t=im["t_true"])
    intr = {0: dict(w=M["width"], h=M["height"], params=M["params"], min=0, n=M["n_levels"], model=0)}
    return M, G, images, intr


@pytest.mark.parametrize("n", [0, 1, 65])
def test_point_radius_minmax_small_inputs(e3d, mr, pinhole_scene, n):
    M, G, images, intr = pinhole_scene
    pts = np.ascontiguousarray(M["pts"][:n])
    gmn, gmx = G.point_radius_minmax(pts)
    omn, omx = mr.point_radius_minmax(pts, images, intr, M["pts"], M["n_levels"])
    assert gmn.shape == gmx.shape == (n,)
    seen = np.isfinite(omn)
    assert np.array_equal(np.isfinite(gmn), seen) and np.array_equal(np.isfinite(gmx), np.isfinite(omx)) and seen.sum() >= min(n, 1)
    assert np.array_equal(gmn[~seen], omn[~seen]) and np.array_equal(gmx[~seen], omx[~seen])        # +inf / -inf kept
    if n:
        tol = 1e-6                      # as test_point_radius_minmax_matches_oracle: shared elementary functions
        assert np.abs(gmn[seen] - omn[seen]).max() <= tol * omn[seen].max()
        assert np.abs(gmx[seen] - omx[seen]).max() <= tol * omx[seen].max()


@pytest.mark.parametrize("n", [0, 1, 65])
def test_point_radius_minmax_without_images(e3d, pinhole_scene, n):
    M = pinhole_scene[0]
    G = e3d.RegProblem(e3d.default_reg_params(image_scale_count=M["n_levels"], point_neighbor_count=M["K"]))
    G.set_intrinsics(0, M["width"], M["height"], M["params"], 0, M["n_levels"], camera_type=0)
    mn, mx = G.point_radius_minmax(np.ascontiguousarray(M["pts"][:n]))
    assert mn.shape == mx.shape == (n,) and (mn == np.inf).all() and (mx == -np.inf).all()


# ---- the reference's own known-answer tests (src/opt/test/test_multi_scale_point_cloud.cc) through the HIP path -------------------
def test_merge_close_points_reference_kat(e3d):
    from test_oracle_multires import MERGE_KAT as K, check_merge_kat
    check_merge_kat(e3d.merge_close_points(K["merge_distance"], K["num_scans"], K["pts"], K["colors"], K["scans"], K["max_radius"]))


def test_create_multi_scale_point_cloud_reference_kat(e3d, mr):
    """:164-289 with the radius range, the observations and their scales from the GPU (the scale loop itself is host code, shared
    with the oracle here; the tool's C++ version of it is covered by tests/test_gpu_cli_reg.py)."""
    from test_oracle_multires import check_multi_scale_kat, multi_scale_kat_inputs
    images, intr, pts, colors, sidx = multi_scale_kat_inputs()
    G = e3d.RegProblem(e3d.default_reg_params(image_scale_count=3, point_neighbor_count=5))
    G.set_intrinsics(0, 640, 480, intr[0]["params"], 0, 3)
    G.set_image(0, 0, images[0]["pyr"]); G.set_image_pose(0, images[0]["q"], images[0]["t"])
    G.set_splat_points(pts)
    mn, mx = G.point_radius_minmax(pts)
    omn, omx = mr.point_radius_minmax(pts, images, intr, pts, 3)
    assert np.array_equal(mn.view(np.uint32), omn.view(np.uint32)) and np.array_equal(mx.view(np.uint32), omx.view(np.uint32))
    scales = mr.create_multi_scale_point_cloud(pts, colors, sidx, 1, mn, mx)

    def obs_scale(p, radius):
        nbr = np.zeros((len(p), 5), np.uint32)
        G.set_point_scale(0, p, radius, nbr, np.zeros((len(p), 5), np.float32))
        G.render_depth(0, 0)
        n = G.observe(0, 0, 0, 0)
        return G.get_observations(0, 0, n)[3]
    check_multi_scale_kat(scales, obs_scale)
