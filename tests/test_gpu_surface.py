"""SurfaceReconstructor on the GPU (e3d_surface_*, bin/SurfaceReconstructor) against the numpy restatement of tests/surface_ref.py.

Every compared case has ZERO ambiguous corners (0 < |S| <= 1e-6 T) and at most 4096 contributors per corner; the test asserts both.
An f64 sum of at most 4096 terms formed in any order is then within 4096 * 2^-53 * T of S, i.e. within 4096 * 2^-53 / 1e-6 ~ 4.5e-7
relative of a non-zero S: the signs of f are identical and t agrees to about 5e-7.  Hence the defined corners, contributor counts,
vertex cells and triangles are compared exactly, f within 1e-9 T / W, W within 1e-9 W, and vertex positions within 1e-5 h (20 times
the derived 5e-7 h) plus one f32 ulp of the largest coordinate."""
import os
import subprocess

import numpy as np
import pytest

import surface_ref as sr
from cli_util import BIN

pytestmark = pytest.mark.gpu

F = np.float32
H = sr.H
MAX_CONTRIBUTORS = 4096


def _reference(xyz, nrm, h, R):
    M = sr.reconstruct(xyz, nrm, h, R)
    assert int(M["ambiguous"].sum()) == 0
    assert int(M["count"].max(initial=0)) <= MAX_CONTRIBUTORS
    return M


def _compare(e3d, xyz, nrm, h, R, M=None, exact_positions=False):
    M = _reference(xyz, nrm, h, R) if M is None else M
    v, t, c = e3d.reconstruct_surface(xyz, nrm, h, R, return_corners=True)
    assert v.dtype == F and t.dtype == np.uint32 and c["ijk"].dtype == np.int32 and c["f"].dtype == np.float64
    assert np.array_equal(c["ijk"], M["ijk"]), (len(c["ijk"]), len(M["ijk"]))
    assert np.array_equal(c["count"], M["count"])
    df = np.abs(c["f"] - M["f"]); dw = np.abs(c["weight"] - M["W"])
    if len(df):
        print("max |df| / (T / W) = %.3g, max |dW| / W = %.3g" % ((df / np.maximum(M["T"] / M["W"], 1e-300)).max(), (dw / M["W"]).max()))
    assert (df <= 1e-9 * M["T"] / M["W"]).all()
    assert (dw <= 1e-9 * M["W"]).all()
    assert np.array_equal(c["cell_ijk"], M["cell_ijk"]), (len(c["cell_ijk"]), len(M["cell_ijk"]))
    assert np.array_equal(t, M["triangles"])
    if exact_positions:
        assert np.array_equal(v.view(np.uint32), M["vertices"].view(np.uint32))
    elif len(v):
        bound = 1e-5 * float(h) + float(np.spacing(F(np.abs(M["vertices"]).max())))
        dv = np.abs(v.astype(np.float64) - M["vertices"].astype(np.float64)).max()
        print("max vertex deviation %.3g (bound %.3g)" % (dv, bound))
        assert dv <= bound
    return v, t, c, M


def oriented_cloud(n, seed, shift=(0.0, 0.0, 0.0)):
    """A jittered sphere of radius 0.5 (normals: the jittered radial direction) plus n // 10 uniform outliers with random normals,
    shifted in f32."""
    rng = np.random.default_rng(seed)
    m = n - n // 10
    d = rng.normal(size=(m, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    p = d * (0.5 + rng.normal(0, 0.004, (m, 1))) + np.array([0.011, -0.017, 0.023])
    nr = d + rng.normal(0, 0.05, (m, 3))
    nr /= np.linalg.norm(nr, axis=1, keepdims=True)
    o = rng.uniform(-0.7, 0.7, (n - m, 3))
    on = rng.normal(size=(n - m, 3))
    on /= np.linalg.norm(on, axis=1, keepdims=True)
    order = rng.permutation(n)
    xyz = np.concatenate([p, o])[order].astype(F)
    nrm = np.concatenate([nr, on])[order].astype(F)
    return (xyz + np.asarray(shift, F)).astype(F), nrm


# ---- random oriented clouds ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", [1.0, 2.0, 3.5])
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 1000, 20000])
def test_random_cloud(e3d, n, ratio):
    xyz, nrm = oriented_cloud(n, seed=100 + n)
    v, t, c, M = _compare(e3d, xyz, nrm, H, F(ratio) * H)
    if n == 0:
        assert len(c["ijk"]) == 0 and v.shape == (0, 3) and t.shape == (0, 3)
    else:
        assert len(c["ijk"]) > 0
    if n == 20000:
        assert len(t) > 1000 and len(c["ijk"]) > 64 * 64                # many bricks, many blocks of every kernel


def test_random_cloud_far_from_the_origin(e3d):
    s = float(2 ** 19) * float(H)
    xyz, nrm = oriented_cloud(1000, seed=7, shift=(s - 3.0, -(s - 3.0), s - 1.0))
    assert np.abs(xyz).max() / float(H) < 2 ** 20
    v, t, c, M = _compare(e3d, xyz, nrm, H, F(2) * H)
    assert len(t) > 0 and np.abs(c["ijk"]).max() > 2 ** 19 - 100


def test_random_cloud_in_negative_coordinates(e3d):
    xyz, nrm = oriented_cloud(1000, seed=8, shift=(-3.0, -2.0, -5.0))
    assert (xyz < 0).all()
    v, t, c, M = _compare(e3d, xyz, nrm, H, F(2) * H)
    assert len(t) > 0 and (c["ijk"] < 0).all()


# ---- the hand-worked cases -----------------------------------------------------------------------------------------------------------
def test_one_point(e3d):
    v, t, c, M = _compare(e3d, *sr.one_point_case())
    assert len(c["ijk"]) == 32 and v.shape == (21, 3) and t.shape == (24, 3) and (v[:, 2] == F(0.5) * H).all()


def test_lattice_plane_tie_rule_exact(e3d):
    v, t, c, M = _compare(e3d, *sr.lattice_plane_case(), exact_positions=True)
    k = c["ijk"][:, 2]
    assert (c["f"][k == 0] == 0).all() and (v[:, 2] == 0).all() and len(t) > 0


@pytest.fixture(scope="module")
def sphere():
    xyz, nrm, h, R = sr.sphere_case()
    return xyz, nrm, h, R, _reference(xyz, nrm, h, R)


def test_sphere(e3d, sphere):
    xyz, nrm, h, R, M = sphere
    v, t, c, _ = _compare(e3d, xyz, nrm, h, R, M)
    assert len(c["ijk"]) == 1879 and v.shape == (698, 3) and t.shape == (1392, 3)
    closed, euler, volume = sr.mesh_stats(v, t)
    assert closed and euler == 2 and abs(volume - 0.1141) < 5e-5


# ---- walls ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gap", [3.0, 1.0])
def test_two_parallel_walls(e3d, gap):
    """Two jittered sheets `gap` voxels apart whose normals face away from each other: a slab seen from both sides."""
    rng = np.random.default_rng(int(gap) + 20)
    g = (np.stack(np.meshgrid(np.arange(40), np.arange(40), indexing="ij"), -1).reshape(-1, 2) * 0.0125 + rng.normal(0, 0.002, (1600, 2)))
    z0 = 0.0131
    lower = np.concatenate([g, np.full((1600, 1), z0) + rng.normal(0, 0.0005, (1600, 1))], 1)
    upper = np.concatenate([g, np.full((1600, 1), z0 + gap * float(H)) + rng.normal(0, 0.0005, (1600, 1))], 1)
    xyz = np.concatenate([lower, upper]).astype(F)
    nrm = np.concatenate([np.tile([[0, 0, -1]], (1600, 1)), np.tile([[0, 0, 1]], (1600, 1))]).astype(F)
    v, t, c, M = _compare(e3d, xyz, nrm, H, F(2) * H)
    assert len(t) > 0


# ---- points that do not contribute -----------------------------------------------------------------------------------------------------
def test_nan_inf_zero_points_change_nothing(e3d):
    xyz, nrm = oriented_cloud(1000, seed=9)
    clean = e3d.reconstruct_surface(xyz, nrm, H, F(2) * H, return_corners=True)
    rng = np.random.default_rng(1)
    bx = rng.uniform(-0.5, 0.5, (60, 3)).astype(F)
    bn = np.tile(np.array([[0, 0, 1]], F), (60, 1))
    bn[0:10] = 0                                                    # zero normals
    bn[10:20, 0] = np.nan; bn[20:30, 2] = np.inf; bn[30:40, 1] = -np.inf
    bx[40:50, 1] = np.nan; bx[50:55, 0] = np.inf; bx[55:60, 2] = -np.inf
    at = np.sort(rng.integers(0, len(xyz), 60))
    mixed_xyz = np.insert(xyz, at, bx, axis=0)
    mixed_nrm = np.insert(nrm, at, bn, axis=0)
    assert not sr.contributing(bx, bn).any()
    mixed = e3d.reconstruct_surface(mixed_xyz, mixed_nrm, H, F(2) * H, return_corners=True)
    assert np.array_equal(mixed[1], clean[1]) and np.array_equal(mixed[2]["ijk"], clean[2]["ijk"])
    assert np.array_equal(mixed[2]["count"], clean[2]["count"]) and np.array_equal(mixed[2]["cell_ijk"], clean[2]["cell_ijk"])
    _compare(e3d, mixed_xyz, mixed_nrm, H, F(2) * H)
    # nothing but such points: an empty mesh
    v, t, c = e3d.reconstruct_surface(bx, bn, H, F(2) * H, return_corners=True)
    assert v.shape == (0, 3) and t.shape == (0, 3) and len(c["ijk"]) == 0


# ---- errors ----------------------------------------------------------------------------------------------------------------------------
def test_errors_and_recovery(e3d):
    xyz, nrm, h, R = sr.one_point_case()
    far = xyz.copy()
    far[0, 1] = F(2 ** 20) * H
    assert float(far[0, 1]) / float(H) == 2 ** 20
    for args in ((xyz, nrm, F(0), R), (xyz, nrm, h, F(np.nan)), (xyz, nrm, h, F(8.5) * h), (far, nrm, h, R),
                 (xyz, nrm, F(-0.05), R), (xyz, nrm, F(np.inf), R), (xyz, nrm, h, F(0))):
        with pytest.raises(e3d.E3DError):
            e3d.reconstruct_surface(*args)
        v, t = e3d.reconstruct_surface(xyz, nrm, h, R)
        assert v.shape == (21, 3) and t.shape == (24, 3)
    # a point out of range that does not contribute is no error; R / h == 8 is allowed
    nn = np.concatenate([nrm, np.zeros((1, 3), F)])
    v, t = e3d.reconstruct_surface(np.concatenate([xyz, far]), nn, h, R)
    assert v.shape == (21, 3)
    e3d.reconstruct_surface(xyz, nrm, h, F(8) * h)


# ---- reproducibility, kernel groups ---------------------------------------------------------------------------------------------------
def test_two_calls_identical_bytes_and_kernel_groups(e3d):
    xyz, nrm = oriented_cloud(20000, seed=11)
    tm = {}
    a = e3d.reconstruct_surface(xyz, nrm, H, F(2) * H, return_corners=True, timings=tm)
    b = e3d.reconstruct_surface(xyz, nrm, H, F(2) * H, return_corners=True)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    for key in ("ijk", "f", "weight", "count", "cell_ijk"):
        assert a[2][key].tobytes() == b[2][key].tobytes()
    assert sorted(tm) == sorted(g + "_ms" for g in ("grid", "candidates", "field", "corners", "extract"))
    assert all(np.isfinite(x) and x >= 0 for x in tm.values()) and tm["field_ms"] > 0


# ---- the chain: SurfaceReconstructor -> SplatCreator -> occlusion depth ---------------------------------------------------------------
def load_ply_mesh(path):
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode().split("\n")
    assert lines[1] == "format binary_little_endian 1.0"
    nv = int([x for x in lines if x.startswith("element vertex")][0].split()[2])
    nf = int([x for x in lines if x.startswith("element face")][0].split()[2])
    v = np.frombuffer(data, "<f4", 3 * nv, end).reshape(-1, 3)
    rec = np.frombuffer(data, np.dtype([("c", "u1"), ("i", "<i4", 3)]), nf, end + 12 * nv)
    assert (rec["c"] == 3).all() and len(data) == end + 12 * nv + 13 * nf
    return v.copy(), rec["i"].astype(np.uint32)


def _write_ply_27(path, xyz, nrm):
    """NormalEstimator's record: position, normal, colour = 27 bytes."""
    rec = np.zeros(len(xyz), dtype=[("p", "<f4", 3), ("n", "<f4", 3), ("c", "u1", 3)])
    rec["p"] = xyz; rec["n"] = nrm; rec["c"] = 128
    with open(path, "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                 "property float normal_x\nproperty float normal_y\nproperty float normal_z\nproperty uchar red\nproperty uchar green\n"
                 "property uchar blue\nend_header\n" % len(xyz)).encode())
        f.write(rec.tobytes())


def test_chain_tool_splats_occlusion_depth(e3d, sphere, tmp_path):
    import splat_ref
    from reg_util import camera_params, look_at_pose, pyramid_u8, quat_from_R, quat_to_R
    xyz, nrm, h, R, _ = sphere
    cloud = str(tmp_path / "cloud.ply"); mesh = str(tmp_path / "surface.ply"); splats = str(tmp_path / "splats.ply")
    _write_ply_27(cloud, xyz, nrm)
    r = subprocess.run([os.path.join(BIN, "SurfaceReconstructor"), "--point_normal_cloud_path", cloud, "--output_path", mesh,
                        "--voxel_size", "0.05", "--support_radius", "0.1", "--timings"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "Finished!" in r.stdout and "698 vertices, 1392 triangles." in r.stderr and "[timings] field" in r.stderr
    V, T = load_ply_mesh(mesh)
    gv, gt = e3d.reconstruct_surface(xyz, nrm, h, R)
    assert np.array_equal(V.view(np.uint32), gv.view(np.uint32)) and np.array_equal(T, gt)
    # SplatCreator on the cloud and that mesh: exactly the restatement's splats
    r = subprocess.run([os.path.join(BIN, "SplatCreator"), "--point_normal_cloud_path", cloud, "--mesh_path", mesh, "--output_path", splats,
                        "--distance_threshold", "0.02"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rv, rf, ra, _ = splat_ref.splats(xyz, nrm, V, T, 0.02)
    SV, ST = load_ply_mesh(splats)
    assert ("Added %d splats." % int(ra.sum())) in r.stderr
    assert np.array_equal(SV.view(np.uint32), np.ascontiguousarray(rv, F).view(np.uint32)) and np.array_equal(ST, rf.astype(np.uint32))
    # the mesh as occlusion geometry of one pinhole view
    W, Hh = 160, 120
    fx = 150.0
    params = camera_params(0, fx, fx, W / 2, Hh / 2)
    eye = np.array([0.013, -1.521, 0.007])
    R0, t = look_at_pose(tuple(eye), (0.013, -0.021, 0.007))
    q = quat_from_R(R0)
    P = e3d.RegProblem(e3d.default_reg_params(image_scale_count=1, point_neighbor_count=5))
    P.set_intrinsics(0, W, Hh, params, 0, 1, camera_type=0)
    P.set_image(0, 0, pyramid_u8(np.zeros((Hh, W), np.uint8), 1)); P.set_image_pose(0, q, t)
    assert P.add_occlusion_mesh(V, T) == 1
    P.set_occlusion_options(0.05, 100.0, False)
    depth = P.render_depth(0, 0, (Hh, W))
    # the sphere (radius 0.3 at distance 1.5) projects to a disc of radius fx * tan(asin(0.2)) = 30.6 px; well inside it
    yy, xx = np.mgrid[0:Hh, 0:W]
    inside = np.hypot(xx + 0.5 - W / 2, yy + 0.5 - Hh / 2) < 25
    assert np.isfinite(depth[inside]).all() and (depth[inside] > 1.15).all() and (depth[inside] < 1.5).all()
    assert (depth[np.hypot(xx + 0.5 - W / 2, yy + 0.5 - Hh / 2) > 36] == 0).all()
