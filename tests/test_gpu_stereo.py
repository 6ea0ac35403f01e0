"""e3d_reg_stereo_plan / e3d_reg_stereo_rectify / e3d_reg_stereo_ground_truth (StereoPairCreator's three rules on the GPU) through
capi.RegProblem against the numpy restatement in tests/stereo_ref.py.  The plan is f64 host arithmetic in a fixed order on f32 border
samples whose bits both sides share; every output pixel of the remap is a few f32 operations without contraction of its own; the ground
truth is integer and minimum work on bit-identical PINHOLE projections: integers, f32 bits, output bytes, validity maps, disparities,
masks and counters are all compared with np.array_equal."""
import ctypes as C
import functools
import math
import os
import sys

import numpy as np
import pytest

import stereo_ref as sr
import undistort_ref as ur
from test_oracle_camera import CAMERAS

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import reg_binding as rb  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32

MODELS = dict(CAMERAS)
MODELS["SIMPLE_RADIAL_FISHEYE_CLASS_NEGATIVE"] = (rb.SIMPLE_RADIAL_FISHEYE_CLASS, [450.0, 319.5, 239.5, -0.3])
# 5 x 4: smaller than a wave; 17 x 13: odd, one workgroup; 64 x 64: exactly one run of a wave per row; 257 x 131: no multiple of the run
# (64) or of a workgroup's rows (4), several workgroups in both axes
SIZES = [(5, 4), (17, 13), (64, 64), (257, 131)]
KINDS = (ur.U8, ur.RGB, ur.MASK, ur.NEAREST)


def rot(axis, degrees):
    a = math.radians(degrees); c, s = math.cos(a), math.sin(a)
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]),
            "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])}[axis]


def pose(R, Cc):
    q = np.array(sr.rotation_quat([float(v) for v in np.asarray(R, np.float64).reshape(9)]), F)
    return q, (-np.asarray(R, np.float64) @ np.asarray(Cc, np.float64)).astype(F)


def _bits(a):
    a = np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _sources(width, height):
    rng = np.random.RandomState(width * 1000 + height + 7)
    depth = rng.uniform(0.5, 20, (height, width)).astype(F)
    depth[rng.rand(height, width) < 0.2] = 0
    depth[height // 2, width // 2] = np.nan; depth[0, 0] = np.inf; depth[height - 1, width - 1] = -np.inf
    return {ur.U8: rng.randint(0, 256, (height, width)).astype(np.uint8), ur.RGB: rng.randint(0, 256, (height, width, 3)).astype(np.uint8),
            ur.MASK: rng.randint(0, 4, (height, width)).astype(np.uint8) * (rng.rand(height, width) < 0.3).astype(np.uint8), ur.NEAREST: depth}


@functools.lru_cache(maxsize=None)
def _camera(name, size):
    t, p = MODELS[name]
    params = ur.scaled_params(p, t, size[0], size[1])
    cam = rb.make_camera(size[0], size[1], params, t)
    return t, params, cam, ur.border_samples(cam)


# ---- the plan ----------------------------------------------------------------------------------------------------------------------------
PLAN_PAIRS = {
    "converging": (rot("y", 6), (0, 0, 0), rot("y", -5), (0.3, 0, 0)),
    "rolled": (rot("z", 8) @ rot("y", 3), (0.1, -0.2, 0.05), rot("z", -4) @ rot("x", 2), (0.45, -0.17, 0.08)),
}
PLAN_MODELS = [("PINHOLE", "PINHOLE"), ("OPENCV", "OPENCV"), ("THIN_PRISM_FISHEYE", "THIN_PRISM_FISHEYE"), ("FOV", "FOV"), ("OPENCV", "THIN_PRISM_FISHEYE")]


def _pair_problem(e3d, names, poses, size=(96, 64)):
    G = e3d.RegProblem(e3d.default_reg_params(image_scale_count=1))
    for i, name in enumerate(names):
        t, params, cam, samples = _camera(name, size)
        G.set_intrinsics(i, size[0], size[1], params, 0, 1, camera_type=t)
        G.set_image(i, i, None)
        G.set_image_pose(i, *poses[i])
    return G


def _same_plan(got, want):
    assert (got.camera.width, got.camera.height) == (want.camera.width, want.camera.height)
    assert np.array_equal(_bits(np.array([got.camera.fx, got.camera.fy, got.camera.cx, got.camera.cy], F)),
                          _bits(np.array([want.camera.fx, want.camera.fy, want.camera.cx, want.camera.cy], F)))
    for field in ("q_rect", "t_left", "t_right", "S_left", "S_right"):
        assert np.array_equal(_bits(np.array(getattr(got, field), F)), _bits(np.asarray(getattr(want, field), F))), field
    assert np.array_equal(_bits(np.array([got.baseline], F)), _bits(np.array([want.baseline], F)))
    assert np.array_equal(_bits(np.array(got.t_left, F)[1:]), _bits(np.array(got.t_right, F)[1:]))


@pytest.mark.parametrize("pair", sorted(PLAN_PAIRS))
@pytest.mark.parametrize("names", PLAN_MODELS, ids=lambda n: "+".join(n))
def test_plan_equals_the_restatement(e3d, names, pair):
    Rl, Cl, Rr_, Cr = PLAN_PAIRS[pair]
    poses = (pose(Rl, Cl), pose(Rr_, Cr))
    G = _pair_problem(e3d, names, poses)
    cams = [_camera(n, (96, 64))[2] for n in names]; samples = [_camera(n, (96, 64))[3] for n in names]
    ran = 0
    for b, limit, focal in ((0.0, -1, 0.0), (0.5, -1, 0.0), (1.0, -1, 0.0), (0.0, 40, 0.0), (1.0, 33, 0.0), (0.0, -1, 50.0)):
        try:
            want = sr.plan(cams, poses, b, limit, focal, samples=samples)
        except ur.Refused:
            with pytest.raises(e3d.E3DError):
                G.stereo_plan(0, 1, b, limit, focal)
            continue
        got = G.stereo_plan(0, 1, b, limit, focal)
        _same_plan(got, want)
        if limit > 0:
            assert max(got.camera.width, got.camera.height) <= limit
        ran += 1
    assert ran >= 3
    # the poses the library used are the ones it reports
    for i in range(2):
        q, t = G.get_image_pose(i)
        assert np.array_equal(q, poses[i][0]) and np.array_equal(t, poses[i][1])


def test_plan_refusals(e3d):
    Rl, Cl, Rr_, Cr = PLAN_PAIRS["converging"]
    left, right = pose(Rl, Cl), pose(Rr_, Cr)
    G = _pair_problem(e3d, ("OPENCV", "OPENCV"), (left, right))
    good = G.stereo_plan(0, 1)
    with pytest.raises(e3d.E3DError, match="swap"):
        G.stereo_plan(1, 0)
    with pytest.raises(e3d.E3DError, match="blank_pixels"):
        G.stereo_plan(0, 1, 1.5)
    with pytest.raises(e3d.E3DError):
        G.stereo_plan(0, 7)                                                  # an unknown image
    assert e3d.lib().e3d_reg_stereo_plan(G._h, 0, 1, 0.0, -1, 0.0, None) < 0
    q, t = pose(Rr_, Cl)                                                     # the same camera centre (the rotation differs)
    G.set_image_pose(1, q, t)
    with pytest.raises(e3d.E3DError, match="baseline"):
        G.stereo_plan(0, 1)
    G.set_image_pose(0, *pose(np.eye(3), (0, 0, 0))); G.set_image_pose(1, *pose(np.eye(3), (0, 0, 0.3)))
    with pytest.raises(e3d.E3DError, match="along the baseline"):
        G.stereo_plan(0, 1)
    G.set_image_pose(1, *pose(rot("y", 100), (0.3, 0, 0)))
    with pytest.raises(e3d.E3DError, match="looks away"):
        G.stereo_plan(0, 1)
    # border samples behind the rectified image plane: skipped at b = 0, refused above
    wide = np.array([20.0, 20.0, 47.5, 31.5], F)
    cam = rb.make_camera(96, 64, wide, rb.PINHOLE)
    poses = (pose(rot("y", 30), (0, 0, 0)), pose(rot("y", -30), (0.3, 0, 0)))
    W = e3d.RegProblem(e3d.default_reg_params(image_scale_count=1))
    W.set_intrinsics(0, 96, 64, wide, 0, 1, camera_type=rb.PINHOLE)
    for i in range(2):
        W.set_image(i, 0, None); W.set_image_pose(i, *poses[i])
    _same_plan(W.stereo_plan(0, 1, 0.0), sr.plan((cam, cam), poses, 0.0))
    with pytest.raises(e3d.E3DError, match="border pixel"):
        W.stereo_plan(0, 1, 0.5)
    # ... and the first handle still computes the same
    G.set_image_pose(0, *left); G.set_image_pose(1, *right)
    again = G.stereo_plan(0, 1)
    assert bytes(again) == bytes(good)


# ---- the remap ---------------------------------------------------------------------------------------------------------------------------
ROTATIONS = {
    "identity": np.eye(3), "x2": rot("x", 2), "y2": rot("y", 2), "z2": rot("z", 2),
    "yaw30_wide": rot("y", 30), "yaw100_wide": rot("y", 100), "yaw100_tele_row": rot("y", 100), "identity_row": np.eye(3),
}


@functools.lru_cache(maxsize=None)
def _target(name, size, rotation):
    """The target lattice of a case: the camera's own plan (W' > W for a barrel model at b = 1), a hand-made wide one whose lattice
    leaves the source and the fisheye cut-offs, or one row."""
    t, params, cam, samples = _camera(name, size)
    W, H = size
    if rotation.endswith("_wide"):
        return ur.Plan(W + W // 2, H + H // 4, F(cam.p[0] * 0.25), F(cam.p[1] * 0.25), F((W + W // 2) // 2), F((H + H // 4) // 2))
    if rotation == "yaw100_tele_row":
        return ur.Plan(W, 1, F(cam.p[0] * 8), F(cam.p[1] * 8), F(W // 2), F(0))
    if rotation == "identity_row":
        return ur.Plan(W, 1, F(cam.p[0]), F(cam.p[1]), F(cam.p[2]), F(0))
    try:
        return ur.plan(cam, 1.0, samples=samples)
    except ur.Refused:
        return ur.plan(cam, 0.0, samples=samples)


@functools.lru_cache(maxsize=None)
def _positions(name, size, rotation):
    cam = _camera(name, size)[2]
    S = ROTATIONS[rotation].astype(F).ravel()
    return (S,) + sr.source_positions(cam, _target(name, size, rotation), S)


def _problem(e3d, name, size):
    t, params, cam, samples = _camera(name, size)
    G = e3d.RegProblem(e3d.default_reg_params(image_scale_count=1))
    G.set_intrinsics(0, size[0], size[1], params, 0, 1, camera_type=t)
    return G


def _check_kinds(e3d, G, pl, S, src, sx, sy, against_undistort=False):
    plan = e3d.UndistortPlan(pl.width, pl.height, float(pl.fx), float(pl.fy), float(pl.cx), float(pl.cy))
    for kind in KINDS:
        want, want_valid = ur.remap(kind, src[kind], sx, sy)
        got, valid = G.stereo_rectify(0, plan, S, kind, src[kind], return_valid=True)
        assert got.dtype == want.dtype and got.shape == want.shape
        assert np.array_equal(valid, want_valid), kind
        assert np.array_equal(_bits(got), _bits(want)), kind
        assert np.array_equal(_bits(G.stereo_rectify(0, plan, S, kind, src[kind])), _bits(want))     # without the validity map
        if against_undistort:
            u, uv = G.undistort(0, plan, kind, src[kind], return_valid=True)
            assert np.array_equal(_bits(got), _bits(u)) and np.array_equal(valid, uv), kind


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", sorted(MODELS))
def test_pixels_equal_the_restatement(e3d, name, size):
    G = _problem(e3d, name, size)
    src = _sources(*size)
    for rotation in ROTATIONS:
        S, sx, sy = _positions(name, size, rotation)
        _check_kinds(e3d, G, _target(name, size, rotation), S, src, sx, sy, against_undistort=rotation.startswith("identity"))
    assert G.stereo_kernel_ms() > 0


def test_cases_cover_what_they_are_meant_to():
    """On the restatement alone: where the interesting cases are."""
    size = (64, 64)
    assert _target("OPENCV", size, "identity").width > 64                    # W' > W
    for name in sorted(MODELS):
        W, H = size
        valid = lambda r: ur.valid_map(*_positions(name, size, r)[1:], W, H)     # noqa: E731
        assert valid("identity").any() and valid("y2").any() and valid("identity_row").any()
        S, sx, sy = _positions(name, size, "yaw100_wide")                    # vz <= 0 on part of the target
        assert 0 < np.isnan(sx).sum() < sx.size
        assert np.isnan(_positions(name, size, "yaw100_tele_row")[1]).all()  # ... and on all of it
        ok = valid("yaw30_wide")
        assert ok.any() and not ok.all()                                     # part of the wide target leaves the source
        S, ux, uy = _positions(name, size, "identity")
        for r in ("x2", "y2", "z2"):
            assert not np.array_equal(_bits(_positions(name, size, r)[1]), _bits(ux))
    for name in ("THIN_PRISM_FISHEYE", "OPENCV_FISHEYE", "RADIAL_FISHEYE_CLASS", "SIMPLE_RADIAL_FISHEYE_CLASS_NEGATIVE"):
        assert np.isinf(_positions(name, size, "yaw30_wide")[1]).any()       # beyond the fisheye cut-offs


def test_rectify_refusals_leave_the_handle_usable(e3d):
    name, size = "OPENCV", (17, 13)
    G = _problem(e3d, name, size)
    src = _sources(*size)
    pl = _target(name, size, "y2")
    S, sx, sy = _positions(name, size, "y2")
    plan = e3d.UndistortPlan(pl.width, pl.height, float(pl.fx), float(pl.fy), float(pl.cx), float(pl.cy))
    for bad in (np.nan, np.inf):
        Sb = S.copy(); Sb[4] = bad
        with pytest.raises(e3d.E3DError, match="not finite"):
            G.stereo_rectify(0, plan, Sb, ur.U8, src[ur.U8])
    out = np.zeros((pl.height, pl.width), np.uint8)
    lib = e3d.lib()

    def raw(intr, plan_, S_, kind, s, d):
        return lib.e3d_reg_stereo_rectify(G._h, intr, C.byref(plan_) if plan_ is not None else None, C.c_void_p(S_.ctypes.data) if S_ is not None else None,
                                          kind, C.c_void_p(s.ctypes.data) if s is not None else None, C.c_void_p(d.ctypes.data) if d is not None else None, None)
    for kind in (-1, 4):
        assert raw(0, plan, S, kind, src[ur.U8], out) < 0
    assert raw(0, None, S, 0, src[ur.U8], out) < 0 and raw(0, plan, None, 0, src[ur.U8], out) < 0
    assert raw(0, plan, S, 0, None, out) < 0 and raw(0, plan, S, 0, src[ur.U8], None) < 0
    with pytest.raises(e3d.E3DError, match="intrinsics"):
        G.stereo_rectify(7, plan, S, ur.U8, src[ur.U8])
    with pytest.raises(e3d.E3DError, match="plan"):
        G.stereo_rectify(0, e3d.UndistortPlan(0, 5, 1.0, 1.0, 0.0, 0.0), S, ur.U8, src[ur.U8])
    _check_kinds(e3d, G, pl, S, src, sx, sy)


# ---- the ground truth --------------------------------------------------------------------------------------------------------------------
GT_W, GT_H, GT_F = 160, 120, 140.0


@functools.lru_cache(maxsize=None)
def _gt_scene():
    """The wall + occluder + clutter scene of test_gpu_reg.py's scan visibility test seen by a rectified pair 0.3 apart that looks along +y."""
    from reg_util import make_multi_image_scene
    M = make_multi_image_scene(n_points=20000, n_images=1, seed=17, perturb=0.0, model=0)
    rng = np.random.RandomState(5)
    bx, bz = np.meshgrid(np.arange(-0.3, 0.2, 0.01), np.arange(-0.2, 0.2, 0.01))
    blocker = np.stack([bx.ravel(), np.full(bx.size, 1.6), bz.ravel()], 1)
    scan = np.concatenate([M["pts"], blocker, rng.uniform(-4, 4, (3000, 3))]).astype(F)
    params = np.array([GT_F, GT_F, 79.0, 59.0], F)
    R = np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]], np.float64) @ rot("x", 1.5) @ rot("z", -1)          # x right, y down, z along +y
    q, tl = pose(R, (-0.15, -0.3, 0.02))
    tr = np.array([F(float(tl[0]) - 0.3), tl[1], tl[2]], F)
    left_excluded = np.zeros((GT_H, GT_W), np.uint8); left_excluded[70:95, 20:60] = 2; left_excluded[5:15, 100:130] = 255
    right_excluded = np.zeros((GT_H, GT_W), np.uint8); right_excluded[30:60, 25:55] = 7
    cam = rb.make_camera(GT_W, GT_H, params, rb.PINHOLE)
    want = sr.ground_truth(scan, scan, 0.03, cam, q, tl, tr, left_excluded, right_excluded)
    return dict(scan=scan, params=params, q=q, tl=tl, tr=tr, left_excluded=left_excluded, right_excluded=right_excluded, cam=cam, want=want)


def _gt_problem(e3d, Sc):
    G = e3d.RegProblem(e3d.default_reg_params(image_scale_count=1))
    G.set_intrinsics(0, GT_W, GT_H, Sc["params"], 0, 1, camera_type=rb.PINHOLE)
    G.set_image(0, 0, None); G.set_image(1, 0, None)
    G.set_image_pose(0, Sc["q"], Sc["tl"]); G.set_image_pose(1, Sc["q"], Sc["tr"])
    G.set_splat_points(Sc["scan"])
    G.set_scan_points(Sc["scan"])
    return G


def test_ground_truth_scene_has_all_three_classes():
    Sc = _gt_scene()
    disparity, mask, D1, counts = Sc["want"]
    for value in (255, 128, 0):
        assert (mask == value).sum() >= 200, value
    assert np.isinf(disparity[mask == 0]).all() and np.isfinite(disparity[mask != 0]).all()
    assert (mask[70:95, 20:60] == 0).all() and (mask[5:15, 100:130] == 0).all()          # the left exclusion blocks
    assert counts.max() == 2 and (counts == 2).sum() > 3000 and (counts == 1).sum() > 500 and (counts == 0).sum() > 2000


def test_ground_truth_equals_the_restatement(e3d):
    Sc = _gt_scene()
    want_disparity, want_mask, want_depth, want_counts = Sc["want"]
    G = _gt_problem(e3d, Sc)
    G.count_scan_observations(0)                                             # counters from an earlier run must not leak in
    disparity, mask, depth = G.stereo_ground_truth(0, 1, Sc["left_excluded"], Sc["right_excluded"], return_depth=True)
    assert np.array_equal(_bits(depth), _bits(want_depth))
    assert np.array_equal(mask, want_mask)
    assert np.array_equal(_bits(disparity), _bits(want_disparity))
    assert np.array_equal(G.scan_observation_counts(), want_counts)
    # the same call again, without the optional depth, and without exclusion maps
    d2, m2 = G.stereo_ground_truth(0, 1, Sc["left_excluded"], Sc["right_excluded"])
    assert np.array_equal(_bits(d2), _bits(disparity)) and np.array_equal(m2, mask)
    free = sr.ground_truth(Sc["scan"], Sc["scan"], 0.03, Sc["cam"], Sc["q"], Sc["tl"], Sc["tr"])
    d3, m3 = G.stereo_ground_truth(0, 1)
    assert np.array_equal(_bits(d3), _bits(free[0])) and np.array_equal(m3, free[1]) and not np.array_equal(m3, mask)
    assert np.array_equal(G.scan_observation_counts(), free[3])


def test_ground_truth_refusals(e3d):
    Sc = _gt_scene()
    G = _gt_problem(e3d, Sc)
    good = G.stereo_ground_truth(0, 1)
    q2 = Sc["q"].copy(); q2[1] = np.nextafter(q2[1], F(2))
    G.set_image_pose(1, q2, Sc["tr"])
    with pytest.raises(e3d.E3DError, match="rotations"):
        G.stereo_ground_truth(0, 1)
    t2 = Sc["tr"].copy(); t2[1] = np.nextafter(t2[1], F(9))
    G.set_image_pose(1, Sc["q"], t2)
    with pytest.raises(e3d.E3DError, match="translations"):
        G.stereo_ground_truth(0, 1)
    G.set_image_pose(1, Sc["q"], Sc["tr"])
    with pytest.raises(e3d.E3DError, match="baseline"):                      # B < 0: swapped; B = 0: the same image twice
        G.stereo_ground_truth(1, 0)
    with pytest.raises(e3d.E3DError, match="baseline"):
        G.stereo_ground_truth(0, 0)
    t, p = MODELS["OPENCV"]
    G.set_intrinsics(1, GT_W, GT_H, ur.scaled_params(p, t, GT_W, GT_H), 0, 1, camera_type=t)
    G.set_image(2, 1, None); G.set_image(3, 1, None)
    G.set_image_pose(2, Sc["q"], Sc["tl"]); G.set_image_pose(3, Sc["q"], Sc["tr"])
    with pytest.raises(e3d.E3DError, match="PINHOLE"):
        G.stereo_ground_truth(2, 3)
    with pytest.raises(e3d.E3DError, match="share"):
        G.stereo_ground_truth(0, 3)
    G.set_intrinsics(2, GT_W, GT_H, np.array([GT_F, GT_F + 1, 79.0, 59.0], F), 0, 1, camera_type=rb.PINHOLE)
    G.set_image(4, 2, None); G.set_image(5, 2, None)
    G.set_image_pose(4, Sc["q"], Sc["tl"]); G.set_image_pose(5, Sc["q"], Sc["tr"])
    with pytest.raises(e3d.E3DError, match="fx == fy"):
        G.stereo_ground_truth(4, 5)
    out = np.zeros((GT_H, GT_W), F); m = np.zeros((GT_H, GT_W), np.uint8)
    lib = e3d.lib()
    assert lib.e3d_reg_stereo_ground_truth(G._h, 0, 1, None, None, None, C.c_void_p(m.ctypes.data), None) < 0
    assert lib.e3d_reg_stereo_ground_truth(G._h, 0, 1, None, None, C.c_void_p(out.ctypes.data), None, None) < 0
    E = e3d.RegProblem(e3d.default_reg_params(image_scale_count=1))          # no scan points
    E.set_intrinsics(0, GT_W, GT_H, Sc["params"], 0, 1, camera_type=rb.PINHOLE)
    E.set_image(0, 0, None); E.set_image(1, 0, None)
    E.set_image_pose(0, Sc["q"], Sc["tl"]); E.set_image_pose(1, Sc["q"], Sc["tr"])
    with pytest.raises(e3d.E3DError, match="scan points"):
        E.stereo_ground_truth(0, 1)
    again = G.stereo_ground_truth(0, 1)
    assert np.array_equal(_bits(again[0]), _bits(good[0])) and np.array_equal(again[1], good[1])
