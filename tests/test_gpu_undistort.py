"""e3d_reg_undistort_plan / e3d_reg_undistort (ImageUndistorter's two rules on the GPU) through capi.RegProblem against the numpy
restatement in tests/undistort_ref.py, for all 13 camera models.  ImageToNormalized and NormalizedToImage have the same bits on both
sides (test_gpu_localize.py, test_gpu_reg.py), the plan is f64 host arithmetic on those f32 samples, and every output pixel is a few
f32 operations without contraction of its own: the plan, every output byte, the f32 bits and the validity map are compared with
np.array_equal.  The restatement of a case is computed once and shared by the four kinds."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

import undistort_ref as ur
from test_oracle_camera import CAMERAS

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import reg_binding as rb  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32

# The 13 classes with the reference's own test parameters, and SIMPLE_RADIAL_FISHEYE with a negative coefficient: the only way that
# model gets a radius cut-off (camera_simple_radial.cc:51-57), which here also leaves border pixels without a finite position.
MODELS = dict(CAMERAS)
MODELS["SIMPLE_RADIAL_FISHEYE_CLASS_NEGATIVE"] = (rb.SIMPLE_RADIAL_FISHEYE_CLASS, [450.0, 319.5, 239.5, -0.3])
# 5 x 4: smaller than a wave; 17 x 13: odd, one workgroup; 64 x 64: exactly one run of a wave per row; 257 x 131: no multiple of the run
# (64) or of a workgroup's rows (4), several workgroups in both axes
SIZES = [(5, 4), (17, 13), (64, 64), (257, 131)]
BLANK = (0.0, 0.5, 1.0)
KINDS = (ur.U8, ur.RGB, ur.MASK, ur.NEAREST)


def _sources(width, height):
    rng = np.random.RandomState(width * 1000 + height)
    depth = rng.uniform(0.5, 20, (height, width)).astype(F)
    depth[rng.rand(height, width) < 0.2] = 0                    # holes
    depth[height // 2, width // 2] = np.nan; depth[0, 0] = np.inf; depth[height - 1, width - 1] = -np.inf
    depth[1, 1] = np.array([0x7fc0beef], np.uint32).view(F)[0]
    return {ur.U8: rng.randint(0, 256, (height, width)).astype(np.uint8), ur.RGB: rng.randint(0, 256, (height, width, 3)).astype(np.uint8),
            ur.MASK: rng.randint(0, 4, (height, width)).astype(np.uint8) * (rng.rand(height, width) < 0.3).astype(np.uint8), ur.NEAREST: depth}


@functools.lru_cache(maxsize=None)
def _camera(name, size):
    t, p = MODELS[name]
    params = ur.scaled_params(p, t, size[0], size[1])
    cam = rb.make_camera(size[0], size[1], params, t)
    return t, params, cam, ur.border_samples(cam)


@functools.lru_cache(maxsize=None)
def _expected(name, size, b, max_image_size=-1):
    """-> (plan, sx, sy) of the restatement, or None where the rule refuses."""
    t, params, cam, samples = _camera(name, size)
    try:
        pl = ur.plan(cam, b, max_image_size, samples=samples)
    except ur.Refused:
        return None
    return (pl,) + ur.source_positions(cam, pl)


def _problem(e3d, name, size):
    t, params, cam, samples = _camera(name, size)
    G = e3d.RegProblem(e3d.default_reg_params(image_scale_count=1))
    G.set_intrinsics(0, size[0], size[1], params, 0, 1, camera_type=t)
    return G


def _same_plan(got, want):
    assert (got.width, got.height) == (want.width, want.height)
    assert np.array_equal(np.array([got.fx, got.fy, got.cx, got.cy], F), np.array([want.fx, want.fy, want.cx, want.cy], F))


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _check_kinds(G, plan, src, sx, sy):
    for kind in KINDS:
        want, want_valid = ur.remap(kind, src[kind], sx, sy)
        got, valid = G.undistort(0, plan, kind, src[kind], return_valid=True)
        assert got.dtype == want.dtype and got.shape == want.shape
        assert np.array_equal(valid, want_valid), kind
        assert np.array_equal(_bits(got), _bits(want)), kind
        assert np.array_equal(_bits(G.undistort(0, plan, kind, src[kind])), _bits(want))       # without the validity map


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", sorted(MODELS))
def test_plan_and_pixels_equal_the_restatement(e3d, name, size):
    G = _problem(e3d, name, size)
    src = _sources(*size)
    ran = 0
    for b in BLANK:
        exp = _expected(name, size, b)
        if exp is None:                                          # a border pixel beyond the cut-off (b > 0), a side without samples
            with pytest.raises(e3d.E3DError):
                G.undistort_plan(0, b)
            continue
        pl, sx, sy = exp
        plan = G.undistort_plan(0, b)
        _same_plan(plan, pl)
        _check_kinds(G, plan, src, sx, sy)
        ran += 1
    assert ran >= 1 or name == "SIMPLE_RADIAL_FISHEYE_CLASS_NEGATIVE"


def test_cases_cover_what_they_are_meant_to():
    """On the restatement alone: where the interesting cases are."""
    for name in ("FOV", "SIMPLE_RADIAL_FISHEYE_CLASS_NEGATIVE"):             # non-finite border samples: skipped at b = 0, refused above
        assert _expected(name, (64, 64), 0.0) is not None and _expected(name, (64, 64), 0.5) is None and _expected(name, (64, 64), 1.0) is None
    pl, sx, sy = _expected("SIMPLE_RADIAL_FISHEYE_CLASS_NEGATIVE", (64, 64), 0.0)
    assert np.isinf(sx).sum() > 100                                          # output pixels beyond the radius cut-off
    for name in ("THIN_PRISM_FISHEYE", "OPENCV_FISHEYE", "RADIAL_FISHEYE_CLASS"):
        assert np.isinf(_expected(name, (257, 131), 1.0)[1]).any()
    pl = _expected("OPENCV", (64, 64), 1.0)[0]
    assert pl.width > 64 and pl.height > 64                                  # W' > W
    mixed = 0                                                                # valid and invalid pixels in one image
    for name in sorted(MODELS):
        ok = ur.valid_map(*_expected(name, (257, 131), 1.0 if _expected(name, (257, 131), 1.0) else 0.0)[1:], 257, 131)
        assert ok.any()
        mixed += int(not ok.all())
    assert mixed >= 9


@functools.lru_cache(maxsize=None)
def _wide(name):
    """A hand-made plan with a quarter of the focal length around the 64 x 64 camera: the lattice reaches far beyond every cut-off."""
    t, params, cam, samples = _camera(name, (64, 64))
    pl = ur.Plan(96, 80, F(cam.p[0] * 0.25), F(cam.p[1] * 0.25), F(47), F(41))
    return (pl,) + ur.source_positions(cam, pl)


@pytest.mark.parametrize("name", [n for n in sorted(MODELS) if MODELS[n][0] in ur.FISHEYE and n != "SIMPLE_RADIAL_FISHEYE_CLASS"])
def test_pixels_beyond_the_radius_cutoff(e3d, name):
    """Every fisheye model that has a cut-off (SIMPLE_RADIAL_FISHEYE gets one from a negative coefficient only)."""
    pl, sx, sy = _wide(name)
    beyond = np.isinf(sx) | np.isinf(sy)
    assert beyond.sum() > 500 and ur.valid_map(sx, sy, 64, 64).sum() > 100
    G = _problem(e3d, name, (64, 64))
    plan = e3d.UndistortPlan(pl.width, pl.height, float(pl.fx), float(pl.fy), float(pl.cx), float(pl.cy))
    _check_kinds(G, plan, _sources(64, 64), sx, sy)


@pytest.mark.parametrize("limit", [100, 31, 8])
def test_max_image_size(e3d, limit):
    name, size = "THIN_PRISM_FISHEYE", (64, 64)
    G = _problem(e3d, name, size)
    for b in (0.0, 1.0):
        pl, sx, sy = _expected(name, size, b, limit)
        plan = G.undistort_plan(0, b, limit)
        _same_plan(plan, pl)
        assert max(plan.width, plan.height) <= limit
        _check_kinds(G, plan, _sources(*size), sx, sy)


def test_refusals_leave_the_handle_usable(e3d):
    name, size = "OPENCV", (17, 13)
    G = _problem(e3d, name, size)
    lib = e3d.lib()
    src = _sources(*size)
    pl, sx, sy = _expected(name, size, 1.0)
    good = G.undistort_plan(0, 1.0)
    plan_out = e3d.UndistortPlan()
    out = np.zeros((pl.height, pl.width, 3), np.uint8)

    def raw(intr, plan, kind, s, d):
        return lib.e3d_reg_undistort(G._h, intr, C.byref(plan) if plan is not None else None, kind,
                                     C.c_void_p(s.ctypes.data) if s is not None else None, C.c_void_p(d.ctypes.data) if d is not None else None, None)
    for b in (-0.001, 1.5, float("nan")):                                    # blank_pixels outside [0, 1]
        with pytest.raises(e3d.E3DError, match="blank_pixels"):
            G.undistort_plan(0, b)
    with pytest.raises(e3d.E3DError, match="intrinsics"):                    # unknown intrinsics id
        G.undistort_plan(7, 0.0)
    with pytest.raises(e3d.E3DError, match="intrinsics"):
        G.undistort(7, good, ur.U8, src[ur.U8])
    assert lib.e3d_reg_undistort_plan(G._h, 0, 0.0, -1, None) < 0            # null output pointers and handles
    assert lib.e3d_reg_undistort_plan(None, 0, 0.0, -1, C.byref(plan_out)) < 0
    assert raw(0, None, 0, src[ur.U8], out) < 0 and raw(0, good, 0, None, out) < 0 and raw(0, good, 0, src[ur.U8], None) < 0
    assert b"null" in lib.e3d_last_error()
    for kind in (-1, 4):
        assert raw(0, good, kind, src[ur.U8], out) < 0
    with pytest.raises(e3d.E3DError, match="no room"):                       # max_image_size below the margin: s <= 0
        G.undistort_plan(0, 0.0, 1)
    assert _expected(name, size, 0.0, 2) is None                             # W' or H' < 2: the size limit leaves one row
    with pytest.raises(e3d.E3DError, match="smaller than 2 x 2"):
        G.undistort_plan(0, 0.0, 2)
    with pytest.raises(e3d.E3DError, match="plan"):
        G.undistort(0, e3d.UndistortPlan(0, 5, 1.0, 1.0, 0.0, 0.0), ur.U8, src[ur.U8])
    with pytest.raises(e3d.E3DError, match="plan"):
        G.undistort(0, e3d.UndistortPlan(5, 5, float("nan"), 1.0, 0.0, 0.0), ur.U8, src[ur.U8])
    with pytest.raises(e3d.E3DError):                                        # a source of another size
        G.undistort(0, good, ur.U8, np.zeros((4, 4), np.uint8))
    # nL >= nR: a mirrored image (negative fx), whose left border lies right of its right border
    G.set_intrinsics(1, 16, 12, np.array([-16.0, 8.0, 7.0, 5.0], F), 0, 1, camera_type=rb.PINHOLE)
    with pytest.raises(e3d.E3DError, match="empty"):
        G.undistort_plan(1, 0.0)
    # a non-finite border sample at b > 0, and the same camera at b = 0
    F_ = _problem(e3d, "FOV", (17, 13))
    with pytest.raises(e3d.E3DError, match="cut-off"):
        F_.undistort_plan(0, 0.5)
    _same_plan(F_.undistort_plan(0, 0.0), _expected("FOV", (17, 13), 0.0)[0])
    # ... and after all of them the first handle still computes the same
    _same_plan(G.undistort_plan(0, 1.0), pl)
    _check_kinds(G, good, src, sx, sy)


def test_the_same_call_twice_gives_the_same_bytes(e3d):
    name, size = "THIN_PRISM_FISHEYE", (257, 131)
    G = _problem(e3d, name, size)
    src = _sources(*size)
    plan = G.undistort_plan(0, 1.0)
    assert G.undistort_plan(0, 1.0).astuple() == plan.astuple()
    for kind in KINDS:
        a = G.undistort(0, plan, kind, src[kind], return_valid=True)
        b = G.undistort(0, plan, kind, src[kind], return_valid=True)
        assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1])
    assert G.undistort_kernel_ms() > 0
