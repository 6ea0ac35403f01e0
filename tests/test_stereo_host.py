"""The numpy restatement of StereoPairCreator's rules (tests/stereo_ref.py) checked on its own, without a GPU: what the plan promises
(an identity for a displaced pair, equal rows and the disparity f B / z for every other pair, the refusals, the size limit), the file
formats, the disparity / mask rule on a hand-made example, and the array form of the remap against a pixel-at-a-time form.
tests/test_gpu_stereo.py then compares the library with this restatement bit for bit."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import stereo_ref as sr  # noqa: E402
import undistort_ref as ur  # noqa: E402
from oracle import reg_binding as rb  # noqa: E402
from test_oracle_camera import CAMERAS  # noqa: E402

F = np.float32


def camera(name, width, height):
    t, p = CAMERAS[name]
    return rb.make_camera(width, height, ur.scaled_params(p, t, width, height), t)


def rot(axis, degrees):
    a = math.radians(degrees); c, s = math.cos(a), math.sin(a)
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]),
            "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])}[axis]


def pose(R, C):
    """image_T_global (q, t) as f32 from a rotation (global -> camera) and the camera centre."""
    q = np.array(sr.rotation_quat([float(v) for v in np.asarray(R, np.float64).reshape(9)]), F)
    return q, (-np.asarray(R, np.float64) @ np.asarray(C, np.float64)).astype(F)


def matrix(q):
    w, x, y, z = (float(v) for v in q)
    n = math.sqrt(w * w + x * x + y * y + z * z)
    return np.array(sr.quat_matrix(w / n, x / n, y / n, z / n)).reshape(3, 3)


PAIRS = {
    # name: (R_left, C_left, R_right, C_right), cameras looking along +z of the global frame, more or less
    "converging": (rot("y", 6), (0, 0, 0), rot("y", -5), (0.3, 0, 0)),
    "rolled": (rot("z", 8) @ rot("y", 3), (0.1, -0.2, 0.05), rot("z", -4) @ rot("x", 2), (0.45, -0.2, 0.05)),
    "vertical_offset": (rot("x", 3), (0, 0, 0), rot("y", -2) @ rot("x", -1), (0.25, 0.06, -0.03)),
}
_TILT = rot("x", 40) @ rot("z", 25)            # a rig that hangs askew in the global frame: the baseline along the rig's own x axis
PAIRS["tilted_world"] = (rot("y", 4) @ _TILT, (1, 2, 3), rot("y", -4) @ _TILT, tuple(np.array([1, 2, 3]) + 0.3 * _TILT[0] + 0.02 * _TILT[1]))


def test_displaced_identical_pinholes_are_an_identity():
    """A power-of-two focal length and an integral principal point: every step of the plan is exact."""
    cam = rb.make_camera(96, 64, np.array([64.0, 64.0, 47.0, 31.0], F), rb.PINHOLE)
    q = np.array([1, 0, 0, 0], F)
    pl = sr.plan((cam, cam), ((q, np.array([0.5, 0.25, -1.0], F)), (q, np.array([0.5 - 0.375, 0.25, -1.0], F))))
    assert np.array_equal(pl.S_left, np.eye(3, dtype=F).ravel()) and np.array_equal(pl.S_right, np.eye(3, dtype=F).ravel())
    assert np.array_equal(pl.q_rect, q) and pl.baseline == F(0.375)
    assert np.array_equal(pl.t_left, np.array([0.5, 0.25, -1.0], F)) and np.array_equal(pl.t_right, np.array([0.125, 0.25, -1.0], F))
    assert pl.camera == ur.Plan(96, 64, F(64), F(64), F(47), F(31))          # S = I: the window is the camera's own
    # a general pose: S = I, q_rect = the pose and B = the displacement to rounding
    R = rot("y", 20) @ rot("x", -35) @ rot("z", 10)
    C0 = np.array([1.0, -2.0, 0.5]); C1 = C0 + 0.42 * R[0]                   # displaced along the cameras' own +x
    pl = sr.plan((cam, cam), (pose(R, C0), pose(R, C1)))
    assert np.abs(pl.S_left.reshape(3, 3) - np.eye(3)).max() < 1e-6 and np.abs(pl.S_right.reshape(3, 3) - np.eye(3)).max() < 1e-6
    assert np.abs(pl.q_rect - pose(R, C0)[0]).max() < 1e-6 and abs(float(pl.baseline) - 0.42) < 1e-6


@pytest.mark.parametrize("name", sorted(PAIRS))
def test_rows_agree_and_columns_differ_by_the_disparity(name):
    Rl, Cl, Rr_, Cr = PAIRS[name]
    cam = rb.make_camera(96, 64, np.array([80.0, 82.0, 47.3, 31.2], F), rb.PINHOLE)
    poses = (pose(Rl, Cl), pose(Rr_, Cr))
    pl = sr.plan((cam, cam), poses)
    assert np.array_equal(pl.t_left[1:].view(np.uint32), pl.t_right[1:].view(np.uint32))
    assert float(pl.t_left[0]) - float(pl.t_right[0]) > 0 and pl.q_rect[0] >= 0
    assert pl.camera.fx == pl.camera.fy == F(81.0)
    R = matrix(pl.q_rect)
    f, cx, cy, B = float(pl.camera.fx), float(pl.camera.cx), float(pl.camera.cy), float(pl.t_left[0]) - float(pl.t_right[0])
    assert abs(B - float(pl.baseline)) < 1e-6
    rng = np.random.RandomState(3)
    mid = 0.5 * (np.asarray(Cl, np.float64) + np.asarray(Cr, np.float64))
    axis = R[2]                                                               # the rectified viewing direction in the global frame
    X = mid + rng.uniform(1.5, 6, (200, 1)) * axis + rng.uniform(-0.8, 0.8, (200, 3))
    pix = []
    for t, S, (q_src, t_src) in ((pl.t_left, pl.S_left, poses[0]), (pl.t_right, pl.S_right, poses[1])):
        p = X @ R.T + t.astype(np.float64)
        assert (p[:, 2] > 0.5).all()
        pix.append((f * p[:, 0] / p[:, 2] + cx, f * p[:, 1] / p[:, 2] + cy, p[:, 2]))
        # the rectified camera sees what the source camera sees: S^T (R_src X + t_src) is the same ray
        d = (X @ matrix(q_src).T + t_src.astype(np.float64)) @ S.reshape(3, 3).astype(np.float64)
        assert np.abs(d[:, :2] / d[:, 2:] - p[:, :2] / p[:, 2:]).max() < 1e-5
    (xl, yl, zl), (xr, yr, zr) = pix
    assert np.abs(yl - yr).max() < 1e-3
    assert np.abs(zl - zr).max() < 1e-6
    assert np.abs((xl - xr) - f * B / zl).max() < 1e-3


def test_refusals():
    cam = rb.make_camera(96, 64, np.array([80.0, 80.0, 47.0, 31.0], F), rb.PINHOLE)
    Rl, Cl, Rr_, Cr = PAIRS["converging"]
    left, right = pose(Rl, Cl), pose(Rr_, Cr)
    samples = [ur.border_samples(cam)] * 2
    assert sr.plan((cam, cam), (left, right), samples=samples).camera.width > 40
    with pytest.raises(sr.Swapped):
        sr.plan((cam, cam), (right, left), samples=samples)
    with pytest.raises(sr.Refused):                                           # zero baseline
        sr.plan((cam, cam), (left, pose(Rr_, Cl)), samples=samples)
    with pytest.raises(sr.Refused) as e:                                      # both cameras look along the baseline
        sr.plan((cam, cam), (pose(np.eye(3), (0, 0, 0)), pose(np.eye(3), (0, 0, 0.3))), samples=samples)
    assert not isinstance(e.value, sr.Swapped)
    with pytest.raises(sr.Refused) as e:                                      # the right camera looks away from the common direction
        sr.plan((cam, cam), (pose(np.eye(3), (0, 0, 0)), pose(rot("y", 100), (0.3, 0, 0))), samples=samples)
    assert not isinstance(e.value, sr.Swapped)
    for b in (-0.1, 1.1, float("nan")):
        with pytest.raises(sr.Refused):
            sr.plan((cam, cam), (left, right), b, samples=samples)


def test_border_samples_behind_the_rectified_plane():
    """A 135-degree camera turned 30 degrees: its outermost border rays make more than 90 degrees with the rectified axis."""
    wide = rb.make_camera(96, 64, np.array([20.0, 20.0, 47.5, 31.5], F), rb.PINHOLE)
    poses = (pose(rot("y", 30), (0, 0, 0)), pose(rot("y", -30), (0.3, 0, 0)))
    samples = [ur.border_samples(wide)] * 2
    B, q, tl, tr, S0, S1 = sr.frame(poses)
    rotated = sr.rotated_samples(samples[0], S0)
    lost = sum(int(np.isnan(a).any(1).sum()) for a in rotated)
    assert 0 < lost < sum(len(a) for a in rotated)
    pl = sr.plan((wide, wide), poses, 0.0, samples=samples)                   # skipped at b = 0
    assert pl.camera.width >= 2 and pl.camera.height >= 2
    for b in (0.25, 1.0):                                                     # refused above
        with pytest.raises(ur.Refused):
            sr.plan((wide, wide), poses, b, samples=samples)


def test_max_image_size_and_focal_length():
    cam = camera("OPENCV", 96, 64)
    Rl, Cl, Rr_, Cr = PAIRS["rolled"]
    poses = (pose(Rl, Cl), pose(Rr_, Cr))
    samples = [ur.border_samples(cam)] * 2
    full = sr.plan((cam, cam), poses, 1.0, samples=samples)
    assert full.camera.fx == F((float(cam.p[0]) + float(cam.p[1]) + float(cam.p[0]) + float(cam.p[1])) / 4.0)
    for limit in (max(full.camera.width, full.camera.height) + 5, 60, 33, 9):
        pl = sr.plan((cam, cam), poses, 1.0, limit, samples=samples)
        assert max(pl.camera.width, pl.camera.height) <= limit
        if limit > max(full.camera.width, full.camera.height):
            assert pl.camera == full.camera
        else:
            assert pl.camera.fx < full.camera.fx and pl.camera.fx == pl.camera.fy
    pl = sr.plan((cam, cam), poses, 1.0, focal_length=40.0, samples=samples)
    assert pl.camera.fx == pl.camera.fy == F(40) and pl.camera.width < full.camera.width


def test_pfm_and_calib_round_trip(tmp_path):
    rng = np.random.RandomState(1)
    d = rng.uniform(0.1, 300, (5, 7)).astype(F); d[1, 2] = np.inf; d[4, 6] = np.inf
    path = str(tmp_path / "disp0GT.pfm")
    sr.write_pfm(path, d)
    raw = open(path, "rb").read()
    assert raw.startswith(b"Pf\n7 5\n-1.0\n") and len(raw) == len(b"Pf\n7 5\n-1.0\n") + 4 * 35
    assert np.array_equal(np.frombuffer(raw[-4 * 7:], "<f4"), d[0])          # the file ends with the top row
    assert np.array_equal(sr.read_pfm(path).view(np.uint32), d.view(np.uint32))
    pl = sr.StereoPlan(ur.Plan(65, 49, F(34.0926), F(34.0926), F(31), F(22)), F(0.30000001), None, None, None, None, None)
    text = sr.calib_text(pl)
    assert text.splitlines()[0] == "cam0=[34.0926018 0 31; 0 34.0926018 22; 0 0 1]" and "\ndoffs=0\nbaseline=0.300000012\nwidth=65\nheight=49\n" in text
    c = sr.parse_calib(text)
    assert np.array_equal(c["cam0"], c["cam1"]) and F(c["cam0"][0, 0]) == pl.camera.fx and F(c["cam0"][1, 2]) == pl.camera.cy
    assert F(c["baseline"]) == pl.baseline and (c["width"], c["height"], c["doffs"]) == (65, 49, 0.0)


def test_disparity_and_mask_by_hand():
    inf = np.inf
    D1 = np.array([[2.0, 4.0, inf, 1.0], [8.0, inf, 2.5, 2.5], [inf, 16.0, 3.0, 0.5]], F)
    D2 = np.array([[2.0, inf, inf, 1.0], [8.5, inf, 2.5, inf], [inf, 16.0, 3.5, 0.5]], F)        # D2 >= D1: a subset of the points
    disparity, mask = sr.disparity_and_mask(D1, D2, F(100), 0.25)
    assert mask.tolist() == [[255, 128, 0, 255], [128, 0, 255, 128], [0, 255, 128, 255]]           # (1, 0) and (2, 2): D2 > D1 -> 128
    want = np.array([[12.5, 6.25, inf, 25.0], [3.125, inf, 10.0, 10.0], [inf, 1.5625, F(25.0 / 3.0), 50.0]], F)
    assert np.array_equal(disparity.view(np.uint32), want.view(np.uint32))
    # the disparity is rounded once, from f64
    d, _ = sr.disparity_and_mask(np.array([[3.0]], F), np.array([[3.0]], F), F(0.1), 0.7)
    assert d[0, 0] == F(float(F(0.1)) * 0.7 / 3.0)


@pytest.mark.parametrize("name", ["OPENCV", "THIN_PRISM_FISHEYE"])
def test_array_form_of_the_remap_equals_the_serial_form(name):
    cam = camera(name, 17, 13)
    pl = ur.plan(cam, 1.0)
    for R in (np.eye(3), rot("y", 2) @ rot("x", -2) @ rot("z", 2), rot("y", 100)):
        S = R.astype(F).ravel()
        a, b = sr.source_positions(cam, pl, S), sr.source_positions_serial(cam, pl, S)
        assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
        if R is not None and np.array_equal(R, np.eye(3)):                    # S = I is the undistorter's rule
            u = ur.source_positions(cam, pl)
            assert np.array_equal(a[0].view(np.uint32), u[0].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), u[1].view(np.uint32))
    assert np.isnan(a[0]).any() and not np.isnan(a[0]).all()                  # 100 degrees: part of the lattice looks backwards
    rng = np.random.RandomState(2)
    src = rng.randint(0, 256, (13, 17)).astype(np.uint8)
    out, valid = ur.remap(ur.U8, src, *a)
    outs, valids = ur.remap_serial(ur.U8, src, *a)
    assert np.array_equal(out, outs) and np.array_equal(valid, valids) and not valid[np.isnan(a[0])].any()
