"""The numpy restatement of ImageUndistorter's two rules (tests/undistort_ref.py) checked on its own, without a GPU: what the rules promise
(an identity for a lattice-aligned PINHOLE, full validity at blank_pixels = 0, full coverage at 1, the size limit), the per-kind
arithmetic on hand-made cases, and the array form against the pixel-at-a-time form.  tests/test_gpu_undistort.py then compares the
library with this restatement bit for bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import undistort_ref as ur  # noqa: E402
from oracle import reg_binding as rb  # noqa: E402
from test_oracle_camera import CAMERAS  # noqa: E402

F = np.float32


def camera(name, width, height):
    t, p = CAMERAS[name]
    return rb.make_camera(width, height, ur.scaled_params(p, t, width, height), t)


def test_aligned_pinhole_is_an_identity():
    """Power-of-two focal lengths and an integral principal point: every step of both rules is exact, so the plan is the source camera
    and the image comes back unchanged with every pixel valid, the last row and column included (the closed interval)."""
    W, H = 16, 12
    cam = rb.make_camera(W, H, np.array([16.0, 8.0, 7.0, 5.0], F), rb.PINHOLE)
    for b in (0.0, 0.5, 1.0):
        pl = ur.plan(cam, b)
        assert pl == ur.Plan(W, H, F(16), F(8), F(7), F(5))
    sx, sy = ur.source_positions(cam, pl)
    assert np.array_equal(sx, np.tile(np.arange(W, dtype=F), (H, 1))) and np.array_equal(sy, np.tile(np.arange(H, dtype=F)[:, None], (1, W)))
    rng = np.random.RandomState(0)
    for kind, src in ((ur.U8, rng.randint(0, 256, (H, W)).astype(np.uint8)), (ur.RGB, rng.randint(0, 256, (H, W, 3)).astype(np.uint8)),
                      (ur.NEAREST, rng.uniform(0.5, 9, (H, W)).astype(F))):
        out, valid = ur.remap(kind, src, sx, sy)
        assert valid.all() and np.array_equal(out, src)
    # a mask ORs the whole 2 x 2 block at (ix, iy), whatever the weights: a masked pixel reaches the output pixels above and left of it
    mask = np.zeros((H, W), np.uint8); mask[3, 4] = 1; mask[H - 1, W - 1] = 2
    out, valid = ur.remap(ur.MASK, mask, sx, sy)
    want = np.zeros((H, W), np.uint8); want[2:4, 3:5] = 1; want[H - 2:, W - 2:] = 2
    assert valid.all() and np.array_equal(out, want)


@pytest.fixture(scope="module")
def barrel():
    cam = camera("OPENCV", 64, 48)
    return cam, ur.border_samples(cam)


def test_barrel_without_blank_pixels_is_valid_everywhere(barrel):
    cam, samples = barrel
    pl = ur.plan(cam, 0.0, samples=samples)
    sx, sy = ur.source_positions(cam, pl)
    assert ur.valid_map(sx, sy, cam.width, cam.height).all()
    assert pl.width >= 48 and pl.height >= 36                   # a crop, not a sliver


def test_barrel_with_blank_pixels_holds_every_source_border_pixel(barrel):
    cam, samples = barrel
    pl = ur.plan(cam, 1.0, samples=samples)
    for s in samples:
        x = float(pl.fx) * s[:, 0].astype(np.float64) + float(pl.cx); y = float(pl.fy) * s[:, 1].astype(np.float64) + float(pl.cy)
        assert (x >= 0).all() and (x <= pl.width - 1).all() and (y >= 0).all() and (y <= pl.height - 1).all()
    p0 = ur.plan(cam, 0.0, samples=samples); ph = ur.plan(cam, 0.5, samples=samples)
    assert p0.width <= ph.width <= pl.width and p0.height <= ph.height <= pl.height and pl.width > p0.width
    assert p0.fx == ph.fx == pl.fx == F(cam.p[0]) and pl.fy == F(cam.p[1])            # the focal length is kept
    assert all(float(v).is_integer() for v in (pl.cx, pl.cy, p0.cx, p0.cy))


def test_max_image_size_is_honoured(barrel):
    cam, samples = barrel
    full = ur.plan(cam, 1.0, samples=samples)
    for limit in (full.width + 10, full.width, 40, 17, 6):
        pl = ur.plan(cam, 1.0, limit, samples=samples)
        assert max(pl.width, pl.height) <= limit
        if limit >= full.width + 1:
            assert pl == full
        else:
            assert pl.fx < full.fx and max(pl.width, pl.height) >= limit - 2


def test_plan_refusals(barrel):
    cam, samples = barrel
    for b in (-0.01, 1.01, float("nan")):
        with pytest.raises(ur.Refused):
            ur.plan(cam, b, samples=samples)
    broken = [s.copy() for s in samples]
    broken[0][3] = np.inf
    assert ur.plan_from_samples(broken, cam.p[0], cam.p[1], 0.0).width >= 48         # skipped at b = 0
    with pytest.raises(ur.Refused):
        ur.plan_from_samples(broken, cam.p[0], cam.p[1], 0.25)
    broken[0][:] = np.nan
    with pytest.raises(ur.Refused):
        ur.plan_from_samples(broken, cam.p[0], cam.p[1], 0.0)
    swapped = (samples[1], samples[0], samples[2], samples[3])
    with pytest.raises(ur.Refused):
        ur.plan_from_samples(swapped, cam.p[0], cam.p[1], 0.0)
    with pytest.raises(ur.Refused):
        ur.plan_from_samples(samples, 1.0, 1.0, 0.0)                                  # a one-pixel image


def _positions(rows):
    a = np.array(rows, F)
    return np.ascontiguousarray(a[..., 0]), np.ascontiguousarray(a[..., 1])


def test_mask_is_the_or_of_the_four_pixels():
    mask = np.array([[0, 1, 0], [0, 0, 2], [0, 0, 0]], np.uint8)
    sx, sy = _positions([[(0.0, 0.0), (0.5, 0.5), (1.25, 0.0)], [(1.0, 1.0), (0.0, 1.5), (2.0, 2.0)], [(-0.01, 0.0), (0.0, 2.01), (np.inf, 1.0)]])
    out, valid = ur.remap(ur.MASK, mask, sx, sy)
    #   (0,0): block rows 0-1, cols 0-1 -> 1     (0.5,0.5): same block -> 1     (1.25,0): cols 1-2 -> 1 | 2 = 3
    #   (1,1): rows 1-2, cols 1-2 -> 2           (0,1.5): rows 1-2, cols 0-1 -> 0     (2,2): clamped to rows 1-2, cols 1-2 -> 2
    assert out.tolist() == [[1, 1, 3], [2, 0, 2], [3, 3, 3]]
    assert valid.tolist() == [[1, 1, 1], [1, 1, 1], [0, 0, 0]]
    assert all(np.array_equal(a, b) for a, b in zip(ur.remap_serial(ur.MASK, mask, sx, sy), (out, valid)))


def test_nearest_copies_bits():
    nan = np.array([0x7fc12345], np.uint32).view(F)[0]             # a NaN with a payload
    depth = np.array([[1.5, nan, 0.0], [np.inf, 2.25, -np.inf], [3.0, 0.0, 7.0]], F)
    sx, sy = _positions([[(0.49, 0.0), (0.5, 0.0), (2.0, 0.4)], [(0.2, 0.5), (1.0, 1.49), (1.5, 1.0)], [(2.0, 2.0), (2.01, 2.0), (np.nan, 0.0)]])
    out, valid = ur.remap(ur.NEAREST, depth, sx, sy)
    want = np.array([[1.5, nan, 0.0], [np.inf, 2.25, -np.inf], [7.0, 0.0, 0.0]], F)
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))
    assert valid.tolist() == [[1, 1, 1], [1, 1, 1], [1, 0, 0]]
    got = ur.remap_serial(ur.NEAREST, depth, sx, sy)
    assert np.array_equal(got[0].view(np.uint32), out.view(np.uint32)) and np.array_equal(got[1], valid)


def test_bilinear_by_hand():
    img = np.array([[0, 100, 200], [50, 150, 250], [10, 20, 30]], np.uint8)
    sx, sy = _positions([[(0.0, 0.0), (0.5, 0.0), (2.0, 0.0)], [(0.25, 0.5), (2.0, 2.0), (1.0, 1.75)], [(2.0001, 0.0), (0.0, -1e-7), (1.005, 1.0)]])
    out, valid = ur.remap(ur.U8, img, sx, sy)
    #   (0.25, 0.5): top 25, bottom 75 -> 50     (1, 1.75): 0.25 * 150 + 0.75 * 20 = 52.5 -> 53     (1.005, 1): 150.5 -> int(151.0) = 151
    assert out.tolist() == [[0, 50, 200], [50, 30, 53], [0, 0, 151]]
    assert valid.tolist() == [[1, 1, 1], [1, 1, 1], [0, 0, 1]]
    rgb = np.stack([img, 255 - img, img // 2], 2)
    out3, valid3 = ur.remap(ur.RGB, rgb, sx, sy)
    assert np.array_equal(valid3, valid) and np.array_equal(out3[..., 0], out)
    assert np.array_equal(out3[..., 1], ur.remap(ur.U8, rgb[..., 1].copy(), sx, sy)[0])


@pytest.mark.parametrize("name", ["OPENCV", "THIN_PRISM_FISHEYE", "FOV"])
def test_array_form_equals_the_serial_form(name):
    cam = camera(name, 17, 13)
    pl = ur.plan(cam, 0.0 if name == "FOV" else 1.0)
    sx, sy = ur.source_positions(cam, pl)
    rng = np.random.RandomState(5)
    depth = rng.uniform(0.5, 9, (13, 17)).astype(F); depth[rng.rand(13, 17) < 0.2] = 0; depth[2, 3] = np.nan
    for kind, src in ((ur.U8, rng.randint(0, 256, (13, 17)).astype(np.uint8)), (ur.RGB, rng.randint(0, 256, (13, 17, 3)).astype(np.uint8)),
                      (ur.MASK, rng.randint(0, 3, (13, 17)).astype(np.uint8)), (ur.NEAREST, depth)):
        a, b = ur.remap(kind, src, sx, sy), ur.remap_serial(kind, src, sx, sy)
        assert np.array_equal(a[0].view(np.uint32) if kind == ur.NEAREST else a[0], b[0].view(np.uint32) if kind == ur.NEAREST else b[0])
        assert np.array_equal(a[1], b[1])


def test_camera_line_uses_the_pixel_corner_convention():
    assert ur.colmap_camera_line(3, ur.Plan(65, 49, F(34.0926), F(34.1124), F(31), F(22))) == "3 PINHOLE 65 49 34.0926018 34.1124001 31.5 22.5"
