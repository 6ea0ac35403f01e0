"""CPU restatement (numpy) of ImageUndistorter's two rules (include/e3d_hip.h, e3d_reg_undistort_plan / e3d_reg_undistort):
the expected values of the tests of the library calls and of bin/ImageUndistorter.  TEST INFRASTRUCTURE ONLY.  Both rules are this
project's own, not COLMAP's.

Plan rule.  The level-0 model (W x H, focal lengths fx, fy) is sampled at its border pixel centres (0, y), (W - 1, y) of every row and
(x, 0), (x, H - 1) of every column; each goes through ImageToNormalized in f32 (localize_ref.normalized_coordinates, the CPU checker's
undistortion lookup: the bits the device computes).  Per side the inner / outer extent of the samples:
    left  L_in = max nx, L_out = min nx     right  R_in = min nx, R_out = max nx
    top   T_in = max ny, T_out = min ny     bottom B_in = min ny, B_out = max ny
In f64 with b = blank_pixels in [0, 1]: nL = b * L_out + (1 - b) * L_in, likewise nR, nT, nB.  s = 1, or, if max_image_size > 0 and
e + 1 + 2 b exceeds it, e = max(fx * (nR - nL), fy * (nB - nT)): s = (max_image_size - 1 - 2 b) / e.  fx' = f32(s * fx), fy' = f32(s * fy).
Inner bounds are rounded inwards, outer bounds outwards, and the two blended as integers:
    x0 = ceil(b * floor(fx' * L_out) + (1 - b) * ceil(fx' * L_in)),  x1 = floor(b * ceil(fx' * R_out) + (1 - b) * floor(fx' * R_in)),
W' = x1 - x0 + 1, cx' = -x0, the same in y.  (An outer bound rounded inwards would leave up to a pixel of the source outside the output
at b = 1, an inner bound rounded outwards a blank pixel at b = 0: tests/test_undistort_host.py checks both promises.)  Non-finite samples are skipped at b = 0 and refused at b > 0; refused as well: a side without a
finite sample, nL >= nR, nT >= nB, W' or H' < 2 (or >= 2^24), a max_image_size that leaves s <= 0, b outside [0, 1].

Remap rule.  Output pixel (x, y): nx = fl((f32(x) - cx') / fx'), ny = fl((f32(y) - cy') / fy'), (sx, sy) = the model's
NormalizedToImage(nx, ny) (reg_binding.cam_project of (nx, ny, 1): the same bits as the device function; +-inf past a cut-off).  Valid iff
sx, sy finite, 0 <= sx <= W - 1, 0 <= sy <= H - 1.  Then ix = min(int(sx), W - 2), iy = min(int(sy), H - 2), ax = sx - ix, ay = sy - iy;
    bilinear  v = (1 - ay) * ((1 - ax) * p00 + ax * p10) + ay * ((1 - ax) * p01 + ax * p11), every operation rounded to f32; u8(int(v + 0.5))
    mask      p00 | p10 | p01 | p11
    nearest   the f32 at (min(int(sx + 0.5), W - 1), min(int(sy + 0.5), H - 1)), bits copied
An invalid pixel is 0 (3 for a mask), its valid flag 0."""
import collections
import math

import numpy as np

import localize_ref as lr

F = np.float32
Plan = collections.namedtuple("Plan", "width height fx fy cx cy")      # fx .. cy are np.float32
U8, RGB, MASK, NEAREST = 0, 1, 2, 3
UNIQUE_FOCAL = (5, 6, 7, 11, 12)
FISHEYE = (2, 3, 9, 11, 12)


class Refused(ValueError):
    pass


def scaled_params(params, camera_type, width, height, from_size=(640, 480)):
    """Parameters given for a from_size image, for the same field of view at width x height (pixel-centre convention)."""
    p = [float(v) for v in params]
    kx, ky = width / from_size[0], height / from_size[1]
    if camera_type in UNIQUE_FOCAL:
        p[0] *= kx; p[1] = (p[1] + 0.5) * kx - 0.5; p[2] = (p[2] + 0.5) * ky - 0.5
    else:
        p[0] *= kx; p[1] *= ky; p[2] = (p[2] + 0.5) * kx - 0.5; p[3] = (p[3] + 0.5) * ky - 0.5
    return np.array(p, F)


def border_pixels(width, height):
    """-> (left, right, top, bottom): the pixel centres of the four border lines, (k, 2) f32 each."""
    ys = np.arange(height, dtype=F); xs = np.arange(width, dtype=F)
    col = lambda x: np.stack([np.full(height, x, F), ys], 1)        # noqa: E731
    row = lambda y: np.stack([xs, np.full(width, y, F)], 1)         # noqa: E731
    return col(0), col(width - 1), row(0), row(height - 1)


def border_samples(cam):
    """ImageToNormalized of the border pixel centres -> four (k, 2) f32 arrays (left, right, top, bottom)."""
    from oracle import multires
    lookup = multires.undistortion_lookup(cam)
    return tuple(lr.normalized_coordinates(cam, px, lookup) for px in border_pixels(cam.width, cam.height))


def plan_from_samples(samples, fx, fy, blank_pixels=0.0, max_image_size=-1):
    """The plan rule from the border samples and the model's focal lengths (f32)."""
    b = float(blank_pixels)
    if not (0.0 <= b <= 1.0):
        raise Refused("blank_pixels outside [0, 1]")
    ext = []
    for s, coordinate, low in zip(samples, (0, 0, 1, 1), (True, False, True, False)):
        s = np.asarray(s, F)
        finite = np.isfinite(s).all(1)
        if not finite.all() and b > 0.0:
            raise Refused("non-finite border sample and blank_pixels > 0")
        v = s[finite, coordinate].astype(np.float64)
        if not len(v):
            raise Refused("a side without a finite sample")
        ext.append((float(v.max()), float(v.min())) if low else (float(v.min()), float(v.max())))      # (inner, outer)
    nL, nR, nT, nB = (b * outer + (1.0 - b) * inner for inner, outer in ext)
    if not (nL < nR) or not (nT < nB):
        raise Refused("empty extent")
    fx = float(F(fx)); fy = float(F(fy))
    s = 1.0
    e = max(fx * (nR - nL), fy * (nB - nT)); margin = 1.0 + 2.0 * b
    if max_image_size > 0 and e + margin > float(max_image_size):
        s = (float(max_image_size) - margin) / e
        if not s > 0.0:
            raise Refused("max_image_size leaves no room")
    fxp, fyp = F(s * fx), F(s * fy)
    low_bound = lambda f, io: math.ceil(b * math.floor(f * io[1]) + (1.0 - b) * math.ceil(f * io[0]))        # noqa: E731
    high_bound = lambda f, io: math.floor(b * math.ceil(f * io[1]) + (1.0 - b) * math.floor(f * io[0]))      # noqa: E731
    x0, x1 = low_bound(float(fxp), ext[0]), high_bound(float(fxp), ext[1])
    y0, y1 = low_bound(float(fyp), ext[2]), high_bound(float(fyp), ext[3])
    w, h = x1 - x0 + 1, y1 - y0 + 1
    if w < 2 or h < 2:
        raise Refused("smaller than 2 x 2")
    if not (abs(x0) < 2 ** 24 and abs(y0) < 2 ** 24 and w < 2 ** 24 and h < 2 ** 24):
        raise Refused("larger than 2^24 a side")
    return Plan(int(w), int(h), fxp, fyp, F(-x0), F(-y0))


def plan(cam, blank_pixels=0.0, max_image_size=-1, samples=None):
    """The plan of a reg_binding camera (its struct holds [fx fy cx cy ...] for every model, fx = fy for the one-focal-length ones)."""
    return plan_from_samples(border_samples(cam) if samples is None else samples, cam.p[0], cam.p[1], blank_pixels, max_image_size)


def normalized_lattice(pl):
    """nx (W',) and ny (H',) of the output lattice: one f32 subtraction and one f32 division each."""
    nx = ((np.arange(pl.width, dtype=F) - F(pl.cx)) / F(pl.fx)).astype(F)
    ny = ((np.arange(pl.height, dtype=F) - F(pl.cy)) / F(pl.fy)).astype(F)
    return nx, ny


def source_positions(cam, pl, project=None):
    """(sx, sy): (H', W') f32 each, the source position of every output pixel."""
    if project is None:
        from oracle import reg_binding as rb
        project = rb.cam_project
    nx, ny = normalized_lattice(pl)
    out = np.zeros((pl.height, pl.width, 2), F)
    P = np.ones(3, F)
    for y in range(pl.height):
        P[1] = ny[y]
        for x in range(pl.width):
            P[0] = nx[x]
            out[y, x] = project(cam, P)
    return out[..., 0], out[..., 1]


def valid_map(sx, sy, width, height):
    with np.errstate(invalid="ignore"):
        return np.isfinite(sx) & np.isfinite(sy) & (sx >= 0) & (sx <= F(width - 1)) & (sy >= 0) & (sy <= F(height - 1))


def remap(kind, src, sx, sy):
    """One source image through the positions -> (output, valid uint8)."""
    src = np.asarray(src)
    H, W = src.shape[:2]
    ok = valid_map(sx, sy, W, H)
    sxv = np.where(ok, sx, F(0)).astype(F); syv = np.where(ok, sy, F(0)).astype(F)
    if kind == NEAREST:
        assert src.dtype == np.float32 and src.ndim == 2
        ix = np.minimum((sxv + F(0.5)).astype(F).astype(np.int64), W - 1); iy = np.minimum((syv + F(0.5)).astype(F).astype(np.int64), H - 1)
        bits = src.view(np.uint32)[iy, ix]
        return np.where(ok, bits, np.uint32(0)).astype(np.uint32).view(np.float32), ok.astype(np.uint8)
    assert src.dtype == np.uint8
    ix = np.minimum(sxv.astype(np.int64), W - 2); iy = np.minimum(syv.astype(np.int64), H - 2)
    if kind == MASK:
        assert src.ndim == 2
        v = src[iy, ix] | src[iy, ix + 1] | src[iy + 1, ix] | src[iy + 1, ix + 1]
        return np.where(ok, v, np.uint8(3)).astype(np.uint8), ok.astype(np.uint8)
    assert (kind == U8 and src.ndim == 2) or (kind == RGB and src.ndim == 3 and src.shape[2] == 3)
    ax = (sxv - ix.astype(F)).astype(F); ay = (syv - iy.astype(F)).astype(F)
    bx = (F(1) - ax).astype(F); by = (F(1) - ay).astype(F)
    if src.ndim == 3:
        ax, ay, bx, by = (a[..., None] for a in (ax, ay, bx, by))
    p00 = src[iy, ix].astype(F); p10 = src[iy, ix + 1].astype(F); p01 = src[iy + 1, ix].astype(F); p11 = src[iy + 1, ix + 1].astype(F)
    top = ((bx * p00).astype(F) + (ax * p10).astype(F)).astype(F)
    bottom = ((bx * p01).astype(F) + (ax * p11).astype(F)).astype(F)
    v = ((by * top).astype(F) + (ay * bottom).astype(F)).astype(F)
    out = (v + F(0.5)).astype(F).astype(np.int64).astype(np.uint8)
    okc = ok[..., None] if src.ndim == 3 else ok
    return np.where(okc, out, np.uint8(0)).astype(np.uint8), ok.astype(np.uint8)


def remap_serial(kind, src, sx, sy):
    """remap() one pixel at a time, as the rule is written (tests/test_undistort_host.py compares the two)."""
    src = np.asarray(src)
    H, W = src.shape[:2]
    out = np.zeros(sx.shape + src.shape[2:], src.dtype); valid = np.zeros(sx.shape, np.uint8)
    for y in range(sx.shape[0]):
        for x in range(sx.shape[1]):
            a, b = sx[y, x], sy[y, x]
            if not (np.isfinite(a) and np.isfinite(b) and 0 <= a <= F(W - 1) and 0 <= b <= F(H - 1)):
                out[y, x] = 3 if kind == MASK else 0
                continue
            valid[y, x] = 1
            if kind == NEAREST:
                out.view(np.uint32)[y, x] = src.view(np.uint32)[min(int(F(b + F(0.5))), H - 1), min(int(F(a + F(0.5))), W - 1)]
                continue
            ix, iy = min(int(a), W - 2), min(int(b), H - 2)
            if kind == MASK:
                out[y, x] = src[iy, ix] | src[iy, ix + 1] | src[iy + 1, ix] | src[iy + 1, ix + 1]
                continue
            ax, ay = F(a - F(ix)), F(b - F(iy))
            bx, by = F(F(1) - ax), F(F(1) - ay)
            for c in range(3 if kind == RGB else 1):
                p = (lambda j, i: F(src[j, i, c])) if kind == RGB else (lambda j, i: F(src[j, i]))
                v = F(F(by * F(F(bx * p(iy, ix)) + F(ax * p(iy, ix + 1)))) + F(ay * F(F(bx * p(iy + 1, ix)) + F(ax * p(iy + 1, ix + 1)))))
                if kind == RGB:
                    out[y, x, c] = int(F(v + F(0.5)))
                else:
                    out[y, x] = int(F(v + F(0.5)))
    return out, valid


def colmap_camera_line(camera_id, pl):
    """The PINHOLE line of calibration/cameras.txt: COLMAP's pixel-corner convention, principal point + 0.5."""
    return "%d PINHOLE %d %d %.9g %.9g %.9g %.9g" % (camera_id, pl.width, pl.height, float(pl.fx), float(pl.fy), float(pl.cx) + 0.5, float(pl.cy) + 0.5)
