"""CPU restatement (numpy) of StereoPairCreator's three rules (include/e3d_hip.h, e3d_reg_stereo_plan / e3d_reg_stereo_rectify /
e3d_reg_stereo_ground_truth): the expected values of the tests of the library calls and of bin/StereoPairCreator.
TEST INFRASTRUCTURE ONLY.  The rules are this project's own, not OpenCV's or Fusiello's.

Plan rule (f64 from the f32 poses image_T_global = (q_i, t_i), every expression left to right as written; Python floats are f64).
    1. q_i / |q_i|; R_i = Eigen's toRotationMatrix; C_i = -R_i^T t_i; b = C_1 - C_0, B = |b|, ex = b / B
    2. zs = row2(R_0) + row2(R_1); ey = normalize(zs x ex), ez = ex x ey; Rr = rows ex, ey, ez
    3. S_i = f32(R_i Rr^T)            4. q_rect = f32(quaternion of Rr, w >= 0)
    5. t_left = f32(-Rr C_0), t_right = f32(-Rr C_0 - (B, 0, 0))
    6. f = f32(focal_length) if > 0 else f32(((fx_0 + fy_0) + (fx_1 + fy_1)) / 4)
    7. each camera's border samples (undistort_ref.border_samples) rotated, r = S_i^T (nx, ny, 1) in f64 with the f32 S_i, sample =
       f32(r.x / r.z, r.y / r.z), NaN where not finite or r.z <= 0; united per side; undistort_ref.plan_from_samples with fx = fy = f
Refused: B not finite or < 1e-9; |zs x ex| < 1e-6 |zs|; ey . (row1(R_0) + row1(R_1)) <= 0 ("swap"); ez . row2(R_i) <= 0; and whatever
plan_from_samples refuses.

Remap rule.  Output pixel (x, y): nx, ny as in undistort_ref; v = S (nx, ny, 1) in f32, each product and sum rounded, (S0 nx + S1 ny) + S2;
invalid if not vz > 0, else (sx, sy) = reg_binding.cam_project(cam, v); from there undistort_ref.remap.

Ground-truth rule.  Counters zero; reg_binding.scan_visibility mode 0 for both rectified images (occlusion depth reg_binding.splat_depth,
exclusion maps normalised to 0 / 1, excluded flag 1); D1, D2 = mode 1 of the left image with min_count 1, 2;
disparity = f32(f64(f) * B / f64(D1)) where D1 is finite else +inf, B = f64(t_left.x) - f64(t_right.x);
mask = 255 where D1 finite and bits(D2) == bits(D1), 128 where D1 finite and they differ, 0 where D1 = +inf."""
import collections
import math

import numpy as np

import undistort_ref as ur

F = np.float32
StereoPlan = collections.namedtuple("StereoPlan", "camera baseline q_rect t_left t_right S_left S_right")


class Refused(ur.Refused):
    pass


class Swapped(Refused):
    """The pair is given right-then-left."""


def quat_matrix(w, x, y, z):
    """Eigen::Quaternion::toRotationMatrix on Python floats, row-major list of 9."""
    tx = 2.0 * x; ty = 2.0 * y; tz = 2.0 * z
    twx = tx * w; twy = ty * w; twz = tz * w
    txx = tx * x; txy = ty * x; txz = tz * x
    tyy = ty * y; tyz = tz * y; tzz = tz * z
    return [1.0 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1.0 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1.0 - (txx + tyy)]


def rotation_quat(R):
    """Quaternion (w, x, y, z) of a row-major rotation, Shepperd's branches, normalised, w >= 0 (Python floats)."""
    tr = R[0] + R[4] + R[8]
    if tr > 0:
        s = math.sqrt(tr + 1.0) * 2
        q = [0.25 * s, (R[7] - R[5]) / s, (R[2] - R[6]) / s, (R[3] - R[1]) / s]
    elif R[0] > R[4] and R[0] > R[8]:
        s = math.sqrt(1.0 + R[0] - R[4] - R[8]) * 2
        q = [(R[7] - R[5]) / s, 0.25 * s, (R[1] + R[3]) / s, (R[2] + R[6]) / s]
    elif R[4] > R[8]:
        s = math.sqrt(1.0 + R[4] - R[0] - R[8]) * 2
        q = [(R[2] - R[6]) / s, (R[1] + R[3]) / s, 0.25 * s, (R[5] + R[7]) / s]
    else:
        s = math.sqrt(1.0 + R[8] - R[0] - R[4]) * 2
        q = [(R[3] - R[1]) / s, (R[2] + R[6]) / s, (R[5] + R[7]) / s, 0.25 * s]
    norm = math.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    sign = -1.0 if q[0] < 0 else 1.0
    return [sign * v / norm for v in q]


def _view(q, t):
    w, x, y, z = (float(F(v)) for v in q)
    n = math.sqrt(w * w + x * x + y * y + z * z)
    R = quat_matrix(w / n, x / n, y / n, z / n)
    t = [float(F(v)) for v in t]
    C = [-(R[k] * t[0] + R[3 + k] * t[1] + R[6 + k] * t[2]) for k in range(3)]
    return R, C


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def frame(poses):
    """Steps 1 - 5 from ((q_left, t_left), (q_right, t_right)) -> (baseline f32, q_rect, t_left, t_right, S_left, S_right), f32 arrays."""
    (R0, C0), (R1, C1) = _view(*poses[0]), _view(*poses[1])
    b = [C1[k] - C0[k] for k in range(3)]
    B = math.sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2])
    if not math.isfinite(B) or B < 1e-9:
        raise Refused("no baseline")
    ex = [v / B for v in b]
    zs = [R0[6 + k] + R1[6 + k] for k in range(3)]
    c = _cross(zs, ex)
    nc = math.sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]); nzs = math.sqrt(zs[0] * zs[0] + zs[1] * zs[1] + zs[2] * zs[2])
    if not (nc >= 1e-6 * nzs) or not nc > 0.0:
        raise Refused("the cameras look along the baseline")
    ey = [v / nc for v in c]
    ez = _cross(ex, ey)
    ys = [R0[3 + k] + R1[3 + k] for k in range(3)]
    if not _dot(ey, ys) > 0.0:
        raise Swapped("right-then-left: swap")
    for R in (R0, R1):
        if not _dot(ez, R[6:9]) > 0.0:
            raise Refused("a camera looks away from the rectified viewing direction")
    Rr = ex + ey + ez
    S = [np.array([R[3 * r] * Rr[3 * k] + R[3 * r + 1] * Rr[3 * k + 1] + R[3 * r + 2] * Rr[3 * k + 2] for r in range(3) for k in range(3)], np.float64).astype(F)
         for R in (R0, R1)]
    q = np.array(rotation_quat(Rr), np.float64).astype(F)
    tl = [-(Rr[3 * k] * C0[0] + Rr[3 * k + 1] * C0[1] + Rr[3 * k + 2] * C0[2]) for k in range(3)]
    tr = [tl[0] - B, tl[1], tl[2]]
    return F(B), q, np.array(tl, np.float64).astype(F), np.array(tr, np.float64).astype(F), S[0], S[1]


def rotated_samples(samples, S):
    """Step 7 for one camera: its four (k, 2) f32 border sample arrays through S^T -> four (k, 2) f32 arrays, NaN = non-finite."""
    s = [float(v) for v in np.asarray(S, F).reshape(9)]
    out = []
    for a in samples:
        nx = np.asarray(a, F)[:, 0].astype(np.float64); ny = np.asarray(a, F)[:, 1].astype(np.float64)
        with np.errstate(all="ignore"):
            rx = s[0] * nx + s[3] * ny + s[6]; ry = s[1] * nx + s[4] * ny + s[7]; rz = s[2] * nx + s[5] * ny + s[8]
            u = rx / rz; v = ry / rz
            ok = (rz > 0.0) & np.isfinite(u) & np.isfinite(v)
            out.append(np.stack([np.where(ok, u, np.nan), np.where(ok, v, np.nan)], 1).astype(F))
    return out


def plan(cams, poses, blank_pixels=0.0, max_image_size=-1, focal_length=0.0, samples=None):
    """The stereo plan of two reg_binding cameras (left, right) at their poses ((q, t), (q, t)); samples: their border samples."""
    if not (0.0 <= float(blank_pixels) <= 1.0):
        raise Refused("blank_pixels outside [0, 1]")
    B, q, tl, tr, S0, S1 = frame(poses)
    if float(focal_length) > 0.0:
        f = F(float(focal_length))
    else:
        f = F(((float(F(cams[0].p[0])) + float(F(cams[0].p[1]))) + (float(F(cams[1].p[0])) + float(F(cams[1].p[1])))) / 4.0)
    if samples is None:
        samples = [ur.border_samples(c) for c in cams]
    rot = [rotated_samples(samples[0], S0), rotated_samples(samples[1], S1)]
    united = [np.concatenate([rot[0][k], rot[1][k]]) for k in range(4)]
    camera = ur.plan_from_samples(united, f, f, blank_pixels, max_image_size)
    return StereoPlan(camera, B, q, tl, tr, S0, S1)


def _rays(pl, S):
    """v = S (nx, ny, 1) of every output pixel in f32: three (H', W') arrays."""
    nx, ny = ur.normalized_lattice(pl)
    nx = nx[None, :]; ny = ny[:, None]
    s = np.asarray(S, F).reshape(9)
    return [(((s[3 * r] * nx).astype(F) + (s[3 * r + 1] * ny).astype(F)).astype(F) + s[3 * r + 2]).astype(F) for r in range(3)]


def source_positions(cam, pl, S, project=None):
    """(sx, sy): (H', W') f32 each; NaN where the ray does not point into the source camera's front half space."""
    if project is None:
        from oracle import reg_binding as rb
        project = rb.cam_project
    vx, vy, vz = _rays(pl, S)
    out = np.full((pl.height, pl.width, 2), np.nan, F)
    P = np.zeros(3, F)
    for y in range(pl.height):
        for x in range(pl.width):
            if vz[y, x] > 0:
                P[0] = vx[y, x]; P[1] = vy[y, x]; P[2] = vz[y, x]
                out[y, x] = project(cam, P)
    return out[..., 0], out[..., 1]


def source_positions_serial(cam, pl, S, project=None):
    """source_positions one pixel at a time with scalar f32 arithmetic, as the rule is written."""
    if project is None:
        from oracle import reg_binding as rb
        project = rb.cam_project
    s = [F(v) for v in np.asarray(S, F).reshape(9)]
    out = np.full((pl.height, pl.width, 2), np.nan, F)
    for y in range(pl.height):
        ny = F(F(F(y) - F(pl.cy)) / F(pl.fy))
        for x in range(pl.width):
            nx = F(F(F(x) - F(pl.cx)) / F(pl.fx))
            v = [F(F(F(s[3 * r] * nx) + F(s[3 * r + 1] * ny)) + s[3 * r + 2]) for r in range(3)]
            if v[2] > 0:
                out[y, x] = project(cam, np.array(v, F))
    return out[..., 0], out[..., 1]


def disparity_and_mask(D1, D2, f, B):
    """The per-pixel rule of the ground truth -> (disparity f32, mask u8)."""
    D1 = np.asarray(D1, F); D2 = np.asarray(D2, F)
    known = np.isfinite(D1)
    with np.errstate(all="ignore"):
        d = (float(F(f)) * float(B) / np.where(known, D1, F(1)).astype(np.float64)).astype(F)
    disparity = np.where(known, d, F(np.inf)).astype(F)
    same = D1.view(np.uint32) == D2.view(np.uint32)
    mask = np.where(known, np.where(same, 255, 128), 0).astype(np.uint8)
    return disparity, mask


def ground_truth(scan, splats, splat_radius, cam, q_rect, t_left, t_right, left_excluded=None, right_excluded=None, occlusion_threshold=0.01):
    """-> (disparity, mask, D1, counts) of the restatement; cam: the rectified reg_binding PINHOLE camera."""
    from oracle import binding as ob
    from oracle import reg_binding as rb
    R = ob.quat_to_R(np.asarray(q_rect, F))
    tl = np.asarray(t_left, F); tr = np.asarray(t_right, F)
    counts = np.zeros(len(scan), np.int32)
    norm = lambda m: None if m is None else (np.asarray(m) != 0).astype(np.uint8)       # noqa: E731
    ml, mr = norm(left_excluded), norm(right_excluded)
    occ_l = rb.splat_depth(splats, R, tl, cam, splat_radius); occ_r = rb.splat_depth(splats, R, tr, cam, splat_radius)
    rb.scan_visibility(scan, R, tr, cam, occ_r, counts, mask=mr, excluded=1, occlusion_threshold=occlusion_threshold)
    rb.scan_visibility(scan, R, tl, cam, occ_l, counts, mask=ml, excluded=1, occlusion_threshold=occlusion_threshold)
    D1 = rb.scan_visibility(scan, R, tl, cam, occ_l, counts, mask=ml, excluded=1, mode=1, min_count=1, occlusion_threshold=occlusion_threshold)
    D2 = rb.scan_visibility(scan, R, tl, cam, occ_l, counts, mask=ml, excluded=1, mode=1, min_count=2, occlusion_threshold=occlusion_threshold)
    B = float(tl[0]) - float(tr[0])
    disparity, mask = disparity_and_mask(D1, D2, cam.p[0], B)
    return disparity, mask, D1, counts


# ---- file formats of bin/StereoPairCreator ----------------------------------------------------------------------------------------------
def write_pfm(path, a):
    """One-channel PFM: 'Pf', 'W H', '-1.0' (little-endian), rows bottom to top."""
    a = np.asarray(a, F)
    with open(path, "wb") as f:
        f.write(b"Pf\n%d %d\n-1.0\n" % (a.shape[1], a.shape[0]))
        f.write(np.ascontiguousarray(a[::-1]).astype("<f4").tobytes())


def read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"Pf"
        w, h = (int(v) for v in f.readline().split())
        scale = float(f.readline())
        data = np.frombuffer(f.read(), "<f4" if scale < 0 else ">f4")
    assert data.size == w * h
    return data.reshape(h, w)[::-1].astype(F)


def calib_text(pl):
    """calib.txt of a StereoPlan: Middlebury's keys, nine digits, pixel-centre principal point, baseline in the scans' unit."""
    c = pl.camera
    k = "[%.9g 0 %.9g; 0 %.9g %.9g; 0 0 1]" % (float(c.fx), float(c.cx), float(c.fx), float(c.cy))
    return "cam0=%s\ncam1=%s\ndoffs=0\nbaseline=%.9g\nwidth=%d\nheight=%d\n" % (k, k, float(pl.baseline), c.width, c.height)


def parse_calib(text):
    """-> dict: cam0 / cam1 as 3 x 3 float arrays, doffs, baseline as floats, width, height as ints."""
    out = {}
    for line in text.splitlines():
        key, value = line.split("=", 1)
        if key in ("cam0", "cam1"):
            out[key] = np.array([[float(v) for v in row.split()] for row in value.strip("[]").split(";")])
        elif key in ("width", "height"):
            out[key] = int(value)
        else:
            out[key] = float(value)
    return out


def colmap_image_lines(pl, names):
    """The two image lines of images.txt (ids 0, 1; camera 0), nine digits, each followed by an empty 2D line."""
    q = [float(v) for v in pl.q_rect]
    lines = []
    for i, (t, name) in enumerate(zip((pl.t_left, pl.t_right), names)):
        lines.append("%d %.9g %.9g %.9g %.9g %.9g %.9g %.9g 0 %s" % ((i,) + tuple(q) + tuple(float(v) for v in t) + (name,)))
        lines.append("")
    return lines
