"""CPU restatement (numpy) of DatasetInspector's pose repair: the expected values of the e3d_reg_pick_scan_points / _image_bearings /
_project_points / e3d_pose_from_bearings tests and of bin/ImageLocalizer.  TEST INFRASTRUCTURE ONLY.

  pick      LocalizeImageTool::mousePressEvent (src/dataset_inspector/localize_image_tool.cc:96-110) over the scan points that
            ImageWidget::UpdateScanPoints keeps (gui_image_widget.cc:521-556): a serial loop, strict < from +inf, every f32 operation
            rounded on its own;
  bearings  ImageToNormalized through the undistortion lookup (camera_base_impl.h:188-211), then Vector3d(nx, ny, 1).normalized();
  solve     the minimiser of sum |f_i - (R p_i + t) / |R p_i + t||^2 by a Gauss-Newton iteration in f64, written from that formula;
  move      MainWindow::MoveImage (gui_main_window.cc:851-865) with Sophus' SE3::exp, in f64;
  distribute_relative_pose   MainWindow::DistributeRelativePoseClicked (:605-655), both branches, in f64.

Visibility, projection and occlusion come from mask_transfer_ref.visibility and the CPU checker's reg_binding.cam_project, as
tests/mask_transfer_ref.py obtains them.  An image is described as there: dict(R, t, cam, occlusion)."""
import numpy as np

import mask_transfer_ref as mt
from debug_cloud_ref import F, transform

OUTSIDE, VISIBLE, OCCLUDED = 0, 1, 2
MAX_CLICKS = 32


# ---- scan points of an image ------------------------------------------------------------------------------------------------------------
def scan_points(pts, image, occlusion_threshold=0.01, project=None):
    """-> dict(visible[n] bool, occluded[n] bool, state[n] uint8, pxy (n, 2) f32: the unrounded position, NaN behind the camera).  The
    positions are the ones mask_transfer_ref.visibility asks the projection for: one call per point in front of the camera."""
    if project is None:
        from oracle import reg_binding as rb
        project = rb.cam_project
    seen = []

    def recording(cam, P):
        p = np.asarray(project(cam, P), F).reshape(2)
        seen.append(p)
        return p
    visible, _, _, occluded = mt.visibility(pts, image, occlusion_threshold, recording)
    pp = transform(image["R"], image["t"], pts)
    front = np.nonzero(pp[:, 2] > F(0))[0]
    assert len(front) == len(seen)
    pxy = np.full((len(pp), 2), np.nan, F)
    if len(front):
        pxy[front] = np.array(seen, F).reshape(-1, 2)
    state = np.zeros(len(pp), np.uint8); state[visible] = VISIBLE; state[occluded] = OCCLUDED
    return dict(visible=visible, occluded=occluded, state=state, pxy=pxy)


def squared_distance(pxy, click):
    """Vector2f::squaredNorm of (pxy - click): fl(fl(dx * dx) + fl(dy * dy)), no fused multiply-add."""
    pxy = np.asarray(pxy, F); click = np.asarray(click, F)
    with np.errstate(all="ignore"):
        dx = pxy[..., 0] - click[0]; dy = pxy[..., 1] - click[1]
        return (dx * dx).astype(F) + (dy * dy).astype(F)


def pick_serial(sp, clicks):
    """The loop as written (:96-110), one point at a time -> (indices int64, pixels (k, 2) f32, distances f32, number of visible points)."""
    clicks = np.asarray(clicks, F).reshape(-1, 2)
    index = np.full(len(clicks), -1, np.int64); pixel = np.full((len(clicks), 2), np.nan, F); dist = np.full(len(clicks), np.inf, F)
    order = np.nonzero(sp["visible"])[0]
    for c, click in enumerate(clicks):
        closest = F(np.inf)
        for i in order:
            d = squared_distance(sp["pxy"][i], click)
            if d < closest:
                closest = d; index[c] = i
        if index[c] >= 0:
            pixel[c] = sp["pxy"][index[c]]; dist[c] = closest
    return index, pixel, dist, int(len(order))


def pick(sp, clicks):
    """pick_serial with the loop over the points as array operations: the first minimum of the finite distances is what the strict <
    keeps (tests/test_localize_host.py compares the two)."""
    clicks = np.asarray(clicks, F).reshape(-1, 2)
    index = np.full(len(clicks), -1, np.int64); pixel = np.full((len(clicks), 2), np.nan, F); dist = np.full(len(clicks), np.inf, F)
    order = np.nonzero(sp["visible"])[0]
    for c, click in enumerate(clicks):
        d = squared_distance(sp["pxy"][order], click)
        d = np.where(np.isfinite(d), d, F(np.inf))
        if len(d) and d.min() < np.inf:
            k = int(np.argmin(d))                       # the first of equal minima: the lowest index
            index[c] = order[k]; pixel[c] = sp["pxy"][order[k]]; dist[c] = d[k]
    return index, pixel, dist, int(len(order))


# ---- bearings -----------------------------------------------------------------------------------------------------------------------------
def normalized_coordinates(cam, pixels, lookup=None):
    """ImageToNormalized of every pixel position -> (k, 2) f32."""
    from oracle import multires
    if lookup is None:
        lookup = multires.undistortion_lookup(cam)
    return np.array([multires.image_to_normalized(cam, lookup, float(F(x)), float(F(y))) for x, y in np.asarray(pixels, F).reshape(-1, 2)], F).reshape(-1, 2)


def bearings_from_normalized(nxy):
    v = np.concatenate([np.asarray(nxy, F).astype(np.float64), np.ones((len(nxy), 1))], 1)
    return v / np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + 1.0)[:, None]


def bearings(cam, pixels, lookup=None):
    return bearings_from_normalized(normalized_coordinates(cam, pixels, lookup))


# ---- rotations in f64 --------------------------------------------------------------------------------------------------------------------
def hat(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], np.float64)


def so3_exp(w):
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    K = hat(w)
    if th < 1e-10:
        return np.eye(3) + K + 0.5 * K @ K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K


def quat_to_R(q):
    w, x, y, z = np.asarray(q, np.float64) / np.linalg.norm(np.asarray(q, np.float64))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], np.float64)


def R_to_quat(R):
    from scipy.spatial.transform import Rotation
    x, y, z, w = Rotation.from_matrix(R).as_quat()
    q = np.array([w, x, y, z], np.float64)
    return q / np.linalg.norm(q) * (-1.0 if q[0] < 0 else 1.0)


def rotation_angle(Ra, Rb):
    """The angle of Ra Rb^T, from the skew part (exact for small angles)."""
    D = Ra @ Rb.T
    s = 0.5 * np.array([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    return float(np.arctan2(np.linalg.norm(s), 0.5 * (np.trace(D) - 1)))


# ---- the solver ---------------------------------------------------------------------------------------------------------------------------
def bearing_residuals(R, t, points, f):
    x = points @ R.T + t
    return f - x / np.linalg.norm(x, axis=1)[:, None], x


def rms_angle(R, t, points, f):
    x = points @ R.T + t
    d = x / np.linalg.norm(x, axis=1)[:, None]
    a = np.arctan2(np.linalg.norm(np.cross(f, d), axis=1), (f * d).sum(1))
    return float(np.sqrt((a * a).mean()))


def solve(points, f, q0, t0, iterations=60):
    """Gauss-Newton on r_i = f_i - d_i, d_i = x_i / |x_i|, x_i = R p_i + t, with x -> exp(w) x + v: d r_i / d (w, v) =
    -(I - d d^T) / |x| [-[x]x | I]; every step solved by least squares on the stacked Jacobian -> (R, t) in f64."""
    points = np.asarray(points, np.float64); f = np.asarray(f, np.float64)
    R = quat_to_R(q0); t = np.asarray(t0, np.float64).copy()
    for _ in range(iterations):
        r, x = bearing_residuals(R, t, points, f)
        J = np.zeros((len(points), 3, 6))
        for i in range(len(points)):
            n = np.linalg.norm(x[i]); d = x[i] / n
            J[i] = -(np.eye(3) - np.outer(d, d)) / n @ np.concatenate([-hat(x[i]), np.eye(3)], 1)
        step = np.linalg.lstsq(J.reshape(-1, 6), -r.reshape(-1), rcond=None)[0]
        E = so3_exp(step[:3])
        R = E @ R; t = E @ t + step[3:]
        if np.linalg.norm(step) < 1e-14:
            break
    return R, t


# ---- MoveImage and the relative-pose distribution, f64 -----------------------------------------------------------------------------------
def se3_exp(upsilon, omega):
    """Sophus SE3::exp of (upsilon, omega) -> (R, t): R = exp(omega), t = V upsilon, V = I + (1 - cos th) / th^2 W + (th - sin th) / th^3 W^2."""
    upsilon = np.asarray(upsilon, np.float64); omega = np.asarray(omega, np.float64)
    th = np.linalg.norm(omega)
    W = hat(omega)
    if th < 1e-10:
        V = np.eye(3) + 0.5 * W + W @ W / 6
    else:
        V = np.eye(3) + (1 - np.cos(th)) / th ** 2 * W + (th - np.sin(th)) / th ** 3 * W @ W
    return so3_exp(omega), V @ upsilon


def move(q, t, tx, ty, tz, yaw, roll, pitch):
    """image_T_global = SE3::exp((tx, ty, tz, pitch, yaw, roll)) * image_T_global -> (R, t)."""
    dR, dt = se3_exp((tx, ty, tz), (pitch, yaw, roll))
    return dR @ quat_to_R(q), dR @ np.asarray(t, np.float64) + dt


def _mul(a, b):
    return a[0] @ b[0], a[0] @ b[1] + a[1]


def _inv(a):
    return a[0].T, -a[0].T @ a[1]


def distribute_relative_pose(poses, rig, frames, image_id):
    """poses: {image id: (R, t) image_T_global}, rig: [(R, t) image_T_rig per camera], frames: [[image id per camera] per image set],
    image_id: the image that was moved.  Returns (new poses, new rig); None if the image belongs to no image set."""
    frame = [f for f in frames if image_id in f]
    if not frame:
        return None
    frame = frame[0]
    k = frame.index(image_id)
    poses = dict(poses); rig = list(rig)
    if k != 0:                                             # :627-637
        new = _mul(poses[image_id], _inv(poses[frame[0]]))
        rig[k] = new
        for f in frames:
            poses[f[k]] = _mul(new, poses[f[0]])
    else:                                                  # :638-654
        new = [None] + [_mul(poses[frame[c]], _inv(poses[image_id])) for c in range(1, len(frame))]
        for c in range(1, len(frame)):
            rig[c] = new[c]
        for f in frames:
            poses[f[0]] = _inv(_mul(_inv(poses[f[1]]), new[1]))
    return poses, rig
