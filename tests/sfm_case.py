"""A synthetic SfMScaleEstimator case (test infrastructure): two scans at known poses, their cube map depth files, and a COLMAP
model whose geometry is the true geometry divided by k.  Used on the CPU (depth files from tests/cubemap_ref.py) and on the GPU
(depth files written by bin/CubeMapRenderer)."""
import os
import re

import numpy as np

import cubemap_ref as cr
from cli_util import write_ply_xyz

F = np.float32
SIZE = 64
R_FACE = {"front": [[1, 0, 0], [0, 1, 0], [0, 0, 1]], "left": [[0, 0, 1], [0, 1, 0], [-1, 0, 0]],
          "back": [[-1, 0, 0], [0, 1, 0], [0, 0, -1]], "right": [[0, 0, -1], [0, 1, 0], [1, 0, 0]],
          "down": [[1, 0, 0], [0, 0, -1], [0, 1, 0]], "up": [[1, 0, 0], [0, 0, 1], [0, -1, 0]]}


def _rot(axis, angle):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def _quat(R):
    """w x y z of a rotation matrix (float64)"""
    w = np.sqrt(max(0.0, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    x = np.sqrt(max(0.0, 1 + R[0, 0] - R[1, 1] - R[2, 2])) / 2
    y = np.sqrt(max(0.0, 1 - R[0, 0] + R[1, 1] - R[2, 2])) / 2
    z = np.sqrt(max(0.0, 1 - R[0, 0] - R[1, 1] + R[2, 2])) / 2
    i = int(np.argmax([w, x, y, z]))
    if i == 0:
        x, y, z = (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)
    elif i == 1:
        w, y, z = (R[2, 1] - R[1, 2]) / (4 * x), (R[0, 1] + R[1, 0]) / (4 * x), (R[0, 2] + R[2, 0]) / (4 * x)
    elif i == 2:
        w, x, z = (R[0, 2] - R[2, 0]) / (4 * y), (R[0, 1] + R[1, 0]) / (4 * y), (R[1, 2] + R[2, 1]) / (4 * y)
    else:
        w, x, y = (R[1, 0] - R[0, 1]) / (4 * z), (R[0, 2] + R[2, 0]) / (4 * z), (R[1, 2] + R[2, 1]) / (4 * z)
    return np.array([w, x, y, z])


def room_scan(seed, n=20000):
    """points of a box room seen from an off-centre scanner, in the scanner's frame, with colours"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    lo, hi = np.array([-3.0, -1.5, -2.5]), np.array([2.0, 2.5, 4.0])
    with np.errstate(divide="ignore"):
        t = np.where(d > 0, hi / d, np.where(d < 0, lo / d, np.inf)).min(1)
    xyz = (d * t[:, None]).astype(F)
    rgb = np.clip(128 + 40 * xyz, 0, 255).astype(np.uint8)
    return xyz, rgb


def build(tmp, k=3.7, with_scan3=True, write_depth=True, seed=5):
    """writes tmp/{scans, images, model}; returns a dict describing the case"""
    rng = np.random.default_rng(seed)
    scans, images, model = (os.path.join(tmp, d) for d in ("scans", "images", "model"))
    for d in (scans, images, model):
        os.makedirs(d, exist_ok=True)
    poses = {"scan1.ply": (_rot([0.2, 1.0, 0.1], 0.7), np.array([1.5, -0.4, 2.25])),
             "scan2.ply": (_rot([1.0, 0.3, -0.5], -1.1), np.array([-2.0, 0.75, 0.5]))}
    face_order = {"scan1.ply": ["left", "front", "back", "right", "down", "up"], "scan2.ply": ["up", "down", "front", "left", "back", "right"]}
    h = F(SIZE // 2)
    image_lines, point_lines, obs_records = [], [], []
    image_id, point_id = 10, 100
    # an image of another camera first, observing nothing useful
    image_lines.append(("3 0.5 0.5 0.5 0.5 0.25 -1.5 2 2 dslr/DSC_0001.JPG", "12.5 40.25 -1 100.5 7.75 -1"))
    for si, (name, (Rs, ts)) in enumerate(poses.items()):
        xyz, rgb = room_scan(seed + si)
        write_ply_xyz(os.path.join(scans, name), xyz, rgb)
        _, depth, _ = cr.render(xyz, rgb, SIZE)
        if write_depth:
            cr.write_depth_files(os.path.join(images, name), depth, SIZE)
        for face in face_order[name]:
            fi = cr.FACES.index(face)
            Rf = np.array(R_FACE[face], float)
            R_ig = Rf @ Rs.T
            C = ts / k                                           # camera centre in the model
            t_ig = -R_ig @ C
            q = _quat(R_ig)
            head = "%d %s %s 1 %s.%s.png" % (image_id, " ".join("%.17g" % v for v in q), " ".join("%.17g" % v for v in t_ig), name, face)
            obs = []
            ys, xs = np.nonzero(np.isfinite(depth[fi]))
            pick = rng.choice(len(ys), 40, replace=False)
            for j in pick:
                x, y = xs[j] + 0.5, ys[j] + 0.25
                z = float(depth[fi, ys[j], xs[j]]) / k * (1 + rng.uniform(-0.02, 0.02))
                p_img = np.array([(x - float(h)) / float(h) * z, (y - float(h)) / float(h) * z, z])
                X = R_ig.T @ p_img + C
                point_lines.append("%d %.17g %.17g %.17g 200 100 50 0.75 %d %d 3 17" % (point_id, X[0], X[1], X[2], image_id, len(obs)))
                obs.append("%.2f %.2f %d" % (x, y, point_id))
                obs_records.append((name, face, x, y, point_id))
                point_id += 1
            # a point behind the camera, observations without a point, on a pixel without depth, and outside the image
            Xb = R_ig.T @ np.array([0.1, 0.1, -1.0]) + C
            point_lines.append("%d %.17g %.17g %.17g 1 2 3 0.5 %d %d" % (point_id, Xb[0], Xb[1], Xb[2], image_id, len(obs)))
            obs.append("%.2f %.2f %d" % (xs[pick[0]] + 0.5, ys[pick[0]] + 0.5, point_id))
            obs_records.append((name, face, xs[pick[0]] + 0.5, ys[pick[0]] + 0.5, point_id))
            point_id += 1
            obs += ["20.50 20.50 -1", "0.50 0.50 %d" % (point_id - 2), "-5.00 10.00 %d" % (point_id - 2), "%d.00 3.00 %d" % (SIZE + 6, point_id - 2)]
            for x, y in ((0.5, 0.5), (-5.0, 10.0), (SIZE + 6.0, 3.0)):
                obs_records.append((name, face, x, y, point_id - 2))
            image_lines.append((head, " ".join(obs)))
            image_id += 1
    image_lines.append(("4 1 0 0 0 0.5 0.5 0.5 2 dslr/DSC_0002.JPG", "1.5 2.5 %d" % 100))
    with open(os.path.join(model, "images.txt"), "w") as f:
        f.write("# Image list with two lines of data per image:\n#   IMAGE_ID, QW, QX, QY, QZ, TX, TY, TZ, CAMERA_ID, NAME\n")
        for a, b in image_lines:
            f.write(a + "\n" + b + "\n")
    with open(os.path.join(model, "points3D.txt"), "w") as f:
        f.write("# 3D point list with one line of data per point:\n")
        f.write("\n".join(point_lines) + "\n")
    with open(os.path.join(model, "cameras.txt"), "w") as f:
        f.write("# Camera list\n1 PINHOLE %d %d %d %d %d %d\n2 PINHOLE 640 480 500 500 320 240\n" % ((SIZE, SIZE) + (SIZE // 2,) * 4))
    with open(os.path.join(model, "rigs.json"), "w") as f:
        f.write("[]")
    if with_scan3:
        write_ply_xyz(os.path.join(scans, "scan3.ply"), np.zeros((3, 3), F), np.zeros((3, 3), np.uint8))
    open(os.path.join(scans, "scanner_notes.ply"), "w").write("not a scan name\n")
    return dict(tmp=tmp, scans=scans, images=images, model=model, out=os.path.join(tmp, "out"), k=k, poses=poses, face_order=face_order,
                image_lines=image_lines, point_lines=point_lines, obs=obs_records)


def expected_factor(case):
    """float64 evaluation of exp(mean(log(measured / estimated))) over the observations the tool uses, from the files it reads,
    and a bound on |tool - this| / this for the tool's f32 evaluation.

    u = 2^-24.  Per term: the estimated depth is R_2 . X + t_2 in f32 -- the quaternion, X and t rounded on reading (1 rounding
    each), each entry of R from <= 5 roundings of values <= 1 in magnitude, three products and three additions: its absolute error
    is at most 12 u (sum_j |X_j| + |t_2|) (|R_2j| <= 1), i.e. relative e_i = 12 u (sum_j |X_j| + |t_2|) / est_i; the division
    adds u, the C library's logf 2 u |log f_i| (1 ulp).  The sequential f32 sum of n terms is off by at most
    (n - 1) u sum_i |log f_i|; the division by n adds u |mean|; these are absolute errors of the exponent = relative errors of
    the result, and expf adds 2 u.
    """
    u = 2.0 ** -24
    pts = {}
    for ln in case["point_lines"]:
        w = ln.split()
        pts.setdefault(int(w[0]), np.array([float(v) for v in w[1:4]]))
    logs, per_term = [], 0.0
    for head, obs in case["image_lines"]:
        w = head.split()
        if int(w[8]) != 1:
            continue
        q = np.array([float(v) for v in w[1:5]]); t = np.array([float(v) for v in w[5:8]])
        qw, qx, qy, qz = q
        R2 = np.array([2 * (qx * qz - qw * qy), 2 * (qy * qz + qw * qx), 1 - 2 * (qx * qx + qy * qy)])
        name = w[9]
        depth = np.fromfile(os.path.join(case["images"], name[:-3] + "depth"), "<f4").reshape(SIZE, SIZE)
        o = obs.split()
        for j in range(0, len(o), 3):
            x, y, pid = float(o[j]), float(o[j + 1]), int(o[j + 2])
            if pid < 0 or not (-1 < x < SIZE and -1 < y < SIZE):
                continue
            d = float(depth[int(y), int(x)])
            if not np.isfinite(d) or d <= 0:
                continue
            est = float(R2 @ pts[pid] + t[2])
            if est <= 0:
                continue
            lf = np.log(d / est)
            logs.append(lf)
            per_term += 12 * u * (np.abs(pts[pid]).sum() + abs(t[2])) / est + u + 2 * u * abs(lf)
    n = len(logs)
    mean = float(np.sum(logs)) / n
    bound = ((n - 1) * u * float(np.abs(logs).sum()) + per_term) / n + u * abs(mean) + 2 * u
    return float(np.exp(mean)), bound, n


def tool_factor(stdout):
    m = re.search(r"Scaling factor: (\S+) \(from (\d+) observations\)", stdout)
    return float(m.group(1)), int(m.group(2))
