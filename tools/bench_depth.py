"""HIP-event times of the depth-map pyramid and the depth-residual kernels on one MI355X.

    python tools/bench_depth.py [--width 6048] [--height 4032] [--points 4000000] [--reps 7]

Per operation: median (min - max) over --reps calls after two warm-up calls.  "kernels" is the HIP-event time of the operation's
kernel group (e3d_reg_profile), "call" the host clock around the whole call, which ends in a stream synchronisation (for the
pyramid that includes the upload of level 0 from pageable host memory).

  e3d_reg_set_depth_map_level0   one --width x --height map, the level count ImageRegistrator gives that camera, both hole modes,
                                 against its algorithmic bytes: level 0 read and written once, every further level written once and
                                 read once (the last one only written)
  numpy + e3d_reg_set_depth_maps the same pyramid built on the host (f64 box means, as the tests restate cv::resize INTER_AREA) and
                                 uploaded level by level: the only route before e3d_reg_set_depth_map_level0 existed
  depth_accumulate / depth_cost  at the shape of tools/bench_reg.py (--points on a wall, 3840 x 2160, 6 levels)"""
import argparse
import importlib
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
e3d = importlib.import_module("dataset-pipeline_amd")


def timed(P, call, group, reps):
    """-> (kernel ms, call ms), each (median, min, max)."""
    kernel, wall = [], []
    for i in range(reps + 2):
        P.profile(True)
        before = P.kernel_groups.get(group, (0.0, 0, 0.0))[0]
        t = time.perf_counter()
        call()
        dt = (time.perf_counter() - t) * 1e3
        P.profile(True)
        if i >= 2:
            kernel.append(P.kernel_groups[group][0] - before)
            wall.append(dt)
    stat = lambda v: (float(np.median(v)), float(min(v)), float(max(v)))
    return stat(kernel), stat(wall)


def fmt(t):
    return "%9.3f ms (%.3f - %.3f)" % t


def host_pyramid(depth, sizes):
    """The numpy route: sanitise, then f64 2 x 2 box means with edge replication, level by level through f32."""
    with np.errstate(invalid="ignore"):
        levels = [np.where(np.isfinite(depth) & (depth > 0), depth, np.float32(0)).astype(np.float32)]
    for w1, h1 in sizes[1:]:
        p = levels[-1].astype(np.float64)
        h, w = p.shape
        y0 = 2 * np.arange(h1); y1 = np.minimum(y0 + 1, h - 1); x0 = 2 * np.arange(w1); x1 = np.minimum(x0 + 1, w - 1)
        levels.append((0.25 * (((p[np.ix_(y0, x0)] + p[np.ix_(y0, x1)]) + p[np.ix_(y1, x0)]) + p[np.ix_(y1, x1)])).astype(np.float32))
    return levels


def bench_pyramid(a):
    W, H = a.width, a.height
    L = max(2, int(1 + math.ceil(math.log(W * H / 32000.0) / math.log(4))))          # Problem::ComputeImageScaleCount, default area
    P = e3d.RegProblem(e3d.default_reg_params(image_scale_count=L))
    P.set_intrinsics(0, W, H, np.array([0.7 * W, 0.7 * W, W / 2 - 0.5, H / 2 - 0.5], np.float32), 0, L)
    sizes = [P.intrinsics_level(0, l)[:2] for l in range(L)]
    P.set_image(0, 0, [np.zeros((h, w), np.uint8) for w, h in sizes])
    rng = np.random.default_rng(0)
    depth = rng.uniform(0.5, 40.0, (H, W)).astype(np.float32)
    depth[rng.random((H, W)) < 0.05] = np.inf
    px = [w * h for w, h in sizes]
    gb = 4.0 * (2 * px[0] + 2 * sum(px[1:-1]) + (px[-1] if L > 1 else 0)) / 1e9
    print("depth pyramid, %d x %d, %d levels (%s), algorithmic bytes %.4f GB" % (W, H, L, " ".join("%dx%d" % s for s in sizes), gb))
    for name, mode in (("strict", 1), ("average", 0)):
        k, c = timed(P, lambda: P.set_depth_map_level0(0, depth, mode), "depth_pyramid.build", a.reps)
        print("  set_depth_map_level0 %-8s kernels %s -> %6.2f TB/s | call incl. upload %s" % (name, fmt(k), gb / k[0], fmt(c)))
    device = P.get_depth_maps(0)
    build, upload = [], []
    for i in range(max(a.reps // 2, 1) + 1):
        t0 = time.perf_counter()
        levels = host_pyramid(depth, sizes)
        t1 = time.perf_counter()
        P.set_depth_maps(0, levels)
        t2 = time.perf_counter()
        if i >= 1:
            build.append((t1 - t0) * 1e3); upload.append((t2 - t1) * 1e3)
    print("  numpy pyramid on the host %9.1f ms (%.1f - %.1f) + set_depth_maps %9.3f ms (%.3f - %.3f)"
          % (np.median(build), min(build), max(build), np.median(upload), min(upload), max(upload)))
    same = all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(device, P.get_depth_maps(0)))
    print("  average-mode pyramid of the device == host pyramid, bit for bit: %s" % same)
    assert same


def bench_residuals(a):
    from reg_util import look_at_pose, pyramid_u8, quat_from_R, quat_to_R, texture
    W, H, K, L = 3840, 2160, 5, 6
    rng = np.random.RandomState(0)
    side = int(np.sqrt(a.points)); n = side * side
    uu, vv = np.meshgrid(np.linspace(-1.6, 1.6, side), np.linspace(-0.9, 0.9, side), indexing="ij")
    uu = uu + rng.uniform(-0.2, 0.2, uu.shape) * (3.2 / side); vv = vv + rng.uniform(-0.2, 0.2, vv.shape) * (1.8 / side)
    pts = np.stack([uu.ravel(), np.full(n, 3.0), vv.ravel()], 1).astype(np.float32)
    idx = np.arange(n).reshape(side, side)
    sh = lambda dx, dy: np.roll(np.roll(idx, dx, 0), dy, 1).ravel()
    nbr = np.stack([sh(1, 0), sh(-1, 0), sh(0, 1), sh(0, -1), sh(1, 1)], 1).astype(np.uint32)
    tex = texture(pts[:, 0].astype(np.float64), pts[:, 2].astype(np.float64))
    fixed = (tex[nbr] - tex[:, None]).astype(np.float32)
    params = np.array([0.55 * W, 0.55 * W, W / 2 - 0.5, H / 2 - 0.5], np.float32)
    R0, t0 = look_at_pose((0.0, 0.0, 0.0), (0, 3, 0)); q = quat_from_R(R0)
    yy, xx = np.mgrid[0:H, 0:W]
    img = (120 + 60 * np.sin(xx / 11.0) * np.cos(yy / 9.0) + 40 * np.sin((xx + 2 * yy) / 31.0)).clip(0, 250).astype(np.uint8)
    P = e3d.RegProblem(e3d.default_reg_params(image_scale_count=L, point_neighbor_count=K, depth_residuals_weight=1.0))
    P.set_intrinsics(0, W, H, params, 0, L); P.set_image(0, 0, pyramid_u8(img, L)); P.set_image_pose(0, q, t0)
    P.set_point_scale(0, pts, 3.2 / side * 0.7, nbr, fixed); P.set_splat_points(pts)
    # depth of the wall y = 3 along each pixel's ray, a little off so that the residuals are not all zero
    R = quat_to_R(q).astype(np.float64)
    d = np.stack([(xx - params[2]) / params[0], (yy - params[3]) / params[1], np.ones((H, W))], -1) @ R
    o = -R.T @ np.asarray(t0, np.float64)
    P.set_depth_map_level0(0, ((3.0 - o[1]) / d[..., 1] * 1.002).astype(np.float32))
    P.render_depth(0, 0)
    nobs = P.observe(0, 0, 0, 1)
    ka, ca = timed(P, lambda: P.depth_accumulate(0, 0), "depth_residuals.accumulate", a.reps)
    kc, cc = timed(P, lambda: P.depth_cost(0, 0), "depth_residuals.cost", a.reps)
    cnt = P.depth_cost(0, 0)[1]
    print("depth residuals, %d points, image %d x %d, %d levels: %d observations, %d residuals" % (n, W, H, L, nobs, cnt))
    print("  depth_accumulate kernels %s (%.1f M residuals/s) | call %s" % (fmt(ka), cnt / ka[0] / 1e3, fmt(ca)))
    print("  depth_cost       kernels %s (%.1f M residuals/s) | call %s" % (fmt(kc), cnt / kc[0] / 1e3, fmt(cc)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=6048)
    ap.add_argument("--height", type=int, default=4032)
    ap.add_argument("--points", type=int, default=4_000_000)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if e3d.lib().e3d_init(0) < 1:
        raise SystemExit("bench_depth.py: no HIP device")
    bench_pyramid(a)
    bench_residuals(a)


if __name__ == "__main__":
    main()
