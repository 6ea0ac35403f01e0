"""HIP-event time of StereoPairCreator's resampling kernel (e3d_reg_stereo_rectify) against the undistorter's, and the
time of e3d_reg_stereo_ground_truth against the four calls that did its work before, on one MI355X.

    python tools/bench_stereo.py [--width 6048] [--height 4032] [--reps 9] [--scan_points 10000000] [--gt_reps 5]

One --width x --height image per call, PINHOLE and THIN_PRISM_FISHEYE with the parameters of tests/test_oracle_camera.py scaled to that
size, the u8 x 3 bilinear and the f32 nearest kind.  The target is the camera's own undistortion plan at blank_pixels 0; k_rectify runs
with a rotation of 1 degree (about the axis (1, 1, 1)), k_undistort on the same target without one.  The two are called alternately in
one session; per kernel the median (min - max) of its HIP-event time over --reps calls after two warm-up calls of each, and the ratio
of the medians.
Ground truth: --scan_points points (a wall, an occluder, clutter) seen by a rectified PINHOLE pair of the same size, the occlusion
geometry 200 000 of them as splats.  e3d_reg_stereo_ground_truth against count_scan_observations for both images + ground_truth_depth
of the left image with min_count 1 and 2 (the same visibility work; four occlusion renderings instead of two, no disparity map),
alternating, host clock around the calls (the copies of masks and maps included), median (min - max) of --gt_reps after one warm-up."""
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

KIND_NAME = {1: "u8 x 3 bilinear", 3: "f32 nearest"}


def stat(v):
    return float(np.median(v)), float(min(v)), float(max(v))


def rotation(degrees):
    """Rodrigues about (1, 1, 1) / sqrt(3), row-major f32."""
    a = math.radians(degrees)
    k = np.ones(3) / math.sqrt(3.0)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return (np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * (K @ K)).astype(np.float32).ravel()


def bench_kernels(a):
    import undistort_ref as ur
    from test_oracle_camera import CAMERAS
    W, H = a.width, a.height
    rng = np.random.default_rng(0)
    src = {1: rng.integers(0, 256, (H, W, 3), dtype=np.uint8), 3: rng.uniform(0.5, 40.0, (H, W)).astype(np.float32)}
    S = rotation(1.0)
    print("one %d x %d image onto its own undistortion plan (blank_pixels 0); k_rectify with a rotation of 1 degree, k_undistort without;" % (W, H))
    print("alternating calls, kernel = HIP events around the one launch, median (min - max) of %d after 2 warm-ups" % a.reps)
    for name in ("PINHOLE", "THIN_PRISM_FISHEYE"):
        t, p = CAMERAS[name]
        P = e3d.RegProblem(e3d.default_reg_params(image_scale_count=1))
        P.set_intrinsics(0, W, H, ur.scaled_params(p, t, W, H), 0, 1, camera_type=t)
        plan = P.undistort_plan(0, 0.0)
        print("%s -> PINHOLE %d x %d f %.6g %.6g c %g %g" % ((name,) + plan.astuple()))
        for kind in (1, 3):
            rect, und = [], []
            valid = None
            for i in range(a.reps + 2):
                out, valid = P.stereo_rectify(0, plan, S, kind, src[kind], return_valid=True)
                r = P.stereo_kernel_ms()
                P.undistort(0, plan, kind, src[kind])
                u = P.undistort_kernel_ms()
                if i >= 2:
                    rect.append(r); und.append(u)
            r, u = stat(rect), stat(und)
            print("  %-16s k_rectify %8.4f ms (%.4f - %.4f) | k_undistort %8.4f ms (%.4f - %.4f) | ratio %.3f | %.1f %% of the rectified pixels valid"
                  % (KIND_NAME[kind], r[0], r[1], r[2], u[0], u[1], u[2], r[0] / u[0], 100.0 * float(valid.mean())))


def bench_ground_truth(a):
    W, H = a.width, a.height
    n = a.scan_points
    rng = np.random.default_rng(1)
    f = 0.56 * W
    n_wall = int(n * 0.9)
    depth = 3.0
    half_x, half_y = 0.55 * W / f * depth, 0.55 * H / f * depth
    wall = np.stack([rng.uniform(-half_x, half_x + 0.3, n_wall), rng.uniform(-half_y, half_y, n_wall), rng.uniform(depth - 0.01, depth + 0.01, n_wall)], 1)
    n_block = int(n * 0.05)
    block = np.stack([rng.uniform(-0.2, 0.4, n_block), rng.uniform(-0.3, 0.3, n_block), np.full(n_block, 1.5)], 1)
    clutter = rng.uniform(-4, 4, (n - n_wall - n_block, 3))
    scan = np.concatenate([wall, block, clutter]).astype(np.float32)
    rng.shuffle(scan)
    P = e3d.RegProblem(e3d.default_reg_params(image_scale_count=1))
    P.set_intrinsics(0, W, H, np.array([f, f, (W - 1) // 2, (H - 1) // 2], np.float32), 0, 1, camera_type=0)
    q = np.array([1, 0, 0, 0], np.float32)
    for i, t in enumerate(([0, 0, 0], [-0.3, 0, 0])):
        P.set_image(i, 0, None)
        P.set_image_pose(i, q, np.array(t, np.float32))
    P.set_splat_points(scan[:200000])
    P.set_scan_points(scan)
    excluded = [np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)]
    excluded[0][H // 3:H // 2, W // 4:W // 3] = 1; excluded[1][H // 2:2 * H // 3, W // 2:2 * W // 3] = 1
    zeros = np.zeros(len(scan), np.int32)
    new, old = [], []
    for i in range(a.gt_reps + 1):
        t0 = time.perf_counter()
        disparity, mask, depth1 = P.stereo_ground_truth(0, 1, excluded[0], excluded[1], return_depth=True)
        t_new = (time.perf_counter() - t0) * 1e3
        P.set_scan_observation_counts(zeros)
        t0 = time.perf_counter()
        P.count_scan_observations(0, excluded[0], excluded_flag=1)
        P.count_scan_observations(1, excluded[1], excluded_flag=1)
        d1, _ = P.ground_truth_depth(0, W, H, mask=excluded[0], excluded_flag=1, min_count=1)
        d2, _ = P.ground_truth_depth(0, W, H, mask=excluded[0], excluded_flag=1, min_count=2)
        t_old = (time.perf_counter() - t0) * 1e3
        if i >= 1:
            new.append(t_new); old.append(t_old)
    same = np.array_equal(d1.view(np.uint32), depth1.view(np.uint32)) and np.array_equal(mask == 255, np.isfinite(d1) & (d1.view(np.uint32) == d2.view(np.uint32)))
    s_new, s_old = stat(new), stat(old)
    print("ground truth of a %d x %d pair, %d scan points, 200000 splats; host clock, median (min - max) of %d after 1 warm-up" % (W, H, len(scan), a.gt_reps))
    print("  e3d_reg_stereo_ground_truth %9.2f ms (%.2f - %.2f) | 2 x count + 2 x ground_truth_depth %9.2f ms (%.2f - %.2f) | ratio %.3f"
          % (s_new[0], s_new[1], s_new[2], s_old[0], s_old[1], s_old[2], s_new[0] / s_old[0]))
    print("  pixels: %d seen by both, %d half-occluded, %d unknown; the two ways agree: %s"
          % (int((mask == 255).sum()), int((mask == 128).sum()), int((mask == 0).sum()), same))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=6048)
    ap.add_argument("--height", type=int, default=4032)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--scan_points", type=int, default=10_000_000)
    ap.add_argument("--gt_reps", type=int, default=5)
    a = ap.parse_args()
    if e3d.lib().e3d_init(0) < 1:
        raise SystemExit("bench_stereo: no HIP device")
    bench_kernels(a)
    bench_ground_truth(a)


if __name__ == "__main__":
    main()
