"""HIP-event time of ImageUndistorter's resampling kernel (e3d_reg_undistort) on one MI355X.

    python tools/bench_undistort.py [--width 6048] [--height 4032] [--reps 9]

One --width x --height image per call.  THIN_PRISM_FISHEYE with the DSLR-like parameters of tests/test_oracle_camera.py scaled to that
size, at blank_pixels 0 and 1, and PINHOLE (no camera arithmetic beyond one multiply-add per axis: the memory side alone); the u8 x 3
bilinear kind that the images take, and the other three kinds once each.  Per case: median (min - max) of the kernel's HIP-event time
(e3d_reg_undistort_kernel_ms) over --reps calls after two warm-up calls, the host clock around the whole call (upload from and
download to pageable memory included), and the algorithmic bytes -- source read once, destination (and nothing else) written once --
over the kernel time as a share of the 8 TB/s HBM peak and of the 6.3 TB/s a streaming kernel reaches on this part."""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
e3d = importlib.import_module("dataset-pipeline_amd")

HBM_PEAK, HBM_STREAM = 8.0e12, 6.3e12
PIXEL = {0: (np.uint8, (), 1), 1: (np.uint8, (3,), 3), 2: (np.uint8, (), 1), 3: (np.float32, (), 4)}
KIND_NAME = {0: "u8 bilinear", 1: "u8 x 3 bilinear", 2: "u8 mask", 3: "f32 nearest"}


def stat(v):
    return float(np.median(v)), float(min(v)), float(max(v))


def run(P, plan, kind, src, reps):
    kernel, wall = [], []
    for i in range(reps + 2):
        t = time.perf_counter()
        out = P.undistort(0, plan, kind, src)
        dt = (time.perf_counter() - t) * 1e3
        if i >= 2:
            kernel.append(P.undistort_kernel_ms()); wall.append(dt)
    return stat(kernel), stat(wall), out


def main():
    import undistort_ref as ur
    from test_oracle_camera import CAMERAS
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=6048)
    ap.add_argument("--height", type=int, default=4032)
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    if e3d.lib().e3d_init(0) < 1:
        raise SystemExit("bench_undistort: no HIP device")
    W, H = a.width, a.height
    rng = np.random.default_rng(0)
    src = {0: rng.integers(0, 256, (H, W), dtype=np.uint8), 1: rng.integers(0, 256, (H, W, 3), dtype=np.uint8),
           2: (rng.random((H, W)) < 0.1).astype(np.uint8), 3: rng.uniform(0.5, 40.0, (H, W)).astype(np.float32)}
    print("undistortion of one %d x %d image; kernel = HIP events around the one launch, call = host clock incl. both copies" % (W, H))
    for name, blanks, kinds in (("THIN_PRISM_FISHEYE", (0.0, 1.0), (1, 0, 2, 3)), ("PINHOLE", (0.0,), (1, 3))):
        t, p = CAMERAS[name]
        P = e3d.RegProblem(e3d.default_reg_params(image_scale_count=1))
        P.set_intrinsics(0, W, H, ur.scaled_params(p, t, W, H), 0, 1, camera_type=t)
        for b in blanks:
            t0 = time.perf_counter()
            plan = P.undistort_plan(0, b)
            plan_ms = (time.perf_counter() - t0) * 1e3
            print("%s blank_pixels %g -> PINHOLE %d x %d f %.6g %.6g c %g %g (plan %.2f ms)" % ((name, b) + plan.astuple() + (plan_ms,)))
            for kind in (kinds if b == blanks[0] else kinds[:1]):
                k, c, out = run(P, plan, kind, src[kind], a.reps)
                bytes_ = PIXEL[kind][2] * (W * H + plan.width * plan.height)
                print("  %-16s kernel %8.4f ms (%.4f - %.4f) | %7.2f MB -> %5.2f TB/s = %4.1f %% of peak, %4.1f %% of streaming | call %7.2f ms (%.2f - %.2f)"
                      % (KIND_NAME[kind], k[0], k[1], k[2], bytes_ / 1e6, bytes_ / (k[0] * 1e-3) / 1e12, 100 * bytes_ / (k[0] * 1e-3) / HBM_PEAK,
                         100 * bytes_ / (k[0] * 1e-3) / HBM_STREAM, c[0], c[1], c[2]))


if __name__ == "__main__":
    main()
