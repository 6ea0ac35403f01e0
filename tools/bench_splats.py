"""SplatCreator measurement: one synthetic room scan (synth.make_scan) with normals from the GPU estimator, against a grid mesh
of the room's floor and walls (no cylinders, a hole in one wall), e3d_create_splats end to end.  Reports the index build and
the splat pass (HIP events inside the call, both ending in a stream synchronise), the whole call's wall time, points/s and the
upper bound of point-to-mesh queries/s (5 per point), and the CPU restatement (tests/splat_ref.py, numpy, one core) on a
subsample against the triangles near it.

    python tools/bench_splats.py [--points 20000000] [--res 0.006] [--cpu-points 2000]
Prints one JSON line.  Not a bench.py line; numbers go to DESIGN.md section 14."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

F = np.float32


def room_mesh(res):
    """floor and walls of the 10 x 10 x 3 m room in the frame of a scan taken at (5, 5, 1.5) with yaw 0; a 2 x 1 m hole in y = +5"""
    parts, base = [], 0
    n10, n3 = int(round(10 / res)) + 1, int(round(3 / res)) + 1
    for axes, w, (u0, u1, v0, v1, nu, nv) in [((0, 1, 2), -1.5, (-5, 5, -5, 5, n10, n10)), ((1, 2, 0), -5, (-5, 5, -1.5, 1.5, n10, n3)),
                                              ((1, 2, 0), 5, (-5, 5, -1.5, 1.5, n10, n3)), ((0, 2, 1), -5, (-5, 5, -1.5, 1.5, n10, n3)),
                                              ((0, 2, 1), 5, (-5, 5, -1.5, 1.5, n10, n3))]:
        us = np.linspace(u0, u1, nu, dtype=F); vs = np.linspace(v0, v1, nv, dtype=F)
        V = np.empty((nv, nu, 3), F)
        V[..., axes[0]] = us[None, :]; V[..., axes[1]] = vs[:, None]; V[..., axes[2]] = F(w)
        idx = np.arange(nv - 1)[:, None] * nu + np.arange(nu - 1)[None, :] + base
        T = np.stack([np.stack([idx, idx + 1, idx + nu], -1), np.stack([idx + 1, idx + nu + 1, idx + nu], -1)], 2).reshape(-1, 3)
        V = V.reshape(-1, 3)
        if axes == (0, 2, 1) and w == 5:
            cen = V[T - base].mean(1)
            T = T[~((np.abs(cen[:, 0]) < 1.0) & (np.abs(cen[:, 2]) < 0.5))]
        parts.append((V, T))
        base += V.shape[0]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]).astype(np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=20_000_000)
    ap.add_argument("--res", type=float, default=0.006, help="grid step of the mesh (0.006: 12.1 M triangles)")
    ap.add_argument("--threshold", type=float, default=0.02)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--cpu-points", type=int, default=2000)
    a = ap.parse_args()
    e3d = importlib.import_module("dataset-pipeline_amd")
    synth = importlib.import_module("dataset-pipeline_amd.synth")
    dev = torch.device("cuda:0")
    xyz, _, _ = synth.make_scan(a.points, (5.0, 5.0, 1.5), 0.0, 5, device=dev)
    nrm, _ = e3d.normals_knn(xyz, 8)
    xyz_h = xyz.cpu().numpy()
    V, T = room_mesh(a.res)
    runs = []
    for _ in range(a.repeat):
        tm = {}
        t0 = time.perf_counter()
        _, _, add, rad = e3d.create_splats(xyz_h, nrm, V, T, a.threshold, float("inf"), timings=tm)
        runs.append((time.perf_counter() - t0, tm["index_ms"], tm["splat_ms"], int(add.sum())))
    best = min(runs, key=lambda r: r[2])
    n = a.points
    out = {"points": n, "triangles": int(T.shape[0]), "splats": best[3], "index_build_ms": round(best[1], 3), "splat_pass_ms": round(best[2], 3),
           "call_wall_s": round(min(r[0] for r in runs), 3), "points_per_s": round(n / (best[2] * 1e-3), 1),
           "queries_per_s_upper": round(5 * n / (best[2] * 1e-3), 1), "runs_ms": [[round(r[1], 3), round(r[2], 3)] for r in runs]}
    # CPU restatement on a subsample: the points' five queries, each against the triangles whose centroid cell is near it
    # (numpy, one core; the time includes the restatement's cell sort of the mesh, once per query set).  The splat radii are
    # the GPU's (the kNN is not what is compared here).
    if a.cpu_points > 0:
        import splat_ref as sr
        rng = np.random.default_rng(1)
        sub = np.sort(rng.choice(n, a.cpu_points, replace=False))
        sub = sub[~np.isnan(nrm[sub]).any(1)]
        q = xyz_h[sub]
        s = rad[sub]
        t0 = time.perf_counter()
        C = sr.corners(q, nrm[sub], s)
        thr2 = F(a.threshold) * F(a.threshold)
        far = np.zeros(len(sub), bool)
        for qq in [q] + [C[:, k] for k in range(4)]:
            d, _ = sr.culled_min_sq(qq, V, T, thr2)
            far |= ~(d <= thr2)
        dt = time.perf_counter() - t0
        out.update({"cpu_points": int(len(sub)), "cpu_s": round(dt, 3),
                    "cpu_points_per_s_1core": round(len(sub) / dt, 1), "cpu_flags_match": bool(np.array_equal(far, add[sub]))})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
