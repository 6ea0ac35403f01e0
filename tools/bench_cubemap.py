"""CubeMapRenderer measurement: a closed box room seen through a blind cone below the scanner (the cloud of the at-size test),
e3d_render_cube_map at --size 2048 with the points already on the device.  Reports the point pass, the resolve, fill-in pass 1
and the dilation (HIP events inside the call), the sweeps and batches, against the floors of DESIGN.md section 15; optionally the
numpy restatement's wall time on this host.

    python tools/bench_cubemap.py [--points 20000000] [--size 2048] [--repeat 5] [--cpu]
The sweeps per look at the flag words come from E3D_CUBEMAP_BATCH (default 32; 1 = one synchronisation per sweep), read when the
library is loaded: run the tool once per setting.  Prints one JSON line.  Not a bench.py line."""
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


def cloud(n, cone_deg, seed=21):
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((int(n / (1 - (1 - np.cos(np.deg2rad(cone_deg))) / 2)) + 1000, 3), dtype=F)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = d[d[:, 1] < np.cos(np.deg2rad(cone_deg))][:n]
    lo, hi = np.array([-4.0, -1.2, -3.0], F), np.array([2.5, 1.6, 5.0], F)
    with np.errstate(divide="ignore"):
        t = np.where(d > 0, hi / d, np.where(d < 0, lo / d, np.inf)).min(1)
    xyz = np.ascontiguousarray((d * t[:, None]).astype(F))
    rgb = np.stack([(xyz[:, 0] * 61) % 256, (xyz[:, 1] * 97 + 50) % 256, (xyz[:, 2] * 43 + 120) % 256], 1).astype(np.uint8)
    return xyz, rgb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=20_000_000)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--cone", type=float, default=25.0)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu", action="store_true", help="also time the numpy restatement (minutes)")
    a = ap.parse_args()
    e3d = importlib.import_module("dataset-pipeline_amd")
    xyz, rgb = cloud(a.points, a.cone)
    dev = torch.device("cuda:0")
    dx, dc = torch.from_numpy(xyz).to(dev), torch.from_numpy(rgb).to(dev)
    runs = []
    for i in range(a.warmup + a.repeat):
        tm = {}
        t0 = time.perf_counter()
        _, depth, sweeps = e3d.render_cube_map(dx, dc, a.size, True, timings=tm)
        tm["call_wall_s"] = time.perf_counter() - t0
        if i >= a.warmup:
            runs.append(tm)
    med = {k: float(np.median([r[k] for r in runs])) for k in runs[0]}
    n, px = len(xyz), 6 * a.size * a.size
    pairs = int(np.isfinite(e3d.render_cube_map(dx, dc, a.size, False)[1]).sum())      # occupied pixels (a lower bound of the accepted pairs)
    n_sweeps = int(sweeps.max())
    out = {"points": n, "size": a.size, "batch": int(os.environ.get("E3D_CUBEMAP_BATCH", "32")), "sweeps": [int(s) for s in sweeps],
           "batches": int(med["batches"]), "sweeps_launched": int(med["sweeps_launched"]),
           "points_ms": round(med["points_ms"], 3), "resolve_ms": round(med["resolve_ms"], 3), "fill_ms": round(med["fill_ms"], 3),
           "dilation_ms": round(med["dilation_ms"], 3), "call_wall_s": round(med["call_wall_s"], 3),
           "points_ms_runs": [round(r["points_ms"], 3) for r in runs], "dilation_ms_runs": [round(r["dilation_ms"], 3) for r in runs],
           "occupied_pixels": pairs,
           "point_read_GBps": round(15 * n / (med["points_ms"] * 1e-3) / 1e9, 1),
           "point_atomics_per_s_lower": round(pairs / (med["points_ms"] * 1e-3), 1),
           "dilation_model_bytes": n_sweeps * 2 * px * 4,
           "dilation_model_GBps": round(n_sweeps * 2 * px * 4 / (med["dilation_ms"] * 1e-3) / 1e9, 1) if med["dilation_ms"] > 0 else None}
    if a.cpu:
        import cubemap_ref as cr
        t0 = time.perf_counter()
        want = cr.render(xyz, rgb, a.size)
        out["numpy_restatement_s"] = round(time.perf_counter() - t0, 1)
        got = e3d.render_cube_map(dx, dc, a.size, True)
        out["equal"] = bool(np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)) and
                            np.array_equal(got[2], want[2]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
