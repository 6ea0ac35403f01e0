"""ReconstructionEvaluator measurement: two synthetic room scans (synth.make_scan) and, as the reconstruction, points sampled from
them with 5 mm noise, e3d_evaluate_reconstruction end to end.  Reports, per kernel group (HIP events inside the call) and for the
whole call (wall time, host copies of the clouds and of the result included), the median (min - max) over --reps calls after two
warm-up calls, with the share of the queries that close at each search level beside them.

    python tools/bench_evaluate.py [--scan_points 10000000] [--scans 2] [--rec_points 20000000] [--noise 0.005] [--reps 7]
Prints one JSON line.  Not a bench.py line; numbers go to DESIGN.md section 20."""
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

GROUPS = ("grid", "search", "range", "voxels")
ORIGINS = ((3.0, 4.0, 1.2), (7.0, 3.0, 1.5), (5.0, 6.5, 1.0), (2.0, 2.0, 1.4))


def summary(values):
    return {"median": round(float(np.median(values)), 3), "min": round(float(np.min(values)), 3), "max": round(float(np.max(values)), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scan_points", type=int, default=10_000_000, help="per scan")
    ap.add_argument("--scans", type=int, default=2)
    ap.add_argument("--rec_points", type=int, default=20_000_000)
    ap.add_argument("--noise", type=float, default=0.005)
    ap.add_argument("--voxel_size", type=float, default=0.01)
    ap.add_argument("--cube_map_size", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    e3d = importlib.import_module("dataset-pipeline_amd")
    synth = importlib.import_module("dataset-pipeline_amd.synth")
    dev = torch.device("cuda:0")
    scans, origins = [], []
    for s in range(a.scans):
        xyz, _, T = synth.make_scan(a.scan_points, ORIGINS[s % len(ORIGINS)], 0.3 * s, 11 + s, device=dev)
        Tt = torch.from_numpy(T).to(dev)
        scans.append((xyz @ Tt[:3, :3].T + Tt[:3, 3]).contiguous())
        origins.append(T[:3, 3])
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    pool = torch.cat(scans)
    pick = torch.randint(0, len(pool), (a.rec_points,), generator=g, device=dev)
    rec = (pool[pick] + a.noise * torch.randn(a.rec_points, 3, generator=g, device=dev)).cpu().numpy()
    scans = [s.cpu().numpy() for s in scans]
    del pool, pick
    torch.cuda.empty_cache()
    runs = []
    res = None
    for rep in range(2 + a.reps):
        tm = {}
        t0 = time.perf_counter()
        res = e3d.evaluate_reconstruction(rec, scans, origins, voxel_size=a.voxel_size, cube_map_size=a.cube_map_size, return_classes=True, timings=tm)
        wall = (time.perf_counter() - t0) * 1e3
        if rep >= 2:
            runs.append([tm[k + "_ms"] for k in GROUPS] + [wall])
    runs = np.array(runs)
    T = len(res["tolerances"])
    out = {"scans": a.scans, "scan_points": a.scan_points, "rec_points": a.rec_points, "noise": a.noise, "voxel_size": a.voxel_size,
           "cube_map_size": a.cube_map_size, "tolerances": [round(float(t), 6) for t in res["tolerances"]], "reps": a.reps,
           "scan_voxels": res["n_scan_voxels"], "rec_voxels": res["n_rec_voxels"], "evaluated_voxels": res["evaluated_voxels"].tolist(),
           "completeness": [round(float(v), 6) for v in res["completeness"]], "accuracy": [round(float(v), 6) for v in res["accuracy"]],
           # share of the queries that close at level i; the last entry: open to the end
           "rec_queries_closing": [round(float(v), 6) for v in np.bincount(res["near_rec"], minlength=T + 1)[:T + 1] / max(1, a.rec_points)],
           "scan_queries_closing": [round(float(v), 6) for v in np.bincount(res["near_scan"], minlength=T + 1)[:T + 1] / max(1, len(res["near_scan"]))],
           "free_classes": [round(float(v), 6) for v in np.bincount(res["free"], minlength=T + 1)[:T + 1] / max(1, a.rec_points)]}
    for i, k in enumerate(GROUPS):
        out[k + "_ms"] = summary(runs[:, i])
    out["kernels_ms"] = summary(runs[:, :len(GROUPS)].sum(1))
    out["call_wall_ms"] = summary(runs[:, -1])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
