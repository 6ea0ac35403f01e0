"""SurfaceReconstructor measurement: one synthetic room scan (synth.make_scan) with normals from the GPU estimator,
e3d_surface_reconstruct end to end.  Reports, per kernel group (HIP events inside the call) and for the whole call (wall time,
host copies of the cloud and of the result included), the median (min - max) over --reps calls after two warm-up calls, with the
point, corner, vertex and triangle counts beside them.

    python tools/bench_surface.py [--points 20000000] [--voxel_size 0.02] [--support_radius 0.04] [--reps 7] [--solids 0]
                                  [--fill_holes 0] [--holes 0]
--solids N > 0 adds N boxes of 0.5 - 2 m per side inside the room (seeded; three of four united, every fourth subtracted, random
rotations) through e3d_surface_reconstruct_csg and reports the sixth kernel group, solids, as well; 0 is the plain call.
--holes K punches K square holes of 0.3 m into the cloud (seeded: every point within 0.15 m of one of K of its points along all
three axes is dropped); --fill_holes N > 0 runs N iterations of hole filling (e3d_surface_reconstruct_filled) and reports the group
fill, the number of filled corners and vertices, and a device-to-device copy rate measured in the same session.
Prints one JSON line.  Not a bench.py line; numbers go to DESIGN.md section 19."""
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

GROUPS = ("grid", "candidates", "field", "corners", "extract")


def summary(values):
    return {"median": round(float(np.median(values)), 3), "min": round(float(np.min(values)), 3), "max": round(float(np.max(values)), 3)}


def room_boxes(count, seed=19):
    """count boxes of 0.5 - 2 m per side with their centres inside the 10 x 10 x 3 m room of synth.make_scan."""
    rng = np.random.default_rng(seed)
    solids = []
    for i in range(count):
        q = rng.normal(size=4)
        w, x, y, z = q / np.linalg.norm(q)
        rotation = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                             [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                             [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        centre = rng.uniform([-4.0, -4.0, -1.0], [4.0, 4.0, 1.0])        # the scan is in the scanner's frame: the room is +-5, +-5, +-1.5
        solids.append(("subtract" if i % 4 == 3 else "union", centre, rotation, 0.5 * rng.uniform(0.5, 2.0, 3)))
    return solids


def punch_holes(xyz, nrm, count, half=0.15, seed=23):
    """The cloud without the points within `half` (Chebyshev) of `count` seeded points of it."""
    rng = np.random.default_rng(seed)
    keep = np.ones(len(xyz), bool)
    for c in xyz[rng.choice(len(xyz), count, replace=False)]:
        keep &= np.abs(xyz - c).max(1) >= half
    return np.ascontiguousarray(xyz[keep]), np.ascontiguousarray(nrm[keep])


def copy_rate_gbs(dev, nbytes=1 << 30, reps=5):
    """Device-to-device copy rate in GB/s (bytes read + bytes written), the best of `reps`."""
    a = torch.empty(nbytes, dtype=torch.uint8, device=dev); b = torch.empty_like(a)
    best = None
    for _ in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); b.copy_(a); e1.record(); torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        best = ms if best is None else min(best, ms)
    return 2 * nbytes / (best * 1e-3) / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=20_000_000)
    ap.add_argument("--voxel_size", type=float, default=0.02)
    ap.add_argument("--support_radius", type=float, default=None, help="default: 2 x voxel_size")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--solids", type=int, default=0, help="number of boxes united with / subtracted from the field (0: the plain call)")
    ap.add_argument("--fill_holes", type=int, default=0, help="iterations of hole filling (0: none)")
    ap.add_argument("--holes", type=int, default=0, help="number of 0.3 m square holes punched into the cloud")
    a = ap.parse_args()
    e3d = importlib.import_module("dataset-pipeline_amd")
    synth = importlib.import_module("dataset-pipeline_amd.synth")
    dev = torch.device("cuda:0")
    xyz, _, _ = synth.make_scan(a.points, (5.0, 5.0, 1.5), 0.0, 5, device=dev)
    nrm, _ = e3d.normals_knn(xyz, 8)
    xyz_h = xyz.cpu().numpy()
    del xyz
    if torch.is_tensor(nrm):
        nrm = nrm.cpu().numpy()
    if a.holes > 0:
        xyz_h, nrm = punch_holes(xyz_h, np.asarray(nrm), a.holes)
    torch.cuda.empty_cache()
    runs = []
    counts = None
    solids = room_boxes(a.solids) if a.solids > 0 else None
    groups = GROUPS + (("solids",) if solids else ()) + (("fill",) if a.fill_holes > 0 else ())
    for rep in range(2 + a.reps):
        tm = {}
        t0 = time.perf_counter()
        v, t, c = e3d.reconstruct_surface(xyz_h, nrm, a.voxel_size, a.support_radius, return_corners=True, timings=tm, solids=solids, fill_iterations=a.fill_holes)
        wall = (time.perf_counter() - t0) * 1e3
        if rep >= 2:
            runs.append([tm[g + "_ms"] for g in groups] + [wall])
        counts = (len(c["ijk"]), len(v), len(t), int(c["count"].max(initial=0)), float(c["count"].mean()) if len(c["count"]) else 0.0)
    runs = np.array(runs)
    out = {"points": len(xyz_h), "contributing_points": int((~np.isnan(nrm).any(1)).sum()), "voxel_size": a.voxel_size,
           "support_radius": a.support_radius if a.support_radius is not None else 2 * a.voxel_size,
           "corners": counts[0], "vertices": counts[1], "triangles": counts[2], "max_contributors": counts[3],
           "mean_contributors": round(counts[4], 1), "reps": a.reps}
    if solids:
        out["solids"] = a.solids
        out["corners_of_solids_alone"] = int((c["count"] == 0).sum())
    if a.holes > 0:
        out["holes"] = a.holes
    if a.fill_holes > 0:
        out["fill_holes"] = a.fill_holes
        out["filled_corners"] = int(c["corner_filled"].sum())
        out["filled_vertices"] = int(c["vertex_filled"].sum())
        out["device_copy_GBps"] = round(copy_rate_gbs(dev), 1)
    for i, g in enumerate(groups):
        out[g + "_ms"] = summary(runs[:, i])
    out["kernels_ms"] = summary(runs[:, :len(groups)].sum(1))
    out["call_wall_ms"] = summary(runs[:, -1])
    evals = counts[0] * counts[4]
    out["counting_point_evaluations_per_s"] = round(evals / (out["field_ms"]["median"] * 1e-3), 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
