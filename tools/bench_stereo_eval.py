"""StereoEvaluator measurement: one 6048 x 4032 pair, synthetic estimates made of the ground truth, Gaussian noise, 2 % gross errors and
5 % invalid pixels, n_est = 1 and 4, inputs resident on the GPU.  Per kernel group (HIP events inside the call,
e3d_disp_eval_kernel_ms) and for the whole call (host clock; device inputs, and host inputs with their upload) the median (min - max)
of --reps calls after two warm-ups.  Beside them, in the same session:
  * the rate of a plain streaming kernel (torch's device-to-device copy of 1 GiB, read + written bytes over HIP-event time) and the
    time the algorithmic bytes of the three passes (gt 4 + mask 1 + estimate 4 bytes per pixel, estimate and pass) take at that rate;
  * the same metrics computed with torch on the same GPU (torch.sort for the quantiles): what a user does without this feature.
--all_equal adds a run whose errors are all 1.5 (every pixel in one histogram bin: the worst case of same-address LDS atomics).

    python tools/bench_stereo_eval.py [--width 6048] [--height 4032] [--reps 9] [--all_equal]
Prints one JSON line.  Not a bench.py line; numbers go to DESIGN.md section 23."""
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

GROUPS = ("classify", "select", "sums")
THRESHOLDS = (0.5, 1.0, 2.0, 4.0)
PERCENTILES = (50, 90, 95, 99)
BYTES_PER_PIXEL = 9                                  # gt f32 + mask u8 + estimate f32, per estimate and pass
PASSES = 3                                           # classify and two refinement passes


def summary(values):
    return {"median": round(float(np.median(values)), 4), "min": round(float(np.min(values)), 4), "max": round(float(np.max(values)), 4)}


def event_ms(fn, reps, warm=2):
    out = []
    for rep in range(warm + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if rep >= warm:
            out.append(a.elapsed_time(b))
    return out


def make_inputs(width, height, n_est, dev, all_equal=False):
    g = torch.Generator(device=dev)
    g.manual_seed(17)
    shape = (height, width)
    gt = torch.rand(shape, generator=g, device=dev) * 200 + 1
    gt[torch.rand(shape, generator=g, device=dev) < 0.25] = float("inf")
    u = torch.rand(shape, generator=g, device=dev)
    mask = torch.where(u < 0.1, 0, torch.where(u < 0.3, 128, 255)).to(torch.uint8)
    est = []
    for _ in range(n_est):
        base = torch.where(torch.isfinite(gt), gt, torch.full_like(gt, 50.0))
        if all_equal:
            e = torch.floor(base) + 1.5                  # against floor(gt): see below
        else:
            e = base + 0.7 * torch.randn(shape, generator=g, device=dev)
            u = torch.rand(shape, generator=g, device=dev)
            e = torch.where(u < 0.02, torch.rand(shape, generator=g, device=dev) * 256, e)
            e[(u > 0.02) & (u < 0.07)] = float("inf")
        est.append(e)
    if all_equal:
        gt = torch.where(torch.isfinite(gt), torch.floor(gt), gt)   # integers below 256: (floor + 1.5) - floor is 1.5 exactly
    return gt.contiguous(), mask.contiguous(), torch.stack(est).contiguous()


def torch_metrics(gt, mask, est):
    """The rules with torch operations; returns a few of the numbers so that the two ways can be compared."""
    known = torch.isfinite(gt)
    regions = (known & (mask != 0), known & (mask == 255))
    thr = torch.tensor(THRESHOLDS, device=gt.device)
    out = []
    for e in est:
        valid = torch.isfinite(e)
        err = (e - gt).abs()
        for reg in regions:
            v = err[reg & valid]
            n = v.numel()
            bad = (v[:, None] > thr[None, :]).sum(0)
            d = v.double()
            s = torch.sort(v).values
            k = torch.tensor([(p * n + 99) // 100 - 1 for p in PERCENTILES], device=gt.device).clamp(min=0)
            out.append((int(reg.sum()), n, bad, d.sum(), (d * d).sum(), s[k] if n else None))
    return out


def run(e3d, width, height, n_est, reps, dev, all_equal, stream_gbs):
    gt, mask, est = make_inputs(width, height, n_est, dev, all_equal)
    host = (gt.cpu().numpy(), mask.cpu().numpy(), est.cpu().numpy())
    runs, host_wall = [], []
    res = None
    for rep in range(2 + reps):
        tm = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = e3d.evaluate_disparity(gt, mask, est, THRESHOLDS, PERCENTILES, timings=tm)
        wall = (time.perf_counter() - t0) * 1e3
        if rep >= 2:
            runs.append([tm[k + "_ms"] for k in GROUPS] + [wall])
    for rep in range(1 + 3):
        t0 = time.perf_counter()
        again = e3d.evaluate_disparity(*host, THRESHOLDS, PERCENTILES)
        if rep >= 1:
            host_wall.append((time.perf_counter() - t0) * 1e3)
    assert again["counts"].tobytes() == res["counts"].tobytes() and again["quantiles"].tobytes() == res["quantiles"].tobytes()
    runs = np.array(runs)
    ref = torch_metrics(gt, mask, est)
    for i, (n_region, n_valid, bad, s1, s2, q) in enumerate(ref):     # the two ways agree
        e, r = divmod(i, 2)
        assert res["counts"][e, r].tolist() == [n_region, n_valid] + bad.tolist(), (e, r)
        assert np.array_equal(res["quantiles"][e, r], q.cpu().numpy()), (e, r)
        assert abs(res["sums"][e, r, 0] - float(s1)) <= 1e-9 * float(s1)
    torch_ms = event_ms(lambda: torch_metrics(gt, mask, est), reps)
    n = width * height
    bytes_all = n_est * n * BYTES_PER_PIXEL * PASSES
    out = {"n_est": n_est, "all_equal": bool(all_equal), "n_valid_all": res["counts"][:, 0, 1].tolist(), "avgerr_all": [round(float(v), 4) for v in res["avgerr"][:, 0]],
           "quantiles_all_est0": [round(float(v), 4) for v in res["quantiles"][0, 0]]}
    for i, k in enumerate(GROUPS):
        out[k + "_ms"] = summary(runs[:, i])
    out["kernels_ms"] = summary(runs[:, :len(GROUPS)].sum(1))
    out["call_wall_ms"] = summary(runs[:, -1])
    out["call_wall_host_inputs_ms"] = summary(host_wall)
    out["algorithmic_MB"] = round(bytes_all / 1e6, 1)
    out["classify_MB"] = round(bytes_all / PASSES / 1e6, 1)
    out["stream_bound_ms"] = round(bytes_all / (stream_gbs * 1e9) * 1e3, 4)
    out["classify_GBs"] = round(bytes_all / PASSES / 1e9 / (out["classify_ms"]["median"] * 1e-3), 1)
    out["select_GBs"] = round(bytes_all * 2 / PASSES / 1e9 / (out["select_ms"]["median"] * 1e-3), 1)
    out["torch_ms"] = summary(torch_ms)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=6048)
    ap.add_argument("--height", type=int, default=4032)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--all_equal", action="store_true")
    a = ap.parse_args()
    e3d = importlib.import_module("dataset-pipeline_amd")
    if e3d.lib().e3d_init(0) < 1:
        raise SystemExit("bench_stereo_eval.py: no HIP device")
    dev = torch.device("cuda:0")
    src = torch.empty(1 << 28, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    copy_ms = event_ms(lambda: dst.copy_(src), a.reps)
    stream_gbs = 2 * src.numel() * 4 / 1e9 / (float(np.median(copy_ms)) * 1e-3)
    del src, dst
    torch.cuda.empty_cache()
    out = {"width": a.width, "height": a.height, "reps": a.reps, "thresholds": THRESHOLDS, "percentiles": PERCENTILES,
           "stream_copy_1GiB_ms": summary(copy_ms), "stream_GBs": round(stream_gbs, 1), "runs": []}
    cases = [(1, False), (4, False)] + ([(1, True)] if a.all_equal else [])
    for n_est, all_equal in cases:
        out["runs"].append(run(e3d, a.width, a.height, n_est, a.reps, dev, all_equal, stream_gbs))
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
