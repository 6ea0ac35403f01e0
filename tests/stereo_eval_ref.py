"""Numpy restatement of the StereoEvaluator rules (include/e3d_hip.h, e3d_evaluate_disparity), written from the rules and not from
the kernels: f32 np.abs(e - gt), integer counts, math.fsum for the sums, np.sort(err)[k] for the quantiles, the palette.  The arbiter of
tests/test_gpu_stereo_eval.py and tests/test_gpu_cli_stereo_eval.py."""
import math

import numpy as np

F = np.float32
DEFAULT_THRESHOLDS = (0.5, 1, 2, 4)
DEFAULT_PERCENTILES = (50, 90, 95, 99)
PALETTE = np.array([(49, 54, 149), (69, 117, 180), (116, 173, 209), (171, 217, 233), (254, 224, 144), (253, 174, 97), (244, 109, 67), (215, 48, 39),
                    (165, 0, 38)], np.uint8)
INVALID_COLOUR = np.array((255, 0, 255), np.uint8)
REGIONS = ("all", "nocc")


def check_arguments(width, height, n_est, thresholds, percentiles):
    """Raises ValueError for what the library refuses; -> (thresholds f32, percentiles int32)."""
    if width < 1 or height < 1 or width * height >= 2 ** 31:
        raise ValueError("size")
    if n_est < 1:
        raise ValueError("no estimate")
    thr = np.asarray(thresholds, F).reshape(-1)
    if not 1 <= len(thr) <= 8:
        raise ValueError("number of thresholds")
    for t in range(len(thr)):
        if not np.isfinite(thr[t]) or not thr[t] >= 0 or (t > 0 and not thr[t] > thr[t - 1]):
            raise ValueError("thresholds")
    pct = np.asarray(percentiles, np.int64).reshape(-1)
    if len(pct) > 8 or any(p < 1 or p > 100 for p in pct):
        raise ValueError("percentiles")
    return thr, pct.astype(np.int32)


def regions(gt, mask):
    """Rule 1 -> (region 0, region 1) as boolean arrays."""
    known = np.isfinite(np.asarray(gt, F))
    if mask is None:
        return known, known.copy()
    mask = np.asarray(mask, np.uint8)
    return known & (mask != 0), known & (mask == 255)


def errors(gt, est):
    """Rules 2 and 3 -> (valid, err f32); err is meaningless where the pixel is unknown or the estimate invalid."""
    gt, est = np.asarray(gt, F), np.asarray(est, F)
    with np.errstate(invalid="ignore", over="ignore"):
        err = np.abs(est - gt).astype(F)
    return np.isfinite(est), err


def quantile_index(p, n):
    """Rule 6: k = ceil(p n / 100) - 1 in integers."""
    return (int(p) * int(n) + 99) // 100 - 1


def scores(counts, sums):
    """Rule 7 from counts[..., 2 + T] and sums[..., 2]; plain Python floats, one element at a time."""
    counts, sums = np.asarray(counts, np.int64), np.asarray(sums, np.float64)
    T = counts.shape[-1] - 2
    lead = counts.shape[:-1]
    out = {"coverage": np.zeros(lead), "avgerr": np.zeros(lead), "rms": np.zeros(lead), "bad": np.zeros(lead + (T,)), "bad_or_missing": np.zeros(lead + (T,))}
    for idx in np.ndindex(*lead):
        n_region, n_valid = int(counts[idx][0]), int(counts[idx][1])
        if n_region:
            out["coverage"][idx] = n_valid / n_region
        if n_valid:
            out["avgerr"][idx] = float(sums[idx][0]) / n_valid
            out["rms"][idx] = math.sqrt(float(sums[idx][1]) / n_valid)
        for t in range(T):
            n_bad = int(counts[idx][2 + t])
            if n_valid:
                out["bad"][idx + (t,)] = n_bad / n_valid
            if n_region:
                out["bad_or_missing"][idx + (t,)] = (n_bad + n_region - n_valid) / n_region
    return out


def error_map(gt, mask, est, thresholds):
    """Rule 8 -> [H, W, 3] uint8."""
    thr = np.asarray(thresholds, F)
    T = len(thr)
    r0, r1 = regions(gt, mask)
    valid, err = errors(gt, est)
    c = np.zeros(err.shape, np.int64)
    for t in range(T):
        c += err > thr[t]
    out = PALETTE[np.where(valid, (c * 8) // T, 0)]
    out[~valid] = INVALID_COLOUR
    out[r0 & ~r1] >>= 1
    out[~r0] = 0
    return out


def evaluate(gt, mask, estimates, thresholds=DEFAULT_THRESHOLDS, percentiles=DEFAULT_PERCENTILES, error_maps=False):
    """Everything e3d.evaluate_disparity returns, under the same keys."""
    gt = np.asarray(gt, F)
    estimates = np.asarray(estimates, F)
    if estimates.ndim == 2:
        estimates = estimates[None]
    H, W = gt.shape
    thr, pct = check_arguments(W, H, len(estimates), thresholds, percentiles)
    T, P = len(thr), len(pct)
    reg = regions(gt, mask)
    counts = np.zeros((len(estimates), 2, 2 + T), np.int64)
    sums = np.zeros((len(estimates), 2, 2), np.float64)
    quantiles = np.full((len(estimates), 2, P), np.nan, F)
    for e, est in enumerate(estimates):
        valid, err = errors(gt, est)
        for r in range(2):
            v = err[reg[r] & valid]
            counts[e, r, 0] = int(reg[r].sum())
            counts[e, r, 1] = len(v)
            for t in range(T):
                counts[e, r, 2 + t] = int((v > thr[t]).sum())
            d = v.astype(np.float64)
            sums[e, r, 0] = math.inf if np.isinf(d).any() else math.fsum(d)
            sums[e, r, 1] = math.inf if np.isinf(d).any() else math.fsum(d * d)
            if len(v):
                s = np.sort(v)
                for k, p in enumerate(pct):
                    quantiles[e, r, k] = s[quantile_index(p, len(v))]
    out = {"thresholds": thr, "percentiles": pct, "counts": counts, "sums": sums, "quantiles": quantiles}
    out.update(scores(counts, sums))
    if error_maps:
        out["error_maps"] = np.stack([error_map(gt, mask, est, thr) for est in estimates])
    return out
