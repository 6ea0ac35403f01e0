"""StereoEvaluator on the GPU (e3d_evaluate_disparity) against the numpy restatement of tests/stereo_eval_ref.py: counts, quantile bits
and error maps equal; the f64 sums within (n_valid - 1) 2^-53 sum, the bound on adding non-negative f64 terms in any order (the
restatement's math.fsum is the correctly rounded sum); the derived scores follow from those.  Shapes that are no multiple of a wave
or a block, one with several blocks per estimate and three estimates; error contents that put everything into one histogram bin, that
differ in the last digit only, zeros, denormals, infinities and invalid estimates."""
import ctypes as C

import numpy as np
import pytest

import stereo_eval_ref as ser

pytestmark = pytest.mark.gpu
F = np.float32
inf, nan = np.inf, np.nan
SHAPES = [(1, 1), (63, 1), (64, 1), (65, 3), (257, 129)]                     # W x H
SETTINGS = [((0.5, 1, 2, 4), (50, 90, 95, 99)), ((1,), ()), ((0, 0.25, 0.5, 1, 2, 4, 8, 16), (1, 25, 50, 75, 99, 100, 100, 1))]


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _from_bits(b):
    return np.ascontiguousarray(b, np.uint32).view(F)


def _gt(rng, W, H):
    """disparities in (0, 64) with a fifth of the pixels unknown"""
    g = rng.uniform(0, 64, (H, W)).astype(F)
    g[rng.random((H, W)) < 0.2] = inf
    return g


def _mask(rng, W, H):
    return rng.choice(np.array([0, 128, 255], np.uint8), (H, W), p=[0.1, 0.3, 0.6])


# ---- error contents: each -> (gt, mask, estimates [n, H, W]) -------------------------------------------------------------------------------
def c_random(rng, W, H):
    """noise, gross errors, negative and invalid estimates, the three mask classes"""
    g = _gt(rng, W, H)
    e = (g + rng.normal(0, 1, (H, W))).astype(F)
    e[~np.isfinite(g)] = rng.uniform(0, 64, (H, W)).astype(F)[~np.isfinite(g)]
    u = rng.random((H, W))
    e[u < 0.05] = rng.uniform(-64, 128, (H, W)).astype(F)[u < 0.05]
    e[(u > 0.90) & (u < 0.93)] = nan
    e[(u > 0.93) & (u < 0.95)] = inf
    e[(u > 0.95) & (u < 0.96)] = -inf
    return g, _mask(rng, W, H), e[None]


def c_all_equal(rng, W, H):
    """every error is 1.5: one bin through every pass"""
    g = np.full((H, W), 8, F)
    return g, _mask(rng, W, H), np.full((1, H, W), 9.5, F)


def c_low_bits(rng, W, H):
    """errors that differ in the lowest 1 to 3 mantissa bits only: the last digit decides"""
    g = np.zeros((H, W), F)
    e = np.stack([_from_bits(0x3FC00000 | rng.integers(0, 1 << k, (H, W)).astype(np.uint32)) for k in (1, 2, 3)])
    return g, None, e * rng.choice(np.array([-1, 1], F), (H, W))


def c_zeros_and_denormals(rng, W, H):
    g = np.zeros((H, W), F)
    e = _from_bits(rng.integers(0, 1200, (H, W)).astype(np.uint32) * (rng.random((H, W)) < 0.7))
    e2 = e.copy()
    e2[rng.random((H, W)) < 0.5] *= F(-1)                                    # -0 and negative denormals
    return g, _mask(rng, W, H), np.stack([e, e2])


def c_at_thresholds(rng, W, H):
    """errors exactly at, one float below and one float above each threshold of every setting"""
    thr = np.array(sorted({t for s in SETTINGS for t in s[0]}), F)
    near = np.concatenate([thr, np.nextafter(thr, F(inf)), np.nextafter(thr[thr > 0], F(-inf))])
    g = rng.integers(0, 32, (H, W)).astype(F)                                # small integers: g + d and (g + d) - g are exact
    d = rng.choice(near, (H, W))
    return g, rng.integers(0, 256, (H, W)).astype(np.uint8), (g + d)[None]


def c_overflow(rng, W, H):
    """e = 3e38 against gt = -3e38 overflows to +inf, which is a valid error; a mask of arbitrary bytes"""
    g, _, e = c_random(rng, W, H)
    k = rng.random((H, W)) < 0.1
    g[k] = -3e38
    e[0][k] = 3e38
    g[0, 0] = -3e38; e[0, 0, 0] = 3e38
    return g, rng.integers(0, 256, (H, W)).astype(np.uint8), e


def c_invalid(rng, W, H):
    """an estimate that is invalid everywhere beside one that is not; mask == NULL"""
    g, _, e = c_random(rng, W, H)
    return g, None, np.stack([np.full((H, W), nan, F), e[0], np.full((H, W), -inf, F)])


def c_tiny_regions(rng, W, H):
    """region 1 with one pixel, of which estimate 0 is valid and estimate 1 is not; region 0 with that pixel and at most one more"""
    g, _, e = c_random(rng, W, H)
    m = np.zeros((H, W), np.uint8)
    g[0, 0] = 3; m[0, 0] = 255
    e = np.stack([e[0], e[0]])
    e[0, 0, 0] = 4.25; e[1, 0, 0] = nan
    if W > 1:
        g[0, W - 1] = 5; m[0, W - 1] = 7; e[:, 0, W - 1] = 5
    return g, m, e


CONTENTS = [c_random, c_all_equal, c_low_bits, c_zeros_and_denormals, c_at_thresholds, c_overflow, c_invalid, c_tiny_regions]


def assert_same(G, R):
    assert np.array_equal(G["counts"], R["counts"])
    assert np.array_equal(_bits(G["quantiles"]), _bits(R["quantiles"]))
    assert G["sums"].shape == R["sums"].shape
    n_valid = R["counts"][..., 1]
    for idx in np.ndindex(*R["sums"].shape):
        g, r = G["sums"][idx], R["sums"][idx]
        if np.isinf(r):
            assert g == r, idx
        else:
            assert abs(g - r) <= max(int(n_valid[idx[:2]]) - 1, 0) * 2.0 ** -53 * r, (idx, g, r)
    if "error_maps" in R:
        assert np.array_equal(G["error_maps"], R["error_maps"])
    for key in ("coverage", "bad", "bad_or_missing"):                        # from the counts alone
        assert np.array_equal(G[key], R[key]), key
    for key in ("avgerr", "rms"):
        assert np.allclose(G[key], R[key], rtol=1e-12, atol=0, equal_nan=True), key


def check(e3d, gt, mask, est, thr, pct):
    G = e3d.evaluate_disparity(gt, mask, est, thr, pct, error_maps=True)
    R = ser.evaluate(gt, mask, est, thr, pct, error_maps=True)
    assert_same(G, R)
    return G, R


@pytest.mark.parametrize("content", CONTENTS, ids=lambda f: f.__name__[2:])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_against_the_restatement(e3d, shape, content):
    W, H = shape
    gt, mask, est = content(np.random.default_rng(1000 * W + H), W, H)
    for thr, pct in SETTINGS:
        check(e3d, gt, mask, est, thr, pct)


@pytest.fixture(scope="module")
def large():
    """1031 x 517, three estimates: several blocks per estimate in every pass, estimate strides that are no multiple of anything"""
    W, H = 1031, 517
    rng = np.random.default_rng(7)
    gt, mask, e0 = c_random(rng, W, H)
    e1 = np.where(np.isfinite(gt), gt, F(0)) + F(1.5)                        # mostly one error value: |(gt + 1.5) - gt| is 1.5 up to rounding
    e2 = gt + _from_bits(0x3FC00000 | rng.integers(0, 8, (H, W)).astype(np.uint32))
    est = np.stack([e0[0], e1.astype(F), np.where(np.isfinite(e2), e2, F(1)).astype(F)])
    thr, pct = SETTINGS[2]
    return gt, mask, est, thr, pct, ser.evaluate(gt, mask, est, thr, pct, error_maps=True)


def test_large_three_estimates(e3d, large):
    gt, mask, est, thr, pct, R = large
    tm = {}
    G = e3d.evaluate_disparity(gt, mask, est, thr, pct, error_maps=True, timings=tm)
    assert_same(G, R)
    assert R["counts"][:, 1, 1].min() > 200000                               # the case is about many valid pixels
    assert sorted(tm) == ["classify_ms", "select_ms", "sums_ms"] and all(v >= 0 for v in tm.values())
    # one estimate at a time gives the same numbers: nothing leaks between the estimates of a call
    for e in range(3):
        one = e3d.evaluate_disparity(gt, mask, est[e], thr, pct, error_maps=True)
        for key in ("counts", "sums", "quantiles", "error_maps"):
            assert one[key][0].tobytes() == G[key][e].tobytes(), (e, key)


def test_two_calls_return_identical_bytes(e3d, large):
    gt, mask, est, thr, pct, _ = large
    a = e3d.evaluate_disparity(gt, mask, est, thr, pct, error_maps=True)
    b = e3d.evaluate_disparity(gt, mask, est, thr, pct, error_maps=True)
    for key in ("counts", "sums", "quantiles", "error_maps", "avgerr", "rms"):
        assert a[key].tobytes() == b[key].tobytes(), key


def test_device_tensors_give_the_same_bytes(e3d, large):
    import torch
    gt, mask, est, thr, pct, _ = large
    a = e3d.evaluate_disparity(gt, mask, est, thr, pct, error_maps=True)
    b = e3d.evaluate_disparity(torch.from_numpy(gt).cuda(), torch.from_numpy(mask).cuda(), torch.from_numpy(est).cuda(), thr, pct, error_maps=True)
    c = e3d.evaluate_disparity(torch.from_numpy(gt), None, torch.from_numpy(est[1]).cuda(), thr, pct)
    d = e3d.evaluate_disparity(gt, None, est[1], thr, pct)
    for key in ("counts", "sums", "quantiles", "error_maps"):
        assert a[key].tobytes() == b[key].tobytes(), key
    for key in ("counts", "sums", "quantiles"):
        assert c[key].tobytes() == d[key].tobytes(), key


def test_refusals_leave_the_library_usable(e3d):
    rng = np.random.default_rng(5)
    gt, mask, est = c_random(rng, 9, 7)
    thr, pct = SETTINGS[0]

    def good():
        check(e3d, gt, mask, est, thr, pct)

    good()
    bad_calls = [
        dict(gt=np.zeros((0, 9), F), mask=None, estimates=np.zeros((0, 9), F)),                        # H < 1
        dict(gt=np.zeros((7, 0), F), mask=None, estimates=np.zeros((7, 0), F)),                        # W < 1
        dict(estimates=np.zeros((0, 7, 9), F)),                                                        # n_est < 1
        dict(thresholds=()), dict(thresholds=tuple(range(9))),                                         # T out of range
        dict(percentiles=tuple(range(1, 10))),                                                         # P out of range
        dict(thresholds=(1, nan)), dict(thresholds=(inf,)), dict(thresholds=(-0.5, 1)), dict(thresholds=(1, 1)), dict(thresholds=(2, 1)),
        dict(percentiles=(0,)), dict(percentiles=(50, 101)), dict(percentiles=(-3,)),
    ]
    for kw in bad_calls:
        args = dict(gt=gt, mask=mask, estimates=est, thresholds=thr, percentiles=pct)
        args.update(kw)
        with pytest.raises(e3d.E3DError):
            e3d.evaluate_disparity(**args)
        good()
    # what the binding cannot express: null pointers and W H >= 2^31 (refused before any memory is touched)
    lib = e3d.lib()
    t = np.array(thr, F); p = np.array(pct, np.int32)
    g, x = np.ascontiguousarray(gt), np.ascontiguousarray(est)
    P = lambda a: C.c_void_p(a.ctypes.data)                                                            # noqa: E731
    raw = [
        (None, None, 9, 7, P(x), 1, P(t), 4, P(p), 4, None),
        (P(g), None, 9, 7, None, 1, P(t), 4, P(p), 4, None),
        (P(g), None, 9, 7, P(x), 1, None, 4, P(p), 4, None),
        (P(g), None, 9, 7, P(x), 1, P(t), 4, None, 4, None),
        (P(g), None, 65536, 32768, P(x), 1, P(t), 4, P(p), 4, None),
        (P(g), None, 9, -7, P(x), 1, P(t), 4, P(p), 4, None),
        (P(g), None, 9, 7, P(x), 0, P(t), 4, P(p), 4, None),
        (P(g), None, 9, 7, P(x), 1, P(t), 0, P(p), 4, None),
        (P(g), None, 9, 7, P(x), 1, P(t), 4, P(p), -1, None),
    ]
    for args in raw:
        assert not lib.e3d_evaluate_disparity(*args)
        assert lib.e3d_last_error()
        good()
