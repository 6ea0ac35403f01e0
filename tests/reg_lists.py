"""Observation lists with partial visibility for the registration tests: the oracle's full list of a scene, thinned at random
or cut down to a spatially compact handful.  In such a list the observation row i differs from the point index o_idx[i], some
neighbour flags are cleared, and (for the short lists) the list ends inside a 64-lane chunk."""
import numpy as np

from reg_util import make_reg_scene

ROBUST = {0: 0.0, 1: 47.434166, 2: 30.0}          # robust weighting type -> parameter (none, Huber, Tukey)
N_POINTS, SEED = 3000, 7
# oracle (f32 residuals and products) against reg_ref (float64): bounds on (sums, H, b) in the normalisation of reg_ref.deviations,
# 10 times the worst deviation measured over the cases of tests/test_reg_ref_host.py (1.2e-7, 8.3e-8, 2.8e-7; the table there)
ORACLE_VS_REF = (1.2e-6, 8.3e-7, 2.8e-6)


def scene(K, model=0):
    return make_reg_scene(n_points=N_POINTS, seed=SEED, K=K, model=model)


def full_list(rb, S):
    """(camera pyramid, (idx, x, y, scale)): what the oracle observes of scene S at image scale 0 with a 1 pixel border."""
    levels = rb.camera_pyramid(rb.make_camera(S["width"], S["height"], S["params"], S["model"]), S["n_levels"])
    depth = rb.splat_depth(S["pts"], S["R"], S["t"], levels[0], 0.03)
    o = rb.observe(S["pts"], S["point_radius"], S["R"], S["t"], levels, 0, S["pyr"], None, depth, 0, 1, 0, S["n_levels"])
    return levels, o


def drop(o, seed, prob=0.1):
    """Every observation is dropped with probability `prob`."""
    keep = np.random.RandomState(seed).uniform(size=len(o[0])) >= prob
    return tuple(a[keep].copy() for a in o[:4])


def compact(pts, o, m):
    """The m observed points nearest to the centroid of the cloud, in index order: neighbours of one another, so that flags are
    set even in a list of a few dozen."""
    c = np.asarray(pts, np.float64).mean(axis=0)
    d = np.linalg.norm(np.asarray(pts, np.float64)[o[0]] - c, axis=1)
    sel = np.sort(np.argsort(d, kind="stable")[:m])
    return tuple(a[sel].copy() for a in o[:4])


def assert_partial(S, o, flags, counts=None):
    """The properties that keep a list away from the trivial case row == point, all flags set, every residual kind everywhere."""
    assert not np.array_equal(o[0], np.arange(len(o[0])))
    share = flags.mean()
    assert 0.3 <= share <= 0.95, share
    if counts is not None:
        assert 0.25 * counts[0] <= counts[1] <= 0.75 * counts[0], counts
