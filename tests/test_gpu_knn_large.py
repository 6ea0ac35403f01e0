"""e3d_local_outlier_removal with 128 <= mean_k <= 1023 (k_knn_large: one wave per query, the k + 1 nearest selected in LDS)
against the CPU oracle: first-pass mean distances bit for bit, inlier masks identical.  The reference's documented ETH3D
cleanup is `--filter 270,1.15 --filter 20,1.15`."""
import numpy as np
import pytest

import knn_large_case as case

pytestmark = pytest.mark.gpu


def _check(e3d, ob, name, mean_k, factor, first=None, twice=False):
    pts = case.cloud(name, first, twice)
    gi, gd = e3d.local_outlier_removal(pts, mean_k, factor, return_distances=True)
    oi, od = case.oracle(ob, name, mean_k, factor, first, twice)
    n_dist = int((gd.view(np.uint32) != od.view(np.uint32)).sum())
    n_mask = int((gi != oi).sum())
    print("%s first=%s twice=%s mean_k=%d: %d points, %d distances differ, %d mask entries differ, inlier share %.4f (oracle %.4f)"
          % (name, first, twice, mean_k, len(pts), n_dist, n_mask, gi.mean(), oi.mean()))
    assert n_dist == 0
    assert n_mask == 0
    return gi, gd


@pytest.mark.parametrize("mean_k,factor", [(127, 1.15), (128, 1.15), (270, 1.15), (511, 1.3), (1023, 1.15)])
def test_room_cloud_matches_oracle(e3d, ob, mean_k, factor):
    """The last k of the per-lane lists (mean_k = 127), the first of the wave-per-query search, the documented value, a middle
    one and the top.  The oracle alone gives inlier shares 0.9602, 0.9495, 0.9790 and 0.9224 for mean_k 128, 270, 511, 1023."""
    gi, _ = _check(e3d, ob, "room", mean_k, factor)
    assert 0.9 < gi.mean() < 0.99
    gn = e3d.local_outlier_removal(case.cloud("room"), mean_k, factor, negative=True)
    assert np.array_equal(gn, ~gi)


def test_distance_ties(e3d, ob):
    """A lattice: hundreds of candidates tie at the k-th distance, so the mask depends on the index tie-break (oracle: 0.9334)."""
    gi, _ = _check(e3d, ob, "lattice", 270, 1.15)
    assert round(float(gi.mean()), 4) == 0.9334


def test_level_retry_to_whole_cloud(e3d, ob):
    """A far cluster of 50 points needs 221 neighbours from the room 30 m away: retried level by level up to the covering block."""
    _check(e3d, ob, "far", 270, 1.15)


@pytest.mark.parametrize("m,kept", [(1, 1), (5, 4), (200, 160), (271, 213), (272, 213), (400, 295)])
def test_small_clouds(e3d, ob, m, kept):
    """Fewer points than k, exactly k, one more: shorter lists (padded with -1), the mean still divides by mean_k."""
    gi, _ = _check(e3d, ob, "room", 270, 1.15, first=m)
    assert int(gi.sum()) == kept


def test_duplicates(e3d, ob):
    """Every point stored twice: entry 0 of a list is the lower index of the pair, the twin follows at distance 0."""
    gi, gd = _check(e3d, ob, "room", 270, 1.15, first=3000, twice=True)
    assert (gd > 0).all() and round(float(gi.mean()), 3) == 0.899


def test_non_finite_points(e3d, ob):
    bad = case.cloud("room").copy()
    bad[[7, 100, 40799]] = [np.nan, 0, 0]
    bad[55, 2] = np.inf
    good = np.isfinite(bad).all(1)
    gi, gd = e3d.local_outlier_removal(bad, 270, 1.15, return_distances=True)
    oi, od = ob.local_outlier_removal(bad[good], 270, 1.15)
    assert not gi[~good].any() and (gd[~good] == 0).all()
    assert np.array_equal(gd[good].view(np.uint32), od.view(np.uint32)) and np.array_equal(gi[good], oi)


def test_range_checks(e3d):
    pts = case.cloud("room", first=400)
    with pytest.raises(e3d.E3DError, match="1023"):
        e3d.local_outlier_removal(pts, 1024, 1.15)
    with pytest.raises(e3d.E3DError):
        e3d.local_outlier_removal(pts, 0, 1.15)


def test_small_k_path_untouched(e3d):
    """The workspace is shared between the searches: a large-k call in between must not change what the k = 32 kernels give."""
    pts = case.cloud("room")
    n0, c0, i0 = e3d.normals_knn(pts, 32, return_knn=True)
    e3d.local_outlier_removal(pts, 270, 1.15)
    n1, c1, i1 = e3d.normals_knn(pts, 32, return_knn=True)
    assert np.array_equal(i0, i1)
    assert np.array_equal(n0.view(np.uint32), n1.view(np.uint32)) and np.array_equal(c0.view(np.uint32), c1.view(np.uint32))
