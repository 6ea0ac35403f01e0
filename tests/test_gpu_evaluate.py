"""ReconstructionEvaluator on the GPU (e3d_evaluate_reconstruction) against the numpy restatement of tests/evaluate_ref.py.

Every class, voxel key and per-tolerance count is compared exactly: the rules fix each f32 step, and a minimum, a maximum and a count
have no order.  The 3 x T scores are f64 sums of at most 3 * 10^5 ratios in [0, 1] formed in another order than the restatement's
serial sums; they are compared at 1e-12 relative, the bound the README states for this project's f64 sums."""
import numpy as np
import pytest

import evaluate_ref as er

pytestmark = pytest.mark.gpu

F = np.float32
TOLERANCES = {1: (0.01,), 6: er.DEFAULT_TOLERANCES, 8: (0.005, 0.01, 0.02, 0.05, 0.1, 0.2, 0.5, 1.0)}
ORIGINS = [(3.0, 4.0, 1.2), (7.0, 3.0, 1.5), (5.0, 6.5, 1.0)]


def room_scans(synth, S, n, seed):
    """S scans of the synthetic room with n points each in the global frame, and the scanner positions."""
    scans, origins = [], []
    for s in range(S):
        if n:
            xyz, _, T = synth.make_scan(n, ORIGINS[s], 0.3 * s, seed + s)
            p = xyz.numpy().astype(np.float64) @ T[:3, :3].astype(np.float64).T + T[:3, 3].astype(np.float64)
        else:
            p, T = np.zeros((0, 3)), np.eye(4, dtype=F)
            T[:3, 3] = ORIGINS[s]
        scans.append(p.astype(F))
        origins.append(T[:3, 3].astype(F))
    return scans, np.stack(origins)


def noisy_resampling(scans, n, seed):
    """n points drawn from the scans with 5 mm noise; every 16th is a gross error somewhere in the room."""
    rng = np.random.default_rng(seed)
    pool = np.concatenate(scans)
    if len(pool) == 0:
        return rng.uniform(0, 3, (n, 3)).astype(F)
    p = pool[rng.integers(0, len(pool), n)].astype(np.float64) + rng.normal(0, 0.005, (n, 3))
    gross = np.arange(n) % 16 == 7
    p[gross] = rng.uniform((0.2, 0.2, 0.1), (9.8, 7.8, 2.8), (int(gross.sum()), 3))
    return p.astype(F)


def compare(e3d, rec, scans, origins, tol, h, N, E=None):
    E = er.evaluate(rec, scans, origins, tol, h, N, device="cuda") if E is None else E
    G = e3d.evaluate_reconstruction(rec, scans, origins, tol, h, N, return_classes=True, return_voxels=True)
    for key in ("near_rec", "free", "near_scan"):
        assert G[key].dtype == np.uint8 and np.array_equal(G[key], E[key]), (key, int((G[key] != E[key]).sum()), len(E[key]))
    assert G["n_scan_voxels"] == E["n_scan_voxels"] and G["n_rec_voxels"] == E["n_rec_voxels"]
    for kind in ("scan_voxels", "rec_voxels"):
        for key in ("ijk", "n_points", "count_a", "count_b"):
            assert G[kind][key].dtype == np.int32 and np.array_equal(G[kind][key], E[kind][key]), (kind, key)
    assert np.array_equal(G["evaluated_voxels"], E["evaluated_voxels"])
    for key in ("completeness", "accuracy", "f1"):
        err = np.abs(G[key] - E[key])
        print(key, "max relative deviation %.3g" % (err / np.maximum(np.abs(E[key]), 1e-300)).max())
        assert (err <= 1e-12 * np.abs(E[key])).all(), (key, G[key], E[key])
    return G, E


def test_the_device_arithmetic_of_the_restatement_is_numpy_s():
    rng = np.random.default_rng(5)
    a = rng.uniform(-1, 1, (1000, 3)).astype(F); b = rng.uniform(-1, 1, (1500, 3)).astype(F)
    b[:200] = a[:200] + F(1.0 / 64.0)
    assert np.array_equal(er.min_d2(a, b).view(np.uint32), er.min_d2(a, b, device="cuda").view(np.uint32))


# every size of one cloud with 1000 and 100 003 of the other; S, N, T and h take turns
SIZES = (0, 1, 63, 64, 65, 1000, 100003)
SIZE_CASES = sorted({(a, b) for a in SIZES for b in (1000, 100003)} | {(b, a) for a in SIZES for b in (1000, 100003)})


@pytest.mark.parametrize("case", range(len(SIZE_CASES)))
def test_room_sizes(e3d, synth, case):
    n_rec, n_scan = SIZE_CASES[case]
    S = (1, 3)[case % 2]
    N = (2, 64, 2048)[case % 3]
    T = (1, 6, 8)[(case // 2) % 3]
    h = (0.01, 0.37)[(case // 3) % 2]
    scans, origins = room_scans(synth, S, n_scan, seed=100 + case)
    rec = noisy_resampling(scans, n_rec, seed=200 + case)
    G, E = compare(e3d, rec, scans, origins, TOLERANCES[T], h, N)
    if n_rec >= 1000 and n_scan >= 1000:
        assert (E["near_rec"] == 0).any() and (E["near_rec"] == T).any() and E["n_rec_voxels"] > 256        # several blocks of the voxel kernels
        if N > 2:
            assert (E["free"] > 0).any()


def test_parameter_values_all_occur():
    cases = range(len(SIZE_CASES))
    assert len(SIZE_CASES) == 24
    assert {(1, 3)[c % 2] for c in cases} == {1, 3} and {(2, 64, 2048)[c % 3] for c in cases} == {2, 64, 2048}
    assert {(1, 6, 8)[(c // 2) % 3] for c in cases} == {1, 6, 8} and {(0.01, 0.37)[(c // 3) % 2] for c in cases} == {0.01, 0.37}


# ---- ties --------------------------------------------------------------------------------------------------------------------------
def tie_clouds(seed, n_scan=3000, n_rec=4000):
    """Clouds on the 1/64 lattice with the tolerances 5, 10, 25 and 50 lattice steps, so that d2 == thr_i and range + t_i == rmin
    happen exactly: a part of the reconstruction is a scan point moved by exactly a tolerance along a lattice direction of integer
    length, another part lies on the ray of a scan point exactly a tolerance in front of it."""
    rng = np.random.default_rng(seed)
    lengths = np.array([5, 10, 25, 50])
    # the integer vectors of length 25: 150 directions, so that the rays from the scanner fall into different pixels.  Those that
    # are 5 x a vector of length 5 (the axes and the (3, 4, 0) family) carry all four tolerances, the others 25 and 50
    dirs = set()
    for v in ((25, 0, 0), (7, 24, 0), (15, 20, 0), (12, 15, 16), (9, 12, 20)):
        for perm in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
            for signs in range(8):
                dirs.add(tuple(v[perm[a]] * (1 - 2 * ((signs >> a) & 1)) for a in range(3)))
    dirs = np.array(sorted(dirs))
    assert len(dirs) == 150 and ((dirs ** 2).sum(1) == 625).all()
    fine = (dirs % 5 == 0).all(1)

    def steps(idx):
        """One vector per direction idx whose length is a tolerance."""
        c = rng.integers(0, 4, len(idx))
        c = np.where(fine[idx], c, 2 + c % 2)
        v = dirs[idx] * lengths[c][:, None]
        assert (v % 25 == 0).all()
        return v // 25

    scan = rng.integers(-256, 257, (n_scan, 3))
    o = np.array([16, -8, 4])
    rec = rng.integers(-320, 321, (n_rec, 3))
    k = n_rec // 10
    # exactly a tolerance away from a scan point
    rec[:k] = scan[rng.integers(0, n_scan, k)] + steps(rng.integers(0, len(dirs), k))
    # exactly a tolerance in front of a scan point, on its ray from the scanner: one scan point and one such point per direction
    on_ray = o + dirs * rng.integers(3, 9, len(dirs))[:, None]
    scan = np.concatenate([scan, on_ray])
    rec[k:k + len(dirs)] = on_ray - steps(np.arange(len(dirs)))
    return (rec / 64.0).astype(F), (scan / 64.0).astype(F), (o / 64.0).astype(F), (lengths / 64.0).astype(F)


@pytest.mark.parametrize("seed", [1, 2])
def test_tie_clouds(e3d, seed):
    rec, scan, o, tol = tie_clouds(seed)
    N = 2048
    d = er.min_d2(rec, scan)
    at_threshold = np.isin(d, er.thresholds(tol)).mean()
    seen, rng_r, rmin = er.seen_ranges(rec, scan, o, N)
    at_minimum = np.any([seen & (rng_r + t == rmin) for t in tol], axis=0).mean()
    print("pairs at a threshold %.3f, points at range + t == rmin %.3f" % (at_threshold, at_minimum))
    assert 0.02 <= at_threshold <= 0.05 and 0.02 <= at_minimum <= 0.05
    G, E = compare(e3d, rec, [scan], [o], tol, 0.37, N)
    assert len(set(E["near_rec"].tolist())) == 5 and len(set(E["free"].tolist())) >= 4


# ---- special layouts ---------------------------------------------------------------------------------------------------------------
def test_origin_outside_the_cloud_and_a_scan_in_one_pixel(e3d, synth):
    scans, origins = room_scans(synth, 2, 5000, seed=31)
    origins[1] = (-20.0, 3.0, 1.0)                                     # far outside the room: the whole scan in a few pixels of one face
    rng = np.random.default_rng(32)
    cluster = (np.array([40.0, 41.0, 42.0]) + rng.normal(0, 0.001, (500, 3))).astype(F)      # seen from (0, 0, 0): one pixel
    scans.append(cluster)
    origins = np.concatenate([origins, np.zeros((1, 3), F)])
    ok, pix, _ = er.pixels(cluster, origins[2], 64)
    assert ok.all() and len(set(pix.tolist())) == 1
    rec = noisy_resampling(scans, 6000, seed=33)
    rec[:200] = (np.array([40.0, 41.0, 42.0]) * rng.uniform(0.2, 1.2, (200, 1))).astype(F)      # along the ray to the cluster, before and behind it
    G, E = compare(e3d, rec, scans, origins, er.DEFAULT_TOLERANCES, 0.05, 64)
    assert (E["free"][:200] == 6).any() and (E["free"][:200] == 0).any()


def test_nan_and_inf_rows(e3d, synth):
    scans, origins = room_scans(synth, 2, 3000, seed=41)
    rec = noisy_resampling(scans, 3000, seed=42)
    rng = np.random.default_rng(43)
    for cloud in (rec, scans[0], scans[1]):
        rows = rng.choice(len(cloud), 60, replace=False)
        cloud[rows[:20], rng.integers(0, 3, 20)] = np.nan
        cloud[rows[20:40], rng.integers(0, 3, 20)] = np.inf
        cloud[rows[40:], rng.integers(0, 3, 20)] = -np.inf
    G, E = compare(e3d, rec, scans, origins, TOLERANCES[8], 0.01, 64)
    assert (E["near_rec"] == 255).sum() == 60 and (E["free"] == 255).sum() == 60 and (E["near_scan"] == 255).sum() == 120
    # nothing but ignored points
    bad = np.full((70, 3), np.nan, F)
    G, E = compare(e3d, bad, [bad], origins[:1], TOLERANCES[6], 0.01, 64)
    assert G["n_rec_voxels"] == 0 and (G["near_rec"] == 255).all() and G["f1"].tolist() == [0.0] * 6


def test_every_search_level_is_reached(e3d):
    """The smallest tolerance is far below the point spacing, the largest spans the whole cloud, and a few points are out of reach of
    all of them: queries close at every level and some stay open to the end."""
    rng = np.random.default_rng(51)
    scan = rng.uniform(0, 1, (3000, 3)).astype(F)
    rec = rng.uniform(-0.5, 1.5, (3000, 3)).astype(F)
    rec[:300] = scan[:300] + rng.normal(0, 3e-5, (300, 3)).astype(F)
    rec[300:310] = rng.uniform(20, 30, (10, 3)).astype(F)
    rec[310:320] = rng.uniform(2.2, 2.6, (10, 3)).astype(F)
    tol =(1e-4, 1e-3, 0.01, 0.03, 0.1, 0.3, 1.0, 3.0)
    G, E = compare(e3d, rec, [scan], [[0.5, 0.5, -2.0]], tol, 0.37, 64)
    assert sorted(set(E["near_rec"].tolist())) == list(range(9)) and (E["near_rec"][300:310] == 8).all()
    assert (E["near_scan"] < 8).all() and len(set(E["near_scan"].tolist())) >= 6


# ---- reproducibility, kernel groups, refusals -------------------------------------------------------------------------------------------
def test_two_calls_identical_bytes_and_kernel_groups(e3d, synth):
    scans, origins = room_scans(synth, 2, 20000, seed=61)
    rec = noisy_resampling(scans, 30000, seed=62)
    tm = {}
    a = e3d.evaluate_reconstruction(rec, scans, origins, return_classes=True, return_voxels=True, timings=tm)
    b = e3d.evaluate_reconstruction(rec, scans, origins, return_classes=True, return_voxels=True)
    for key in ("completeness", "accuracy", "f1", "evaluated_voxels", "near_rec", "free", "near_scan"):
        assert a[key].tobytes() == b[key].tobytes(), key
    for kind in ("scan_voxels", "rec_voxels"):
        for key in ("ijk", "n_points", "count_a", "count_b"):
            assert a[kind][key].tobytes() == b[kind][key].tobytes()
    assert a["tolerances"].tolist() == np.array(er.DEFAULT_TOLERANCES, F).tolist() and 0 < a["f1"][0] < a["f1"][5] <= 1
    assert sorted(tm) == sorted(g + "_ms" for g in ("grid", "search", "range", "voxels"))
    assert all(np.isfinite(x) and x >= 0 for x in tm.values()) and tm["search_ms"] > 0


def test_torch_device_reconstruction(e3d, synth):
    import torch
    scans, origins = room_scans(synth, 1, 2000, seed=71)
    rec = noisy_resampling(scans, 2000, seed=72)
    a = e3d.evaluate_reconstruction(rec, scans, origins, return_classes=True)
    b = e3d.evaluate_reconstruction(torch.from_numpy(rec).cuda(), scans, origins, return_classes=True)
    for key in ("f1", "near_rec", "free", "near_scan"):
        assert a[key].tobytes() == b[key].tobytes()


def test_refusals_and_recovery(e3d):
    rng = np.random.default_rng(81)
    scan = rng.uniform(0, 1, (100, 3)).astype(F)
    rec = rng.uniform(0, 1, (100, 3)).astype(F)
    o = [[0.5, 0.5, 0.5]]
    good = e3d.evaluate_reconstruction(rec, [scan], o, (0.05, 0.1), 0.1, 64)
    far = rec.copy()
    far[7, 2] = -F(2 ** 20) * F(0.1)
    assert abs(float(far[7, 2] / F(0.1))) >= 2 ** 20
    bad_calls = [dict(tolerances=()), dict(tolerances=(0.1, 0.05)), dict(tolerances=(0.05, 0.05)), dict(tolerances=(0.0, 0.1)), dict(tolerances=(-0.1,)),
                 dict(tolerances=(np.nan,)), dict(tolerances=(0.1, np.inf)), dict(tolerances=tuple(0.01 * k for k in range(1, 10))),
                 dict(voxel_size=0.0), dict(voxel_size=-0.1), dict(voxel_size=np.nan), dict(voxel_size=np.inf),
                 dict(cube_map_size=63), dict(cube_map_size=0), dict(cube_map_size=1), dict(cube_map_size=8194), dict(cube_map_size=-2),
                 dict(rec=far), dict(scans=[scan, far]), dict(scans=[], origins=np.zeros((0, 3), F))]
    for kw in bad_calls:
        args = dict(rec=rec, scans=[scan], origins=o, tolerances=(0.05, 0.1), voxel_size=0.1, cube_map_size=64)
        args.update(kw)
        if len(args["scans"]) == 2:
            args["origins"] = o * 2
        with pytest.raises(e3d.E3DError):
            e3d.evaluate_reconstruction(**args)
        with pytest.raises(ValueError):
            er.evaluate(args["rec"], args["scans"], args["origins"], args["tolerances"], args["voxel_size"], args["cube_map_size"])
        again = e3d.evaluate_reconstruction(rec, [scan], o, (0.05, 0.1), 0.1, 64)
        assert again["f1"].tobytes() == good["f1"].tobytes()
    # allowed: eight tolerances, N = 2 and 8192, an ignored point out of range
    far[7, 0] = np.nan
    e3d.evaluate_reconstruction(far, [scan], o, tuple(0.01 * k for k in range(1, 9)), 0.1, 2)
    compare(e3d, rec, [scan], o, (0.05,), 0.1, 8192)
