"""The image-registration kernels on observation lists with partial visibility and at neighbour counts other than 5.

In the scenes of tests/test_gpu_reg.py every point is observed in every image: the observation row equals the point index, every
neighbour flag is set and only K = 5 runs.  Here the lists are subsets of the oracle's full list (tests/reg_lists.py), handed to
both sides with set_observations; the device computes its own flags and neighbour rows from them.  Every result is compared with
the CPU oracle at the tolerances of test_gpu_reg.test_accumulate_and_cost and with the float64 numpy restatement tests/reg_ref.py
(fed the device's own pass-1 rows) at those tolerances plus the oracle-against-numpy bounds of tests/test_reg_ref_host.py."""
import functools

import numpy as np
import pytest

import reg_lists
import reg_ref
import test_gpu_reg as base

pytestmark = pytest.mark.gpu

PARAM_COUNT = {0: 4, 1: 8, 2: 12, 4: 5}
GPU_VS_ORACLE = (1e-9, 1e-6, 1e-5)               # sums, H, b: test_accumulate_and_cost (b: its 10 * tol)


@functools.lru_cache(maxsize=None)
def _scene(K, model):
    from oracle import reg_binding as rb
    S = reg_lists.scene(K, model)
    levels, full = reg_lists.full_list(rb, S)
    return S, levels, full


def _problem(e3d, rb, S, rtype=1, **pk):
    P, levels = base._setup(e3d, rb, S, robust_weighting_type=rtype, robust_weighting_parameter=reg_lists.ROBUST[rtype], **pk)
    return P


def _within(got, want, tols, what):
    e = reg_ref.deviations(got[0], got[1], got[2], want[0], want[1], want[2])
    print("%s: sums %.2e H %.2e b %.2e" % (what, e[0], e[1], e[2]))
    assert e[0] <= tols[0] and e[1] <= tols[1] and e[2] <= tols[2], (what, e, tols)


def _compare(rb, P, image_id, pts, radius, nbr, K, fixed, var, obs_counts, cam, pyr, R, t, o, rtype, what, w_fixed=1.0, w_var=1.0,
             rig=None, rparam=None):
    """Set the list `o` on the device, then flags, accumulate and cost against the oracle and reg_ref.  -> (flags, device results)"""
    n_pts, n = len(pts), len(o[0])
    rparam = reg_lists.ROBUST[rtype] if rparam is None else rparam
    P.set_observations(image_id, 0, *o)
    g = P.get_observations(image_id, 0, n)
    of = rb.neighbors_observed(n_pts, o[0], nbr, K)
    assert np.array_equal(g[0], o[0]) and np.array_equal(g[4], of) and np.array_equal(of, reg_ref.flags(n_pts, o[0], nbr))
    H, b, sums, counts = P.accumulate(image_id, 0)
    Ho, bo, so, co = rb.accumulate(pts, radius, nbr, K, fixed, var, obs_counts, cam, 0, pyr, R, t, o, of, rtype, rparam, w_fixed, w_var, rig=rig)
    s2, c2 = P.cost(image_id, 0)
    so2, co2 = rb.cost(n_pts, nbr, K, fixed, var, obs_counts, 0, pyr, o, of, rtype, rparam, w_fixed, w_var)
    assert np.array_equal(counts, co) and np.array_equal(c2, co2) and np.array_equal(counts, c2)
    assert H.shape == Ho.shape and np.array_equal(np.tril(H, -1), np.zeros_like(H))
    I, JI, JP = P.pass1(image_id, 0, n)
    if rig is None:
        J = np.concatenate([JI, JP], axis=1)
    else:      # the binding's pass1 leaves out the rig-extrinsics block of a dependent image: that block from the oracle's pass 1
        Io, JIo, JPo, JRo = rb.pass1(pts, radius, cam, 0, pyr, R, t, o, rig=rig)
        assert np.array_equal(I.view(np.uint32), Io.view(np.uint32))
        J = np.concatenate([JI, JRo, JP], axis=1)
    rparam32 = float(np.float32(rparam))
    Hr, br, sr, cr = reg_ref.accumulate(I, J, o[0], of, nbr, fixed, var, obs_counts, rtype, rparam32, w_fixed, w_var)
    sr2, cr2 = reg_ref.cost(I, o[0], of, nbr, fixed, var, obs_counts, rtype, rparam32, w_fixed, w_var)
    assert np.array_equal(counts, cr) and np.array_equal(counts, cr2)
    if not counts.any():
        for a in (H, b, sums, s2, Ho, bo, so, so2, Hr, br, sr, sr2):
            assert not np.asarray(a).any()
        return of, (H, b, sums, counts, s2, c2)
    _within((H, b, sums), (Ho, bo, so), GPU_VS_ORACLE, what + " vs oracle")
    assert np.abs(s2 - so2).max() <= 1e-12 * np.abs(so2).max()
    assert np.abs(s2 - sums).max() <= 1e-9 * np.abs(sums).max()          # the cost pass sees the residuals of the accumulate pass
    both = tuple(a + c for a, c in zip(GPU_VS_ORACLE, reg_lists.ORACLE_VS_REF))
    _within((H, b, sums), (Hr, br, sr), both, what + " vs numpy")
    assert np.abs(s2 - sr2).max() <= both[0] * np.abs(sr2).max()
    return of, (H, b, sums, counts, s2, c2)


def _compare_scene(e3d, rb, K, model, o, rtype, what, **weights):
    S, levels, full = _scene(K, model)
    pk = {}
    if "w_fixed" in weights:
        pk["fixed_residuals_weight"] = weights["w_fixed"]
    if "w_var" in weights:
        pk["variable_residuals_weight"] = weights["w_var"]
    P = _problem(e3d, rb, S, rtype, **pk)
    return _compare(rb, P, 0, S["pts"], S["point_radius"], S["nbr"], K, S["fixed_desc"], S["var_desc"], S["obs_counts"], levels[0],
                    S["pyr"], S["R"], S["t"], o, rtype, what, **weights)


# ---- C1: thinned lists at every neighbour count -------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,rtype", [(0, 1), (1, 1), (2, 1), (4, 1), (0, 2), (2, 2), (1, 0)])      # V = 10, 14, 18, 11
@pytest.mark.parametrize("K", [1, 3, 5, 8])
def test_thinned_list(e3d, rb, K, model, rtype):
    """Each observation dropped with probability 0.1: K = 5 runs the matrix-core pass 2 for V > 10, every other K the per-thread
    kernel with its row splits (two launches for V = 11 and 14, three for 18) and the run-time-K flag, cost and colour kernels."""
    S, levels, full = _scene(K, model)
    o = reg_lists.drop(full, 100 + K)
    of, (H, b, sums, counts, s2, c2) = _compare_scene(e3d, rb, K, model, o, rtype, "K %d model %d robust %d" % (K, model, rtype))
    reg_lists.assert_partial(S, o, of, counts)
    assert H.shape == (PARAM_COUNT[model] + 6,) * 2 and counts[0] == of.sum() > 1000
    print("K %d model %d: %d observations, flag share %.3f, counts %s" % (K, model, len(o[0]), of.mean(), counts))


# ---- C2: a weight of zero switches a residual kind off -------------------------------------------------------------------------------
@pytest.mark.parametrize("K,model", [(3, 1), (5, 1), (5, 0)])
def test_weight_zero_skips_a_kind_on_a_thinned_list(e3d, rb, K, model):
    S, levels, full = _scene(K, model)
    o = reg_lists.drop(full, 100 + K)
    _, both = _compare_scene(e3d, rb, K, model, o, 1, "K %d both kinds" % K)
    for kind, weights in ((1, dict(w_var=0.0)), (0, dict(w_fixed=0.0))):
        _, one = _compare_scene(e3d, rb, K, model, o, 1, "K %d without kind %d" % (K, kind), **weights)
        H, b, sums, counts, s2, c2 = one
        assert sums[kind] == 0 and counts[kind] == 0 and s2[kind] == 0 and c2[kind] == 0
        # the other kind is untouched, to the bit: its sum and count do not depend on what else the pass accumulates
        assert sums[1 - kind] == both[2][1 - kind] and counts[1 - kind] == both[3][1 - kind] > 100
        assert s2[1 - kind] == both[4][1 - kind] and c2[1 - kind] == both[5][1 - kind]
        assert not np.array_equal(H, both[0]) and not np.array_equal(b, both[1])


# ---- C3: colour update over two different lists ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3, 5, 8])
def test_color_update_on_two_thinned_lists(e3d, rb, K):
    """Counts 0, 1 and >= 2 all occur, so the divide-only-if-more-than-one rule is exercised on every branch.  Bit-exact against the
    oracle; reg_ref within the f32 rounding of the differences, their sum and the division: 2^-23 of the largest difference."""
    S, levels, full = _scene(K, 0)
    n = len(S["pts"])
    P = _problem(e3d, rb, S)
    do = np.zeros((n, K), np.float32); co = np.zeros(n, np.int32)
    dr = np.zeros((n, K)); cr = np.zeros(n, np.int64)
    largest = 0.0
    P.color_begin(0)
    for seed in (100 + K, 200 + K):
        o = reg_lists.drop(full, seed)
        of = rb.neighbors_observed(n, o[0], S["nbr"], K)
        P.set_observations(0, 0, *o)
        assert np.array_equal(P.get_observations(0, 0, len(o[0]))[4], of)
        P.color_accumulate(0, 0)
        rb.color_accumulate(n, S["nbr"], K, 0, S["pyr"], o, of, do, co)
        I = P.pass1(0, 0, len(o[0]))[0]
        reg_ref.color_accumulate(I, o[0], reg_ref.flags(n, o[0], S["nbr"]), S["nbr"], dr, cr)
        one = np.zeros((n, K)); reg_ref.color_accumulate(I, o[0], of, S["nbr"], one, np.zeros(n, np.int64))
        largest = max(largest, np.abs(one).max())
    P.color_finish(0)
    rb.color_finish(K, do, co); reg_ref.color_finish(dr, cr)
    d, c = P.get_variable_descriptors(0, n)
    assert np.array_equal(c, co) and np.array_equal(d.view(np.uint32), do.view(np.uint32))
    assert np.array_equal(c, cr)
    assert (c == 0).sum() > 50 and (c == 1).sum() > 50 and (c >= 2).sum() > 50
    assert largest > 10 and np.abs(d - dr).max() <= 2.0 ** -23 * largest


# ---- C4: short compact lists: the tails of the 64-lane chunks --------------------------------------------------------------------------
COMPACT_M = [1, 2, 9, 63, 64, 65, 255, 256, 257]
FLAGS_SET = {(5, 63): 48, (5, 64): 49, (5, 65): 50, (5, 255): 219, (5, 256): 220, (5, 257): 220, (3, 64): 53, (3, 65): 54,
             (8, 64): 41, (8, 65): 42}           # measured on the host (tests/test_reg_ref_host.py prints them)


@pytest.mark.parametrize("K,model,m", [(5, model, m) for model in (1, 2, 0) for m in COMPACT_M]
                         + [(K, 1, m) for K in (3, 8) for m in (1, 64, 65)])
def test_compact_list(e3d, rb, K, model, m):
    """The m observed points nearest to the centroid: the list ends inside a chunk (or fills it exactly), part of the lanes of a
    chunk have their flag cleared.  Model 1: one 16 x 16 tile; 2: the folded tile (V = 18); 0: per-thread accumulators."""
    S, levels, full = _scene(K, model)
    o = reg_lists.compact(S["pts"], full, m)
    of, (H, b, sums, counts, s2, c2) = _compare_scene(e3d, rb, K, model, o, 1, "K %d model %d m %d" % (K, model, m))
    if m == 1:
        assert not of.any() and not H.any() and not b.any() and not sums.any() and not counts.any() and not s2.any() and not c2.any()
    if (K, m) in FLAGS_SET:
        assert of.sum() == FLAGS_SET[(K, m)] == counts[0] and 0 < counts[1] < counts[0]
        assert not np.array_equal(o[0], np.arange(m))


@functools.lru_cache(maxsize=None)
def _rig(e3d, model):
    """Both sides of a two-frame rig problem with their observations; the tests only replace the list of image 1."""
    from reg_util import make_rig_scene
    G, O = base._build_rig_both(e3d, make_rig_scene(n_points=3000, seed=9, model=model))
    G.update_observations(1); O.update_observations(1)
    return G, O


@pytest.mark.parametrize("model", [1, 2])            # V = 20 and 24: the kernel with more than one 16 x 16 tile
@pytest.mark.parametrize("m", COMPACT_M)
def test_compact_list_of_a_dependent_rig_image(e3d, rb, model, m):
    G, O = _rig(e3d, model)
    S = O.scales[0]; im = O.images[1]; full = O.obs[(1, 0)]
    assert len(full[0]) >= 257
    o = reg_lists.compact(S["pts"], full, m)
    of, (H, b, sums, counts, s2, c2) = _compare(rb, G, 1, S["pts"], float(S["radius"]), S["nbr"], O.K, S["fixed"], S["var"], S["counts"],
                                                O.intr[0]["levels"][0], im["pyr"], O._R(im), im["t"], o, O.robust_type,
                                                "rig model %d m %d" % (model, m), rig=O._rig_link(1), rparam=O.robust_param)
    assert H.shape == (PARAM_COUNT[model] + 12,) * 2
    if m == 1:
        assert not of.any() and not H.any() and not counts.any()
    if m >= 63:
        assert 0 < of.sum() < m and counts[0] == of.sum()


@pytest.mark.parametrize("K,model", [(5, 1), (5, 2), (5, 0), (3, 1)])
def test_empty_list(e3d, rb, K, model):
    """An image that sees nothing: set_observations takes an empty list, one block runs whose loops do not, and accumulate and cost
    return zeros."""
    S, levels, full = _scene(K, model)
    P = _problem(e3d, rb, S)
    P.set_observations(0, 0, *[a[:0] for a in full])
    g = P.get_observations(0, 0, 0)
    assert all(len(a) == 0 for a in g)
    H, b, sums, counts = P.accumulate(0, 0)
    s2, c2 = P.cost(0, 0)
    assert H.shape == (PARAM_COUNT[model] + 6,) * 2
    for a in (H, b, sums, counts, s2, c2):
        assert not a.any()
    P.color_begin(0); P.color_accumulate(0, 0); P.color_finish(0)
    d, c = P.get_variable_descriptors(0, len(S["pts"]))
    assert not d.any() and not c.any()
    # and a list after the empty one works as usual
    o = reg_lists.compact(S["pts"], full, 65)
    P.set_observations(0, 0, *o)
    assert P.accumulate(0, 0)[3][0] == rb.neighbors_observed(len(S["pts"]), o[0], S["nbr"], K).sum() > 0


# ---- C6: whole steps at other neighbour counts ------------------------------------------------------------------------------------------
def _multi_image_scene_with_gaps(K, model):
    """make_multi_image_scene plus two points far outside every frustum and an image mask (kObs) on image 1."""
    from scipy.spatial import cKDTree
    from reg_util import make_multi_image_scene, texture
    M = make_multi_image_scene(n_points=6000, n_images=3, seed=5, model=model, K=K)
    pts = np.concatenate([M["pts"], np.array([[50, 3, 0], [0, -5, 0]], np.float32)])
    nbr = cKDTree(pts).query(pts, k=K + 1)[1][:, 1:].astype(np.uint32)
    tex = texture(pts[:, 0].astype(np.float64), pts[:, 2].astype(np.float64))
    M.update(pts=pts, nbr=nbr, fixed_desc=(tex[nbr] - tex[:, None]).astype(np.float32))
    mask = np.zeros((M["height"], M["width"]), np.uint8); mask[60:120, 80:170] = 1
    M["masks"] = {1: base._mask_pyramid(mask, M["n_levels"])}
    return M


def _build_both_with_masks(e3d, M):
    from oracle.reg_driver import OracleRegProblem
    prm = e3d.default_reg_params(image_scale_count=M["n_levels"], point_neighbor_count=M["K"])
    G = e3d.RegProblem(prm)
    O = OracleRegProblem(K=M["K"], image_scale_count=M["n_levels"])
    G.set_intrinsics(0, M["width"], M["height"], M["params"], 0, M["n_levels"], camera_type=M["model"])
    O.set_intrinsics(0, M["width"], M["height"], M["params"], 0, M["n_levels"], model=M["model"])
    for P in (G, O):
        P.set_point_scale(0, M["pts"], M["point_radius"], M["nbr"], M["fixed_desc"])
        P.set_splat_points(M["pts"])
        for i, im in enumerate(M["images"]):
            P.set_image(i, 0, im["pyr"], M["masks"].get(i))
            P.set_image_pose(i, im["q_init"], im["t_init"])
    return G, O


@pytest.mark.parametrize("model", [0, 2, 9])
@pytest.mark.parametrize("K", [3, 8])
def test_whole_problem_steps_match_oracle_at_other_neighbour_counts(e3d, K, model):
    """test_gpu_reg.test_whole_problem_steps_match_oracle with its assertions, at K = 3 and 8, on lists with gaps."""
    M = _multi_image_scene_with_gaps(K, model)
    G, O = _build_both_with_masks(e3d, M)
    G.update_observations(1); O.update_observations(1)
    for i in range(3):
        n = len(O.obs[(i, 0)][0])
        g = G.get_observations(i, 0, n)
        assert np.array_equal(g[0], O.obs[(i, 0)][0]) and np.array_equal(g[4], O.obs[(i, 0)][4])
        assert n < len(M["pts"]) and not np.isin([len(M["pts"]) - 2, len(M["pts"]) - 1], g[0]).any()
    f1 = O.obs[(1, 0)][4]
    assert 0.3 < f1.mean() < 1 and len(f1) < len(O.obs[(0, 0)][0]) - 200          # the masked image: fewer observations, cleared flags
    G.color_update(); O.color_update()
    d, c = G.get_variable_descriptors(0, len(M["pts"]))
    assert np.array_equal(c, O.scales[0]["counts"]) and np.abs(d - O.scales[0]["var"]).max() <= 2e-4
    assert (c == 0).any() and (c == 3).any() and ((c > 0) & (c < 3)).any()
    cg, co = G.compute_cost(), O.compute_cost()
    assert abs(cg - co) <= 1e-6 * co
    ag, lg, mg = G.apply(64.0); ao, lo, mo = O.apply(64.0)
    assert ag == ao and lg == lo and abs(mg - mo) <= 1e-3 * abs(mo) + 1e-6
    assert ao                                                                      # the oracle accepts the step
    for i in range(3):
        ang, tr = base._pose_delta(*G.get_image_pose(i), *O.get_image_pose(i))
        assert ang <= 1e-5 and tr <= 1e-5
    w, h, pg, _ = G.intrinsics_level(0, 0)
    po = O.intr[0]["params"]
    assert np.abs(pg[:4] - po[:4]).max() <= 1e-3 and np.abs(pg[4:] - po[4:]).max() <= 1e-5 if len(pg) > 4 else True


# ---- C7: parameter checks -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [0, 9])
def test_neighbour_count_out_of_range(e3d, K):
    with pytest.raises(e3d.E3DError, match="point_neighbor_count"):
        e3d.RegProblem(e3d.default_reg_params(point_neighbor_count=K))
    P = e3d.RegProblem(e3d.default_reg_params(point_neighbor_count=5))
    with pytest.raises(e3d.E3DError, match="point_neighbor_count"):
        P.set_params(e3d.default_reg_params(point_neighbor_count=K))


def test_neighbour_count_is_fixed_once_points_are_set(e3d, rb):
    S, levels, full = _scene(5, 0)
    P = e3d.RegProblem(e3d.default_reg_params(image_scale_count=S["n_levels"], point_neighbor_count=5))
    P.set_params(e3d.default_reg_params(image_scale_count=S["n_levels"], point_neighbor_count=3))      # nothing set yet: allowed
    P.set_params(e3d.default_reg_params(image_scale_count=S["n_levels"], point_neighbor_count=5))
    P.set_point_scale(0, S["pts"], S["point_radius"], S["nbr"], S["fixed_desc"])
    with pytest.raises(e3d.E3DError, match="cannot change"):
        P.set_params(e3d.default_reg_params(image_scale_count=S["n_levels"], point_neighbor_count=3))
    P.set_params(e3d.default_reg_params(image_scale_count=S["n_levels"], point_neighbor_count=5, robust_weighting_type=2))


@pytest.mark.parametrize("K", [1, 3, 8])
def test_determine_point_neighbors_at_other_counts(e3d, K):
    """What test_gpu_reg.test_determine_point_neighbors_shuffle_stream asserts for 5 of 25."""
    from scipy.spatial import cKDTree
    rng = np.random.RandomState(3)
    pts = rng.uniform(-1, 1, (4000, 3)).astype(np.float32)
    nb = e3d.determine_point_neighbors(pts, K, 25)
    assert nb.shape == (4000, K)
    _, nn = cKDTree(pts.astype(np.float64)).query(pts.astype(np.float64), k=26)
    for i in range(0, 4000, 7):
        assert i not in nb[i] and set(nb[i].tolist()) <= set(nn[i, 1:].tolist()) and len(set(nb[i].tolist())) == K
    assert np.array_equal(nb, e3d.determine_point_neighbors(pts, K, 25))
