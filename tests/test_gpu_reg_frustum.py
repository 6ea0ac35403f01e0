"""The registration kernels on a cloud that fills more than the frustum (reg_util.make_frustum_scene): points behind the camera, outside
the image, at its borders, beyond the cut-off radius, under masks and over-saturated pixels; observation scales on every level pair;
cameras whose pyramid starts at min_image_scale > 0; odd image sizes at every halving.  test_scene_takes_every_branch states, from
the CPU oracle's output alone, that the scene does reach these branches (it needs no GPU); the other tests compare the HIP kernels
with the oracle under the assertions and tolerances of test_gpu_reg.py."""
import functools

import numpy as np
import pytest

from reg_util import camera_space, cutoff_straddlers, frustum_mask_pyramid, make_frustum_scene, pad_to_levels, straddle_spots

MODELS = list(range(13))
IMAGE_SCALE_COUNT = 4
CONFIGS = {"A": (323, 243, 4, 0), "B": (163, 121, 3, 1), "C": (83, 61, 2, 2)}      # width, height, levels, min_image_scale
# Cloud sizes and occluder strides.  200 observations at EACH border of a 42 x 31 level take far more than the 40 000 points that
# give 1 000 per level pair (a 1.5 px band is 5 % of such a level and the kept points spread over all of it): sizes chosen so that
# the oracle keeps >= 200 there for every model, with about the same number of occluding splats (300, 160, 80) per configuration.
CLOUD = {"A": (120000, 384), "B": (160000, 1024), "C": (240000, 3072)}
ACC_CASES = [(0, 1, 47.434166), (0, 2, 30.0), (0, 0, 0.0), (1, 1, 47.434166), (2, 1, 47.434166), (2, 2, 30.0), (3, 1, 47.434166)]


@functools.lru_cache(maxsize=None)
def _scene(cfg, model, K=5):
    w, h, n_levels, min_scale = CONFIGS[cfg]
    S = make_frustum_scene(model, w, h, n_levels, min_scale, IMAGE_SCALE_COUNT, n_points=CLOUD[cfg][0], K=K, splat_stride=CLOUD[cfg][1])
    imask = np.zeros((h, w), np.uint8); imask[h // 3:h // 2, w - w // 6:] = 1                 # MaskType::kObs, touching the right border
    cmask = np.zeros((h, w), np.uint8); cmask[h - h // 6:, w // 4:w // 2] = 2                 # MaskType::kEvalObs, touching the bottom border
    S["image_masks"] = frustum_mask_pyramid(S, imask)
    S["camera_masks"] = frustum_mask_pyramid(S, cmask)
    S["union_masks"] = [a | b for a, b in zip(S["image_masks"], S["camera_masks"])]
    for v in S.values():
        for a in (v if isinstance(v, list) else [v]):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)                                                       # shared between tests: read-only
    return S


def _levels(rb, S):
    return rb.camera_pyramid(rb.make_camera(S["width"], S["height"], S["params"], S["model"]), S["n_levels"])


@functools.lru_cache(maxsize=None)
def _oracle_observe(cfg, model, image_scale_offset=0, border=1, masked=False, splat=True, max_valid=252.0, current=0, K=5):
    """(idx, x, y, scale, neighbour flags) of the oracle for one setting of the switches; image scale = min_image_scale + offset"""
    from oracle import reg_binding as rb
    S = _scene(cfg, model, K)
    levels = _levels(rb, S)
    image_scale = S["min_image_scale"] + image_scale_offset
    cam = levels[image_scale_offset]
    depth = rb.splat_depth(S["splat_pts"], S["R"], S["t"], cam, 0.03) if splat else np.full((cam.height, cam.width), np.inf, np.float32)
    o = rb.observe(S["pts"], S["point_radius"], S["R"], S["t"], levels, S["min_image_scale"], S["pyr"], S["union_masks"] if masked else None,
                   depth, image_scale, border, current, IMAGE_SCALE_COUNT, max_valid_intensity=max_valid)
    o = o + (rb.neighbors_observed(len(S["pts"]), o[0], S["nbr"], S["K"]),)
    for a in o:
        a.setflags(write=False)
    return o


def _border_counts(S, levels, o):
    """observations within 1.5 px of the left / top / right / bottom border (the outermost pixel centres) of their own level"""
    li = o[3].astype(np.int32) + 1 - S["min_image_scale"]
    w = np.array([levels[l].width for l in range(S["n_levels"])])[li]; h = np.array([levels[l].height for l in range(S["n_levels"])])[li]
    return [int((o[1] < 1.5).sum()), int((o[2] < 1.5).sum()), int((w - 1 - o[1] < 1.5).sum()), int((h - 1 - o[2] < 1.5).sum())]


def _has_cutoff(cam):
    return bool(np.isfinite(cam.cutoff2) or np.isfinite(cam.inner_cutoff2))


@pytest.mark.parametrize("model", MODELS)
def test_scene_takes_every_branch(rb, model):
    """Coverage of the scene, from the oracle's output only (no GPU)."""
    report = []
    for cfg in CONFIGS:
        S = _scene(cfg, model); levels = _levels(rb, S)
        base = _oracle_observe(cfg, model)
        floors = base[3].astype(np.int32)
        per_floor = {f: int((floors == f).sum()) for f in range(S["min_image_scale"], IMAGE_SCALE_COUNT - 1)}
        borders = _border_counts(S, levels, base)
        report.append((cfg, len(base[0]), per_floor, borders))
        assert set(np.unique(floors)) == set(per_floor) and min(per_floor.values()) >= 1000, (cfg, per_floor)
        assert min(borders) >= 200, (cfg, borders)
        assert base[4].sum() > 1000                                               # points whose neighbours are all observed
        # every rejection decides something: the kept count strictly drops when one switch changes
        n = len(base[0])
        assert n < len(_oracle_observe(cfg, model, splat=False)[0])               # occlusion by the splats
        assert len(_oracle_observe(cfg, model, masked=True)[0]) < n               # image mask / camera mask
        assert n < len(_oracle_observe(cfg, model, max_valid=255.0)[0])           # over-saturated pixels
        assert len(_oracle_observe(cfg, model, current=S["min_image_scale"] + 1)[0]) < n      # scale below the current image scale
        assert len(_oracle_observe(cfg, model, border=3)[0]) < n                  # border
        c = camera_space(S)
        assert (c[:, 2] < 0).sum() >= len(c) // 25 and (np.abs(c[:, 2]) < 1e-5).sum() >= 50       # behind / in the camera plane
        # above the coarsest level pair and below the finest: both scale rejections fire (pinhole estimate, factor 2 of margin)
        rp = 2 * S["point_radius"] * float(levels[0].p[0]) / np.maximum(c[:, 2], 1e-9)
        assert ((c[:, 2] > 0) & (rp > 2.0 * 2.0 ** (IMAGE_SCALE_COUNT - 1 - S["min_image_scale"]))).sum() > 100
        assert ((c[:, 2] > 0) & (rp < 0.5)).sum() > 100
        if _has_cutoff(levels[0]):
            st = cutoff_straddlers(S, levels[0], c)
            inside = 0
            for i in np.nonzero(st)[0]:
                ip = rb.cam_project(levels[0], c[i])
                inside += bool(np.isfinite(ip).all() and 1 <= ip[0] <= S["width"] - 2 and 1 <= ip[1] <= S["height"] - 2)
            report[-1] += (int(st.sum()), inside)
            if straddle_spots(rb, levels[0], S["point_radius"]):
                assert inside >= 5, (cfg, int(st.sum()), inside)
            else:
                # no point of such a cloud can straddle the cut-off and project into this image, whatever its seed (straddle_spots):
                # SIMPLE_RADIAL's cut-off circle (r = 1.82) projects far outside the image, SimpleRadialFisheye's inner cut-off
                # (theta^2 = 15.1) lies beyond atan's range; at 83 x 61 "1 px inside" is also more than some corners leave
                assert inside == 0 and (model in (6, 12) or cfg != "A"), (cfg, inside)
    # splats (configuration A): full-size ones (both half-extents at the 10 px clamp), small ones, centres outside the image
    S = _scene("A", model); levels = _levels(rb, S); c = camera_space(S)
    full = small = 0
    for i in range(0, len(c), 64):
        if c[i, 2] > 0:
            d = rb.cam_deriv_by_world(levels[0], c[i])
            r = np.sqrt((d.astype(np.float64) ** 2).sum(1)) * 0.03
            full += bool(r.min() >= 10.5); small += bool(0.5 < r.max() <= 9.5)
    assert full >= 20 and small >= 100, (full, small)
    print("\nfrustum scene, model %d: " % model + "; ".join(
        "%s kept %d per floor %s borders l/t/r/b %s%s" % (r[0], r[1], r[2], r[3], (" straddlers %d (in image %d)" % r[4:6]) if len(r) > 4 else "")
        for r in report))


# ---- the HIP kernels against the oracle ---------------------------------------------------------------------------------------------
def _setup(e3d, rb, S, masks=False, **pk):
    prm = e3d.default_reg_params(image_scale_count=IMAGE_SCALE_COUNT, point_neighbor_count=S["K"], **pk)
    P = e3d.RegProblem(prm)
    P.set_intrinsics(0, S["width"], S["height"], S["params"], S["min_image_scale"], S["n_levels"], camera_type=S["model"])
    P.set_image(0, 0, S["pyr"], S["image_masks"] if masks else None)
    if masks:
        P.set_camera_mask(0, S["camera_masks"])
    P.set_image_pose(0, S["q"], S["t"])
    P.set_point_scale(0, S["pts"], S["point_radius"], S["nbr"], S["fixed_desc"])
    P.set_variable_descriptors(0, S["var_desc"], S["obs_counts"])
    P.set_splat_points(S["splat_pts"])
    return P, _levels(rb, S)


def _same_observations(g, o):
    """the assertions of test_gpu_reg.py::test_observations_match_oracle"""
    assert len(g[0]) == len(o[0])
    assert np.array_equal(g[0], o[0])                                        # same points, same (point) order
    assert np.array_equal(g[1].view(np.uint32), o[1].view(np.uint32)) and np.array_equal(g[2].view(np.uint32), o[2].view(np.uint32))
    assert np.array_equal(g[3].view(np.uint32), o[3].view(np.uint32))       # observation scale (log2f) too
    assert np.array_equal(g[4], o[4])


@pytest.mark.gpu
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_observations_match_oracle(e3d, rb, cfg, model):
    """All-points pass after render_depth at image scale min_image_scale and min_image_scale + 1, borders 1 and 3, with an image
    mask and a camera mask (bit-equal, as test_gpu_reg.py::test_observations_match_oracle), then the indexed pass."""
    S = _scene(cfg, model)
    P, levels = _setup(e3d, rb, S, masks=True)
    for off in (0, 1):
        image_scale = S["min_image_scale"] + off
        P.render_depth(0, image_scale)
        for border in (1, 3):
            o = _oracle_observe(cfg, model, off, border, masked=True)
            n = P.observe(0, 0, image_scale, border)
            assert n == len(o[0]) and (n > 1000 or off == 1)
            _same_observations(P.get_observations(0, 0, n), o)
    # indexed variant (fixed visibility list, no occlusion / mask tests): every third kept index plus 100 indices the indexed pass
    # rejects (behind the camera, outside the image, out of the scale range, straddling the cut-off: the last points of the cloud)
    kept = _oracle_observe(cfg, model)[0]
    n_pts = len(S["pts"])
    all_idx = rb.observe(S["pts"], S["point_radius"], S["R"], S["t"], levels, S["min_image_scale"], S["pyr"], None, None, S["min_image_scale"], 1,
                         0, IMAGE_SCALE_COUNT, indices=np.arange(n_pts, dtype=np.uint32))[0]
    rejected = np.setdiff1d(np.arange(n_pts, dtype=np.uint32), all_idx)
    rejected = np.concatenate([rejected[:len(rejected) - 40:max(1, (len(rejected) - 40) // 60)][:60], rejected[-40:]])
    assert len(rejected) == 100
    indices = np.sort(np.concatenate([kept[::3], rejected])).astype(np.uint32)
    o2 = rb.observe(S["pts"], S["point_radius"], S["R"], S["t"], levels, S["min_image_scale"], S["pyr"], None, None, S["min_image_scale"], 1, 0,
                    IMAGE_SCALE_COUNT, indices=indices)
    assert len(o2[0]) == len(indices) - 100 and np.array_equal(o2[0], kept[::3])      # all 100 drop out: the compaction path runs
    n2 = P.observe(0, 0, S["min_image_scale"], 1, indices=indices)
    assert n2 == len(o2[0])
    _same_observations(P.get_observations(0, 0, n2), o2 + (rb.neighbors_observed(n_pts, o2[0], S["nbr"], S["K"]),))


@pytest.mark.gpu
@pytest.mark.parametrize("model", MODELS)
def test_splat_depth_bit_exact_at_every_level(e3d, rb, model):
    """render_depth against the oracle at each level of configuration A (full-size and small splats, centres outside the image,
    points behind the camera; no level is a multiple of the 32-pixel tiles)"""
    S = _scene("A", model)
    P, levels = _setup(e3d, rb, S)
    for dense in (False, True):                        # the sparse occluders of the other tests (holes stay +inf), then the whole cloud
        if dense:
            P.set_splat_points(S["pts"])
        for l in range(S["n_levels"]):
            g = P.render_depth(0, l, (levels[l].height, levels[l].width))
            o = rb.splat_depth(S["pts" if dense else "splat_pts"], S["R"], S["t"], levels[l], 0.03)
            assert np.isfinite(o).all() if dense else (np.isfinite(o).sum() > 0.1 * o.size and np.isinf(o).sum() > 0.1 * o.size)
            assert np.array_equal(g.view(np.uint32), o.view(np.uint32)), (dense, l)


@pytest.mark.gpu
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_pass1_rows_per_level_pair(e3d, rb, cfg, model):
    """Intensities bit-equal; Jacobian columns within 1e-5 * max|column| (test_gpu_reg.py::test_pass1_rows), applied to the rows of each
    level pair (floor of the observation scale) on their own.  (Measured on gfx950: every column of every pair and model equals the
    oracle's bit for bit -- the bound is not approached by a pair with small entries either.)"""
    S = _scene(cfg, model)
    P, levels = _setup(e3d, rb, S)
    o = _oracle_observe(cfg, model)
    P.set_observations(0, 0, *o[:4])                    # identical inputs (incl. scale) for both sides
    I, ji, jp = P.pass1(0, 0, len(o[0]))
    Io, jio, jpo = rb.pass1(S["pts"], S["point_radius"], levels[0], S["min_image_scale"], S["pyr"], S["R"], S["t"], o[:4])
    assert np.array_equal(I.view(np.uint32), Io.view(np.uint32))
    assert ji.shape == jio.shape == (len(o[0]), rb.PARAM_COUNT[model])
    assert np.isfinite(jio).all() and np.isfinite(jpo).all()
    floors = o[3].astype(np.int32)
    tol = 1e-5
    for f in range(S["min_image_scale"], IMAGE_SCALE_COUNT - 1):
        sel = floors == f
        assert sel.sum() >= 1000
        ratios = [np.abs(ji[sel, c] - jio[sel, c]).max() / (np.abs(jio[sel, c]).max() + 1e-30) for c in range(ji.shape[1])]
        pose_ratio = np.abs(jp[sel] - jpo[sel]).max() / np.abs(jpo[sel]).max()
        print("pass1 %s model %d pair (%d, %d): worst intrinsics column %.3g, pose %.3g (of max|column|)" % (cfg, model, f, f + 1, max(ratios), pose_ratio))
        for c in range(ji.shape[1]):                   # per parameter column (their magnitudes differ by orders)
            assert np.abs(ji[sel, c] - jio[sel, c]).max() <= tol * np.abs(jio[sel, c]).max() + 1e-30, (f, c)
        assert np.abs(jp[sel] - jpo[sel]).max() <= tol * np.abs(jpo[sel]).max(), f


def _accumulate_and_cost(e3d, rb, cfg, model, rtype, rparam, K):
    """the assertions of test_gpu_reg.py::test_accumulate_and_cost"""
    S = _scene(cfg, model, K)
    P, levels = _setup(e3d, rb, S, robust_weighting_type=rtype, robust_weighting_parameter=rparam)
    o = _oracle_observe(cfg, model, K=K); of = o[4]; o = o[:4]
    P.set_observations(0, 0, *o)
    H, b, sums, counts = P.accumulate(0, 0)
    Ho, bo, so, co = rb.accumulate(S["pts"], S["point_radius"], S["nbr"], S["K"], S["fixed_desc"], S["var_desc"], S["obs_counts"], levels[0],
                                   S["min_image_scale"], S["pyr"], S["R"], S["t"], o, of, rtype, rparam, 1.0, 1.0)
    assert np.array_equal(counts, co) and counts[0] > 1000 and counts[1] > 100
    assert np.abs(sums - so).max() <= 1e-9 * np.abs(so).max()
    V = rb.PARAM_COUNT[model] + 6
    assert H.shape == Ho.shape == (V, V)
    assert np.array_equal(np.tril(H, -1), np.zeros_like(H))                 # upper triangle only, like the reference's H
    scale = np.sqrt(np.outer(np.diag(Ho), np.diag(Ho)))                     # entries span many orders of magnitude
    tol = 1e-6
    print("accumulate %s model %d K %d: H %.3g b %.3g" % (cfg, model, K, (np.abs(H - Ho) / scale).max(),
                                                         (np.abs(b - bo) / np.sqrt(np.diag(Ho))).max() / np.abs(bo / np.sqrt(np.diag(Ho))).max()))
    assert (np.abs(H - Ho) / scale).max() <= tol
    assert (np.abs(b - bo) / np.sqrt(np.diag(Ho))).max() <= tol * np.abs(bo / np.sqrt(np.diag(Ho))).max() * 10
    s2, c2 = P.cost(0, 0)
    so2, co2 = rb.cost(len(S["pts"]), S["nbr"], S["K"], S["fixed_desc"], S["var_desc"], S["obs_counts"], S["min_image_scale"], S["pyr"], o, of,
                       rtype, rparam, 1.0, 1.0)
    assert np.array_equal(c2, co2) and np.abs(s2 - so2).max() <= 1e-12 * np.abs(so2).max()
    assert np.abs(s2 - sums).max() <= 1e-9 * np.abs(sums).max()   # cost pass == residual sums of the accumulate pass


@pytest.mark.gpu
@pytest.mark.parametrize("model,rtype,rparam", ACC_CASES)
def test_accumulate_and_cost_min_image_scale_1(e3d, rb, model, rtype, rparam):
    _accumulate_and_cost(e3d, rb, "B", model, rtype, rparam, 5)


@pytest.mark.gpu
@pytest.mark.parametrize("model", MODELS)
def test_accumulate_and_cost_three_neighbours(e3d, rb, model):
    _accumulate_and_cost(e3d, rb, "A", model, 1, 47.434166, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("model", [0, 2])
def test_depth_residual_blocks_min_image_scale_1(e3d, rb, model):
    """depth_accumulate / depth_cost on configuration B with the helper and the bounds of
    test_gpu_reg.py::test_depth_residual_blocks_match_oracle (Tukey weights, maps with a hole of zeros)"""
    from test_gpu_reg import _synthetic_depth_pyramid
    rtype, rparam = 2, 0.02
    S = _scene("B", model)
    P, levels = _setup(e3d, rb, S, depth_residuals_weight=0.7, depth_robust_weighting_type=rtype, depth_robust_weighting_parameter=rparam)
    o = _oracle_observe("B", model)[:4]
    P.set_observations(0, 0, *o)
    dm = pad_to_levels(_synthetic_depth_pyramid(S["width"], S["height"], S["n_levels"]), levels)
    P.set_depth_maps(0, dm)
    H, b, sm, cn = P.depth_accumulate(0, 0)
    res, JI, JP = rb.depth_rows(S["pts"], S["point_radius"], levels[0], S["min_image_scale"], dm, S["R"], S["t"], S["q"], o)
    Ho, bo, so, co = rb.depth_accumulate(res, JI, JP, rtype, rparam, 0.7)
    assert cn == co == len(o[0]) and cn > 1000
    assert abs(sm - so) <= 1e-10 * abs(so)
    V = rb.PARAM_COUNT[model] + 6
    assert H.shape == Ho.shape == (V, V) and np.array_equal(np.tril(H, -1), np.zeros_like(H))
    scale = np.sqrt(np.outer(np.diag(Ho), np.diag(Ho)))
    assert np.all(np.diag(Ho) > 0)
    assert (np.abs(H - Ho) / scale).max() <= 1e-6
    assert (np.abs(b - bo) / np.sqrt(np.diag(Ho))).max() <= 1e-5 * np.abs(bo / np.sqrt(np.diag(Ho))).max()
    s2, c2 = P.depth_cost(0, 0)
    so2, co2 = rb.depth_cost(S["pts"], S["min_image_scale"], dm, S["q"], S["t"], o, rtype, rparam)
    assert c2 == co2 == cn and abs(s2 - so2) <= 1e-12 * abs(so2)
    assert abs(s2 - sm) <= 1e-10 * abs(sm)           # the cost pass sees the residuals of the accumulate pass


@pytest.mark.gpu
@pytest.mark.parametrize("model", [0, 2])
def test_whole_problem_with_two_camera_resolutions(e3d, rb, model):
    """Two cameras in one problem, 323 x 243 (min_image_scale 0, 4 levels) and 163 x 121 (min_image_scale 1, 3 levels), two images
    each: observations, colour update, cost and one LM step under the bounds of test_gpu_reg.py::test_whole_problem_steps_match_oracle."""
    from oracle.reg_driver import OracleRegProblem
    from reg_util import make_multi_image_scene
    from test_gpu_reg import _pose_delta
    cams = [make_multi_image_scene(n_points=6000, n_images=4, width=w, height=h, n_levels=n, seed=5, model=model)
            for (w, h, n, _) in (CONFIGS["A"], CONFIGS["B"])]
    M = cams[0]
    G = e3d.RegProblem(e3d.default_reg_params(image_scale_count=IMAGE_SCALE_COUNT, point_neighbor_count=M["K"]))
    O = OracleRegProblem(K=M["K"], image_scale_count=IMAGE_SCALE_COUNT)
    for iid, (C, cfg) in enumerate(zip(cams, ("A", "B"))):
        assert np.array_equal(C["pts"], M["pts"])
        G.set_intrinsics(iid, C["width"], C["height"], C["params"], CONFIGS[cfg][3], C["n_levels"], camera_type=model)
        O.set_intrinsics(iid, C["width"], C["height"], C["params"], CONFIGS[cfg][3], C["n_levels"], model=model)
    for P in (G, O):
        P.set_point_scale(0, M["pts"], M["point_radius"], M["nbr"], M["fixed_desc"])
        P.set_splat_points(M["pts"])
        for i in range(4):
            im = cams[i // 2]["images"][i]
            P.set_image(i, i // 2, pad_to_levels(im["pyr"], O.intr[i // 2]["levels"]))
            P.set_image_pose(i, im["q_init"], im["t_init"])
    G.update_observations(1); O.update_observations(1)
    for i in range(4):
        n = len(O.obs[(i, 0)][0])
        g = G.get_observations(i, 0, n)
        assert n > 1000 and np.array_equal(g[0], O.obs[(i, 0)][0]) and np.array_equal(g[4], O.obs[(i, 0)][4])
        assert np.all(O.obs[(i, 0)][3].astype(np.int32) == i // 2)           # the small camera's observations sit on level pair (1, 2)
    G.color_update(); O.color_update()
    d, c = G.get_variable_descriptors(0, len(M["pts"]))
    assert np.array_equal(c, O.scales[0]["counts"]) and np.abs(d - O.scales[0]["var"]).max() <= 2e-4
    cg, co = G.compute_cost(), O.compute_cost()
    assert abs(cg - co) <= 1e-6 * co
    ag, lg, mg = G.apply(64.0); ao, lo, mo = O.apply(64.0)
    assert ag == ao and lg == lo and abs(mg - mo) <= 1e-3 * abs(mo) + 1e-6
    for i in range(4):
        ang, tr = _pose_delta(*G.get_image_pose(i), *O.get_image_pose(i))
        assert ang <= 1e-5 and tr <= 1e-5
    for iid in range(2):
        w, h, pg, _ = G.intrinsics_level(iid, 0)
        po = O.intr[iid]["params"]
        assert np.abs(pg[:4] - po[:4]).max() <= 1e-3 and (len(pg) == 4 or np.abs(pg[4:] - po[4:]).max() <= 1e-5)
