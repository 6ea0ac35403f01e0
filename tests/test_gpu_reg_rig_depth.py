"""Depth residuals of the non-reference images of a camera rig (e3d_reg_set_rig_depth_residuals): the case the reference leaves
at LOG(FATAL) << "Not implemented yet" (intrinsics_and_pose_optimizer.cc:1199-1209) and whose test it keeps commented out
(FourFrame_DepthResidualVerification_Rig, test_alignment.cc:698-705).

The oracle has no rig variant of its depth rows and needs none: a dependent image's residual and intrinsics columns are those of
an ordinary image at the composed pose image_T_rig * rig_T_global, its extrinsics block is the ordinary pose block JP there, and
its rig-pose block follows from JP's translation columns (= a - jpi e_z): J_rig = JP[:, :3] R_image_rig [I | -[G]x], G =
rig_T_global * point.  The expected normal equations are accumulated from these rows in f64."""
import numpy as np
import pytest

import reg_ref
from reg_util import make_rig_scene, plane_depth_pyramid, quat_to_R

pytestmark = pytest.mark.gpu

DEPTH_WEIGHT = 0.7
# one camera model per local system size of a dependent image: I = 3, 4, 5, 7, 8, 12 -> V = I + 12 = 15, 16, 17, 19, 20, 24
SIZE_MODELS = [5, 0, 4, 8, 1, 2]


def _pose_delta(qa, ta, qb, tb):
    Ra, Rb = quat_to_R(qa).astype(np.float64), quat_to_R(qb).astype(np.float64)
    S = Ra.T @ Rb
    ang = 0.5 * np.linalg.norm([S[2, 1] - S[1, 2], S[0, 2] - S[2, 0], S[1, 0] - S[0, 1]])
    return ang, np.linalg.norm(np.asarray(ta, np.float64) - np.asarray(tb, np.float64))


def _wavy_depth_pyramid(M, im, hole):
    """The wall's true depth map times (1 + 8 % of a smooth wave): inverse-depth residuals up to ~0.027, on both sides of Tukey's
    0.02, and a depth gradient the projection terms see.  `hole`: a block of zeros, what a rendered depth map has where nothing was
    drawn (the depth == 0 quirk: a NaN Jacobian that only a zero robust weight keeps out of H).  Coarser levels: 2 x 2 means."""
    d = plane_depth_pyramid(M, im)[0].astype(np.float64)
    yy, xx = np.mgrid[0:M["height"], 0:M["width"]].astype(np.float64)
    d = d * (1.0 + 0.08 * np.sin(xx / 31.0) * np.cos(yy / 23.0))
    if hole:
        d[(yy > 0.3 * M["height"]) & (yy < 0.4 * M["height"]) & (xx > 0.55 * M["width"]) & (xx < 0.7 * M["width"])] = 0
    maps = [d]
    for _ in range(1, M["n_levels"]):
        p = maps[-1]
        maps.append(0.25 * (p[0::2, 0::2] + p[1::2, 0::2] + p[0::2, 1::2] + p[1::2, 1::2]))
    return [m.astype(np.float32) for m in maps]


def _rig_problem(e3d, M, depth_maps, switch=True, **params):
    prm = e3d.default_reg_params(image_scale_count=M["n_levels"], point_neighbor_count=M["K"], **params)
    G = e3d.RegProblem(prm)
    G.set_intrinsics(0, M["width"], M["height"], M["params"], 0, M["n_levels"], camera_type=M["model"])
    G.set_point_scale(0, M["pts"], M["point_radius"], M["nbr"], M["fixed_desc"])
    G.set_splat_points(M["pts"])
    for i, im in enumerate(M["images"]):
        G.set_image(i, 0, im["pyr"])
        if "q_init" in im:
            G.set_image_pose(i, im["q_init"], im["t_init"])
    G.set_rig(0, M["rig_init"])
    for ids in M["frames"]:
        G.add_rig_images(0, ids)
    for i in range(len(M["images"])):
        G.set_depth_maps(i, depth_maps[i])
    if switch:
        G.set_rig_depth_residuals(True)
    return G, prm


def _observations(G, image_id):
    """The stored observation list (index, x, y, scale) of point scale 0; the depth cost counts every observation."""
    _, n = G.depth_cost(image_id, 0)
    return G.get_observations(image_id, 0, n)[:4]


def _skew_block(ar, X):
    """ar^T [I | -[X]x] per observation: [n, 6]"""
    return np.concatenate([ar, np.cross(X, ar)], 1)


def _expected_rows(rb, G, M, image_id, ref_id, dm, obs, drop_jpi=False):
    """Residuals (f32, the oracle's) and the f64 row [J_intrinsics, J_extrinsics, J_rigpose] of a dependent image.
    drop_jpi: without the two terms the reference leaves open (d z / d extrinsics and d z / d rig pose)."""
    levels = rb.camera_pyramid(rb.make_camera(M["width"], M["height"], M["params"], M["model"]), M["n_levels"])
    q, t = G.get_image_pose(image_id)                                  # the composed pose image_T_rig * rig_T_global
    res, JI, JP = rb.depth_rows(M["pts"], M["point_radius"], levels[0], 0, dm, quat_to_R(q), t, q, obs)
    P = M["pts"][obs[0]].astype(np.float64)
    R_ir = quat_to_R(G.get_rig(0, 1)[0]).astype(np.float64)
    qr, tr = G.get_image_pose(ref_id)
    Gp = P @ quat_to_R(qr).astype(np.float64).T + tr.astype(np.float64)
    JP = JP.astype(np.float64)
    a = JP[:, :3].copy()                                               # a - jpi e_z
    if drop_jpi:
        T = P @ quat_to_R(q).astype(np.float64).T + t.astype(np.float64)
        a[:, 2] += -1.0 / (T[:, 2] * T[:, 2])                          # a alone
        JP = _skew_block(a, T)
    J = np.concatenate([JI.astype(np.float64), JP, _skew_block(a @ R_ir, Gp)], 1)
    return res, J, (JI, JP)


def _expected_system(res, J, rtype, rparam, weight):
    """AccumulateOnHAndB over the rows: a zero weight skips the row (whatever its Jacobian holds)."""
    w = reg_ref.robust_weight(rtype, rparam, res) * weight
    use = w != 0
    Ju, wu, ru = J[use], w[use], res[use].astype(np.float64)
    H = np.triu((Ju * wu[:, None]).T @ Ju)
    b = Ju.T @ (wu * ru)
    return H, b, float(reg_ref.robust_residual(rtype, rparam, res).sum()), len(res)


def _check_blocks(e3d, rb, model, rtype, rparam, hole, seed):
    M = make_rig_scene(n_points=4000, seed=seed, model=model)
    dms = [_wavy_depth_pyramid(M, im, hole) for im in M["images"]]
    G, _ = _rig_problem(e3d, M, dms, depth_residuals_weight=DEPTH_WEIGHT, depth_robust_weighting_type=rtype,
                        depth_robust_weighting_parameter=rparam)
    G.update_observations(1)
    I = rb.PARAM_COUNT[model]
    V = I + 12
    for image_id, ref_id in ((1, 0), (3, 2)):
        obs = _observations(G, image_id)
        H, b, sm, cn = G.depth_accumulate(image_id, 0)
        res, J, (JI, JP) = _expected_rows(rb, G, M, image_id, ref_id, dms[image_id], obs)
        He, be, se, ce = _expected_system(res, J, rtype, rparam, DEPTH_WEIGHT)
        # sum and count: against the oracle's own accumulation of the same residuals (f32 rho, f64 sum -- what the kernel does) ...
        Ho, bo, so, co = rb.depth_accumulate(res, JI, JP.astype(np.float32), rtype, rparam, DEPTH_WEIGHT)
        print("model", model, "image", image_id, "n", cn, "sum", sm, so, se)
        assert cn == co == ce == len(obs[0]) and cn > 500
        assert abs(sm - so) <= 1e-10 * abs(so)
        # ... and against rho in f64 (reg_ref): the f32 evaluation of rho is a few ulp per residual
        assert abs(sm - se) <= 1e-6 * abs(se)
        assert H.shape == (V, V) and np.array_equal(np.tril(H, -1), np.zeros_like(H))
        assert np.isfinite(H).all() and np.isfinite(He).all() and np.all(np.diag(He) > 0)
        scale = np.sqrt(np.outer(np.diag(He), np.diag(He)))
        sb = np.sqrt(np.diag(He))
        print("  H", (np.abs(H - He) / scale).max(), "b", (np.abs(b - be) / sb).max(), "of", np.abs(be / sb).max())
        assert (np.abs(H - He) / scale).max() <= 1e-5
        assert (np.abs(b - be) / sb).max() <= 1e-5 * np.abs(be / sb).max()
        # the [intrinsics, extrinsics] corner is the oracle's block of an ordinary image at the composed pose
        assert (np.abs(H[:I + 6, :I + 6] - Ho) / scale[:I + 6, :I + 6]).max() <= 1e-6
        # these inputs tell the two open terms of the reference apart: without them the tz / tz entries are off by more than 1 %
        _, Jn, _ = _expected_rows(rb, G, M, image_id, ref_id, dms[image_id], obs, drop_jpi=True)
        Hn = _expected_system(res, Jn, rtype, rparam, DEPTH_WEIGHT)[0]
        for k in (I + 2, I + 6 + 2):
            assert abs(Hn[k, k] - He[k, k]) > 0.01 * abs(He[k, k]), (k, Hn[k, k], He[k, k])
            assert abs(H[k, k] - He[k, k]) < abs(H[k, k] - Hn[k, k])
    return G, M, dms


@pytest.mark.parametrize("model", SIZE_MODELS)
def test_rig_depth_blocks_match_expected_rows(e3d, rb, model):
    """Tukey 0.02 on a depth map with a hole, one model per rig system size (every E3D_ROWS split of 15 ... 24 unknowns), and the
    cost pass on the same residuals."""
    G, M, dms = _check_blocks(e3d, rb, model, 2, 0.02, True, 31 + model)
    for image_id in (1, 3):
        obs = _observations(G, image_id)
        q, t = G.get_image_pose(image_id)
        s, c = G.depth_cost(image_id, 0)
        so, co = rb.depth_cost(M["pts"], 0, dms[image_id], q, t, obs, 2, 0.02)
        assert c == co and abs(s - so) <= 1e-12 * abs(so)
        assert abs(s - G.depth_accumulate(image_id, 0)[2]) <= 1e-10 * abs(s)       # the cost pass sees the accumulate pass's residuals


@pytest.mark.parametrize("model,rtype,rparam", [(0, 1, 0.01), (2, 0, 0.0)])
def test_rig_depth_blocks_huber_and_unweighted(e3d, rb, model, rtype, rparam):
    """Huber and no robust weighting: every row counts, so the depth map has no hole (a zero depth is a NaN row there)."""
    _check_blocks(e3d, rb, model, rtype, rparam, False, 41 + model)


def _cost_value(prm, sums, counts):
    """Problem::ComputeCost (problem.cc:602-631) from [fixed colour, variable colour, depth] sums and counts"""
    weights = (prm.fixed_residuals_weight, prm.variable_residuals_weight, prm.depth_residuals_weight)
    r = 0.0
    for w, s, c in zip(weights, sums, counts):
        if w > 0 and c > 0:
            r += w * s / c
    return r


def test_rig_depth_cost_is_part_of_compute_cost(e3d, rb):
    M = make_rig_scene(n_points=4000, seed=51)
    dms = [plane_depth_pyramid(M, im) for im in M["images"]]
    G, prm = _rig_problem(e3d, M, dms, depth_residuals_weight=DEPTH_WEIGHT)
    G.update_observations(1)
    sums = [0.0, 0.0, 0.0]; counts = [0, 0, 0]
    for i in range(4):
        s2, c2 = G.cost(i, 0)
        sd, cd = G.depth_cost(i, 0)
        q, t = G.get_image_pose(i)
        so, co = rb.depth_cost(M["pts"], 0, dms[i], q, t, _observations(G, i), 2, 0.02)
        assert cd == co and cd > 500 and abs(sd - so) <= 1e-12 * abs(so)
        sums[0] += s2[0]; sums[1] += s2[1]; sums[2] += sd
        counts[0] += int(c2[0]); counts[1] += int(c2[1]); counts[2] += cd
    want = _cost_value(prm, sums, counts)
    got = G.compute_cost()
    assert np.isfinite(want) and sums[2] > 0 and abs(got - want) <= 1e-12 * want
    assert want > _cost_value(prm, sums[:2] + [0.0], counts[:2] + [0])           # the depth term is in it


def test_rig_depth_residuals_in_the_optimizer(e3d):
    """Colour and depth residuals together on the perturbed rig scene: one Apply is accepted and lowers the cost; a whole
    RunOnCurrentScale moves the composed poses of all four images towards the truth."""
    M = make_rig_scene(n_points=6000, seed=52)
    dms = [plane_depth_pyramid(M, im) for im in M["images"]]
    G, _ = _rig_problem(e3d, M, dms, depth_residuals_weight=1.0)
    G.update_observations(1)
    c0 = G.compute_cost()
    applied, lam, change = G.apply(64.0)
    c1 = G.compute_cost()
    print("apply:", applied, lam, change, c0, c1)
    assert applied and np.isfinite(c0) and c1 < c0
    G, _ = _rig_problem(e3d, M, dms, depth_residuals_weight=1.0)
    start = [G.get_image_pose(i) for i in range(4)]
    converged, cost, its = G.run_on_current_scale(6, 0.0, 15, False)
    err0 = err1 = 0.0
    for i, im in enumerate(M["images"]):
        a0, t0 = _pose_delta(*start[i], im["q_true"], im["t_true"])
        a1, t1 = _pose_delta(*G.get_image_pose(i), im["q_true"], im["t_true"])
        err0 += a0 + t0; err1 += a1 + t1
    print("run:", converged, cost, its, "pose error", err0, "->", err1)
    assert np.isfinite(cost) and err1 < err0


def test_rig_depth_switch_semantics(e3d):
    M = make_rig_scene(n_points=3000, seed=53)
    dms = [plane_depth_pyramid(M, im) for im in M["images"]]
    G, prm = _rig_problem(e3d, M, dms, switch=False, depth_residuals_weight=1.0)
    G.update_observations(1)
    I = 4
    with pytest.raises(e3d.E3DError, match="rig"):                   # the default: the reference's behaviour
        G.compute_cost()
    with pytest.raises(e3d.E3DError, match="rig"):
        G.depth_accumulate(1, 0)
    H_off = G.depth_accumulate(0, 0)                                 # a reference image of a rig: an ordinary I + 6 block
    G.set_rig_depth_residuals(True)
    assert np.isfinite(G.compute_cost())
    G.set_params(prm)                                                # the switch belongs to the handle, not to the parameters
    assert np.isfinite(G.compute_cost())
    assert G.depth_accumulate(1, 0)[0].shape == (I + 12, I + 12)
    H_on = G.depth_accumulate(0, 0)
    assert H_on[0].shape == (I + 6, I + 6) and H_on[3] > 500
    assert np.array_equal(H_on[0], H_off[0]) and np.array_equal(H_on[1], H_off[1]) and H_on[2:] == H_off[2:]
    G.set_rig_depth_residuals(False)
    with pytest.raises(e3d.E3DError, match="rig"):
        G.compute_cost()
    with pytest.raises(e3d.E3DError, match="rig"):
        G.apply(64.0)


def _multi_res_scales(e3d, G, pts, colors, min_radius_bias=1.05, merge_distance_factor=4.0, need=26):
    """CreateMultiScalePointCloud (multi_scale_point_cloud.cc:264-369) over the C-ABI, for one scan: [(points, radius)]"""
    mn, mx = G.point_radius_minmax(pts)
    assert np.isfinite(mn.min())
    radius = float(np.float32(mn.min() * np.float32(min_radius_bias)))
    sidx = np.zeros(len(pts), np.uint8)
    sel = radius >= mn
    last = (pts[sel], colors[sel], sidx[sel], mx[sel])
    out = []
    last_radius = -1.0
    while True:
        if last_radius > 0:
            keep = radius <= last[3]
            new = (last_radius < mn) & (radius >= mn)
            last = tuple(np.concatenate([a[keep], b[new]]) for a, b in zip(last, (pts, colors, sidx, mx)))
        merged = e3d.merge_close_points(merge_distance_factor * radius, 1, *last) if len(last[0]) else last
        out.append((merged[0], radius))
        last_radius = float(np.float32(radius))
        radius *= 2
        if radius >= mx.max() * np.float32(0.99):
            break
        last = merged
    return [(p, r) for p, r in out if len(p) >= need]


def test_reference_four_frame_depth_residual_verification_rig(e3d):
    """FourFrame_DepthResidualVerification_Rig (commented out in the reference, test_alignment.cc:698-705, because :1199-1209
    aborts): the four-frame scene with the ground-truth depth maps as fixed depth maps, no colour residuals, and the two cameras
    as one rig -- image_T_rig[1] = T_init(0, 1) * T_init(0, 0)^-1, camera 0 the reference image of both frames (:418-461).  The
    thresholds are those of the whole family: every component of log(result * ground_truth^-1) <= 0.0016 and mean optical flow
    <= 0.07 px, over all four images on the composed poses."""
    from reg_util import make_four_frame_scene, pyramid_u8, se3_log
    S = make_four_frame_scene(seed=0)
    W, H, n_levels = S["width"], S["height"], 3                   # max_initial_image_area_in_pixels = 64 * 64 -> 256, 128, 64
    prm = e3d.default_reg_params(point_neighbor_count=5, robust_weighting_type=2, robust_weighting_parameter=5.0, fixed_residuals_weight=0.0,
                                 variable_residuals_weight=0.0, depth_residuals_weight=1.0, occlusion_depth_threshold=0.05,
                                 image_scale_count=n_levels, current_image_scale=n_levels - 2)
    G = e3d.RegProblem(prm)
    fx, fy, cx, cy = S["params"]
    G.set_intrinsics(0, W, H, S["params"], 0, n_levels)
    keys = [(0, 0), (0, 1), (1, 0), (1, 1)]
    for i, k in enumerate(keys):
        im = S["images"][k]
        gray = np.rint(im["color"].astype(np.float64) @ [0.299, 0.587, 0.114]).astype(np.uint8)
        G.set_image(i, 0, pyramid_u8(gray, n_levels))
        G.set_image_pose(i, [1, 0, 0, 0], im["t_init"])
        dm = [im["depth"]]
        for l in range(1, n_levels):                                                            # cv::resize(..., 0.5, 0.5, INTER_AREA) of CV_32F
            p = dm[-1].astype(np.float64)
            dm.append((0.25 * (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2])).astype(np.float32))
        G.set_depth_maps(i, dm)
    # the initial poses are pure translations: T_init(0, 1) * T_init(0, 0)^-1 is the difference of the two
    ident = (np.array([1, 0, 0, 0], np.float32), np.zeros(3, np.float32))
    t_rig = (np.asarray(S["images"][(0, 1)]["t_init"], np.float64) - np.asarray(S["images"][(0, 0)]["t_init"], np.float64)).astype(np.float32)
    G.set_rig(0, [ident, (ident[0], t_rig)])
    G.add_rig_images(0, [0, 1])
    G.add_rig_images(0, [2, 3])
    G.set_rig_depth_residuals(True)
    intensity = (S["rgb"].astype(np.float64) @ [0.299, 0.587, 0.114]).astype(np.float32)
    scales = _multi_res_scales(e3d, G, S["pts"], intensity)
    assert len(scales) >= 2
    for s, (p, r) in enumerate(scales):
        G.set_point_scale(s, p, r, e3d.determine_point_neighbors(p, 5, 25), np.zeros((len(p), 5), np.float32))
    G.set_splat_points(S["pts"])
    costs = []
    for scale in range(n_levels - 2, -1, -1):                                                   # Optimizer::NextScale
        prm.current_image_scale = scale
        G.set_params(prm)
        converged, cost, its = G.run_on_current_scale(500, 1e-20, 25, False)
        costs.append((scale, cost, its))
    worst = 0.0
    flow_sum = flow_count = 0
    w, h, pg, _ = G.intrinsics_level(0, 0)
    rfx, rfy, rcx, rcy = [float(v) for v in pg[:4]]
    for i, k in enumerate(keys):
        q, t = G.get_image_pose(i)
        im = S["images"][k]
        Tr = np.eye(4); Tr[:3, :3] = quat_to_R(q).astype(np.float64); Tr[:3, 3] = t
        Tg = np.eye(4); Tg[:3, :3] = im["R"]; Tg[:3, 3] = im["t"]
        worst = max(worst, np.abs(se3_log(Tr @ np.linalg.inv(Tg))).max())
        ys, xs = np.nonzero(im["depth"] > 0)
        dd = im["depth"][ys, xs].astype(np.float64)
        Q = Tr @ np.linalg.inv(Tg) @ np.stack([dd * (xs - cx) / fx, dd * (ys - cy) / fy, dd, np.ones_like(dd)], 0)
        ok = Q[2] > 0
        flow_sum += np.hypot(rfx * Q[0, ok] / Q[2, ok] + rcx - xs[ok], rfy * Q[1, ok] / Q[2, ok] + rcy - ys[ok]).sum(); flow_count += ok.sum()
    print("rig, depth only:", costs, "worst log component", worst, "mean flow px", flow_sum / flow_count)
    assert worst <= 0.0016 and flow_sum / flow_count <= 0.07, (worst, flow_sum / flow_count, costs)
