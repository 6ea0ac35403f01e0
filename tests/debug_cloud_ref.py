"""CPU restatement (numpy, f32 operation by operation) of Problem::DebugWriteColoredPointCloud (src/opt/problem.cc:642-704), the
expected values of the e3d_reg_scan_colors_* tests.  TEST INFRASTRUCTURE ONLY.

Per image, in ascending image id: observations without scale test (visibility_estimator.cc:117-138, :297-364), a bilinear sample
of the colour image per observation (interpolate_bilinear.h:117-146) at image_x/y_at_scale(min_image_scale)
(point_observation.h:84-93), f32 colour sums and int counts per point; then (uint8)(sum / count + 0.5f).

Scene description (as oracle.reg_driver.OracleRegProblem keeps it):
  intrinsics {id: dict(w, h, params, min, n, model, cam_masks=[per level] or None)}
  images     {id: dict(intr, pyr=[per level], masks=[per level] or None, q, t, color=(rows, cols, 3) uint8 R G B)}
"""
import numpy as np

F = np.float32

# why a point got no colour from an image (0 = it did)
COLOURED, BEHIND, OUTSIDE, OCCLUDED, IMAGE_MASK, CAMERA_MASK, SATURATED, SAMPLE_REJECTED = range(8)


def best_available_image_scale(min_image_scale, n_levels, current_image_scale, min_occlusion_check_image_scale=0):
    """Intrinsics::best_available_image_scale(max(min_occlusion_check_image_scale, current_image_scale))."""
    want = max(min_occlusion_check_image_scale, current_image_scale)
    return min(min_image_scale + n_levels - 1, max(min_image_scale, want))


def transform(R, t, pts):
    """image_R_global * p + image_T_global in f32: each row e0 + (e1 + e2), then + t (Eigen's 3-vector product order)."""
    R = np.asarray(R, F); t = np.asarray(t, F); p = np.asarray(pts, F)
    out = np.empty_like(p)
    for r in range(3):
        e0 = R[r, 0] * p[:, 0]; e1 = R[r, 1] * p[:, 1]; e2 = R[r, 2] * p[:, 2]
        out[:, r] = (e0 + (e1 + e2)) + t[r]
    return out


def _trunc_int(v):
    """static_cast<int>(float) where it is defined; None otherwise (every caller rejects such a point)."""
    v = float(v)
    if not np.isfinite(v) or v >= 2147483648.0 or v < -2147483648.0:
        return None
    return int(v)          # truncates toward zero


def observations_no_scale(pts, R, t, cam, image_scale, img, mask, cam_mask, occlusion, occlusion_threshold=0.01,
                          max_valid_intensity=252.0, project=None):
    """_AppendObservationsForImageNoScale for all points.  cam / img / mask / cam_mask / occlusion: of the level `image_scale`.
    -> (reason[n] (0 = observed, else BEHIND .. SATURATED), x[n], y[n], returned_scale): x / y at the smaller interpolation scale."""
    if project is None:
        from oracle import reg_binding as rb
        project = rb.cam_project
    pp = transform(R, t, pts)
    n = len(pp)
    reason = np.zeros(n, np.int32)
    ox = np.zeros(n, F); oy = np.zeros(n, F)
    returned_scale = F(image_scale) - F(1e-6)
    halve = returned_scale < F(0)
    if halve:
        returned_scale = F(0)
    thr = F(occlusion_threshold)
    for i in range(n):
        if not pp[i, 2] > F(0):
            reason[i] = BEHIND
            continue
        ixy = project(cam, pp[i])
        ax = F(ixy[0]) + F(0.5); ay = F(ixy[1]) + F(0.5)
        ix = _trunc_int(ax); iy = _trunc_int(ay)
        if not (ax >= 0 and ay >= 0 and ix is not None and iy is not None and 0 <= ix < cam.width and 0 <= iy < cam.height):
            reason[i] = OUTSIDE
            continue
        if not (F(occlusion[iy, ix]) + thr >= pp[i, 2]):
            reason[i] = OCCLUDED
            continue
        if mask is not None and mask[iy, ix] != 0:
            reason[i] = IMAGE_MASK
            continue
        if cam_mask is not None and cam_mask[iy, ix] != 0:
            reason[i] = CAMERA_MASK
            continue
        if F(img[iy, ix]) > F(max_valid_intensity):
            reason[i] = SATURATED
            continue
        x = F(ixy[0]); y = F(ixy[1])
        if halve:
            x = F(0.5) * (x + F(0.5)) - F(0.5)
            y = F(0.5) * (y + F(0.5)) - F(0.5)
        ox[i] = x; oy[i] = y
    return reason, ox, oy, returned_scale


def image_xy_at_scale(x, y, returned_scale, desired_image_scale):
    """PointObservation::image_x/y_at_scale: 2^(smaller_interpolation_scale - desired) * (x + 0.5f) - 0.5f (the factor is a power of
    two, so the f32 form equals the reference's double one)."""
    up = F(2.0 ** ((int(returned_scale) + 1) - desired_image_scale))
    return up * (np.asarray(x, F) + F(0.5)) - F(0.5), up * (np.asarray(y, F) + F(0.5)) - F(0.5)


def bilinear_vec3(color, x, y):
    """InterpolateBilinearVec3 on a (rows, cols, 3) uint8 image -> f32[3], or None where the reference returns false."""
    x = F(x); y = F(y)
    rows, cols = color.shape[:2]
    if x < F(0) or y < F(0):
        return None
    ix = _trunc_int(x); iy = _trunc_int(y)
    if ix is None or iy is None or ix >= cols - 1 or iy >= rows - 1:
        return None
    fx = x - F(ix); fx_inv = F(1) - fx
    fy = y - F(iy); fy_inv = F(1) - fy
    tl = color[iy, ix].astype(F); tr = color[iy, ix + 1].astype(F)
    bl = color[iy + 1, ix].astype(F); br = color[iy + 1, ix + 1].astype(F)
    # fx_inv * fy_inv * tl + fx * fy_inv * tr + fx_inv * fy * bl + fx * fy * br, left to right, no FMA
    return (((fx_inv * fy_inv) * tl + (fx * fy_inv) * tr) + (fx_inv * fy) * bl) + (fx * fy) * br


def add_image(sums, counts, pts, R, t, cam, image_scale, min_image_scale, img, mask, cam_mask, occlusion, color,
              occlusion_threshold=0.01, max_valid_intensity=252.0):
    """One image of problem.cc:655-682: sums (n, 3) f32 and counts (n,) int32 are updated in place.  -> reason[n]."""
    reason, ox, oy, rs = observations_no_scale(pts, R, t, cam, image_scale, img, mask, cam_mask, occlusion, occlusion_threshold,
                                               max_valid_intensity)
    x, y = image_xy_at_scale(ox, oy, rs, min_image_scale)
    for i in np.nonzero(reason == 0)[0]:
        c = bilinear_vec3(color, x[i], y[i])
        if c is None:
            reason[i] = SAMPLE_REJECTED
            continue
        sums[i] = sums[i] + c
        counts[i] += 1
    return reason


def finish(sums, counts):
    """(uint8)(sum / count + 0.5f), f32 divide then truncation; 0 0 0 where count == 0."""
    sums = np.asarray(sums, F); counts = np.asarray(counts, np.int32)
    out = np.zeros((len(counts), 3), np.uint8)
    seen = counts > 0
    v = sums[seen] / counts[seen].astype(F)[:, None] + F(0.5)
    assert v.dtype == F
    out[seen] = np.trunc(v).astype(np.uint8)
    return out


def add_rank_ordered(partials):
    """[(sums, counts) per rank] -> totals added in rank order: ((rank 0 + rank 1) + rank 2) ..., f32 sums and int counts."""
    sums = np.array(partials[0][0], F, copy=True); counts = np.array(partials[0][1], np.int32, copy=True)
    for s, c in partials[1:]:
        sums = sums + np.asarray(s, F)
        counts = counts + np.asarray(c, np.int32)
    return sums, counts


def colour_cloud(pts, intrinsics, images, splat_points, current_image_scale, splat_radius=0.03, occlusion_threshold=0.01,
                 max_valid_intensity=252.0, image_ids=None):
    """The whole pass over `image_ids` (default: all, ascending) -> (sums, counts, {image id: reason[n]}).  The occlusion depth of
    every image is the oracle's splat rendering of splat_points at the level the visibility test runs on."""
    from oracle import binding as ob
    from oracle import reg_binding as rb
    pts = np.ascontiguousarray(pts, F)
    sums = np.zeros((len(pts), 3), F); counts = np.zeros(len(pts), np.int32)
    reasons = {}
    for iid in (sorted(images) if image_ids is None else image_ids):
        im = images[iid]; I = intrinsics[im["intr"]]
        levels = rb.camera_pyramid(rb.make_camera(I["w"], I["h"], I["params"], I.get("model", 0)), I["n"])
        scale = best_available_image_scale(I["min"], I["n"], current_image_scale)
        lvl = scale - I["min"]
        cam = levels[lvl]
        R = ob.quat_to_R(np.asarray(im["q"], F))
        occ = rb.splat_depth(splat_points, R, im["t"], cam, splat_radius)
        mask = im["masks"][lvl] if im.get("masks") is not None else None
        cam_mask = I["cam_masks"][lvl] if I.get("cam_masks") is not None else None
        reasons[iid] = add_image(sums, counts, pts, R, im["t"], cam, scale, I["min"], im["pyr"][lvl], mask, cam_mask, occ, im["color"],
                                 occlusion_threshold, max_valid_intensity)
    return sums, counts, reasons


def colour_cloud_sharded(pts, intrinsics, images, splat_points, current_image_scale, world, **kw):
    """Image id mod world == rank owns the image; partial sums per rank, added in rank order -> (sums, counts, partials)."""
    partials = []
    for rank in range(world):
        ids = [i for i in sorted(images) if i % world == rank]
        s, c, _ = colour_cloud(pts, intrinsics, images, splat_points, current_image_scale, image_ids=ids, **kw)
        partials.append((s, c))
    s, c = add_rank_ordered(partials)
    return s, c, partials
