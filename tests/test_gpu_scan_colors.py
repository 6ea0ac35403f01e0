"""e3d_reg_scan_colors_* (Problem::DebugWriteColoredPointCloud on the GPU) through capi.RegProblem against the CPU restatement in
tests/debug_cloud_ref.py: colour sums, observation counts and final colours bit for bit, at current_image_scale 0 (positions halved
to scale 1 and scaled back) and 1 (level-1 masks, grey values and occlusion depth)."""
import numpy as np
import pytest

import debug_cloud_ref as ref
from reg_util import camera_params, look_at_pose, pyramid_u8, quat_from_R

pytestmark = pytest.mark.gpu

N_LEVELS = 3
SPLAT_RADIUS = 0.03


def _mask_pyramid(m):
    """Image::BuildMaskPyramid: a coarser pixel carries the OR of its four."""
    lv = [m]
    for _ in range(1, N_LEVELS):
        a = lv[-1]; h, w = (a.shape[0] // 2) * 2, (a.shape[1] // 2) * 2
        lv.append(a[0:h:2, 0:w:2] | a[0:h:2, 1:w:2] | a[1:h:2, 0:w:2] | a[1:h:2, 1:w:2])
    return lv


def _fit(a, w, h):
    """Edge-pad a pyramid level to the camera level's size (the camera pyramid rounds odd sizes up, the image pyramid truncates)."""
    if a.shape == (h, w):
        return np.ascontiguousarray(a)
    return np.ascontiguousarray(a[np.minimum(np.arange(h), a.shape[0] - 1)][:, np.minimum(np.arange(w), a.shape[1] - 1)])


def _back_project(R, t, fx, fy, cx, cy, px, py, depth):
    """The global point a pinhole camera (R, t = image_T_global) sees at pixel (px, py) and camera depth `depth`."""
    d = np.array([(px - cx) / fx * depth, (py - cy) / fy * depth, depth], np.float64)
    return R.astype(np.float64).T @ (d - t.astype(np.float64))


def _build_scene():
    rng = np.random.RandomState(42)
    intrinsics = {
        0: dict(w=40, h=30, params=camera_params(0, 30.0, 29.5, 19.6, 15.3), min=0, n=N_LEVELS, model=0, cam_masks=None),
        1: dict(w=64, h=48, params=camera_params(2, 46.0, 45.5, 31.6, 24.3), min=0, n=N_LEVELS, model=2, cam_masks=None),   # THIN_PRISM_FISHEYE
    }
    cmask = np.zeros((48, 64), np.uint8); cmask[:, :9] = 2; cmask[40:, 50:] = 1
    intrinsics[1]["cam_masks"] = _mask_pyramid(cmask)
    eyes = [(-0.3, -0.2, 0.1), (0.25, -0.1, -0.05), (0.0, -0.4, 0.15)]
    images = {}
    for i, eye in enumerate(eyes):
        I = intrinsics[0 if i == 0 else 1]
        R0, t0 = look_at_pose(eye, (0.05 * i, 3.0, 0.02 * i))
        grey = rng.randint(0, 251, (I["h"], I["w"])).astype(np.uint8)
        masks = None
        if i == 1:                                             # an image mask with both flag values (kObs = 1, kEvalObs = 2)
            m = np.zeros((I["h"], I["w"]), np.uint8); m[36:, :] = 1; m[4:14, 44:58] = 2
            masks = _mask_pyramid(m)
        if i == 2:                                             # an over-saturated patch
            grey[16:30, 20:36] = 255
        images[i] = dict(intr=0 if i == 0 else 1, pyr=pyramid_u8(grey, N_LEVELS), masks=masks, q=quat_from_R(R0), t=t0.astype(np.float32),
                         color=rng.randint(0, 256, (I["h"], I["w"], 3)).astype(np.uint8))
    # a wall, a second wall behind it (occluded), points all around the cameras (behind them, outside the images)
    front = np.stack([rng.uniform(-1.5, 1.5, 2000), np.full(2000, 3.0), rng.uniform(-1.1, 1.1, 2000)], 1)
    back = np.stack([rng.uniform(-1.4, 1.4, 1200), np.full(1200, 3.6), rng.uniform(-1.0, 1.0, 1200)], 1)
    box = rng.uniform(-4.0, 4.0, (500, 3))
    # points of image 0 (the pinhole camera) on its last column, its last row and left of the first pixel centre: visible, but the
    # bilinear sample has no right / lower neighbour (or x < 0) and is rejected -- at scale 0 and, projected to level 1, at scale 1
    from oracle import binding as ob
    R = ob.quat_to_R(images[0]["q"]); t = images[0]["t"]
    fx, fy, cx, cy = [float(v) for v in intrinsics[0]["params"]]
    edge = [_back_project(R, t, fx, fy, cx, cy, px, py, 2.0) for px, py in ((39.2, 12.0), (39.1, 20.5), (15.0, 29.3), (24.6, 29.2), (-0.3, 8.0))]
    pts = np.concatenate([front, back, box, np.array(edge)]).astype(np.float32)
    return dict(pts=pts, intrinsics=intrinsics, images=images, n_edge=len(edge))


@pytest.fixture(scope="module")
def scene():
    """The scene and its expected values, computed once on the CPU: {current_image_scale: (sums, counts, reasons)}."""
    S = _build_scene()
    S["expected"] = {s: ref.colour_cloud(S["pts"], S["intrinsics"], S["images"], S["pts"], s, splat_radius=SPLAT_RADIUS) for s in (0, 1)}
    return S


def _make_problem(e3d, S, current_image_scale, shard=None):
    G = e3d.RegProblem(e3d.default_reg_params(image_scale_count=N_LEVELS, current_image_scale=current_image_scale, splat_radius=SPLAT_RADIUS))
    if shard is not None:            # the colouring calls no collective: the callbacks only have to exist
        G.set_shard(shard[0], shard[1], lambda buf: None, lambda ptr, count, dtype: None)
    for iid, I in S["intrinsics"].items():
        G.set_intrinsics(iid, I["w"], I["h"], I["params"], I["min"], I["n"], camera_type=I["model"])
    dims = {iid: [G.intrinsics_level(iid, l)[:2] for l in range(N_LEVELS)] for iid in S["intrinsics"]}
    for iid, I in S["intrinsics"].items():
        if I["cam_masks"] is not None:
            G.set_camera_mask(iid, [_fit(m, *dims[iid][l]) for l, m in enumerate(I["cam_masks"])])
    G.set_splat_points(S["pts"])
    for i, im in S["images"].items():
        if shard is not None and i % shard[1] != shard[0]:
            G.set_image(i, im["intr"], None)
        else:
            d = dims[im["intr"]]
            G.set_image(i, im["intr"], [_fit(a, *d[l]) for l, a in enumerate(im["pyr"])],
                        [_fit(a, *d[l]) for l, a in enumerate(im["masks"])] if im["masks"] is not None else None)
        G.set_image_pose(i, im["q"], im["t"])
    G.set_scan_points(S["pts"])
    return G


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_matches(G, S, scale):
    sums, counts, _ = S["expected"][scale]
    G.scan_colors_begin()
    for i in sorted(S["images"]):
        G.scan_colors_add_image(i, S["images"][i]["color"])
    g_sums, g_counts = G.scan_colors_sums()
    assert np.array_equal(g_counts, counts)
    assert np.array_equal(_bits(g_sums), _bits(sums))
    rgb = G.scan_colors_finish()
    assert np.array_equal(rgb, ref.finish(sums, counts))
    return rgb


def test_scene_takes_every_branch(scene):
    """Conditions on the scene, from the CPU helper alone: enough points coloured by two images, enough by none, every way a point
    can miss its colour occurs -- at both image scales."""
    n = len(scene["pts"])
    assert 3500 <= n <= 4500
    for s in (0, 1):
        sums, counts, reasons = scene["expected"][s]
        assert (counts >= 2).mean() >= 0.25 and (counts == 0).mean() >= 0.10
        taken = set(np.concatenate(list(reasons.values())).tolist())
        assert taken == {ref.COLOURED, ref.BEHIND, ref.OUTSIDE, ref.OCCLUDED, ref.IMAGE_MASK, ref.CAMERA_MASK, ref.SATURATED, ref.SAMPLE_REJECTED}
        # the points placed on the last column, the last row and left of the first pixel centre of image 0: seen, sample rejected
        assert (reasons[0][-scene["n_edge"]:] == ref.SAMPLE_REJECTED).all()
        assert ref.IMAGE_MASK in reasons[1] and ref.CAMERA_MASK in reasons[2] and ref.SATURATED in reasons[2]
    # the two scales do not see the same thing
    assert not np.array_equal(scene["expected"][0][1], scene["expected"][1][1])


@pytest.mark.parametrize("scale", [0, 1])
def test_scan_colors_match_reference_bit_for_bit(e3d, scene, scale):
    G = _make_problem(e3d, scene, scale)
    G.profile(True)
    rgb = _assert_matches(G, scene, scale)
    assert (rgb.max(1) > 0).mean() > 0.4
    G.profile(False)
    assert G.kernel_groups["debug.scan_colors"][1:] == (3, 3.0 * len(scene["pts"]))
    assert G.kernel_groups["debug.scan_colors_finish"][1:] == (1, float(len(scene["pts"])))
    # a second pass on the same handle starts from zero again
    _assert_matches(G, scene, scale)


def test_scan_colors_sharded_partial_sums(e3d, scene):
    """Two handles, images id mod 2: counts add up exactly, the sums added in rank order equal the helper's, set_sums + finish on rank 0
    gives the helper's colours -- at most one level per channel from the single-handle result."""
    S = scene
    sums, counts, _ = S["expected"][0]
    e_sums, e_counts, e_partials = ref.colour_cloud_sharded(S["pts"], S["intrinsics"], S["images"], S["pts"], 0, 2, splat_radius=SPLAT_RADIUS)
    ranks = [_make_problem(e3d, S, 0, shard=(r, 2)) for r in range(2)]
    parts = []
    for r, G in enumerate(ranks):
        G.scan_colors_begin()
        for i in sorted(S["images"]):
            if i % 2 == r:
                G.scan_colors_add_image(i, S["images"][i]["color"])
            else:
                with pytest.raises(e3d.E3DError):              # another rank's image
                    G.scan_colors_add_image(i, S["images"][i]["color"])
        parts.append(G.scan_colors_sums())
        assert np.array_equal(parts[r][1], e_partials[r][1]) and np.array_equal(_bits(parts[r][0]), _bits(e_partials[r][0]))
    assert np.array_equal(parts[0][1] + parts[1][1], counts)
    total = parts[0][0] + parts[1][0]
    assert total.dtype == np.float32 and np.array_equal(_bits(total), _bits(e_sums)) and np.array_equal(e_counts, counts)
    ranks[0].scan_colors_set_sums(total, parts[0][1] + parts[1][1])
    rgb = ranks[0].scan_colors_finish()
    assert np.array_equal(rgb, ref.finish(e_sums, e_counts))
    single = ref.finish(sums, counts)
    assert np.abs(rgb.astype(np.int32) - single.astype(np.int32)).max() <= 1
    # set_sums alone (no begin) on a fresh handle is enough for finish
    F = _make_problem(e3d, S, 0)
    F.scan_colors_set_sums(total, e_counts)
    assert np.array_equal(F.scan_colors_finish(), rgb)


def test_scan_colors_without_points(e3d, scene):
    G = _make_problem(e3d, scene, 0)
    G.set_scan_points(np.zeros((0, 3), np.float32))
    G.scan_colors_begin()
    G.scan_colors_add_image(0, scene["images"][0]["color"])
    s, c = G.scan_colors_sums()
    assert s.shape == (0, 3) and c.shape == (0,) and G.scan_colors_finish().shape == (0, 3)


def test_scan_colors_errors_leave_the_handle_usable(e3d, scene):
    G = _make_problem(e3d, scene, 0)
    color = scene["images"][0]["color"]
    with pytest.raises(e3d.E3DError):
        G.scan_colors_add_image(0, color)                      # before begin
    with pytest.raises(e3d.E3DError):
        G.scan_colors_finish()
    G.scan_colors_begin()
    with pytest.raises(e3d.E3DError):
        G.scan_colors_add_image(99, color)                     # unknown image
    with pytest.raises(e3d.E3DError):
        G.scan_colors_add_image(0, np.zeros((1, 1, 3), np.uint8))
    with pytest.raises(e3d.E3DError):
        G.scan_colors_add_image(0, np.zeros((1, 40, 3), np.uint8))
    _assert_matches(G, scene, 0)
    # new scan points need a new begin
    G.set_scan_points(scene["pts"])
    with pytest.raises(e3d.E3DError):
        G.scan_colors_add_image(0, color)
    _assert_matches(G, scene, 0)
    # no scan points at all
    H = e3d.RegProblem(e3d.default_reg_params(image_scale_count=N_LEVELS))
    with pytest.raises(e3d.E3DError):
        H.scan_colors_begin()


def test_scan_colors_bounds_follow_the_colour_image(e3d, scene):
    """A colour image one column narrower than its camera (40 x 30 -> 39 x 30): the sample is rejected by the colour image's own size
    and the rows are 39 pixels long."""
    S = scene
    narrow = np.ascontiguousarray(S["images"][0]["color"][:, :39])
    images = dict(S["images"]); images[0] = dict(images[0], color=narrow)
    sums, counts, reasons = ref.colour_cloud(S["pts"], S["intrinsics"], images, S["pts"], 0, splat_radius=SPLAT_RADIUS, image_ids=[0])
    full = ref.colour_cloud(S["pts"], S["intrinsics"], S["images"], S["pts"], 0, splat_radius=SPLAT_RADIUS, image_ids=[0])
    assert (reasons[0] == ref.SAMPLE_REJECTED).sum() > (full[2][0] == ref.SAMPLE_REJECTED).sum()     # the column 38 <= x < 39 is lost
    assert not np.array_equal(_bits(sums), _bits(full[0]))
    G = _make_problem(e3d, S, 0)
    G.scan_colors_begin()
    G.scan_colors_add_image(0, narrow)
    g_sums, g_counts = G.scan_colors_sums()
    assert np.array_equal(g_counts, counts) and np.array_equal(_bits(g_sums), _bits(sums))
    assert np.array_equal(G.scan_colors_finish(), ref.finish(sums, counts))
