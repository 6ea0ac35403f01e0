"""Known answers, worked by hand, for tests/debug_cloud_ref.py -- the CPU restatement of Problem::DebugWriteColoredPointCloud that the
GPU tests of e3d_reg_scan_colors_* compare against bit for bit.  Every weight below is a dyadic fraction, so the f32 results are exact."""
import numpy as np

import debug_cloud_ref as ref

F = np.float32


def test_bilinear_2x2_at_quarter_three_quarters():
    # x = 0.25, y = 0.75: fx = 1/4, fx_inv = 3/4, fy = 3/4, fy_inv = 1/4 -> weights tl 3/16, tr 1/16, bl 9/16, br 3/16
    color = np.array([[[16, 0, 255], [32, 0, 255]],
                      [[64, 0, 255], [128, 255, 255]]], np.uint8)
    c = ref.bilinear_vec3(color, 0.25, 0.75)
    assert c.dtype == F
    # r: 3 + 2 + 36 + 24 = 65; g: 255 * 3/16 = 47.8125; b: 47.8125 + 15.9375 + 143.4375 + 47.8125 = 255
    assert c.tolist() == [65.0, 47.8125, 255.0]


def test_bilinear_3x3_uses_the_last_admissible_texels():
    # x = 1.5, y = 1.25 in a 3 x 3 image: ix = iy = 1 = cols - 2; weights tl 3/8, tr 3/8, bl 1/8, br 1/8
    color = np.zeros((3, 3, 3), np.uint8)
    color[1, 1] = (8, 16, 200); color[1, 2] = (16, 48, 200); color[2, 1] = (64, 0, 40); color[2, 2] = (128, 80, 40)
    c = ref.bilinear_vec3(color, 1.5, 1.25)
    # r: 3 + 6 + 8 + 16 = 33; g: 6 + 18 + 0 + 10 = 34; b: 75 + 75 + 5 + 5 = 160
    assert c.tolist() == [33.0, 34.0, 160.0]
    # integer position: the top-left texel alone
    assert ref.bilinear_vec3(color, 1.0, 1.0).tolist() == [8.0, 16.0, 200.0]


def test_bilinear_rejections():
    color = np.full((3, 2, 3), 7, np.uint8)          # rows = 3, cols = 2
    assert ref.bilinear_vec3(color, -0.25, 0.5) is None                 # x < 0
    assert ref.bilinear_vec3(color, 0.5, -1e-6) is None                 # y < 0
    assert ref.bilinear_vec3(color, 1.0, 0.5) is None                   # (int)x == cols - 1
    assert ref.bilinear_vec3(color, 0.5, 2.0) is None                   # (int)y == rows - 1
    assert ref.bilinear_vec3(color, 0.5, 2.75) is None
    assert ref.bilinear_vec3(color, np.nan, 0.5) is None
    # just inside on both axes; -0.0 is not < 0
    assert ref.bilinear_vec3(color, np.nextafter(F(1), F(0)), np.nextafter(F(2), F(0))).tolist() == [7.0, 7.0, 7.0]
    assert ref.bilinear_vec3(color, -0.0, 0.0).tolist() == [7.0, 7.0, 7.0]


def test_finish_rounding_and_unseen_points():
    sums = np.array([[5.0, 4.98, 510.0],       # count 2: 2.5 + 0.5 = 3.0 -> 3; 2.49 + 0.5 -> 2; 255 + 0.5 -> 255
                     [0.0, 1.0, 254.5],        # count 1: 0.5 -> 0; 1.5 -> 1; 255.0 -> 255
                     [9.0, 9.0, 9.0],          # count 0: 0 0 0 whatever the sums hold
                     [7.0, 8.0, 765.0]], F)    # count 3: 7 / 3 + 0.5 = 2.83 -> 2; 8 / 3 + 0.5 = 3.17 -> 3; 255.5 -> 255
    counts = np.array([2, 1, 0, 3], np.int32)
    assert ref.finish(sums, counts).tolist() == [[3, 2, 255], [0, 1, 255], [0, 0, 0], [2, 3, 255]]
    assert ref.finish(np.zeros((0, 3), F), np.zeros(0, np.int32)).shape == (0, 3)


def test_rank_ordered_sums_are_f32_left_to_right():
    big, one = F(16777216.0), F(1.0)                # 2^24 + 1 is not an f32
    p = lambda v, c: (np.full((1, 3), v, F), np.array([c], np.int32))
    s, c = ref.add_rank_ordered([p(big, 1), p(one, 2), p(one, 3)])
    assert s.dtype == F and s.tolist() == [[16777216.0] * 3] and c.tolist() == [6]          # (2^24 + 1) + 1, each + 1 lost
    s, c = ref.add_rank_ordered([p(one, 0), p(one, 0), p(big, 1)])
    assert s.tolist() == [[16777218.0] * 3] and c.tolist() == [1]                            # (1 + 1) + 2^24
    a = (np.ones((2, 3), F), np.ones(2, np.int32))
    ref.add_rank_ordered([a, a])
    assert a[0].tolist() == [[1.0] * 3] * 2 and a[1].tolist() == [1, 1]                       # the partials stay as they were


def test_image_xy_at_scale():
    # scale 1 - 1e-6 -> smaller interpolation scale 1; to scale 0: 2 * (x + 0.5) - 0.5
    x, y = ref.image_xy_at_scale(F(2.0), F(0.25), F(1) - F(1e-6), 0)
    assert (float(x), float(y)) == (4.5, 1.0)
    # returned scale 0 (the halved case) has the same smaller interpolation scale; to scale 1 nothing changes
    x, y = ref.image_xy_at_scale(F(2.0), F(0.25), F(0), 1)
    assert (float(x), float(y)) == (2.0, 0.25)


class _Cam:
    width, height = 8, 6


def _project(cam, P):                                # pinhole fx = fy = 10, cx = 3.5, cy = 2.5, in f32
    return np.array([F(10) * (P[0] / P[2]) + F(3.5), F(10) * (P[1] / P[2]) + F(2.5)], F)


def test_observations_no_scale_branches_and_halving():
    R = np.eye(3, dtype=F); t = np.zeros(3, F)
    pts = np.array([[0.0, 0.0, 2.0],         # 0: pixel (3.5, 2.5) -> rounds to (4, 3): observed
                    [0.0, 0.0, -1.0],        # 1: behind
                    [2.0, 0.0, 2.0],         # 2: x = 13.5: outside
                    [0.2, 0.0, 2.0],         # 3: (4.5, 2.5) -> (5, 3): occluded below
                    [-0.2, 0.0, 2.0],        # 4: (2.5, 2.5) -> (3, 3): image mask
                    [-0.4, 0.0, 2.0],        # 5: (1.5, 2.5) -> (2, 3): camera mask
                    [0.0, -0.2, 2.0],        # 6: (3.5, 1.5) -> (4, 2): over-saturated
                    [-0.8, -0.52, 2.0]], F)  # 7: (-0.5, -0.1) -> (0, 0) after + 0.5: observed at the corner
    occ = np.full((6, 8), np.inf, F); occ[3, 5] = 1.5
    mask = np.zeros((6, 8), np.uint8); mask[3, 3] = 1
    cmask = np.zeros((6, 8), np.uint8); cmask[3, 2] = 2
    img = np.full((6, 8), 100, np.uint8); img[2, 4] = 253
    reason, x, y, rs = ref.observations_no_scale(pts, R, t, _Cam, 0, img, mask, cmask, occ, project=_project)
    assert reason.tolist() == [0, ref.BEHIND, ref.OUTSIDE, ref.OCCLUDED, ref.IMAGE_MASK, ref.CAMERA_MASK, ref.SATURATED, 0]
    # image scale 0: the returned scale is clamped to 0 and the position halved about the pixel centre: 0.5 * (3.5 + 0.5) - 0.5
    assert rs == F(0) and (float(x[0]), float(y[0])) == (1.5, 1.0)
    # ... and back at scale 0 it is the projection again
    bx, by = ref.image_xy_at_scale(x[0], y[0], rs, 0)
    assert (float(bx), float(by)) == (3.5, 2.5)
    # image scale 1: 1 - 1e-6, positions as projected
    reason, x, y, rs = ref.observations_no_scale(pts[:1], R, t, _Cam, 1, img, None, None, occ, project=_project)
    assert reason.tolist() == [0] and rs == F(1) - F(1e-6) and int(rs) == 0 and (float(x[0]), float(y[0])) == (3.5, 2.5)
    # a grey value equal to the limit is kept, the occlusion threshold is inclusive
    img[3, 4] = 252; occ[3, 4] = F(2.0) - F(0.01)
    assert ref.observations_no_scale(pts[:1], R, t, _Cam, 1, img, None, None, occ, project=_project)[0].tolist() == [0]
    occ[3, 4] = np.nextafter(F(2.0) - F(0.01), F(0)) - F(1e-6)
    assert ref.observations_no_scale(pts[:1], R, t, _Cam, 1, img, None, None, occ, project=_project)[0].tolist() == [ref.OCCLUDED]
