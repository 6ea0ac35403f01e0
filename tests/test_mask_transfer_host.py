"""MaskTransfer without a GPU: the rules of the label transfer pinned on the CPU restatement (tests/mask_transfer_ref.py) with a
hand-made case, the scene of the GPU tests (tests/test_gpu_mask_transfer.py imports it from here) checked for the conditions that
keep the GPU comparison from passing on an empty mask, and the argument handling of bin/MaskTransfer."""
import functools
import os
import subprocess

import numpy as np

import mask_transfer_ref as ref
from cli_util import BIN

F = np.float32
WIDTH, HEIGHT, N_POINTS, N_LEVELS = 248, 180, 20000, 3       # 248: no multiple of 32 or 64; 180: no multiple of 8, 16 or 32
SPLAT_RADIUS, OCCLUSION_THRESHOLD = 0.03, 0.01               # the defaults of default_reg_params (parameters.h)
SOURCE, TARGETS = 0, (1, 2)


# ---- the scene of the GPU tests -----------------------------------------------------------------------------------------------------
def make_scan(M, seed=5):
    """The scan: the wall of make_multi_image_scene (y = 3; it fills the middle of the images only), the occluder in front of part of
    it and the clutter behind the cameras / outside the images of the visibility test (test_gpu_reg.py), and points that reach past
    every image border: on the left a frame in front of the wall (y = 2.5, open where the wall is), on the right a second wall behind
    it (y = 3.5).  Seen from another camera the near points move one way and the far points the other, so labels arrive in the
    first column and in the last column, in the first row and beyond it."""
    rng = np.random.RandomState(seed)
    bx, bz = np.meshgrid(np.arange(-0.3, 0.2, 0.01), np.arange(-0.2, 0.2, 0.01))
    blocker = np.stack([bx.ravel(), np.full(bx.size, 1.6), bz.ravel()], 1)
    clutter = rng.uniform(-4, 4, (3000, 3))
    u = rng.uniform(-2.1, 0.0, 9000); v = rng.uniform(-1.5, 1.5, 9000)
    keep = ~((u > -0.97) & (np.abs(v) < 0.72))
    near = np.stack([u[keep], np.full(keep.sum(), 2.5), v[keep]], 1)[:5000]
    far = np.stack([rng.uniform(0.0, 2.6, 5000), np.full(5000, 3.5), rng.uniform(-2.0, 2.0, 5000)], 1)
    assert len(near) == 5000
    return np.concatenate([M["pts"], blocker, clutter, near, far]).astype(np.float32)


def source_mask():
    """Image 0's mask: a kObs rectangle on the left and top borders (corner included) and a kObs band along the rest of the top border, a
    kEvalObs rectangle on the right border with a kObs rectangle below it, a kObs rectangle over wall points that the occluder hides in
    image 1 with a kEvalObs strip at its lower edge, one isolated masked pixel."""
    m = np.zeros((HEIGHT, WIDTH), np.uint8)
    m[0:60, 0:70] = 1
    m[0:34, 70:WIDTH] = 1
    m[60:130, 196:WIDTH] = 2
    m[130:HEIGHT, 196:WIDTH] = 1
    m[136:HEIGHT:8, 196:WIDTH] = 2
    m[70:112, 96:150] = 1
    m[112:118, 100:140] = 2
    m[150, 30] = 1
    return m


def existing_mask():
    """Image 1's current mask: a kEvalObs block and a kObs block, both under what arrives."""
    m = np.zeros((HEIGHT, WIDTH), np.uint8)
    m[10:40, 20:60] = 2
    m[118:160, 192:240] = 1
    m[140:170, 100:160] = 1          # and a kObs block nothing arrives at: it stays
    return m


@functools.lru_cache(maxsize=None)
def scene(model):
    """dict(M, scan, images={id: the restatement's image description}, q, t) for one camera model; computed once per model."""
    from oracle import binding as ob
    from oracle import reg_binding as rb
    from reg_util import make_multi_image_scene
    M = make_multi_image_scene(n_points=N_POINTS, n_images=3, width=WIDTH, height=HEIGHT, n_levels=N_LEVELS, seed=17, perturb=0.0, model=model)
    scan = make_scan(M)
    cam = rb.camera_pyramid(rb.make_camera(WIDTH, HEIGHT, M["params"], model), N_LEVELS)[0]
    images = {}
    for i, im in enumerate(M["images"]):
        R = ob.quat_to_R(np.asarray(im["q_init"], F))
        images[i] = dict(R=R, t=np.asarray(im["t_init"], F), cam=cam, occlusion=rb.splat_depth(scan, R, im["t_init"], cam, SPLAT_RADIUS))
    return dict(M=M, scan=scan, images=images, model=model)


@functools.lru_cache(maxsize=None)
def scene_visibility(model, image_id):
    S = scene(model)
    return ref.visibility(S["scan"], S["images"][image_id], OCCLUSION_THRESHOLD)


@functools.lru_cache(maxsize=None)
def expected(model, target, transfer_eval_obs, with_existing, source=SOURCE):
    """The restatement's result for one (model, source -> target, flag, existing mask or none), computed once and shared."""
    labels = ref.point_labels(scene_visibility(model, source), source_mask(), transfer_eval_obs)
    r = ref.transfer_from_labels(labels, scene_visibility(model, target), (HEIGHT, WIDTH), transfer_eval_obs,
                                 existing_mask() if with_existing else None)
    r["labels"] = labels; r["n_labelled"] = int((labels != 0).sum())
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


# ---- the hand-made case ----------------------------------------------------------------------------------------------------------------
class _Cam:
    width, height = 12, 9


def _hand_project(cam, P):
    """A pinhole camera with f = 1 and the principal point at pixel (0, 0): the point (x, y, 1) lands on pixel (x, y)."""
    return np.array([F(P[0]) / F(P[2]), F(P[1]) / F(P[2])], F)


def _hand_images(shift=(0.0, 0.0)):
    """Source: the identity pose.  Target: moved so that the source's pixel (x, y) is the target's (x + shift[0], y + shift[1])."""
    occ = np.full((9, 12), np.inf, F)
    src = dict(R=np.eye(3, dtype=F), t=np.zeros(3, F), cam=_Cam, occlusion=occ)
    tgt = dict(R=np.eye(3, dtype=F), t=np.array([shift[0], shift[1], 0], F), cam=_Cam, occlusion=occ.copy())
    return src, tgt


def _at(*pixels):
    return np.array([[x, y, 1.0] for x, y in pixels], F)


def _run(pts, smask, eval_obs, existing=None, shift=(0.0, 0.0), images=None):
    src, tgt = images if images is not None else _hand_images(shift)
    return ref.transfer_labels(pts, src, tgt, smask, eval_obs, existing, project=_hand_project)


def test_hand_made_visibility():
    ones = np.ones((9, 12), np.uint8)
    # a point behind the camera, one outside the image, points left of / above pixel 0 whose truncated position would be 0, the last pixel
    pts = np.array([[3, 3, -1], [12, 3, 1], [-0.7, 3, 1], [-0.4, 3, 1], [3, -0.6, 1], [11.4, 8.4, 1], [11.5, 8, 1]], F)
    r = _run(pts, ones, False)
    assert r["labels"].tolist() == [0, 0, 0, 1, 0, 1, 0]                            # -0.7 + 0.5 < 0: rejected although (int)(-0.2) == 0
    assert r["point_mask"][3, 0] == 1 and r["point_mask"][8, 11] == 1 and r["stats"][0] == 2
    # occlusion + threshold >= z decides, in the source and in the target
    src, tgt = _hand_images()
    src["occlusion"][3, 3] = F(0.98); src["occlusion"][3, 4] = F(0.995)
    tgt["occlusion"][3, 5] = F(0.5)
    r = _run(_at((3, 3), (4, 3), (5, 3)), ones, False, images=(src, tgt))
    assert r["labels"].tolist() == [0, 1, 1] and r["point_mask"][3, 4] == 1 and r["point_mask"][3, 5] == 0 and r["stats"][0] == 1
    # the target's own pose: moved by (3, 2) pixels at depth 1, half of that at depth 2
    smask = np.zeros((9, 12), np.uint8); smask[4, 2] = 1; smask[4, 3] = 2
    pts = np.array([[2, 4, 1], [6, 8, 2]], F)                                       # source pixels (2, 4) and (3, 4)
    r = _run(pts, smask, True, shift=(3.0, 2.0))
    # (6 + 3) / 2 = 4.5 -> (int)(4.5 + 0.5) = 5; (8 + 2) / 2 = 5
    assert r["labels"].tolist() == [1, 2] and r["point_mask"][6, 5] == 1 and r["point_mask"][5, 5] == 2 and r["stats"][0] == 2


class _Quarter(_Cam):
    """The target camera of the next test: a quarter of the source's focal length, so that several source pixels share a target pixel."""


def _project_quarter(cam, P):
    p = _hand_project(cam, P)
    return p * F(0.25) if cam is _Quarter else p


def test_hand_made_highest_index_wins_a_pixel():
    """Points from source pixels with different values that fall on one target pixel: the last one in cloud order decides."""
    smask = np.zeros((9, 12), np.uint8); smask[2, 2] = 1; smask[4, 2] = 2
    src, tgt = _hand_images()
    tgt = dict(tgt, cam=_Quarter)
    a, c = [2, 2, 1], [2, 3.9, 1]                       # source pixels (2, 2) = kObs and (2, 4) = kEvalObs; target (0.5, 0.5) and (0.5, 0.975) -> (1, 1)
    for order, winner in (([a, c], 2), ([c, a], 1), ([a, c, a], 1), ([c, a, c], 2), ([c, c, a, [5, 5, 1]], 1)):
        r = ref.transfer_labels(np.array(order, F), src, tgt, smask, True, project=_project_quarter)
        assert r["point_mask"][1, 1] == winner and r["stats"][0] == 1, order
    # without transfer_eval_obs the kEvalObs points never take part: kObs stays whatever the order
    for order in ([a, c], [c, a]):
        r = ref.transfer_labels(np.array(order, F), src, tgt, smask, False, project=_project_quarter)
        assert r["point_mask"][1, 1] == 1 and r["n_labelled"] == 1


def test_hand_made_fill_in_threshold_and_clipped_window():
    ones = np.ones((9, 12), np.uint8)
    # two neighbours do not fill, three do
    r = _run(_at((4, 4), (6, 4)), ones, False)
    assert np.array_equal(r["filled"], r["point_mask"]) and r["stats"][:2] == (2, 2)
    r = _run(_at((4, 4), (6, 4), (5, 6)), ones, False)
    f = r["filled"]
    # the windows that hold all three points: rows 4 .. 6 and columns 4 .. 6 (|dy| <= 2 and |dx| <= 2 from every point)
    exp = np.zeros((9, 12), np.uint8); exp[4:7, 4:7] = 1; exp[4, 4] = exp[4, 6] = exp[6, 5] = 1
    assert np.array_equal(f, exp) and r["stats"][:2] == (3, 9)
    # the fill is not recursive: pixels filled above do not vote (a fourth point far away stays alone)
    r = _run(_at((4, 4), (6, 4), (5, 6), (9, 7)), ones, False)
    assert r["filled"][6, 7] == 1                                                  # (7, 6) sees (6, 4), (5, 6) and (9, 7)
    assert r["filled"][7, 8] == 0 and r["filled"][6, 8] == 0 and r["filled"][7, 9] == 1      # (8, 7) sees (9, 7) and FILLED pixels only
    # the window is clipped at the corner: three points in rows 0 .. 2, columns 0 .. 2 fill the 3 x 3 corner, nothing wraps around
    r = _run(_at((0, 0), (2, 0), (1, 2)), ones, False)
    exp = np.zeros((9, 12), np.uint8); exp[0:3, 0:3] = 1
    assert np.array_equal(r["filled"], exp)
    assert r["filled"][:, 11].sum() == 0 and r["filled"][8, :].sum() == 0
    # ... and at the bottom right: pixel (11, 8) sees rows 6 .. 8, columns 9 .. 11 only
    r = _run(_at((9, 6), (11, 6), (9, 8)), ones, False)
    exp = np.zeros((9, 12), np.uint8); exp[6:9, 9:12] = 1
    assert np.array_equal(r["filled"], exp)
    # clipped, not clamped: two points in the corner's column would count twice each with a clamped window
    r = _run(_at((0, 0), (0, 1)), ones, False)
    assert r["stats"][:2] == (2, 2)


def test_hand_made_eval_obs_rules():
    smask = np.ones((9, 12), np.uint8); smask[:, 6:] = 2
    pts = _at((4, 4), (5, 4), (4, 6), (6, 5))                                      # three kObs and one kEvalObs point next to them
    # transfer_eval_obs = 1: [QUIRK] the kEvalObs pixel's window holds >= 3 kObs and < 3 kEvalObs pixels: it becomes kObs
    r = _run(pts, smask, True)
    assert r["point_mask"][5, 6] == 2 and r["filled"][5, 6] == 1 and r["n_labelled"] == 4
    # three kEvalObs pixels win over three kObs pixels in the same window
    pts2 = _at((3, 4), (5, 4), (4, 6), (6, 4), (7, 6), (6, 6))
    r = _run(pts2, smask, True)
    assert r["filled"][5, 5] == 2 and r["filled"][5, 3] == 1 and r["filled"][5, 8] == 2
    # transfer_eval_obs = 0 drops the 2s before the point pass: no kEvalObs label, no kEvalObs pixel, no vote
    r = _run(pts2, smask, False)
    assert r["n_labelled"] == 3 and (r["point_mask"] == 2).sum() == 0 and (r["filled"] == 2).sum() == 0
    assert r["filled"][5, 5] == 1 and r["filled"][5, 8] == 0


def test_hand_made_merge_and_empty_source():
    ones = np.ones((9, 12), np.uint8)
    pts = _at((4, 4), (6, 4), (5, 6))
    existing = np.zeros((9, 12), np.uint8); existing[4, 4] = 2; existing[5, 5] = 2; existing[4, 6] = 1; existing[0, 0] = 1; existing[8, 11] = 2
    smask = ones.copy(); smask[4, 6] = 2                                           # the point at (6, 4) carries kEvalObs
    r = _run(pts, smask, True, existing=existing)
    out = r["mask_out"]
    assert out[4, 4] == 2 and out[5, 5] == 2                                       # an existing kEvalObs survives an incoming kObs
    assert r["filled"][4, 6] == 2 and out[4, 6] == 2                               # an existing kObs is overwritten by what arrives
    assert out[0, 0] == 1 and out[8, 11] == 2                                      # nothing arrives: kept
    assert out[6, 5] == 1 and existing[6, 5] == 0
    assert r["stats"][2] == int((out != existing).sum()) > 0
    # without an existing mask the new mask is the result
    r0 = _run(pts, smask, True)
    assert np.array_equal(r0["mask_out"], r0["filled"]) and r0["stats"][2] == r0["stats"][1]
    # a source without a mask: nothing happens
    assert _run(pts, None, True, existing=existing) is None
    # an all-zero source mask: no label, the existing mask comes back
    r = _run(pts, np.zeros((9, 12), np.uint8), True, existing=existing)
    assert r["n_labelled"] == 0 and np.array_equal(r["mask_out"], existing) and r["stats"] == (0, 0, 0)


# ---- the GPU scene, checked on the CPU -------------------------------------------------------------------------------------------
GPU_CASES = [(t, f, e) for t in TARGETS for f in (False, True) for e in (False, True)]


def test_gpu_scene_is_not_trivial():
    """Conditions on the inputs of the GPU tests (PINHOLE; the other models see nearly the same picture), from the restatement alone."""
    model = 0
    smask, emask = source_mask(), existing_mask()
    assert smask[0, 0] == 1 and (smask[:, 0] == 1).any() and (smask[0, :] == 1).any() and (smask[:, -1] == 2).any()
    assert smask[150, 30] == 1 and smask[148:153, 28:33].sum() == 1                # the isolated pixel
    sv = scene_visibility(model, SOURCE)
    for target, flag, with_existing in GPU_CASES:
        r = expected(model, target, flag, with_existing)
        pm, filled, out = r["point_mask"], r["filled"], r["mask_out"]
        assert r["stats"][0] >= 300, (target, flag, r["stats"])
        assert ((pm == 0) & (filled != 0)).sum() >= 150, (target, flag)
        only_filled = (pm == 0) & (filled != 0)
        assert only_filled[0, :].any() and only_filled[:, 0].any() and only_filled[:, -1].any(), (target, flag)
        if flag:
            assert ((pm == 2) & (filled == 1)).sum() >= 1, target               # the quirk fires
        tv = scene_visibility(model, target)
        rejected = (r["labels"] != 0) & tv[3]
        if target == 1:
            assert rejected.sum() >= 100, (flag, int(rejected.sum()))
        if with_existing:
            assert ((emask == 2) & (filled != 0) & (out == 2)).sum() >= 20
            assert ((emask == 1) & (filled != 0)).sum() >= 20                    # an existing kObs is overwritten ...
            if flag:
                assert ((emask == 1) & (out == 2)).sum() >= 20                   # ... visibly so where kEvalObs arrives
            assert np.array_equal(out[140:170, 100:160] == 1, (emask[140:170, 100:160] == 1) | (filled[140:170, 100:160] == 1))
    assert sv[0].sum() > 5000 and sv[3].sum() > 500                               # the source sees much of the scan and has occluded points too


# ---- the tool ----------------------------------------------------------------------------------------------------------------------
def _tool(*args):
    return subprocess.run([os.path.join(BIN, "MaskTransfer")] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


def _write_state(d, names, width=12, height=9):
    os.makedirs(os.path.join(d, "state"), exist_ok=True)
    with open(os.path.join(d, "state", "cameras.txt"), "w") as f:
        f.write("# cameras\n7 PINHOLE %d %d 10 10 6 4.5\n" % (width, height))
    with open(os.path.join(d, "state", "images.txt"), "w") as f:
        f.write("# images\n")
        for i, name in enumerate(names):
            f.write("%d 1 0 0 0 0 0 0 7 %s\n\n" % (10 + i, name))


def test_tool_is_built_and_checks_its_arguments(tmp_path):
    subprocess.check_call(["make", "-s", "-C", os.path.join(os.path.dirname(BIN), "csrc", "host")])
    assert os.path.isfile(os.path.join(BIN, "MaskTransfer")) and os.access(os.path.join(BIN, "MaskTransfer"), os.X_OK)
    d = str(tmp_path)
    names = ["dslr/img_%d.png" % i for i in range(3)]
    _write_state(d, names)
    paths = ["--scan_alignment_path", os.path.join(d, "scans.mlp"), "--image_base_path", os.path.join(d, "images"), "--state_path", os.path.join(d, "state")]
    out = ["--output_folder_path", os.path.join(d, "out")]
    r = _tool()
    assert r.returncode != 0 and "Please specify all the required paths." in r.stderr
    r = _tool(*paths[:4], "--source_image", names[0], *out)
    assert r.returncode != 0 and "Please specify all the required paths." in r.stderr
    r = _tool(*paths, *out)
    assert r.returncode != 0 and "--source_image" in r.stderr
    r = _tool(*paths, "--source_image", names[0])
    assert r.returncode != 0 and "exactly one of --output_folder_path and --in_place" in r.stderr
    r = _tool(*paths, "--source_image", names[0], *out, "--in_place", "1")
    assert r.returncode != 0 and "exactly one of --output_folder_path and --in_place" in r.stderr
    r = _tool(*paths, "--source_image", "dslr/none.png", *out)
    assert r.returncode != 0 and "is not an image of the state" in r.stderr
    r = _tool(*paths, "--source_image", names[0], "--target_images", "dslr/none.png", *out)
    assert r.returncode != 0 and "is not an image of the state" in r.stderr
    # a source without a mask file: the GUI silently does nothing, the tool says so -- by name and by id
    for source in (names[0], "0"):
        r = _tool(*paths, "--source_image", source, *out)
        assert r.returncode != 0 and "has no mask" in r.stderr and "masks_for_images/dslr/img_0.png" in r.stderr, r.stderr
    assert not os.path.exists(os.path.join(d, "out"))
