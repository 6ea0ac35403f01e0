"""e3d_reg_pick_scan_points / _image_bearings / _project_points (DatasetInspector's "Localize image" on the GPU) through capi.RegProblem,
and bin/ImageLocalizer around them, against the CPU restatement in tests/localize_ref.py.  Projection and occlusion depth are
bit-identical on both sides for every camera model (test_gpu_reg.py) and the distance of the pick is three f32 operations without
contraction, so indices, positions and distances are compared with np.array_equal.  The scene, its clicks and the repair case come from
tests/test_localize_host.py, which checks on the CPU that they hold what these tests rely on."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import localize_ref as lr
import test_localize_host as host
import test_mask_transfer_host as mth
from cli_util import BIN, ROOT
from test_localize_host import IMAGE
from test_mask_transfer_host import HEIGHT, N_LEVELS, OCCLUSION_THRESHOLD, SPLAT_RADIUS, WIDTH

pytestmark = pytest.mark.gpu
sys.path.insert(0, ROOT)

MODELS = list(range(13))
F = np.float32
TOOL = os.path.join(BIN, "ImageLocalizer")


def _problem(e3d, S, scan=None, shard=None):
    M = S["M"]
    G = e3d.RegProblem(e3d.default_reg_params(image_scale_count=N_LEVELS))
    if shard is not None:
        G.set_shard(shard[0], shard[1], lambda buf: None, lambda ptr, count, dtype: None)
    G.set_intrinsics(0, WIDTH, HEIGHT, M["params"], 0, N_LEVELS, camera_type=S["model"])
    G.set_splat_points(S["scan"])
    for i, im in enumerate(M["images"]):
        G.set_image(i, 0, im["pyr"] if shard is None or i % shard[1] == shard[0] else None)
        G.set_image_pose(i, im["q_init"], im["t_init"])
    if scan is not None:
        G.set_scan_points(scan)
    return G


def _same(got, want):
    """indices, positions (NaN = NaN), distances and the visible count: all equal."""
    assert got[0].dtype == np.int64 and got[1].dtype == np.float32 and got[2].dtype == np.float32
    assert np.array_equal(got[0], want[0]), (got[0], want[0])
    assert np.array_equal(got[1], want[1], equal_nan=True)
    assert np.array_equal(got[2], want[2])
    assert got[3] == want[3]


@pytest.mark.parametrize("model", MODELS)
def test_pick_equals_the_restatement(e3d, model):
    """1, 8, 9 and 32 clicks (one lane group of 1, 8, 16 and 32 lanes) on the whole scene: ties, occluded and behind-camera points next to
    the click, a click far outside, a NaN click."""
    L = host.localize_scene(model)
    G = _problem(e3d, L["S"], L["scan"])
    want = lr.pick(L["sp"], L["clicks"])
    assert want[3] > 5000
    for k in (32, 9, 8, 1):
        got = G.pick_scan_points(IMAGE, L["clicks"][:k])
        _same(got, tuple(w[:k] for w in want[:3]) + (want[3],))
    # other starts into the list: every kind of click alone and first
    for first in (3, 5, 7, 8):
        _same(G.pick_scan_points(IMAGE, L["clicks"][first:first + 1]), tuple(w[first:first + 1] for w in want[:3]) + (want[3],))
    # pixel_out is the unrounded position of the winner, distance_out its squared distance
    got = G.pick_scan_points(IMAGE, L["clicks"])
    ok = got[0] >= 0
    assert np.array_equal(got[1][ok], L["sp"]["pxy"][got[0][ok]]) and (got[1][ok] != np.rint(got[1][ok])).any()
    assert np.array_equal(got[2][ok], np.array([lr.squared_distance(p, c) for p, c in zip(got[1][ok], L["clicks"][ok])], F))


def test_pick_rules_on_the_scene(e3d):
    L = host.localize_scene(0)
    G = _problem(e3d, L["S"], L["scan"])
    idx, px, d, n = G.pick_scan_points(IMAGE, L["clicks"])
    n_base = len(L["S"]["scan"])
    assert idx[0:3].tolist() == L["doubled"].tolist() and (idx[0:3] < n_base).all() and (d[0:3] == 0).all()       # the copy at the end loses
    assert all(idx[k] != i and idx[k] >= 0 and d[k] > 0 for k, i in zip((3, 4), L["occluded"]))                      # occluded: not taken
    assert all(idx[k] != i and idx[k] >= 0 and d[k] > 0 for k, i in zip((5, 6), L["behind"]))                        # behind the camera: not taken
    assert idx[7] >= 0 and d[7] > 1e7 and L["sp"]["visible"][idx[7]]                                                 # far outside: the nearest visible point
    assert idx[8] == -1 and np.isposinf(d[8]) and np.isnan(px[8]).all()                                              # NaN click
    assert n == int(L["sp"]["visible"].sum())
    # the copies first: now THEY have the lower index
    order = np.concatenate([np.arange(n_base, n_base + host.N_DUPLICATES), np.arange(n_base)])
    G.set_scan_points(L["scan"][order])
    idx2 = G.pick_scan_points(IMAGE, L["clicks"][:3])[0]
    assert idx2.tolist() == [0, 1, 2]


@pytest.mark.parametrize("model", [0, 2])
def test_pick_point_counts(e3d, model):
    """0, 1, 63, 65, 257 points and the whole scan: partial waves, partial blocks, one block, several; the occlusion geometry as it was."""
    L = host.localize_scene(model)
    G = _problem(e3d, L["S"], L["scan"])
    for n in (0, 1, 63, 65, 257, 12345, len(L["scan"])):
        G.set_scan_points(L["scan"][:n])
        want = lr.pick(host.cut(L["sp"], n), L["clicks"])
        for k in (32, 5):
            _same(G.pick_scan_points(IMAGE, L["clicks"][:k]), tuple(w[:k] for w in want[:3]) + (want[3],))
        if n == 0:
            assert (want[0] == -1).all() and want[3] == 0
    # a visible point as the only one, and an invisible one
    v = int(np.nonzero(L["sp"]["visible"])[0][0]); o = int(L["occluded"][0])
    G.set_scan_points(L["scan"][v:v + 1])
    assert G.pick_scan_points(IMAGE, L["clicks"][9:12])[0].tolist() == [0, 0, 0]
    G.set_scan_points(L["scan"][o:o + 1])
    got = G.pick_scan_points(IMAGE, L["clicks"][9:12])
    assert got[0].tolist() == [-1, -1, -1] and got[3] == 0


def test_pick_over_several_grid_strides(e3d):
    """More points than one sweep of the fixed grid (2048 blocks of 256): the scan repeated 27 times, 640 000 points.  Every copy of a
    point ties with the original; the lowest index wins."""
    L = host.localize_scene(0)
    n = len(L["scan"])
    reps = 27
    G = _problem(e3d, L["S"], np.tile(L["scan"], (reps, 1)))
    assert reps * n > 2048 * 256
    want = lr.pick(L["sp"], L["clicks"])
    got = G.pick_scan_points(IMAGE, L["clicks"])
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2]) and got[3] == reps * want[3]
    # the last copy alone visible-side: drop the first copies' winners by picking from the tail only
    G.set_scan_points(np.concatenate([np.zeros((2048 * 256 + 77, 3), F) + F([0, -50, 0]), L["scan"]]))       # points behind every camera first
    got = G.pick_scan_points(IMAGE, L["clicks"])
    shifted = np.where(want[0] >= 0, want[0] + 2048 * 256 + 77, -1)
    assert np.array_equal(got[0], shifted) and np.array_equal(got[2], want[2]) and got[3] == want[3]


def _test_pixels(rng):
    """Corners, borders, the clamped last column and row, positions outside the image, and off-lattice positions."""
    fixed = [(0, 0), (WIDTH - 1, 0), (0, HEIGHT - 1), (WIDTH - 1, HEIGHT - 1), (WIDTH - 1.0005, HEIGHT - 1.0005), (WIDTH - 1.5, HEIGHT - 1.5),
             (0, 77.3), (123.6, 0), (WIDTH - 1, 50.5), (100.25, HEIGHT - 1), (-3, -2), (WIDTH + 5, HEIGHT + 2), (0.5, 0.5), (17, 23), (WIDTH / 2, HEIGHT / 2)]
    return np.concatenate([np.array(fixed, F), np.stack([rng.uniform(0, WIDTH - 1, 24), rng.uniform(0, HEIGHT - 1, 24)], 1).astype(F)])


@pytest.mark.parametrize("model", MODELS)
def test_bearings_equal_the_restatement(e3d, model):
    """ImageToNormalized through the four lattice entries computed on the device against the checker's table and interpolation, with
    the tolerance tests/test_gpu_multires.py gives the same function (1e-6 of the largest value; the unit bearings' largest
    component is 1).  The same f64 normalisation on both sides, so equal normalised coordinates give equal bearings: the number of
    bit-equal bearings is printed."""
    S = mth.scene(model)
    G = _problem(e3d, S)
    pixels = _test_pixels(np.random.RandomState(3))
    got = G.image_bearings(IMAGE, pixels)
    want = lr.bearings(S["images"][IMAGE]["cam"], pixels)
    assert got.shape == (len(pixels), 3) and got.dtype == np.float64
    assert np.abs(np.linalg.norm(got, axis=1) - 1).max() < 1e-14
    diff = np.abs(got - want).max()
    print("model %d: bearings differ by at most %.3g; %d of %d bit-equal" % (model, diff, int((got == want).all(1).sum()), len(pixels)))
    assert diff <= 1e-6
    # the centre pixel looks along the axis of a camera without tangential terms only roughly; but the bearings spread over the field of view
    assert got[:, 2].min() < 0.97 and got[:, 2].max() > 0.999
    assert G.image_bearings(IMAGE, np.zeros((0, 2), F)).shape == (0, 3)


@pytest.mark.parametrize("model", [0, 2, 4, 12])
def test_project_points_against_visibility(e3d, model):
    L = host.localize_scene(model)
    G = _problem(e3d, L["S"])
    pixel, state = G.project_points(IMAGE, L["scan"])
    sp = L["sp"]
    assert state.dtype == np.uint8 and np.array_equal(state, sp["state"])
    assert np.array_equal(pixel, sp["pxy"], equal_nan=True)
    assert (state == lr.VISIBLE).sum() > 5000 and (state == lr.OCCLUDED).sum() > 500 and np.isnan(pixel[:, 0]).sum() > 100
    assert (state[~np.isnan(pixel[:, 0])] == lr.OUTSIDE).sum() > 100                  # in front of the camera and outside the image
    # a handful of points, a single one, none
    for n in (5, 1, 0):
        p, s = G.project_points(IMAGE, L["scan"][:n])
        assert np.array_equal(s, sp["state"][:n]) and np.array_equal(p, sp["pxy"][:n], equal_nan=True)


def test_profile_group(e3d):
    L = host.localize_scene(0)
    G = _problem(e3d, L["S"], L["scan"])
    G.profile(True)
    G.pick_scan_points(IMAGE, L["clicks"])
    G.pick_scan_points(IMAGE, L["clicks"][:1])
    G.profile(False)
    ms, launches, units = G.kernel_groups["localize.pick"]
    assert launches == 2 and units == 2.0 * len(L["scan"]) and ms >= 0


def test_errors_leave_the_handle_usable(e3d):
    import ctypes as C
    L = host.localize_scene(0)
    S = L["S"]
    lib = e3d.lib()
    clicks = np.ascontiguousarray(L["clicks"][:4]); index = np.zeros(32, np.int64)

    def raw_pick(G, image_id, c, n, out):
        return G._chk(lib.e3d_reg_pick_scan_points(G._h, image_id, C.c_void_p(c.ctypes.data) if c is not None else None, n,
                                                   C.c_void_p(out.ctypes.data) if out is not None else None, None, None), "e3d_reg_pick_scan_points")
    G = _problem(e3d, S)
    with pytest.raises(e3d.E3DError, match="no scan points"):
        G.pick_scan_points(IMAGE, clicks)
    G.set_scan_points(L["scan"])
    with pytest.raises(e3d.E3DError, match="n_clicks 0 outside 1 .. 32"):
        raw_pick(G, IMAGE, clicks, 0, index)
    with pytest.raises(e3d.E3DError, match="n_clicks 33 outside 1 .. 32"):
        G.pick_scan_points(IMAGE, np.zeros((33, 2), F))
    with pytest.raises(e3d.E3DError, match="null argument"):
        raw_pick(G, IMAGE, None, 4, index)
    with pytest.raises(e3d.E3DError, match="null argument"):
        raw_pick(G, IMAGE, clicks, 4, None)
    assert lib.e3d_reg_pick_scan_points(None, IMAGE, C.c_void_p(clicks.ctypes.data), 4, C.c_void_p(index.ctypes.data), None, None) < 0
    for call in (lambda: G.pick_scan_points(99, clicks), lambda: G.image_bearings(99, clicks), lambda: G.project_points(99, L["scan"][:3])):
        with pytest.raises(e3d.E3DError, match="image 99 not set"):
            call()
    out = np.zeros(12, np.float64)
    assert lib.e3d_reg_image_bearings(G._h, IMAGE, None, 4, C.c_void_p(out.ctypes.data)) < 0
    assert lib.e3d_reg_image_bearings(G._h, IMAGE, C.c_void_p(clicks.ctypes.data), 4, None) < 0
    assert lib.e3d_reg_image_bearings(G._h, IMAGE, C.c_void_p(clicks.ctypes.data), -1, C.c_void_p(out.ctypes.data)) < 0
    assert lib.e3d_reg_project_points(G._h, IMAGE, C.c_void_p(L["scan"].ctypes.data), 3, None, None) < 0
    # the failed calls changed nothing
    want = lr.pick(L["sp"], clicks)
    _same(G.pick_scan_points(IMAGE, clicks), want)
    # optional outputs left out: the indices alone
    raw_pick(G, IMAGE, clicks, 4, index)
    assert index[:4].tolist() == want[0].tolist()
    # an image owned by another rank
    R0 = _problem(e3d, S, L["scan"], shard=(0, 2))
    for call in (lambda: R0.pick_scan_points(1, clicks), lambda: R0.image_bearings(1, clicks), lambda: R0.project_points(1, L["scan"][:3])):
        with pytest.raises(e3d.E3DError, match="image 1 belongs to rank 1"):
            call()
    _same(R0.pick_scan_points(IMAGE, clicks), want)


# ---- end to end: an image at a wrong pose comes back -------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", [0, 2])
def test_pose_repair_end_to_end(e3d, model):
    """Image 0 off by 3 degrees and 10 cm; 8 clicks near 8 scan points as they appear at the wrong pose, each with the pixel where the
    point belongs; pick, bearings and solve through RegProblem: the chosen points are picked and the pose is the true one within the
    exact-data bound of the solver widened by the bearings' own error (test_localize_host.repair_bounds; measured: 9.2e-8 rad of
    bearing error for PINHOLE, 3.6e-6 rad for THIN_PRISM_FISHEYE, whose undistortion the 248 x 180 lookup interpolates)."""
    C = host.repair_case(model)
    S = C["S"]
    G = _problem(e3d, S, S["scan"])
    G.set_image_pose(IMAGE, C["q_wrong"], C["t_wrong"])
    idx, px, d, n = G.pick_scan_points(IMAGE, C["clicks"])
    assert idx.tolist() == C["chosen"].tolist() and (d < 0.09).all() and n == int(C["sp"]["visible"].sum())
    _same((idx, px, d, n), lr.pick(C["sp"], C["clicks"]))
    before, state = G.project_points(IMAGE, S["scan"][idx])
    assert (state == lr.VISIBLE).all() and np.linalg.norm(before - C["pixels"], axis=1).min() > 3       # pixels off at the wrong pose
    b = G.image_bearings(IMAGE, C["pixels"])
    ref_b = lr.bearings(S["images"][IMAGE]["cam"], C["pixels"])
    e, rot_bound, t_bound = host.repair_bounds(C, b)
    print("model %d: bearing error %.3g rad; device vs restatement bearings %.3g" % (model, e, np.abs(b - ref_b).max()))
    assert np.abs(b - ref_b).max() <= 1e-6
    q, t, stats = G.pose_from_bearings(S["scan"][idx].astype(np.float64), b, *G.get_image_pose(IMAGE))
    rot = lr.rotation_angle(lr.quat_to_R(q), C["R_true"]); dt = float(np.linalg.norm(t.astype(np.float64) - C["t_true"]))
    print("model %d: rotation %.3g rad (bound %.3g), translation %.3g m (bound %.3g)" % (model, rot, rot_bound, dt, t_bound))
    assert stats[3] and stats[0] > 0.02 and rot <= rot_bound and dt <= t_bound
    G.set_image_pose(IMAGE, q, t)
    after, _ = G.project_points(IMAGE, S["scan"][idx])
    assert np.linalg.norm(after - C["pixels"], axis=1).max() < 0.01


# ---- bin/ImageLocalizer end to end -----------------------------------------------------------------------------------------------------
def _printed_poses(stdout, prefix):
    return [host._printed_pose(l) for l in stdout.split("\n") if l.startswith(prefix)]


def _run(d, script, extra=()):
    path = os.path.join(d, "script_%d.txt" % len(os.listdir(d)))
    open(path, "w").write(script)
    out = os.path.join(d, "out_%d" % len(os.listdir(d)))
    r = subprocess.run([TOOL, "--scan_alignment_path", os.path.join(d, "scans.mlp"), "--image_base_path", os.path.join(d, "images"), "--state_path",
                        os.path.join(d, "state"), "--script", path, "--output_folder_path", out] + list(extra), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout, out


def _tool_camera(d, width, height):
    """The level-0 camera as the tool builds it: the parameters through their text, cx cy moved by -0.5f."""
    from oracle import reg_binding as rb
    cam_line = [l for l in open(os.path.join(d, "state", "cameras.txt")) if not l.startswith("#")][0].split()
    params = np.array([float(v) for v in cam_line[4:]], np.float64).astype(F)
    params[2] += F(-0.5); params[3] += F(-0.5)
    return rb.make_camera(width, height, params, 0), params


def _repair_script(M, cam, name, q_start, t_start, q_true, t_true):
    """-> (script, chosen point indices, the pixels): 8 picks at the start pose plus an offset, each with the point's pixel at the true pose."""
    from oracle import binding as ob
    from oracle import reg_binding as rb
    rng = np.random.RandomState(5)
    images = {}
    for key, (q, t) in (("start", (q_start, t_start)), ("true", (q_true, t_true))):
        R = ob.quat_to_R(np.asarray(q, F))
        images[key] = dict(R=R, t=np.asarray(t, F), cam=cam, occlusion=rb.splat_depth(M["pts"], R, np.asarray(t, F), cam, SPLAT_RADIUS))
    sp = lr.scan_points(M["pts"], images["start"], OCCLUSION_THRESHOLD)
    sp_true = lr.scan_points(M["pts"], images["true"], OCCLUSION_THRESHOLD)
    chosen = np.array(host.spread_points(sp, sp_true["state"] != lr.OUTSIDE, M["width"], M["height"]))
    clicks = (sp["pxy"][chosen] + rng.uniform(-0.2, 0.2, (8, 2)).astype(F)).astype(F)
    pixels = sp_true["pxy"][chosen]
    text = "# repair %s\nimage %s\n" % (name, name)
    text += "".join("pick %.9g %.9g %.9g %.9g\n" % (c[0], c[1], p[0], p[1]) for c, p in zip(clicks, pixels)) + "solve\n"
    return text, chosen, pixels, clicks


def test_cli_end_to_end(tmp_path, e3d):
    """A dataset on disk whose image 1 is off by 3 degrees and 10 cm: the tool's picks are the chosen scan points, its pose is what the
    same calls give through the binding (all nine digits) and the true pose within the bound of the end-to-end test; the state it
    writes carries that pose and the tool reads it again."""
    from reg_util import make_multi_image_scene
    from test_gpu_cli_reg import _write_dataset
    M = make_multi_image_scene(n_points=6000, n_images=3, seed=12, perturb=0.0)
    W, H = M["width"], M["height"]
    names = ["dslr/img_%d.png" % i for i in range(3)]
    through_text = lambda v: np.array(["%.9g" % x for x in v], np.float64).astype(F)
    q_true, t_true = through_text(M["images"][1]["q_init"]), through_text(M["images"][1]["t_init"])
    axis = np.array([0.4, 0.5, -0.75]); axis /= np.linalg.norm(axis)
    q_wrong = lr.R_to_quat(host._rotvec(np.deg2rad(3.0) * axis) @ lr.quat_to_R(q_true)).astype(F)
    t_wrong = (t_true + F([0.06, -0.06, 0.05])).astype(F)
    M["images"][1]["q_init"], M["images"][1]["t_init"] = q_wrong, t_wrong
    d = _write_dataset(tmp_path, M, names)
    cam, params = _tool_camera(d, W, H)
    text, chosen, pixels, clicks = _repair_script(M, cam, names[1], q_wrong, t_wrong, q_true, t_true)
    stdout, out = _run(d, text)
    # the same through the binding
    G = e3d.RegProblem(e3d.default_reg_params(image_scale_count=1))
    G.set_intrinsics(0, W, H, params, 0, 1)
    G.set_splat_points(M["pts"])
    for i, im in enumerate(M["images"]):
        G.set_image(i, 0, [im["pyr"][0]])
        G.set_image_pose(i, through_text(im["q_init"]), through_text(im["t_init"]))
    G.set_scan_points(M["pts"])
    idx = G.pick_scan_points(1, clicks)[0]
    assert idx.tolist() == chosen.tolist()
    b = G.image_bearings(1, pixels)
    q, t, stats = G.pose_from_bearings(M["pts"][idx].astype(np.float64), b, q_wrong, t_wrong)
    lines = [l for l in stdout.split("\n") if l.startswith("  correspondence ")]
    assert [int(re.search(r"scan point (\d+)", l).group(1)) for l in lines] == chosen.tolist()
    errors = [(float(m.group(1)), float(m.group(2))) for m in (re.search(r"error (\S+) px \(state \d\) -> (\S+) px", l) for l in lines)]
    assert min(e[0] for e in errors) > 3 and max(e[1] for e in errors) < 0.01
    (tq, tt), = _printed_poses(stdout, "Solved image 1")
    assert np.array_equal(tq.astype(F), q) and np.array_equal(tt.astype(F), t)
    R_true = lr.quat_to_R(q_true)
    C = dict(S=dict(scan=M["pts"]), chosen=chosen, R_true=R_true, t_true=t_true)
    e, rot_bound, t_bound = host.repair_bounds(C, b)
    assert lr.rotation_angle(lr.quat_to_R(tq), R_true) <= rot_bound and np.linalg.norm(tt - t_true) <= t_bound
    # ... and the restatement's own pick, bearings and solver end at the same pose
    Rr, tr = lr.solve(M["pts"][chosen].astype(np.float64), lr.bearings(cam, pixels), q_wrong, t_wrong)
    assert lr.rotation_angle(lr.quat_to_R(tq), Rr) <= rot_bound and np.linalg.norm(tt - tr) <= t_bound
    # the state: six digits of that pose, the other images as they were, and the tool reads it back
    st = host._read_images_txt(os.path.join(out, "images.txt"))
    assert np.array_equal(st[1][0], [float("%.6g" % v) for v in q]) and np.array_equal(st[1][1], [float("%.6g" % v) for v in t])
    for i in (0, 2):
        assert np.array_equal(st[i][0], [float("%.6g" % v) for v in through_text(M["images"][i]["q_init"])])
    open(os.path.join(d, "again.txt"), "w").write("image %s\nmove 0 0 0 0 0 0\n" % names[1])
    r = subprocess.run([TOOL, "--image_base_path", os.path.join(d, "images"), "--state_path", out, "--script", os.path.join(d, "again.txt"),
                        "--output_folder_path", os.path.join(d, "again")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "Moved image 1" in r.stdout, r.stderr


def test_cli_rig_repair_and_distribution(tmp_path, e3d):
    """A two-camera rig in two image sets; the second camera's image of set 0 is repaired and its relative pose distributed: both sets end
    with the relative pose of the repaired image, the repaired image at the true pose."""
    from reg_util import make_rig_scene
    from test_gpu_cli_reg import _write_dataset
    M = make_rig_scene(n_points=6000, seed=13)
    names = ["cam%d/frame_%d.png" % (i % 2, i // 2) for i in range(4)]
    for im in M["images"]:
        im["q_init"], im["t_init"] = im["q_true"], im["t_true"]
    axis = np.array([0.4, 0.5, -0.75]); axis /= np.linalg.norm(axis)
    true = (np.asarray(M["images"][1]["q_true"], F), np.asarray(M["images"][1]["t_true"], F))
    M["images"][1]["q_init"] = lr.R_to_quat(host._rotvec(np.deg2rad(3.0) * axis) @ lr.quat_to_R(true[0])).astype(F)
    M["images"][1]["t_init"] = (true[1] + F([0.06, -0.06, 0.05])).astype(F)
    rigs = [{"ref_camera_id": 7, "cameras": [{"camera_id": 7, "image_prefix": "cam0"}, {"camera_id": 7, "image_prefix": "cam1"}]}]
    d = _write_dataset(tmp_path, M, names, rigs=rigs)
    cam, _ = _tool_camera(d, M["width"], M["height"])
    # AssignRigs averages the rig over the two sets: the pose image 1 starts from is the tool's to tell (a move by nothing prints it)
    open(os.path.join(d, "probe.txt"), "w").write("image %s\nmove 0 0 0 0 0 0\n" % names[1])
    r = subprocess.run([TOOL, "--image_base_path", os.path.join(d, "images"), "--state_path", os.path.join(d, "state"), "--script",
                        os.path.join(d, "probe.txt"), "--output_folder_path", os.path.join(d, "probe")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    (q_start, t_start), = _printed_poses(r.stdout, "Moved image 1")
    assert 0.005 < lr.rotation_angle(lr.quat_to_R(q_start), lr.quat_to_R(true[0])) < 0.06
    text, chosen, pixels, clicks = _repair_script(M, cam, names[1], q_start.astype(F), t_start.astype(F), *true)
    stdout, out = _run(d, text + "distribute_relative_pose\n")
    lines = [l for l in stdout.split("\n") if l.startswith("  correspondence ")]
    assert [int(re.search(r"scan point (\d+)", l).group(1)) for l in lines] == chosen.tolist()
    (tq, tt), = _printed_poses(stdout, "Solved image 1")
    b = lr.bearings(cam, pixels)
    C = dict(S=dict(scan=M["pts"]), chosen=chosen, R_true=lr.quat_to_R(true[0]), t_true=true[1])
    e, rot_bound, t_bound = host.repair_bounds(C, b)
    assert lr.rotation_angle(lr.quat_to_R(tq), C["R_true"]) <= rot_bound and np.linalg.norm(tt - true[1]) <= t_bound
    assert "Distributed the relative pose of image 1 to 2 images" in stdout
    st = host._read_images_txt(os.path.join(out, "images.txt"))
    T = {i: (lr.quat_to_R(st[i][0]), st[i][1]) for i in st}
    rels = [lr._mul(T[2 * f + 1], lr._inv(T[2 * f])) for f in range(2)]
    # six digits in the file: 2e-5 as in the host test
    assert lr.rotation_angle(rels[0][0], rels[1][0]) <= 4e-5 and np.linalg.norm(rels[0][1] - rels[1][1]) <= 4e-5
    assert lr.rotation_angle(T[1][0], C["R_true"]) <= rot_bound + 2e-5 and np.linalg.norm(T[1][1] - true[1]) <= t_bound + 2e-5 * (1 + np.linalg.norm(true[1]))
    assert os.path.isfile(os.path.join(out, "rigs.json"))
