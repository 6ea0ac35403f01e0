"""ImageLocalizer without a GPU: e3d_pose_from_bearings (host only) against known poses and against the restatement's own solver,
MoveImage and the relative-pose distribution of bin/ImageLocalizer against their f64 evaluation (tests/localize_ref.py), the rules
of the scan-point pick on a hand-made case, the tool's refusals, and the scene of the GPU tests (tests/test_gpu_localize.py imports
it from here) checked for the conditions those tests rely on."""
import functools
import json
import os
import re
import subprocess

import numpy as np
import pytest

import localize_ref as lr
import test_mask_transfer_host as mth
from cli_util import BIN
from test_mask_transfer_host import OCCLUSION_THRESHOLD, SPLAT_RADIUS

F = np.float32
EPS = float(np.finfo(np.float32).eps)            # 2^-23
TOOL = os.path.join(BIN, "ImageLocalizer")


def _rotvec(v):
    from scipy.spatial.transform import Rotation
    return Rotation.from_rotvec(v).as_matrix()


# ---- the solver ----------------------------------------------------------------------------------------------------------------------------
def _pose_case(seed, n=12, noise_px=0.0, focal=210.0):
    """n points in front of a camera with a known pose, their bearings (optionally from pixels with uniform noise of +- noise_px at the
    given focal length), and a start 5 degrees and 0.2 m off."""
    rng = np.random.RandomState(seed)
    P = rng.uniform(-1.5, 1.5, (n, 3)) + np.array([0, 0, 4.0])
    R = _rotvec(rng.normal(size=3) * 0.3); t = rng.uniform(-0.5, 0.5, 3)
    x = P @ R.T + t
    nxy = x[:, :2] / x[:, 2:3]
    if noise_px:
        nxy = nxy + rng.uniform(-noise_px, noise_px, nxy.shape) / focal
    f = np.concatenate([nxy, np.ones((n, 1))], 1); f /= np.linalg.norm(f, axis=1)[:, None]
    axis = rng.normal(size=3); axis /= np.linalg.norm(axis)
    shift = rng.normal(size=3); shift *= 0.2 / np.linalg.norm(shift)
    q0 = lr.R_to_quat(_rotvec(np.deg2rad(5.0) * axis) @ R).astype(F)
    t0 = (t + shift).astype(F)
    return P, f, R, t, q0, t0


@pytest.mark.parametrize("seed", range(6))
def test_solver_exact_data(e3d, seed):
    """The true pose is the global minimiser at cost 0: what remains is the f32 rounding of the output."""
    P, f, R, t, q0, t0 = _pose_case(seed)
    q, tt, stats = e3d.pose_from_bearings(P, f, q0, t0)
    assert q.dtype == np.float32 and abs(float(np.linalg.norm(q.astype(np.float64))) - 1) < 4 * EPS and q[0] >= 0
    assert lr.rotation_angle(lr.quat_to_R(q), R) <= 1e-6
    assert np.linalg.norm(tt.astype(np.float64) - t) <= 1e-6 * (1 + np.linalg.norm(t))
    before, after, iterations, converged = stats
    assert 0.01 < before < 0.2 and after < 1e-9 and 1 <= iterations <= 100 and converged
    assert before == pytest.approx(lr.rms_angle(lr.quat_to_R(q0), t0.astype(np.float64), P, f), rel=1e-9)


# the library's and the restatement's poses on noisy data: rounding the library's result to f32 moves a unit quaternion by at most
# 2^-24 per component (~1.2e-7 rad of rotation) and a translation component below 1 m by 2^-25; both iterations stop within
# 1e-12 of the minimiser.  Measured here over the 6 seeds: rotation 3.1e-8 rad, translation 1.1e-8 m; the bounds are 10 x that
# (DESIGN.md section 18).
NOISY_ROTATION_BOUND, NOISY_TRANSLATION_BOUND = 3.1e-7, 1.1e-7


@pytest.mark.parametrize("seed", range(6))
def test_solver_noisy_data_matches_the_restatement(e3d, seed):
    P, f, R, t, q0, t0 = _pose_case(100 + seed, noise_px=0.5)
    q, tt, stats = e3d.pose_from_bearings(P, f, q0, t0)
    Rr, tr = lr.solve(P, f, q0, t0)
    d_rot = lr.rotation_angle(lr.quat_to_R(q), Rr); d_t = float(np.linalg.norm(tt.astype(np.float64) - tr))
    print("noisy data, seed %d: library vs restatement: rotation %.3g rad, translation %.3g m" % (seed, d_rot, d_t))
    assert d_rot <= NOISY_ROTATION_BOUND and d_t <= NOISY_TRANSLATION_BOUND
    # the noise is felt: the minimiser is not the true pose, and the RMS angle after is the restatement's
    assert lr.rotation_angle(Rr, R) > 1e-4 and 1e-4 < stats[1] < 1e-2
    assert stats[1] == pytest.approx(lr.rms_angle(lr.quat_to_R(q), tt.astype(np.float64), P, f), rel=1e-6) and stats[3]


def test_solver_refusals(e3d):
    P, f, R, t, q0, t0 = _pose_case(3, n=6)
    q, tt, _ = e3d.pose_from_bearings(P, f, q0, t0)                                  # n = 6 works
    assert lr.rotation_angle(lr.quat_to_R(q), R) <= 1e-6
    with pytest.raises(e3d.E3DError, match="at least 6"):
        e3d.pose_from_bearings(P[:5], f[:5], q0, t0)
    line = np.outer(np.linspace(1, 3, 8), [0.1, 0.2, 1.0])                           # all points on one line through no special place
    x = line @ R.T + t
    with pytest.raises(e3d.E3DError, match="LDLT"):
        e3d.pose_from_bearings(line, x / np.linalg.norm(x, axis=1)[:, None], q0, t0)
    for bad in ("point", "bearing", "q", "t"):
        P2, f2, q2, t2 = P.copy(), f.copy(), q0.copy(), t0.copy()
        {"point": P2, "bearing": f2, "q": q2, "t": t2}[bad].flat[1] = np.nan
        with pytest.raises(e3d.E3DError, match="not finite"):
            e3d.pose_from_bearings(P2, f2, q2, t2)
    # the same through RegProblem's static method
    assert np.array_equal(e3d.RegProblem.pose_from_bearings(P, f, q0, t0)[0], q)


# ---- the pick on a hand-made case ------------------------------------------------------------------------------------------------------
def _hand_image():
    return dict(R=np.eye(3, dtype=F), t=np.zeros(3, F), cam=mth._Cam, occlusion=np.full((9, 12), np.inf, F))


def _hand_pick(pts, clicks, image=None):
    sp = lr.scan_points(np.asarray(pts, F), image or _hand_image(), project=mth._hand_project)
    a, b = lr.pick_serial(sp, clicks), lr.pick(sp, clicks)
    for u, v in zip(a[:3], b[:3]):
        assert np.array_equal(u, v, equal_nan=True)
    assert a[3] == b[3]
    return a


def test_hand_made_pick_rules():
    # the nearest point, its unrounded position and the squared distance, f32 operation by operation
    pts = [[2.25, 3.5, 1], [6, 4, 2], [9, 1, 1]]                                      # positions (2.25, 3.5), (3, 2), (9, 1)
    idx, px, d, n = _hand_pick(pts, [[2, 3], [3.1, 2.2], [8, 1], [100, -50]])
    assert idx.tolist() == [0, 1, 2, 2] and n == 3
    assert np.array_equal(px[0], F([2.25, 3.5])) and d[0] == F(0.25) * F(0.25) + F(0.5) * F(0.5)
    assert d[1] == (F(3) - F(3.1)) * (F(3) - F(3.1)) + (F(2) - F(2.2)) * (F(2) - F(2.2))
    assert d[3] == F(91) * F(91) + F(51) * F(51)                                      # far outside the image: still the nearest visible point
    # equal distances: the lowest index, whatever the order of the two
    for order, want in (([[4, 4, 1], [6, 4, 1]], 0), ([[6, 4, 1], [4, 4, 1]], 0), ([[1, 1, 1], [4, 4, 1], [4, 4, 1]], 1)):
        assert _hand_pick(order, [[5, 4]])[0].tolist() == [want]
    # behind the camera, outside the image, left of pixel 0 by more than half a pixel: never picked, although nearer
    pts = [[3, 3, -1], [12, 3, 1], [-0.7, 3, 1], [-0.4, 3, 1], [5, 5, 1]]
    idx, px, d, n = _hand_pick(pts, [[3, 3], [12, 3], [-0.7, 3], [4.9, 5]])
    assert idx.tolist() == [4, 4, 3, 4] and n == 2
    # behind the occlusion depth: not picked; at the threshold: picked
    im = _hand_image()
    im["occlusion"][3, 3] = F(0.98); im["occlusion"][3, 4] = F(0.995)
    idx, _, _, n = _hand_pick([[3, 3, 1], [4, 3, 1], [8, 3, 1]], [[3, 3], [4.2, 3]], im)
    assert idx.tolist() == [1, 1] and n == 2
    # a NaN click and a cloud with no visible point: -1, NaN position, +inf
    idx, px, d, n = _hand_pick([[3, 3, 1]], [[np.nan, 2], [2, np.nan], [3, 3]])
    assert idx.tolist() == [-1, -1, 0] and np.isnan(px[0]).all() and np.isposinf(d[0]) and d[2] == 0
    idx, px, d, n = _hand_pick([[3, 3, -1]], [[3, 3]])
    assert idx.tolist() == [-1] and n == 0 and np.isposinf(d[0])
    idx, _, _, n = _hand_pick(np.zeros((0, 3)), [[3, 3]])
    assert idx.tolist() == [-1] and n == 0
    # an infinite distance never wins: a click so far away that the squared distance overflows
    assert _hand_pick([[3, 3, 1]], [[3e19, 3]])[0].tolist() == [-1]
    # states: outside, visible, occluded
    sp = lr.scan_points(F([[3, 3, 1], [4, 3, 1], [20, 3, 1], [1, 1, -2]]), im, project=mth._hand_project)
    assert sp["state"].tolist() == [lr.OCCLUDED, lr.VISIBLE, lr.OUTSIDE, lr.OUTSIDE] and np.isnan(sp["pxy"][3]).all()
    assert np.array_equal(sp["pxy"][2], F([20, 3]))


# ---- the scene of the GPU tests ----------------------------------------------------------------------------------------------------------
IMAGE = 0
N_DUPLICATES = 3


@functools.lru_cache(maxsize=None)
def localize_scene(model):
    """The MaskTransfer GPU scene (248 x 180, the frame in front and the second wall behind) with three visible points of image 0
    repeated at the end of the scan (exact ties), the restatement's scan points of image 0, and 32 clicks:
      0 .. 2   on points that appear twice (distance 0 to both);      3, 4   on occluded points;
      5, 6     on the mirrored position of points behind the camera;  7      far outside the image;       8   NaN;
      9 ..     anywhere in the image and up to 20 pixels around it."""
    from oracle import reg_binding as rb
    S = mth.scene(model)
    image = S["images"][IMAGE]
    base = lr.scan_points(S["scan"], image, OCCLUSION_THRESHOLD)
    rng = np.random.RandomState(7)
    doubled = rng.choice(np.nonzero(base["visible"])[0], N_DUPLICATES, replace=False)
    scan = np.concatenate([S["scan"], S["scan"][doubled]]).astype(F)
    sp = {k: np.concatenate([v, v[doubled]]) for k, v in base.items()}               # the occlusion geometry stays the scan without the copies
    occluded = rng.choice(np.nonzero(sp["occluded"])[0], 2, replace=False)
    pp = lr.transform(image["R"], image["t"], scan)
    behind = []
    for i in np.nonzero(pp[:, 2] < F(-0.5))[0]:
        m = np.asarray(rb.cam_project(image["cam"], pp[i]), F)                       # x / z, y / z of a point behind the camera: its mirror image
        if np.isfinite(m).all() and 10 < m[0] < mth.WIDTH - 10 and 10 < m[1] < mth.HEIGHT - 10:
            behind.append((i, m))
        if len(behind) == 2:
            break
    clicks = np.zeros((32, 2), F)
    clicks[0:3] = sp["pxy"][doubled]
    clicks[3:5] = sp["pxy"][occluded]
    clicks[5:7] = [m for _, m in behind]
    clicks[7] = (1.0e4, -3.0e3)
    clicks[8] = (np.nan, 50)
    clicks[9:] = np.stack([rng.uniform(-20, mth.WIDTH + 20, 23), rng.uniform(-20, mth.HEIGHT + 20, 23)], 1)
    return dict(S=S, scan=scan, sp=sp, image=image, clicks=clicks, doubled=doubled, occluded=occluded, behind=[i for i, _ in behind])


def cut(sp, n):
    return {k: v[:n] for k, v in sp.items()}


def test_gpu_scene_has_what_the_gpu_tests_rely_on():
    for model in (0, 2):
        L = localize_scene(model)
        sp, clicks = L["sp"], L["clicks"]
        idx, px, d, n = lr.pick(sp, clicks)
        assert n == int(sp["visible"].sum()) > 5000 and sp["occluded"].sum() > 500 and len(L["behind"]) == 2
        # ties: the original wins over its copy at the end of the scan, at distance 0
        assert idx[0:3].tolist() == L["doubled"].tolist() and (d[0:3] == 0).all() and (L["doubled"] < len(L["S"]["scan"])).all()
        for k, i in enumerate(L["doubled"]):
            assert np.array_equal(sp["pxy"][i], sp["pxy"][len(L["S"]["scan"]) + k]) and sp["visible"][len(L["S"]["scan"]) + k]
        # the occluded points are the nearest projected points of their clicks (distance 0) and are not taken
        for k, i in zip((3, 4), L["occluded"]):
            assert lr.squared_distance(sp["pxy"][i], clicks[k]) == 0 and idx[k] != i and idx[k] >= 0 and d[k] > 0
        # ... and so are the mirror images of the points behind the camera
        for k, i in zip((5, 6), L["behind"]):
            assert not sp["visible"][i] and np.isnan(sp["pxy"][i]).all() and idx[k] >= 0 and d[k] > 0
        assert idx[7] >= 0 and d[7] > 1e7 and idx[8] == -1 and (idx[9:] >= 0).all()
        assert len(set(idx[9:].tolist())) >= 20                                     # the clicks do not all end at one point
        # the vectorised pick is the serial loop (a few clicks: the loop is slow)
        a = lr.pick_serial(sp, clicks[[0, 3, 5, 7, 8, 12]]); b = lr.pick(sp, clicks[[0, 3, 5, 7, 8, 12]])
        assert all(np.array_equal(u, v, equal_nan=True) for u, v in zip(a[:3], b[:3]))


# ---- the end-to-end case: an image whose pose is off by 3 degrees and 10 cm ---------------------------------------------------------------
def spread_points(sp, usable, width, height):
    """8 visible points near 8 places spread over a width x height image, each with no other visible point within 1 pixel, all usable."""
    vis = np.nonzero(sp["visible"])[0]
    chosen = []
    for fx, fy in [(0.16, 0.2), (0.5, 0.17), (0.83, 0.22), (0.24, 0.5), (0.73, 0.53), (0.18, 0.83), (0.48, 0.8), (0.8, 0.78)]:
        order = vis[np.argsort(((sp["pxy"][vis] - F([fx * width, fy * height])) ** 2).sum(1))]
        for i in order[:3000]:
            d = np.sqrt(((sp["pxy"][vis] - sp["pxy"][i]).astype(np.float64) ** 2).sum(1))
            if (d < 1.0).sum() == 1 and usable[i] and int(i) not in chosen:
                chosen.append(int(i)); break
    assert len(chosen) == 8
    return chosen


@functools.lru_cache(maxsize=None)
def repair_case(model):
    """Image 0 of the scene at a wrong pose; 8 visible scan points spread over the image with no other visible point within 1 pixel (the click
    offsets stay below 0.3 px, so each click is nearer to its point than to any other);
    per point the click (its position under the wrong pose plus an offset below 0.3 px) and the pixel it belongs at (its position
    under the true pose) -> dict."""
    from oracle import binding as ob
    from oracle import reg_binding as rb
    S = mth.scene(model)
    true = S["images"][IMAGE]
    q_true = np.asarray(S["M"]["images"][IMAGE]["q_init"], F); t_true = np.asarray(S["M"]["images"][IMAGE]["t_init"], F)
    rng = np.random.RandomState(11)
    axis = np.array([0.5, -0.7, 0.5]); axis /= np.linalg.norm(axis)
    shift = np.array([0.06, -0.05, 0.0625]); shift *= 0.1 / np.linalg.norm(shift)
    R_true = lr.quat_to_R(q_true)
    q_wrong = lr.R_to_quat(_rotvec(np.deg2rad(3.0) * axis) @ R_true).astype(F)
    t_wrong = (t_true.astype(np.float64) + shift).astype(F)
    Rw = ob.quat_to_R(q_wrong)
    wrong = dict(R=Rw, t=t_wrong, cam=true["cam"], occlusion=rb.splat_depth(S["scan"], Rw, t_wrong, true["cam"], SPLAT_RADIUS))
    sp = lr.scan_points(S["scan"], wrong, OCCLUSION_THRESHOLD)
    sp_true = lr.scan_points(S["scan"], true, OCCLUSION_THRESHOLD)
    chosen = spread_points(sp, sp_true["state"] != lr.OUTSIDE, mth.WIDTH, mth.HEIGHT)
    chosen = np.array(chosen)
    clicks = (sp["pxy"][chosen] + rng.uniform(-0.2, 0.2, (8, 2)).astype(F)).astype(F)
    pixels = sp_true["pxy"][chosen]
    return dict(S=S, q_true=q_true, t_true=t_true, q_wrong=q_wrong, t_wrong=t_wrong, wrong=wrong, sp=sp, chosen=chosen, clicks=clicks,
                pixels=pixels, R_true=R_true)


def repair_bounds(C, bearings):
    """The pose error allowed after the repair: the exact-data bound of the solver test, widened by what the bearings are off.  The
    bearings come from f32 pixel positions through the bilinear undistortion lookup, so they miss the true directions by an angle e
    (returned; measured against the true camera-space directions of the chosen points).  With 8 points spread over the whole image a
    bearing error e turns the camera by about e and moves it by about e times the depth of the scene; 10 e and 10 e z_max are
    allowed."""
    x = C["S"]["scan"][C["chosen"]].astype(np.float64) @ C["R_true"].T + C["t_true"].astype(np.float64)
    d = x / np.linalg.norm(x, axis=1)[:, None]
    e = float(np.arctan2(np.linalg.norm(np.cross(bearings, d), axis=1), (bearings * d).sum(1)).max())
    t = np.linalg.norm(C["t_true"].astype(np.float64))
    return e, 1e-6 + 10 * e, 1e-6 * (1 + t) + 10 * e * float(x[:, 2].max())


def test_repair_case_on_the_cpu(e3d):
    """The end-to-end case with the restatement's pick and bearings and the library's (host-only) solver: the chosen points are picked,
    the pose returns to the truth.  The bearing errors e printed here are the figures of DESIGN.md section 18."""
    for model in (0, 2):
        C = repair_case(model)
        idx, px, d, n = lr.pick(C["sp"], C["clicks"])
        assert idx.tolist() == C["chosen"].tolist() and (d < 0.09).all()
        b = lr.bearings(C["S"]["images"][IMAGE]["cam"], C["pixels"])
        e, rot_bound, t_bound = repair_bounds(C, b)
        q, t, stats = e3d.pose_from_bearings(C["S"]["scan"][C["chosen"]].astype(np.float64), b, C["q_wrong"], C["t_wrong"])
        rot = lr.rotation_angle(lr.quat_to_R(q), C["R_true"]); dt = float(np.linalg.norm(t.astype(np.float64) - C["t_true"]))
        print("repair case, model %d: bearing error %.3g rad, rotation %.3g (bound %.3g), translation %.3g (bound %.3g)" % (model, e, rot, rot_bound, dt, t_bound))
        assert lr.rotation_angle(lr.quat_to_R(C["q_wrong"]), C["R_true"]) > 0.05 and e < 1e-4
        assert rot <= rot_bound and dt <= t_bound and stats[3]


# ---- bin/ImageLocalizer without a GPU ------------------------------------------------------------------------------------------------------
def _tool(*args):
    return subprocess.run([TOOL] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


def _write_state(d, poses, names, rigs=None):
    """poses: [(q, t)] -> <d>/state with image ids 10, 11, ... of one PINHOLE camera (id 7)."""
    os.makedirs(os.path.join(d, "state"), exist_ok=True)
    with open(os.path.join(d, "state", "cameras.txt"), "w") as f:
        f.write("# cameras\n7 PINHOLE 240 180 210 208 120.1 90.8\n")
    with open(os.path.join(d, "state", "images.txt"), "w") as f:
        f.write("# images\n")
        for i, ((q, t), name) in enumerate(zip(poses, names)):
            f.write("%d %s %s 7 %s\n\n" % (10 + i, " ".join("%.9g" % v for v in q), " ".join("%.9g" % v for v in t), name))
    if rigs is not None:
        json.dump(rigs, open(os.path.join(d, "state", "rigs.json"), "w"), indent=4)


def _read_images_txt(path):
    out = {}
    for line in open(path):
        v = line.split()
        if len(v) == 10 and not line.startswith("#"):
            out[int(v[0])] = (np.array(v[1:5], np.float64), np.array(v[5:8], np.float64), int(v[8]), v[9])
    return out


def _printed_pose(line):
    v = [float(x) for x in re.search(r"q (\S+) (\S+) (\S+) (\S+) t (\S+) (\S+) (\S+)", line).groups()]
    return np.array(v[:4]), np.array(v[4:])


def _script(d, text):
    path = os.path.join(d, "script.txt")
    open(path, "w").write(text)
    return path


def _base(d):
    return ["--image_base_path", os.path.join(d, "images"), "--state_path", os.path.join(d, "state"), "--output_folder_path", os.path.join(d, "out")]


def test_tool_is_built_and_refuses_what_it_cannot_run(tmp_path):
    subprocess.check_call(["make", "-s", "-C", os.path.join(os.path.dirname(BIN), "csrc", "host")])
    assert os.path.isfile(TOOL) and os.access(TOOL, os.X_OK)
    d = str(tmp_path)
    ident = (np.array([1.0, 0, 0, 0]), np.zeros(3))
    names = ["dslr/img_%d.png" % i for i in range(3)]
    _write_state(d, [ident] * 3, names)
    r = _tool()
    assert r.returncode != 0 and "Please specify all the required paths." in r.stderr
    r = _tool(*_base(d))
    assert r.returncode != 0 and "Please specify all the required paths." in r.stderr
    r = _tool(*_base(d), "--script", os.path.join(d, "none.txt"))
    assert r.returncode != 0 and "Cannot read the script" in r.stderr
    points = ["point %d %d 3 %d %d\n" % (k, k % 2, 10 * k, 7 * k) for k in range(6)]
    six, five = "".join(points), "".join(points[:5])
    for text, message in (("image %s\nturn 1 2 3\n" % names[0], "script.txt:2: unknown operation 'turn'"),
                          ("image %s\nmove 1 2 3\n" % names[0], "'move' takes 6 arguments, got 3"),
                          ("image %s\npick 1 2 3\n" % names[0], "'pick' takes 4 arguments, got 3"),
                          ("image %s\npoint 1 2 3 4 5 6\n" % names[0], "'point' takes 5 arguments, got 6"),
                          ("image %s\nsolve 1\n" % names[0], "'solve' takes 0 arguments, got 1"),
                          ("image\n", "'image' takes 1 arguments, got 0"),
                          ("# nothing yet\nmove 0 0 0 0 0 0\nimage %s\n" % names[0], "script.txt:2: 'move' before any 'image' line"),
                          ("image %s\nmove 0 0 x 0 0 0\n" % names[0], "'x' is not a finite number"),
                          ("image %s\nmove 0 0 nan 0 0 0\n" % names[0], "'nan' is not a finite number"),
                          ("image dslr/none.png\nmove 0 0 0 0 0 0\n", "dslr/none.png is not an image of the state"),
                          ("image %s\ndistribute_relative_pose\n" % names[0], "This image does not belong to a rig."),
                          ("image %s\n%ssolve\n" % (names[0], five), "script.txt:7: solve needs at least 6 correspondences, the list holds 5"),
                          ("image %s\n%simage %s\nsolve\n" % (names[0], six, names[1]), "solve needs at least 6 correspondences, the list holds 0")):
        r = _tool(*_base(d), "--script", _script(d, text), "--scan_alignment_path", os.path.join(d, "scans.mlp"))
        assert r.returncode != 0 and message in r.stderr, (text, r.stderr)
        assert "Loading point clouds" not in r.stdout
    # a pick or a solve needs the scans: said before anything is read
    r = _tool(*_base(d), "--script", _script(d, "image %s\n%ssolve\n" % (names[0], six)))
    assert r.returncode != 0 and "--scan_alignment_path" in r.stderr
    assert not os.path.exists(os.path.join(d, "out"))


# MoveImage in f32 against its f64 evaluation, on the poses the tool prints with nine digits.  Bounds from the rounding of the f32
# operations (eps = 2^-23): the quaternion product and its normalisation, the sine and cosine of the half angle: 16 eps of rotation;
# the translation R_delta t + V upsilon: 16 eps (|t| + |upsilon|), and 2 eps |upsilon| / theta on top for a rotation by theta: Sophus
# forms (1 - cos theta) / theta^2 in f32, where 1 - cos theta has an absolute error of eps / 2.  Measured maxima over the steps below:
# rotation 9.7e-8 rad (bound 1.9e-6), translation 0.033 of its bound.
MOVES = [(0.1, 0, 0, 0, 0, 0), (0, -0.25, 0, 0, 0, 0), (0, 0, 0.5, 0, 0, 0), (0.3, -0.2, 0.1, 0, 0, 0),
         (0, 0, 0, 0.02, 0, 0), (0, 0, 0, 0, -0.1, 0), (0, 0, 0, 0, 0, 0.5), (0, 0, 0, 0.3, -0.2, 0.25),
         (0.05, 0.02, -0.03, 0.01, 0.02, -0.015), (0.3, -0.4, 0.2, -0.35, 0.2, 0.28), (-0.5, 0.1, 0.4, 0.1, 0.45, -0.15),
         (0.2, 0.2, 0.2, 1e-6, 0, 0), (0.01, 0, 0, 0, 0, 0.004)]


def test_tool_move_image_against_f64(tmp_path):
    d = str(tmp_path)
    q0 = lr.R_to_quat(_rotvec([0.3, -0.5, 0.2])).astype(F); t0 = F([0.4, -1.2, 2.5])
    names = ["dslr/img_%d.png" % i for i in range(len(MOVES))]
    _write_state(d, [(q0, t0)] * len(MOVES), names)
    text = "".join("image %s\nmove %s   # step %d\n" % (n, " ".join("%.9g" % v for v in m), k) for k, (n, m) in enumerate(zip(names, MOVES)))
    r = _tool(*_base(d), "--script", _script(d, text))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Loading point clouds" not in r.stdout and "LoadImages" not in r.stdout        # no scans, no images, no device
    moved = [l for l in r.stdout.split("\n") if l.startswith("Moved image ")]
    assert len(moved) == len(MOVES)
    worst_rot = worst_t = 0.0
    for line, m in zip(moved, MOVES):
        q, t = _printed_pose(line)
        R, tt = lr.move(q0, t0, *[float(F(v)) for v in m])
        theta = float(np.linalg.norm(F(m[3:]))); ups = float(np.linalg.norm(F(m[:3])))
        t_bound = 16 * EPS * (float(np.linalg.norm(t0)) + ups) + (2 * EPS * ups / theta if theta > 0 else 0.0)
        rot = lr.rotation_angle(lr.quat_to_R(q), R); dt = float(np.linalg.norm(t - tt))
        worst_rot = max(worst_rot, rot); worst_t = max(worst_t, dt / t_bound)
        assert rot <= 16 * EPS and dt <= t_bound, (m, rot, dt, t_bound)
        assert abs(np.linalg.norm(q) - 1) < 4 * EPS
    print("MoveImage f32 vs f64: rotation %.3g rad (bound %.3g), translation %.3g of its bound" % (worst_rot, 16 * EPS, worst_t))
    # the state files carry the same poses with six digits, and the existing reader parses them
    st = _read_images_txt(os.path.join(d, "out", "images.txt"))
    assert sorted(st) == list(range(len(MOVES)))
    for k, line in enumerate(moved):
        q, t = _printed_pose(line)
        assert np.array_equal(st[k][0], [float("%.6g" % v) for v in q]) and np.array_equal(st[k][1], [float("%.6g" % v) for v in t])
        assert st[k][3] == names[k]
    cams = [l.split() for l in open(os.path.join(d, "out", "cameras.txt")) if not l.startswith("#")]
    assert cams == [["0", "PINHOLE", "240", "180", "210", "208", "120.1", "90.8"]]
    assert os.path.isfile(os.path.join(d, "out", "points3D.txt")) and not os.path.exists(os.path.join(d, "out", "rigs.json"))


def _rig_state(d, n_frames=3):
    """make_rig_scene's rig (two cameras) in n_frames image sets whose poses agree with the rig exactly (to the nine digits of the
    state file), so that AssignRigs leaves them where they are -> (poses by image id in f64, rig, frames, names)."""
    from reg_util import make_rig_scene
    M = make_rig_scene(n_points=50, n_frames=n_frames, seed=13)
    qr, tr = M["rig_true"][1]
    rel = (lr.quat_to_R(qr), np.asarray(tr, np.float64))
    poses = {}
    for f in range(n_frames):
        ref = (lr.quat_to_R(M["images"][2 * f]["q_true"]), np.asarray(M["images"][2 * f]["t_true"], np.float64))
        poses[2 * f] = ref
        poses[2 * f + 1] = lr._mul(rel, ref)
    names = ["cam%d/frame_%d.png" % (i % 2, i // 2) for i in range(2 * n_frames)]
    rigs = [{"ref_camera_id": 7, "cameras": [{"camera_id": 7, "image_prefix": "cam0"}, {"camera_id": 7, "image_prefix": "cam1"}]}]
    _write_state(d, [(lr.R_to_quat(poses[i][0]), poses[i][1]) for i in range(2 * n_frames)], names, rigs)
    return poses, [(np.eye(3), np.zeros(3)), rel], [[2 * f, 2 * f + 1] for f in range(n_frames)], names


# the tool's poses after move + distribute_relative_pose against the f64 evaluation: the state is read with nine digits, AssignRigs
# averages rig poses that agree to f32 rounding, every step is a handful of f32 pose products (<= 16 eps each, see above), and the
# output has six digits (5e-6 relative per value): 2e-5 rad and 2e-5 (1 + |t|) cover the chain with room to spare
@pytest.mark.parametrize("moved_camera", [1, 0])
def test_tool_distribute_relative_pose(tmp_path, moved_camera):
    d = str(tmp_path)
    poses, rig, frames, names = _rig_state(d)
    image_id = frames[1][moved_camera]
    step = (0.05, -0.02, 0.03, 0.02, -0.01, 0.015)
    r = _tool(*_base(d), "--script", _script(d, "image %s\nmove %s\ndistribute_relative_pose\n" % (names[image_id], " ".join("%.9g" % v for v in step))))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "AssignRigs(): assigned 6 out of 6 images to rig(s)" in r.stdout and "Loading point clouds" not in r.stdout
    want = dict(poses)
    want[image_id] = lr.move(lr.R_to_quat(poses[image_id][0]), poses[image_id][1], *step)
    want, new_rig = lr.distribute_relative_pose(want, rig, frames, image_id)
    st = _read_images_txt(os.path.join(d, "out", "images.txt"))
    assert sorted(st) == list(range(6))
    for i in range(6):
        assert lr.rotation_angle(lr.quat_to_R(st[i][0]), want[i][0]) <= 2e-5, i
        assert np.linalg.norm(st[i][1] - want[i][1]) <= 2e-5 * (1 + np.linalg.norm(want[i][1])), i
    # every image set is consistent with one relative pose afterwards, and it is the moved set's
    T = {i: (lr.quat_to_R(st[i][0]), st[i][1]) for i in st}
    rels = [lr._mul(T[f[1]], lr._inv(T[f[0]])) for f in frames]
    for rel in rels:
        assert lr.rotation_angle(rel[0], new_rig[1][0]) <= 4e-5 and np.linalg.norm(rel[1] - new_rig[1][1]) <= 4e-5
    assert lr.rotation_angle(new_rig[1][0], rig[1][0]) > 5e-3                       # the rig did change
    if moved_camera == 1:      # the reference images stay, the other sets' second images follow
        assert all(lr.rotation_angle(T[f[0]][0], poses[f[0]][0]) <= 2e-5 for f in frames)
        assert lr.rotation_angle(T[frames[0][1]][0], poses[frames[0][1]][0]) > 5e-3
    else:                      # the second images stay, the reference images are placed from them
        assert all(lr.rotation_angle(T[f[1]][0], poses[f[1]][0]) <= 2e-5 for f in frames)
        assert lr.rotation_angle(T[frames[0][0]][0], poses[frames[0][0]][0]) > 5e-3
    assert json.load(open(os.path.join(d, "out", "rigs.json"))) == [{"ref_camera_id": 0, "cameras": [{"camera_id": 0, "image_prefix": "cam0"}, {"camera_id": 0, "image_prefix": "cam1"}]}]


def test_restatement_distribute_relative_pose():
    """The f64 evaluation itself: both branches leave every set consistent; an image without a set is refused."""
    rng = np.random.RandomState(2)
    rel = (_rotvec([0.01, -0.04, 0.02]), np.array([-0.12, 0.01, 0.005]))
    frames = [[0, 1], [2, 3], [4, 5]]
    poses = {}
    for f in frames:
        poses[f[0]] = (_rotvec(rng.normal(size=3) * 0.3), rng.uniform(-1, 1, 3)); poses[f[1]] = lr._mul(rel, poses[f[0]])
    poses[9] = (np.eye(3), np.zeros(3))
    assert lr.distribute_relative_pose(poses, [None, rel], frames, 9) is None
    for image_id in (3, 2):
        moved = dict(poses); moved[image_id] = lr._mul((_rotvec([0.02, 0.01, -0.03]), np.array([0.05, 0, -0.02])), poses[image_id])
        new, rig = lr.distribute_relative_pose(moved, [(np.eye(3), np.zeros(3)), rel], frames, image_id)
        want = lr._mul(moved[3], lr._inv(moved[2]))
        for f in frames:
            got = lr._mul(new[f[1]], lr._inv(new[f[0]]))
            assert np.abs(got[0] - want[0]).max() < 1e-12 and np.abs(got[1] - want[1]).max() < 1e-12
        assert np.abs(rig[1][0] - want[0]).max() < 1e-12
        kept = 0 if image_id == 3 else 1                                               # the camera whose images stay where they are
        assert all(np.array_equal(new[f[kept]][0], moved[f[kept]][0]) for f in frames if f != [2, 3])
