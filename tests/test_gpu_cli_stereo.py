"""bin/StereoPairCreator on a dataset in tmp_path against the numpy restatement (tests/stereo_ref.py): the rectified images and the mask
bit for bit, calib.txt / cameras.txt / images.txt against the plan, disp0GT.pfm against the restatement's disparities, and the ways the
pairs are given."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import stereo_ref as sr
import undistort_ref as ur
from cli_util import BIN, ROOT, write_mlp, write_ply_xyz
from test_oracle_camera import CAMERAS

sys.path.insert(0, ROOT)
from oracle import reg_binding as rb  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
TOOL = os.path.join(BIN, "StereoPairCreator")
W, H = 96, 64
CAMS = [(7, "OPENCV", "left"), (8, "THIN_PRISM_FISHEYE", "right")]       # COLMAP camera id, model, image folder = rig camera prefix
FRAMES = ["f0.png", "f1.png"]


def _rot(axis, degrees):
    a = math.radians(degrees); c, s = math.cos(a), math.sin(a)
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]),
            "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])}[axis]


def _pose(R, Cc):
    q = np.array(sr.rotation_quat([float(v) for v in np.asarray(R, np.float64).reshape(9)]), F)
    return q, (-np.asarray(R, np.float64) @ np.asarray(Cc, np.float64)).astype(F)


# the cameras look along +z at the scan; f2 exists in the state only: the left camera of frame 0 turned on the spot (no baseline)
POSES = {"left/f0.png": _pose(np.eye(3), (0, 0, 0)), "right/f0.png": _pose(_rot("y", -3), (0.3, 0.01, 0)),
         "left/f1.png": _pose(_rot("x", 2), (0.05, -0.1, 0.1)), "right/f1.png": _pose(_rot("y", -2) @ _rot("z", 1), (0.36, -0.09, 0.1)),
         "left/f2.png": _pose(_rot("y", 5), (0, 0, 0))}


def _png(path, img):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(np.ascontiguousarray(img, np.uint8)).save(path)


def _read(path):
    from PIL import Image
    return np.array(Image.open(path))


def _camera_text(cid, name, width, height):
    """-> (the cameras.txt line, the model's type, the f32 pixel-centre parameters the tool derives from that text)"""
    t, p = CAMERAS[name]
    p = ur.scaled_params(p, t, width, height).astype(np.float64)
    p[2] += 0.5; p[3] += 0.5                                               # COLMAP's pixel-corner convention
    text = ["%.9g" % v for v in p]
    parsed = np.array([float(v) for v in text], np.float64).astype(F)
    parsed[2] += F(-0.5); parsed[3] += F(-0.5)
    return "%d %s %d %d %s\n" % (cid, name, width, height, " ".join(text)), t, parsed


def _dataset(d):
    rng = np.random.RandomState(21)
    os.makedirs(os.path.join(d, "state"), exist_ok=True)
    D = dict(cams={}, images={}, masks={})
    with open(os.path.join(d, "state", "cameras.txt"), "w") as f:
        f.write("# cameras\n")
        for cid, name, folder in CAMS:
            line, t, params = _camera_text(cid, name, W, H)
            f.write(line)
            D["cams"][folder] = rb.make_camera(W, H, params, t)
    with open(os.path.join(d, "state", "images.txt"), "w") as f:
        f.write("# images\n")
        for k, (name, (q, t)) in enumerate(POSES.items()):
            cid = 7 if name.startswith("left") else 8
            f.write("%d %s %s %d %s\n\n" % (30 + k, " ".join("%.9g" % v for v in q), " ".join("%.9g" % v for v in t), cid, name))
            if name.endswith("f2.png"):
                continue
            yy, xx = np.mgrid[0:H, 0:W]
            img = np.stack([(xx * 2 + k * 40) % 256, (yy * 3 + xx) % 256, rng.randint(0, 256, (H, W))], 2).astype(np.uint8)
            _png(os.path.join(d, "images", name), img)
            D["images"][name] = img
    json.dump([{"ref_camera_id": 7, "cameras": [{"camera_id": 7, "image_prefix": "left"}, {"camera_id": 8, "image_prefix": "right"}]}],
              open(os.path.join(d, "state", "rigs.json"), "w"), indent=4)
    mask = np.zeros((H, W), np.uint8); mask[20:40, 30:55] = 2; mask[45:55, 5:25] = 1          # a kEvalObs block and a kObs block
    _png(os.path.join(d, "images", "masks_for_images", "left", "f0.png"), mask)
    D["masks"]["left/f0.png"] = mask
    # the scan: a wall at z = 3, an occluder in front of part of it, clutter all around
    wall = np.concatenate([rng.uniform(-2.5, 2.5, (30000, 2)), rng.uniform(2.98, 3.02, (30000, 1))], 1)
    bx, by = np.meshgrid(np.arange(-0.2, 0.4, 0.01), np.arange(-0.3, 0.3, 0.01))
    blocker = np.stack([bx.ravel(), by.ravel(), np.full(bx.size, 1.5)], 1)
    D["scan"] = np.concatenate([wall, blocker, rng.uniform(-4, 4, (2000, 3))]).astype(F)
    write_ply_xyz(os.path.join(d, "scan.ply"), D["scan"])
    write_mlp(os.path.join(d, "scans.mlp"), [("scan", "scan.ply", np.eye(4))])
    return D


def _run(d, out, extra=(), check=True):
    cmd = [TOOL, "--state_path", os.path.join(d, "state"), "--image_base_path", os.path.join(d, "images"), "--output_folder_path", out] + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if check:
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def _files(root):
    return sorted(os.path.relpath(os.path.join(dp, f), root) for dp, _, fs in os.walk(root) for f in fs)


def _expected(D, frame, blank=0.0, scans=True):
    """The restatement of one pair of the rig: plan, images, exclusion maps, ground truth."""
    names = ("left/" + frame, "right/" + frame)
    cams = (D["cams"]["left"], D["cams"]["right"])
    pl = sr.plan(cams, (POSES[names[0]], POSES[names[1]]), blank)
    E = dict(plan=pl, images=[], excluded=[])
    for cam, name, S in zip(cams, names, (pl.S_left, pl.S_right)):
        sx, sy = sr.source_positions(cam, pl.camera, S)
        img, valid = ur.remap(ur.RGB, D["images"][name], sx, sy)
        excluded = (valid == 0)
        if name in D["masks"]:
            excluded |= (ur.remap(ur.MASK, D["masks"][name], sx, sy)[0] & 2) != 0
        E["images"].append(img); E["excluded"].append(excluded.astype(np.uint8))
    if scans:
        c = pl.camera
        rect = rb.make_camera(c.width, c.height, np.array([c.fx, c.fy, c.cx, c.cy], F), rb.PINHOLE)
        E["disparity"], E["mask"], _, _ = sr.ground_truth(D["scan"], D["scan"], 0.03, rect, pl.q_rect, pl.t_left, pl.t_right, E["excluded"][0], E["excluded"][1])
    return E


def _check_pair(folder, E, scans=True):
    pl = E["plan"]
    assert np.array_equal(_read(os.path.join(folder, "im0.png")), E["images"][0])
    assert np.array_equal(_read(os.path.join(folder, "im1.png")), E["images"][1])
    assert open(os.path.join(folder, "calib.txt")).read() == sr.calib_text(pl)
    c = sr.parse_calib(open(os.path.join(folder, "calib.txt")).read())
    assert F(c["cam0"][0, 0]) == pl.camera.fx and F(c["cam0"][0, 2]) == pl.camera.cx and F(c["cam1"][1, 2]) == pl.camera.cy
    assert F(c["baseline"]) == pl.baseline and c["doffs"] == 0 and (c["width"], c["height"]) == (pl.camera.width, pl.camera.height)
    lines = [ln.strip() for ln in open(os.path.join(folder, "cameras.txt")) if not ln.startswith("#")]
    assert lines == [ur.colmap_camera_line(0, pl.camera)]
    lines = [ln.rstrip("\n") for ln in open(os.path.join(folder, "images.txt")) if not ln.startswith("#")]
    assert lines == sr.colmap_image_lines(pl, ("im0.png", "im1.png"))
    got = [ln.split() for ln in lines if ln]
    for g, t in zip(got, (pl.t_left, pl.t_right)):                           # nine digits carry the f32 poses
        assert np.array_equal(np.array(g[1:8], np.float64).astype(F), np.concatenate([pl.q_rect, t]))
    if scans:
        assert np.array_equal(_read(os.path.join(folder, "mask0nocc.png")), E["mask"])
        assert np.array_equal(sr.read_pfm(os.path.join(folder, "disp0GT.pfm")).view(np.uint32), E["disparity"].view(np.uint32))


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("stereo"))
    D = _dataset(d)
    out = os.path.join(d, "out_rig")
    r = _run(d, out, ["--camera_pair", "7,8", "--scan_alignment_path", os.path.join(d, "scans.mlp")])
    return d, D, out, r


def test_camera_pair_outputs_equal_the_restatement(dataset):
    d, D, out, r = dataset
    per_pair = ["calib.txt", "cameras.txt", "disp0GT.pfm", "im0.png", "im1.png", "images.txt", "mask0nocc.png"]
    assert _files(out) == sorted(stem + "/" + f for stem in ("f0", "f1") for f in per_pair)
    assert "swapped" not in r.stdout
    for frame in FRAMES:
        E = _expected(D, frame)
        _check_pair(os.path.join(out, frame[:-4]), E)
        for value in (255, 128, 0):
            assert (E["mask"] == value).sum() >= 50, (frame, value)
        assert "Pair %s: PINHOLE %d x %d" % (frame[:-4], E["plan"].camera.width, E["plan"].camera.height) in r.stdout
    # the kEvalObs block of the left image's mask leaves no ground truth; its kObs block does not matter
    E = _expected(D, "f0.png")
    free = dict(D, masks={})
    assert (E["mask"] == 0).sum() > (_expected(free, "f0.png")["mask"] == 0).sum() + 100


def test_pairs_file_right_then_left_is_swapped(dataset, tmp_path):
    d, D, out, _ = dataset
    pairs = tmp_path / "pairs.txt"
    pairs.write_text("# right-then-left, and a pair with a name of its own\nright/f0.png left/f0.png\nleft/f1.png right/f1.png second   # trailing comment\n\n")
    o = str(tmp_path / "out")
    r = _run(d, o, ["--pairs", str(pairs), "--scan_alignment_path", os.path.join(d, "scans.mlp")])
    assert "Pair f0: given right-then-left, swapped." in r.stdout and r.stdout.count("swapped") == 1
    assert _files(o) == [f.replace("f1/", "second/") for f in _files(out)]
    for a, b in (("f0", "f0"), ("f1", "second")):
        for f in os.listdir(os.path.join(out, a)):
            assert open(os.path.join(out, a, f), "rb").read() == open(os.path.join(o, b, f), "rb").read(), (a, f)


def test_a_pair_without_baseline_ends_the_run_before_anything_is_written(dataset, tmp_path):
    d, D, out, _ = dataset
    pairs = tmp_path / "pairs.txt"
    pairs.write_text("left/f0.png right/f0.png\nleft/f0.png left/f2.png turned\n")
    o = str(tmp_path / "out")
    r = _run(d, o, ["--pairs", str(pairs)], check=False)
    assert r.returncode != 0 and "baseline" in r.stderr and "f2.png" in r.stderr and not os.path.exists(o)
    r = _run(d, o, [], check=False)                                          # no pairs at all
    assert r.returncode != 0 and "--pairs" in r.stderr and not os.path.exists(o)
    pairs.write_text("left/f0.png right/nowhere.png\n")
    r = _run(d, o, ["--pairs", str(pairs)], check=False)
    assert r.returncode != 0 and "nowhere.png" in r.stderr and not os.path.exists(o)


def test_without_scans_only_images_and_calibration(dataset, tmp_path):
    d, D, out, _ = dataset
    o = str(tmp_path / "out")
    _run(d, o, ["--camera_pair", "7,8", "--blank_pixels", "1"])
    assert _files(o) == sorted(stem + "/" + f for stem in ("f0", "f1") for f in ["calib.txt", "cameras.txt", "im0.png", "im1.png", "images.txt"])
    E = _expected(D, "f1.png", 1.0, scans=False)
    _check_pair(os.path.join(o, "f1"), E, scans=False)
    assert E["excluded"][0].any() and E["plan"].camera.width > _expected(D, "f1.png", scans=False)["plan"].camera.width
