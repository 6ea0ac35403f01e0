"""bin/ImageUndistorter on a dataset in tmp_path against the numpy restatement (tests/undistort_ref.py): images, masks and depth maps bit
for bit, calibration/ against the plans, and the output as the input of GroundTruthCreator."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import undistort_ref as ur
from cli_util import BIN, ROOT, write_mlp, write_ply_xyz
from test_oracle_camera import CAMERAS

sys.path.insert(0, ROOT)
from oracle import reg_binding as rb  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
TOOL = os.path.join(BIN, "ImageUndistorter")
W, H = 96, 64
# COLMAP camera id, model name, images; image poses: looking along +z at the scan
CAMS = [(7, "OPENCV", ["dslr/img_0.png", "dslr/img_1.png"]), (8, "THIN_PRISM_FISHEYE", ["fish/img_2.png"])]
POSES = [((1.0, 0.0, 0.0, 0.0), (0.0, 0.0, 0.0)), ((0.99875026, 0.0, 0.049979169, 0.0), (0.1, 0.0, 0.0)),
         ((0.99875026, 0.049979169, 0.0, 0.0), (0.0, -0.1, 0.05))]


def _png(path, img):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(np.ascontiguousarray(img, np.uint8)).save(path)


def _read(path):
    from PIL import Image
    return np.array(Image.open(path))


def _camera_text(cid, name, width, height):
    """-> (the cameras.txt line, the f32 pixel-centre parameters the tool derives from that text)"""
    t, p = CAMERAS[name]
    p = ur.scaled_params(p, t, width, height).astype(np.float64)
    p[2] += 0.5; p[3] += 0.5                                               # COLMAP's pixel-corner convention
    text = ["%.9g" % v for v in p]
    parsed = np.array([float(v) for v in text], np.float64).astype(F)
    parsed[2] += F(-0.5); parsed[3] += F(-0.5)
    return "%d %s %d %d %s\n" % (cid, name, width, height, " ".join(text)), t, parsed


def _dataset(d):
    """Two cameras, three images, one image mask, one camera mask, a depth map per image (one of them gzip, all with holes)."""
    rng = np.random.RandomState(11)
    os.makedirs(os.path.join(d, "state"), exist_ok=True)
    D = dict(cams={}, images={}, masks={}, cmasks={}, depth={}, poses={})
    with open(os.path.join(d, "state", "cameras.txt"), "w") as f:
        f.write("# cameras\n")
        for cid, name, _ in CAMS:
            line, t, params = _camera_text(cid, name, W, H)
            f.write(line)
            D["cams"][cid] = rb.make_camera(W, H, params, t)
    k = 0
    with open(os.path.join(d, "state", "images.txt"), "w") as f:
        f.write("# images\n")
        for cid, _, names in CAMS:
            for name in names:
                q, t = POSES[k]
                f.write("%d %s %s %d %s\n\n" % (20 + k, " ".join("%.9g" % v for v in q), " ".join("%.9g" % v for v in t), cid, name))
                yy, xx = np.mgrid[0:H, 0:W]
                img = np.stack([(xx * 2 + k * 40) % 256, (yy * 3 + xx) % 256, rng.randint(0, 256, (H, W))], 2).astype(np.uint8)
                _png(os.path.join(d, "images", name), img)
                depth = rng.uniform(1, 9, (H, W)).astype(F)
                depth[rng.rand(H, W) < 0.25] = 0; depth[5, 7] = np.inf
                path = os.path.join(d, "depth", name)
                os.makedirs(os.path.dirname(path), exist_ok=True)
                if k == 1:
                    with gzip.open(path + ".gz", "wb") as g:
                        g.write(depth.tobytes())
                else:
                    depth.tofile(path)
                D["images"][name] = (cid, img); D["depth"][name] = depth; D["poses"][name] = (q, t)
                k += 1
    mask = np.zeros((H, W), np.uint8); mask[10:30, 20:60] = 1; mask[40:50, 5:25] = 2
    _png(os.path.join(d, "images", "masks_for_images", "dslr", "img_0.png"), mask)
    D["masks"]["dslr/img_0.png"] = mask
    cmask = np.zeros((H, W), np.uint8); cmask[:, :6] = 1; cmask[H - 4:, :] = 1
    _png(os.path.join(d, "images", "masks_for_cameras", "fish.png"), cmask)
    D["cmasks"]["fish"] = (8, cmask)
    return D


def _run(d, out, extra=(), check=True):
    cmd = [TOOL, "--state_path", os.path.join(d, "state"), "--image_base_path", os.path.join(d, "images"), "--output_folder_path", out] + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if check:
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def _images_txt(path):
    out = []
    for line in open(path):
        v = line.split()
        if len(v) == 10 and not line.startswith("#"):
            out.append((int(v[0]), np.array(v[1:8], np.float64).astype(F), int(v[8]), v[9]))
    return out


def _files(root):
    return sorted(os.path.relpath(os.path.join(dp, f), root) for dp, _, fs in os.walk(root) for f in fs)


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("undistort"))
    return d, _dataset(d)


@pytest.mark.parametrize("blank", ["0", "1"])
def test_outputs_equal_the_restatement(dataset, blank):
    d, D = dataset
    out = os.path.join(d, "out_b" + blank)
    r = _run(d, out, ["--blank_pixels", blank, "--depth_maps_path", os.path.join(d, "depth"), "--compress_depth_maps", blank])
    plans = {cid: ur.plan(cam, float(blank)) for cid, cam in D["cams"].items()}
    pos = {cid: ur.source_positions(D["cams"][cid], plans[cid]) for cid in plans}
    assert _files(out) == sorted(
        ["calibration/cameras.txt", "calibration/images.txt", "calibration/points3D.txt", "images/masks_for_cameras/fish.png",
         "images/masks_for_images/dslr/img_0.png"] + ["images/" + n for n in D["images"]] +
        ["ground_truth_depth/" + n + (".gz" if blank == "1" else "") for n in D["images"]])
    for name, (cid, img) in D["images"].items():
        want, _ = ur.remap(ur.RGB, img, *pos[cid])
        assert np.array_equal(_read(os.path.join(out, "images", name)), want), name
        path = os.path.join(out, "ground_truth_depth", name)
        raw = gzip.open(path + ".gz").read() if blank == "1" else open(path, "rb").read()
        want, _ = ur.remap(ur.NEAREST, D["depth"][name], *pos[cid])
        assert np.array_equal(np.frombuffer(raw, np.uint32), want.view(np.uint32).ravel()), name
        assert (want == 0).sum() > 500 and np.isfinite(want[want != 0]).sum() > 2000
    want, _ = ur.remap(ur.MASK, D["masks"]["dslr/img_0.png"], *pos[7])
    assert np.array_equal(_read(os.path.join(out, "images", "masks_for_images", "dslr", "img_0.png")), want) and (want == 1).any() and (want == 2).any()
    want, _ = ur.remap(ur.MASK, D["cmasks"]["fish"][1], *pos[8])
    assert np.array_equal(_read(os.path.join(out, "images", "masks_for_cameras", "fish.png")), want)
    if blank == "1":
        assert (want == 3).any() and plans[7].width > W                     # blank pixels carry both flags
    # calibration: the plans in COLMAP's convention, cameras renumbered from 0 as ExportToColmap does; poses and names as they came
    lines = [ln.strip() for ln in open(os.path.join(out, "calibration", "cameras.txt")) if not ln.startswith("#")]
    assert lines == [ur.colmap_camera_line(i, plans[cid]) for i, (cid, _, _) in enumerate(CAMS)]
    got = _images_txt(os.path.join(out, "calibration", "images.txt"))
    assert [g[3] for g in got] == list(D["images"]) and [g[2] for g in got] == [0, 0, 1] and [g[0] for g in got] == [0, 1, 2]
    for g in got:
        q, t = D["poses"][g[3]]
        assert np.array_equal(g[1], np.array(list(q) + list(t), F))
    # one line per camera: old model and size -> new size and parameters
    for i, (cid, name, _) in enumerate(CAMS):
        assert "Camera %d: %s %d x %d -> PINHOLE %d x %d" % (i, name, W, H, plans[cid].width, plans[cid].height) in r.stdout


def test_output_is_a_dataset_for_ground_truth_creator(dataset, tmp_path):
    """The written model loads again as a state, with the written images below it: GroundTruthCreator's depth maps come out at the new
    sizes."""
    d, D = dataset
    out = os.path.join(d, "out_gt")
    _run(d, out)
    plans = {cid: ur.plan(cam, 0.0) for cid, cam in D["cams"].items()}
    rng = np.random.RandomState(3)
    pts = np.concatenate([rng.uniform(-2, 2, (4000, 2)), rng.uniform(2, 3, (4000, 1))], 1).astype(F)
    write_ply_xyz(os.path.join(d, "scan.ply"), pts, rgb=np.full((len(pts), 3), 128, np.uint8))
    write_mlp(os.path.join(d, "scans.mlp"), [("scan", "scan.ply", np.eye(4))])
    gt = str(tmp_path / "gt")
    r = subprocess.run([os.path.join(BIN, "GroundTruthCreator"), "--scan_alignment_path", os.path.join(d, "scans.mlp"), "--image_base_path",
                        os.path.join(out, "images"), "--state_path", os.path.join(out, "calibration"), "--output_folder_path", gt,
                        "--write_point_cloud", "0"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    for name, (cid, _) in D["images"].items():
        depth = np.fromfile(os.path.join(gt, "ground_truth_depth", name), F)
        assert depth.size == plans[cid].width * plans[cid].height


def test_jpeg_stays_jpeg_and_max_image_size(dataset, tmp_path):
    from PIL import Image
    d, D = dataset
    j = str(tmp_path / "jpeg")
    os.makedirs(os.path.join(j, "state")); os.makedirs(os.path.join(j, "images", "dslr"))
    line, t, params = _camera_text(7, "OPENCV", W, H)
    open(os.path.join(j, "state", "cameras.txt"), "w").write(line)
    with open(os.path.join(j, "state", "images.txt"), "w") as f:
        for k, name in enumerate(["dslr/a.jpg", "dslr/b.png"]):
            f.write("%d 1 0 0 0 0 0 0 7 %s\n\n" % (k, name))
            Image.fromarray(D["images"]["dslr/img_%d.png" % k][1]).save(os.path.join(j, "images", name), quality=95)
    out = str(tmp_path / "out")
    _run(j, out, ["--blank_pixels", "1", "--max_image_size", "50"])
    pl = ur.plan(rb.make_camera(W, H, params, t), 1.0, 50)
    assert max(pl.width, pl.height) <= 50
    raw = open(os.path.join(out, "images", "dslr", "a.jpg"), "rb").read()
    assert raw[:2] == b"\xff\xd8" and Image.open(os.path.join(out, "images", "dslr", "a.jpg")).size == (pl.width, pl.height)
    assert _read(os.path.join(out, "images", "dslr", "b.png")).shape == (pl.height, pl.width, 3)
    lines = [ln.strip() for ln in open(os.path.join(out, "calibration", "cameras.txt")) if not ln.startswith("#")]
    assert lines == [ur.colmap_camera_line(0, pl)]


def test_errors(dataset, tmp_path):
    d, D = dataset
    r = subprocess.run([TOOL, "--state_path", os.path.join(d, "state")], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "required paths" in r.stderr
    r = _run(d, str(tmp_path / "o1"), ["--blank_pixels", "1.5"], check=False)
    assert r.returncode != 0 and "blank_pixels" in r.stderr
    r = _run(d, str(tmp_path / "o1"), ["--blank_pixels", "o.5"], check=False)           # a typo is not 0
    assert r.returncode != 0 and "not a number" in r.stderr and not os.path.exists(str(tmp_path / "o1"))
    # a missing image
    m = str(tmp_path / "missing")
    os.makedirs(os.path.join(m, "state")); os.makedirs(os.path.join(m, "images", "dslr"))
    open(os.path.join(m, "state", "cameras.txt"), "w").write(_camera_text(7, "OPENCV", W, H)[0])
    open(os.path.join(m, "state", "images.txt"), "w").write("0 1 0 0 0 0 0 0 7 dslr/img_0.png\n\n1 1 0 0 0 0 0 0 7 dslr/gone.png\n\n")
    _png(os.path.join(m, "images", "dslr", "img_0.png"), D["images"]["dslr/img_0.png"][1])
    r = _run(m, str(tmp_path / "o2"), check=False)
    assert r.returncode != 0 and "Cannot read image" in r.stderr and "gone.png" in r.stderr
    # an image of another size than its camera
    _png(os.path.join(m, "images", "dslr", "gone.png"), np.zeros((H, W + 1, 3), np.uint8))
    r = _run(m, str(tmp_path / "o3"), check=False)
    assert r.returncode != 0 and "size differs" in r.stderr
    # an output folder that cannot be written: its parent is a file
    blocker = tmp_path / "file"
    blocker.write_text("x")
    r = _run(d, str(blocker / "out"), check=False)
    assert r.returncode != 0 and "annot write" in r.stderr
    # depth maps asked for, none there
    r = _run(d, str(tmp_path / "o4"), ["--depth_maps_path", str(tmp_path / "nowhere")], check=False)
    assert r.returncode != 0 and "depth map" in r.stderr
