"""ImageRegistrator --write_debug_point_clouds (src/exe/image_registrator.cc:200-215, :286-295): the scans coloured by the images, once
at the initial state and once after every image scale.  The initial cloud must equal, bit for bit, what e3d_reg_scan_colors_* gives
through the Python binding for the same state and Pillow's decoding of the same image files."""
import glob
import os
import shutil
import subprocess

import numpy as np
import pytest

from cli_util import BIN
from reg_util import make_multi_image_scene, pyramid_u8
from test_gpu_cli_reg import _write_dataset

pytestmark = pytest.mark.gpu

NAMES = ["dslr/img_0.png", "dslr/img_1.jpg", "dslr/img_2.png"]


def _colour_version(grey):
    """A colour image that keeps the texture (so that the registration has something to align) with three different channels, all
    dark enough that no grey conversion of it -- nor a JPEG's ringing -- comes near maximum_valid_intensity (252)."""
    yy, xx = np.mgrid[0:grey.shape[0], 0:grey.shape[1]]
    base = grey.astype(np.int32) * 230 // 250
    return np.stack([base + 20, base + 5, (xx * 3 + yy * 5) % 240], -1).astype(np.uint8)


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from PIL import Image
    M = make_multi_image_scene(n_points=6000, n_images=3, seed=12, perturb=0.006)
    # a few points off the wall: behind the cameras and outside the images
    M = dict(M, pts=np.concatenate([M["pts"], np.random.RandomState(3).uniform(-4, 4, (300, 3)).astype(np.float32)]))
    full = M["pts"]
    M_cache = dict(M, pts=full[:6000])                       # the multi-resolution cloud: the wall alone (its neighbour graph stays valid)
    d = _write_dataset(tmp_path_factory.mktemp("debug_cloud"), M_cache, NAMES)
    from cli_util import write_ply_xyz
    write_ply_xyz(os.path.join(d, "scan.ply"), full, rgb=np.full((len(full), 3), 128, np.uint8))
    for im, name in zip(M["images"], NAMES):
        col = _colour_version(im["pyr"][0])
        path = os.path.join(d, "images", name)
        if name.endswith(".jpg"):
            Image.fromarray(col, "RGB").save(path, "JPEG", quality=90, subsampling=2)
        else:
            Image.fromarray(col, "RGB").save(path)
    return d, M


def _run(d, out, extra=(), images="images"):
    cmd = [os.path.join(BIN, "ImageRegistrator"), "--scan_alignment_path", os.path.join(d, "scans.mlp"), "--multi_res_point_cloud_directory_path",
           os.path.join(d, "cache"), "--image_base_path", os.path.join(d, images), "--state_path", os.path.join(d, "state"),
           "--output_folder_path", os.path.join(d, out), "--observations_cache_path", os.path.join(d, out + "_obs_cache"),
           "--max_iterations", "2", "--max_initial_image_area_in_pixels", "3000"] + list(extra)
    return subprocess.run(cmd, capture_output=True, text=True, timeout=600)


def _read_xyzrgb(path):
    """pcl::io::savePLYFileBinary of a PointXYZRGB cloud: 15 bytes per vertex, then PCL's camera element."""
    raw = open(path, "rb").read()
    h = raw.index(b"end_header\n") + 11
    header = raw[:h].decode()
    n = int(header.split("element vertex ")[1].split()[0])
    assert "format binary_little_endian 1.0" in header and "comment PCL generated" in header and "element camera 1" in header
    assert "property float x\nproperty float y\nproperty float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n" in header
    assert len(raw) - h - 15 * n == 4 * 12 + 4 * 5 + 4 * 2 + 4 * 2
    rec = np.frombuffer(raw, dtype=[("p", "<f4", 3), ("c", "u1", 3)], count=n, offset=h)
    return rec["p"].copy(), rec["c"].copy()


def _clouds(out_dir):
    return sorted(os.path.basename(p) for p in glob.glob(os.path.join(out_dir, "*point_cloud*")))


def test_debug_point_clouds_written_and_initial_cloud_matches_binding(dataset, e3d):
    from PIL import Image
    d, M = dataset
    r = _run(d, "out_on", ["--write_debug_point_clouds", "1"])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = os.path.join(d, "out_on")
    states = sorted(os.path.basename(p) for p in glob.glob(os.path.join(out, "scale_*_state")))
    assert states == ["scale_0.5_state", "scale_1_state"]
    assert _clouds(out) == sorted(["initial_point_cloud.ply"] + [s[:-len("_state")] + "_final_point_cloud.ply" for s in states])
    lines = r.stdout.splitlines()
    assert lines.count("Writing initial point cloud ...") == 1 and lines.count("Wrote initial_point_cloud.ply") == 1
    assert lines.count("Writing point cloud ...") == 2
    assert "Wrote scale_0.5_final_point_cloud.ply" in lines and "Wrote scale_1_final_point_cloud.ply" in lines
    first = lambda text: next(k for k, l in enumerate(lines) if text in l)
    assert first("Wrote initial_point_cloud.ply") < first("--- Optimizing at scaling factor 0.5 ---") < first("Wrote state to")
    assert first("Wrote state to") < first("Wrote scale_0.5_final_point_cloud.ply") < first("--- Optimizing at scaling factor 1 ---")
    # the same colouring through the binding: the state the tool read (poses of the input model, %.9g text is exact for f32), the
    # files as Pillow decodes them.  No grey value is near maximum_valid_intensity, so the grey conversion plays no part.
    G = e3d.RegProblem(e3d.default_reg_params(image_scale_count=3, current_image_scale=0))
    G.set_intrinsics(0, M["width"], M["height"], M["params"], 0, 3)
    G.set_splat_points(M["pts"])
    colours = []
    for i, (im, name) in enumerate(zip(M["images"], NAMES)):
        col = np.array(Image.open(os.path.join(d, "images", name)).convert("RGB"))
        grey = ((col[..., 0].astype(np.int64) * 4899 + col[..., 1].astype(np.int64) * 9617 + col[..., 2].astype(np.int64) * 1868 + 8192) >> 14).astype(np.uint8)
        assert grey.max() <= 250
        G.set_image(i, 0, pyramid_u8(grey, 3)); G.set_image_pose(i, im["q_init"], im["t_init"])
        colours.append(col)
    G.set_scan_points(M["pts"])
    G.scan_colors_begin()
    for i, col in enumerate(colours):
        G.scan_colors_add_image(i, col)
    expected = G.scan_colors_finish()
    xyz, rgb = _read_xyzrgb(os.path.join(out, "initial_point_cloud.ply"))
    assert np.array_equal(xyz.view(np.uint32), M["pts"].view(np.uint32))          # all scan points, input order, the same bits
    assert np.array_equal(rgb, expected)
    assert (rgb.max(1) > 0).mean() >= 0.25
    assert len(np.unique(rgb[rgb.max(1) > 0], axis=0)) > 100 and (rgb[:, 0] != rgb[:, 2]).any()
    # the final clouds: the poses that made them are only known as text with fewer digits -- shape, points and coverage
    for s in states:
        fxyz, frgb = _read_xyzrgb(os.path.join(out, s[:-len("_state")] + "_final_point_cloud.ply"))
        assert np.array_equal(fxyz.view(np.uint32), M["pts"].view(np.uint32)) and frgb.shape == (len(M["pts"]), 3)
        assert (frgb.max(1) > 0).mean() >= 0.25


@pytest.mark.parametrize("extra", [[], ["--write_debug_point_clouds", "0"]])
def test_no_debug_point_clouds_without_the_flag(dataset, extra):
    d, _ = dataset
    out = "out_off_%d" % len(extra)
    r = _run(d, out, extra)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert os.path.isdir(os.path.join(d, out, "scale_1_state")) and _clouds(os.path.join(d, out)) == []
    assert "Writing initial point cloud ..." not in r.stdout and "Writing point cloud ..." not in r.stdout


def test_existing_initial_point_cloud_is_kept(dataset):
    d, _ = dataset
    out = os.path.join(d, "out_keep")
    os.makedirs(out)
    sentinel = b"sentinel, not a point cloud\n"
    open(os.path.join(out, "initial_point_cloud.ply"), "wb").write(sentinel)
    r = _run(d, "out_keep", ["--write_debug_point_clouds", "1"])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert open(os.path.join(out, "initial_point_cloud.ply"), "rb").read() == sentinel
    assert "Not writing initial point cloud since initial_point_cloud.ply already exists." in r.stdout.splitlines()
    assert "Writing initial point cloud ..." not in r.stdout
    assert os.path.isfile(os.path.join(out, "scale_1_final_point_cloud.ply"))


def test_unreadable_image_file_fails(dataset):
    d, _ = dataset
    bad = os.path.join(d, "images_bad")
    shutil.copytree(os.path.join(d, "images"), bad)
    open(os.path.join(bad, NAMES[2]), "wb").write(b"not an image")
    r = _run(d, "out_bad", ["--write_debug_point_clouds", "1"], images="images_bad")
    assert r.returncode == 1 and "Cannot read image:" in r.stderr
    assert _clouds(os.path.join(d, "out_bad")) == []
