"""Depth maps from files, the parts that need no GPU: ImageRegistrator's early argument checks (they come before the library is
loaded) and the reader of GroundTruthCreator's map format (csrc/host/io_depth.h) through the e3d_read_depth helper."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from cli_util import BIN

OLD_MESSAGE = ("--depth_residuals_weight > 0: the tool has no way to load depth maps (nor has the reference's: only "
               "Problem::SetFixedDepthMaps / e3d_reg_set_depth_maps feed them).")


def _registrator(tmp, extra):
    """Every required path is given (none needs to exist: the checks under test come first)."""
    d = str(tmp)
    cmd = [os.path.join(BIN, "ImageRegistrator"), "--scan_alignment_path", os.path.join(d, "scans.mlp"), "--multi_res_point_cloud_directory_path",
           os.path.join(d, "cache"), "--image_base_path", os.path.join(d, "images"), "--state_path", os.path.join(d, "state"),
           "--output_folder_path", os.path.join(d, "out"), "--observations_cache_path", os.path.join(d, "obs_cache")] + list(extra)
    return subprocess.run(cmd, capture_output=True, text=True, timeout=60)


def test_weight_without_a_path_keeps_its_message(tmp_path):
    r = _registrator(tmp_path, ["--depth_residuals_weight", "1"])
    assert r.returncode == 1 and r.stderr.strip() == OLD_MESSAGE
    assert not os.path.exists(os.path.join(str(tmp_path), "out"))


@pytest.mark.parametrize("value", ["lenient", "STRICT", "1"])
def test_bad_hole_mode_fails_before_anything_is_loaded(tmp_path, value):
    os.makedirs(os.path.join(str(tmp_path), "depth"))
    r = _registrator(tmp_path, ["--depth_residuals_weight", "1", "--depth_maps_path", os.path.join(str(tmp_path), "depth"), "--depth_hole_mode", value])
    assert r.returncode == 1 and r.stderr.strip() == "--depth_hole_mode %s: expected average or strict." % value
    assert "Loading point clouds" not in r.stdout and not os.path.exists(os.path.join(str(tmp_path), "out"))


@pytest.mark.parametrize("weight", ["1", "0"])
def test_depth_maps_path_must_be_a_directory(tmp_path, weight):
    d = str(tmp_path)
    open(os.path.join(d, "a_file"), "wb").write(b"x")
    for path in (os.path.join(d, "missing"), os.path.join(d, "a_file")):
        r = _registrator(tmp_path, ["--depth_residuals_weight", weight, "--depth_maps_path", path, "--depth_hole_mode", "average"])
        assert r.returncode == 1 and r.stderr.strip() == "--depth_maps_path %s is not a directory." % path
        assert "Loading point clouds" not in r.stdout and not os.path.exists(os.path.join(d, "out"))


# ---- the reader ----------------------------------------------------------------------------------------------------------------------
W, H = 37, 21


def _read(tmp, depth_dir, image_path, w=W, h=H):
    out = os.path.join(str(tmp), "out.raw")
    if os.path.exists(out):
        os.remove(out)
    r = subprocess.run([os.path.join(BIN, "e3d_read_depth"), depth_dir, image_path, str(w), str(h), out], capture_output=True, text=True, timeout=60)
    return r, (np.fromfile(out, np.float32) if r.returncode == 0 else None)


@pytest.fixture()
def maps(tmp_path):
    """<dir>/dslr/a.png raw, <dir>/dslr/b.png.gz compressed, both the same map with the values a ground-truth map holds (+inf holes)."""
    rng = np.random.RandomState(3)
    m = rng.uniform(0.5, 20.0, (H, W)).astype(np.float32)
    m[rng.uniform(size=m.shape) < 0.3] = np.inf
    m[0, 0] = np.nan; m[0, 1] = -0.0
    d = os.path.join(str(tmp_path), "ground_truth_depth")
    os.makedirs(os.path.join(d, "dslr"))
    m.tofile(os.path.join(d, "dslr", "a.png"))
    with gzip.open(os.path.join(d, "dslr", "b.png.gz"), "wb") as f:
        f.write(m.tobytes())
    return d, m


def test_raw_and_gzip_maps_read_identically(tmp_path, maps):
    d, m = maps
    for name in ("a.png", "b.png"):
        # <dir>/<filename(parent(file_path))>/<filename(file_path)>: only the last two components of the image path count
        r, got = _read(tmp_path, d, "/somewhere/else/images/dslr/" + name)
        assert r.returncode == 0, r.stderr
        assert np.array_equal(got.view(np.uint32), m.ravel().view(np.uint32))            # bit for bit, NaN and -0 included
    # the raw file wins where both exist, and a trailing slash of the directory does not matter
    np.zeros((H, W), np.float32).tofile(os.path.join(d, "dslr", "b.png"))
    r, got = _read(tmp_path, d + "/", "dslr/b.png")
    assert r.returncode == 0 and not got.any()


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("delta", [-4, -1, 1, 4096])
def test_wrong_payload_size_is_refused(tmp_path, maps, packed, delta):
    d, m = maps
    want = 4 * W * H
    payload = (m.tobytes() + b"\0" * 5000)[:want + delta]
    path = os.path.join(d, "dslr", "c.png" + (".gz" if packed else ""))
    if packed:
        with gzip.open(path, "wb") as f:
            f.write(payload)
    else:
        open(path, "wb").write(payload)
    r, _ = _read(tmp_path, d, "images/dslr/c.png")
    assert r.returncode != 0
    assert r.stderr.strip() == "Depth map %s holds %d bytes, expected %d (%d x %d f32)" % (path, want + delta, want, W, H)


def test_a_gzip_stream_that_ends_early_is_refused(tmp_path, maps):
    d, m = maps
    blob = open(os.path.join(d, "dslr", "b.png.gz"), "rb").read()
    path = os.path.join(d, "dslr", "e.png.gz")
    open(path, "wb").write(blob[:len(blob) // 2])
    r, _ = _read(tmp_path, d, "images/dslr/e.png")
    assert r.returncode != 0 and r.stderr.startswith("Depth map %s holds " % path) and "expected %d (%d x %d f32)" % (4 * W * H, W, H) in r.stderr


def test_missing_map_names_both_candidates(tmp_path, maps):
    d, _ = maps
    r, _ = _read(tmp_path, d, "images/dslr/nope.png")
    base = os.path.join(d, "dslr", "nope.png")
    assert r.returncode != 0 and r.stderr.strip() == "Cannot find a depth map: tried %s and %s.gz" % (base, base)
    r, _ = _read(tmp_path, d, "images/other_camera/a.png")                                   # the camera folder is part of the place
    assert r.returncode != 0 and "tried %s " % os.path.join(d, "other_camera", "a.png") in r.stderr
