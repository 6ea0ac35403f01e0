"""How the tools that read the scans of a MeshLab project refuse a project they cannot use, without a GPU: every case ends before the
first call of the library.  The five tools share the per-scan loader (csrc/host/scan_loader.h) and differ on purpose in what surrounds
it -- whether a project without meshes is refused, which messages an unreadable project or scan gets, and when "Done." is printed; this
file pins those differences."""
import os
import subprocess

import numpy as np
import pytest

import test_localize_host as lh
import test_mask_transfer_host as mth
from cli_util import BIN, read_ply_normals, write_mlp

LOADING, DONE = "Loading point clouds ...", "Done."
CANNOT_LOAD, CANNOT_READ_POSES, EMPTY = "Cannot load scan point clouds.", "Cannot read scan poses from", "Point cloud is empty."
NAMES = ["dslr/img_%d.png" % i for i in range(3)]


@pytest.fixture(scope="module", autouse=True)
def _build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(os.path.dirname(BIN), "csrc", "host")])


def _run(tool, *args):
    return subprocess.run([os.path.join(BIN, tool)] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


def _ground_truth_creator(d, project):
    return _run("GroundTruthCreator", "--scan_alignment_path", project, "--image_base_path", os.path.join(d, "images"),
                "--state_path", os.path.join(d, "state"), "--output_folder_path", os.path.join(d, "gt_out"))


def _image_registrator(d, project):
    return _run("ImageRegistrator", "--scan_alignment_path", project, "--image_base_path", os.path.join(d, "images"),
                "--state_path", os.path.join(d, "state"), "--output_folder_path", os.path.join(d, "reg_out"),
                "--multi_res_point_cloud_directory_path", os.path.join(d, "multi_res"), "--observations_cache_path", os.path.join(d, "cache"))


def _normal_estimator(d, project):
    return _run("NormalEstimator", "-i", project, "-o", os.path.join(d, "normals.ply"))


def _mask_transfer(d, project):
    """A state MaskTransfer accepts (the one of test_mask_transfer_host.py) and a source mask of the camera's size: the scans come next."""
    from PIL import Image
    mth._write_state(d, NAMES)
    mask = os.path.join(d, "images", "masks_for_images", "dslr", "img_0.png")      # next to <image base>/dslr/img_0.png
    os.makedirs(os.path.dirname(mask), exist_ok=True)
    m = np.zeros((9, 12), np.uint8); m[2:5, 3:7] = 1
    Image.fromarray(m).save(mask)
    return _run("MaskTransfer", "--scan_alignment_path", project, "--image_base_path", os.path.join(d, "images"),
                "--state_path", os.path.join(d, "state"), "--output_folder_path", os.path.join(d, "mt_out"), "--source_image", NAMES[0])


def _image_localizer(d, project):
    """The state of test_localize_host.py and a script with a pick, which needs the scans."""
    ident = (np.array([1.0, 0, 0, 0]), np.zeros(3))
    lh._write_state(d, [ident] * 3, NAMES)
    return _run("ImageLocalizer", *lh._base(d), "--script", lh._script(d, "image %s\npick 10 20 11 21\n" % NAMES[0]), "--scan_alignment_path", project)


SCAN_TOOLS = [_ground_truth_creator, _image_registrator, _mask_transfer, _image_localizer]


def _project(d, entries, name="scans.mlp"):
    path = os.path.join(d, name)
    write_mlp(path, entries)
    return path


@pytest.mark.parametrize("tool", SCAN_TOOLS)
def test_missing_scan_file(tmp_path, tool):
    d = str(tmp_path)
    r = tool(d, _project(d, [("scan", "missing.ply", np.eye(4))]))
    assert r.returncode == 1, r.stdout + r.stderr
    assert LOADING in r.stdout and DONE not in r.stdout
    assert "[loadPLYFile] cannot open " + os.path.join(d, "missing.ply") in r.stderr
    assert r.stderr.count(CANNOT_LOAD) == 1 and CANNOT_READ_POSES not in r.stderr
    assert r.stderr.index("[loadPLYFile]") < r.stderr.index(CANNOT_LOAD)


def test_missing_scan_file_normal_estimator(tmp_path):
    d = str(tmp_path)
    r = _normal_estimator(d, _project(d, [("scan", "missing.ply", np.eye(4))]))
    assert r.returncode == 1, r.stdout + r.stderr
    assert "[loadPLYFile] cannot open " + os.path.join(d, "missing.ply") in r.stderr and CANNOT_LOAD not in r.stderr
    assert "Loading point clouds" not in r.stdout and not os.path.exists(os.path.join(d, "normals.ply"))


@pytest.mark.parametrize("tool", [_ground_truth_creator, _mask_transfer, _image_localizer])
def test_project_without_meshes_is_refused(tmp_path, tool):
    d = str(tmp_path)
    project = _project(d, [])
    r = tool(d, project)
    assert r.returncode == 1, r.stdout + r.stderr
    assert CANNOT_READ_POSES + " " + project in r.stderr and CANNOT_LOAD not in r.stderr and EMPTY not in r.stderr
    assert "Loading point clouds" not in r.stdout


def test_project_without_meshes_image_registrator(tmp_path):
    """Read, then refused as an empty cloud -- before "Done." is printed."""
    d = str(tmp_path)
    r = _image_registrator(d, _project(d, []))
    assert r.returncode == 1, r.stdout + r.stderr
    assert LOADING in r.stdout and DONE not in r.stdout
    assert EMPTY in r.stderr and CANNOT_READ_POSES not in r.stderr and CANNOT_LOAD not in r.stderr


def test_project_without_meshes_normal_estimator(tmp_path):
    """Accepted: an output file without vertices."""
    d = str(tmp_path)
    r = _normal_estimator(d, _project(d, []))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Finished!" in r.stdout and "Loading point clouds" not in r.stdout and r.stderr == ""
    header, rec, _ = read_ply_normals(os.path.join(d, "normals.ply"))          # after the vertices: PCL's camera element
    assert header.startswith("ply\n") and "element vertex 0\n" in header and len(rec) == 0


def test_missing_project_file(tmp_path):
    d = str(tmp_path)
    project = os.path.join(d, "none.mlp")
    r = _image_registrator(d, project)
    assert r.returncode == 1 and "Loading point clouds" not in r.stdout
    assert CANNOT_READ_POSES + " " + project in r.stderr and r.stderr.count(CANNOT_LOAD) == 1
    assert r.stderr.index(CANNOT_READ_POSES) < r.stderr.index(CANNOT_LOAD)
    for tool in (_ground_truth_creator, _mask_transfer, _image_localizer, _normal_estimator):
        r = tool(d, project)
        assert r.returncode == 1 and "Loading point clouds" not in r.stdout, tool.__name__
        assert CANNOT_READ_POSES + " " + project in r.stderr and CANNOT_LOAD not in r.stderr, tool.__name__


@pytest.mark.parametrize("tool", SCAN_TOOLS + [_normal_estimator])
def test_absolute_scan_file_name_is_not_joined_to_the_project_directory(tmp_path, tool):
    d = str(tmp_path)
    os.makedirs(os.path.join(d, "project"))
    absolute = os.path.join(d, "elsewhere", "scan.ply")
    r = tool(d, _project(os.path.join(d, "project"), [("scan", absolute, np.eye(4))]))
    assert r.returncode == 1, r.stdout + r.stderr
    assert "[loadPLYFile] cannot open " + absolute + "\n" in r.stderr
    assert os.path.join(d, "project") + "/" not in r.stderr
