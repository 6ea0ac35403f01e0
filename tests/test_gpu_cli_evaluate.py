"""bin/ReconstructionEvaluator end to end: a two-scan scene as PLY + .mlp with a non-identity scan pose, its four stdout lines, the
JSON and both coloured clouds against the numpy restatement (tests/evaluate_ref.py), and the errors that need the loaded files."""
import json
import os
import subprocess

import numpy as np
import pytest

import evaluate_ref as er
from cli_util import BIN, write_mlp, write_ply_xyz

pytestmark = pytest.mark.gpu

F = np.float32
TOOL = os.path.join(BIN, "ReconstructionEvaluator")
TOLERANCES = (0.01, 0.03, 0.1)


def _run(args):
    return subprocess.run([TOOL] + args, capture_output=True, text=True, timeout=120)


@pytest.fixture(scope="module")
def scene(tmp_path_factory, synth):
    """Two scans of the room, each in its own frame with the scanner at the origin of its file.  Scan 0 is stored turned by 180
    degrees about z, scan 1 only shifted: both poses are exact in f32 (signs and dyadic translations), so a point's global
    coordinates are one f32 addition of its stored ones, for the tool's transform and for numpy alike."""
    d = tmp_path_factory.mktemp("evaluate")
    poses = []
    for origin, sign in (((3.0, 4.0, 1.25), -1.0), ((7.0, 3.0, 1.5), 1.0)):
        T = np.eye(4)
        T[0, 0] = T[1, 1] = sign
        T[:3, 3] = origin
        poses.append(T)
    scans = []
    for s, T in enumerate(poses):
        xyz, _, _ = synth.make_scan(4000, tuple(T[:3, 3]), 0.0, 300 + s)
        local = xyz.numpy() * np.array([T[0, 0], T[1, 1], 1.0], F)
        if s == 1:
            local[17] = np.nan
        write_ply_xyz(str(d / ("scan%d.ply" % s)), local)
        scans.append((local * np.array([T[0, 0], T[1, 1], 1.0], F) + T[:3, 3].astype(F)).astype(F))
    write_mlp(str(d / "scans.mlp"), [("scan%d" % s, "scan%d.ply" % s, T) for s, T in enumerate(poses)])
    origins = np.array([T[:3, 3] for T in poses], F)
    rng = np.random.default_rng(9)
    pool = np.concatenate(scans)
    pool = pool[np.isfinite(pool).all(1)]
    rec = (pool[rng.integers(0, len(pool), 5000)].astype(np.float64) + rng.normal(0, 0.008, (5000, 3))).astype(F)
    gross = np.arange(5000) % 10 == 3
    rec[gross] = rng.uniform((0.2, 0.2, 0.1), (9.8, 7.8, 2.8), (500, 3)).astype(F)
    rec[11] = (np.nan, 0, 0)
    write_ply_xyz(str(d / "rec.ply"), rec)
    return d, rec, scans, origins, er.evaluate(rec, scans, origins, TOLERANCES, 0.05, 64, device="cuda")


@pytest.mark.parametrize("cloud_tolerance,level", [(None, 0), ("0.03", 1)])
def test_scores_json_and_clouds(scene, cloud_tolerance, level):
    d, rec, scans, origins, E = scene
    acc_path, comp_path, js_path = str(d / "acc.ply"), str(d / "comp.ply"), str(d / "scores.json")
    args = ["--reconstruction_ply_path", str(d / "rec.ply"), "--ground_truth_mlp_path", str(d / "scans.mlp"), "--tolerances", "0.01,0.03,0.1",
            "--voxel_size", "0.05", "--cube_map_size", "64", "--scores_json", js_path, "--accuracy_cloud_output_path", acc_path,
            "--completeness_cloud_output_path", comp_path, "--timings"]
    if cloud_tolerance:
        args += ["--cloud_tolerance", cloud_tolerance]
    r = _run(args)
    assert r.returncode == 0, r.stderr
    assert 0 < E["f1"][0] < E["f1"][2] < 1 and (E["free"] > 0).any()
    lines = r.stdout.strip().split("\n")
    assert len(lines) == 4 and lines[0] == "Tolerances: 0.01 0.03 0.1"
    for line, name, key in zip(lines[1:], ("Completenesses:", "Accuracies:", "F1-scores:"), ("completeness", "accuracy", "f1")):
        assert line.split()[0] == name and len(line.split()) == 4
        got = np.array([float(x) for x in line.split()[1:]])
        assert np.allclose(got, E[key], rtol=1e-5, atol=0)                # the stream's six significant digits of the same value
    J = json.load(open(js_path))
    assert J["tolerances"] == [float(F(t)) for t in TOLERANCES]
    for key in ("completeness", "accuracy", "f1"):
        assert (np.abs(np.array(J[key]) - E[key]) <= 1e-12 * np.abs(E[key])).all(), (key, J[key], E[key])
    assert J["n_scan_voxels"] == E["n_scan_voxels"] and J["n_rec_voxels"] == E["n_rec_voxels"] and J["evaluated_voxels"] == E["evaluated_voxels"].tolist()
    keep, rgb = er.colours(E["near_rec"], E["free"], level)
    assert (~keep).sum() == 1 and len({tuple(c) for c in rgb.tolist()}) == 3
    assert open(acc_path, "rb").read() == er.pcl_ply_bytes(rec[keep], rgb)
    keep, rgb = er.colours(E["near_scan"], None, level)
    assert (~keep).sum() == 1 and len({tuple(c) for c in rgb.tolist()}) == 2
    assert open(comp_path, "rb").read() == er.pcl_ply_bytes(np.concatenate(scans)[keep], rgb)
    assert "[timings] search" in r.stderr and "[timings] voxels" in r.stderr


def test_errors_after_loading(scene, tmp_path):
    d = scene[0]
    write_ply_xyz(str(tmp_path / "rec.ply"), np.zeros((3, 3), F))
    # a scan file that does not exist
    write_mlp(str(tmp_path / "broken.mlp"), [("scan", "missing.ply", np.eye(4))])
    r = _run(["--reconstruction_ply_path", str(tmp_path / "rec.ply"), "--ground_truth_mlp_path", str(tmp_path / "broken.mlp")])
    assert r.returncode == 1 and "Cannot load scan point clouds." in r.stderr and r.stdout == ""
    # a point the voxel key cannot hold: the library's message
    far = np.zeros((3, 3), F)
    far[1, 0] = 2.0 ** 20 * 0.01 * 1.5
    write_ply_xyz(str(tmp_path / "far.ply"), far)
    r = _run(["--reconstruction_ply_path", str(tmp_path / "far.ply"), "--ground_truth_mlp_path", str(d / "scans.mlp"), "--cube_map_size", "64"])
    assert r.returncode == 1 and "a reconstruction point lies at |coordinate| / voxel size >= 2^20" in r.stderr and r.stdout == ""
    # an output that cannot be written
    r = _run(["--reconstruction_ply_path", str(tmp_path / "rec.ply"), "--ground_truth_mlp_path", str(d / "scans.mlp"), "--cube_map_size", "64",
              "--accuracy_cloud_output_path", str(tmp_path / "no_such_dir" / "acc.ply")])
    assert r.returncode == 1 and "cannot open" in r.stderr
