"""ReconstructionEvaluator without a GPU: the numpy restatement of the rules (tests/evaluate_ref.py) on hand-worked cases, and the
tool's argument handling (every argument is checked before anything is loaded, so no device is needed)."""
import os
import subprocess

import numpy as np
import pytest

import evaluate_ref as er
from cli_util import write_mlp, write_ply_xyz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "dataset-pipeline_amd", "bin", "ReconstructionEvaluator")
F = np.float32


def wall():
    """A wall at x = 2, 1 m x 1 m, sampled every centimetre, seen from the origin."""
    g = np.arange(-50, 51) * 0.01
    yy, zz = np.meshgrid(g, g, indexing="ij")
    return np.stack([np.full(yy.size, 2.0), yy.ravel(), zz.ravel()], 1).astype(F)


def verdicts(E, i):
    """'a' accurate, 'i' inaccurate, 'u' unobserved per reconstruction point at tolerance index i (rule 5)."""
    acc = E["near_rec"] <= i
    return np.where(acc, "a", np.where(i < E["free"], "i", "u"))


def test_wall_seen_from_the_origin():
    scan = wall()
    yz = np.array([[0.003, 0.004], [0.104, 0.057], [-0.201, 0.152], [0.048, -0.303]])
    on = np.concatenate([np.full((4, 1), 2.0), yz], 1)
    front = np.concatenate([np.full((4, 1), 1.97), yz], 1)
    behind = np.concatenate([np.full((4, 1), 2.03), yz], 1)
    side = np.array([[0.0, 5.0, 0.1]])
    rec = np.concatenate([on, front, behind, side]).astype(F)
    E = er.evaluate(rec, [scan], [[0, 0, 0]], (0.01, 0.02, 0.05), 0.01, 256)
    assert "".join(verdicts(E, 0)) == "aaaa" + "iiii" + "uuuu" + "u"
    assert "".join(verdicts(E, 1)) == "aaaa" + "iiii" + "uuuu" + "u"
    assert "".join(verdicts(E, 2)) == "aaaa" + "aaaa" + "aaaa" + "u"
    assert (E["free"][4:8] == 2).all() and (E["free"][8:] == 0).all()          # 1.97 + 0.05 reaches the wall; behind it nothing is free
    assert E["near_rec"][12] == 3 and E["free"][12] == 0                        # an empty pixel
    # every voxel holds one point: accuracy = accurate / (accurate + inaccurate) voxels; the unobserved ones are not counted
    assert E["evaluated_voxels"].tolist() == [8, 8, 12] and E["accuracy"].tolist() == [0.5, 0.5, 1.0]
    assert E["n_rec_voxels"] == 13
    # the scan points within the tolerance of a reconstruction point are complete
    assert 0 < E["completeness"][0] < E["completeness"][2] < 0.1


def test_distance_equal_to_the_threshold_is_within():
    s = 1.0 / 64.0
    scan = np.array([[0, 0, 0]], F)
    rec = np.array([[16 * s, 0, 0], [0, -32 * s, 0], [0, 0, 33 * s], [12 * s, 0, 16 * s], [-16 * s, s, 0]], F)
    t = np.array([0.25, 0.5], F)
    assert er.thresholds(t).tolist() == [0.0625, 0.25]
    assert er.min_d2(rec, scan).tolist() == [0.0625, 0.25, (33 * s) ** 2, 0.09765625, 0.0625 + s * s]
    E = er.evaluate(rec, [scan], [[5, 5, 5]], t, 0.37, 2)
    assert E["near_rec"].tolist() == [0, 1, 2, 1, 1]
    assert E["near_scan"].tolist() == [0]


def test_pixel_rules():
    N = 64
    p = np.array([[1, 1, 0], [-1, 1, 0.5], [0.5, -1, 1], [0, 0, 0], [0.25, 0.5, -0.125], [1, -1, -1]], F)
    ok, pix, rng = er.pixels(p, np.zeros(3, F), N)
    face, row, col = pix // (N * N), (pix // N) % N, pix % N
    assert ok.tolist() == [True, True, True, False, True, True]
    assert face[0] == 0 and col[0] == N - 1 and row[0] == N // 2          # |dx| == |dy| picks x; a / m == 1 lands in column N - 1
    assert face[1] == 1 and col[1] == N - 1 and row[1] == 48              # x negative: (a, b) = (y, z)
    assert face[2] == 3 and col[2] == N - 1 and row[2] == 48              # |dy| == |dz| picks y, negative: (a, b) = (z, x)
    assert face[4] == 2 and col[4] == 24 and row[4] == 48                 # y: (a, b) = (z, x) = (-0.125, 0.25) / 0.5
    assert face[5] == 0 and col[5] == 0 and row[5] == 0
    assert rng[0] == F(np.sqrt(F(2))) and rng[4] == np.sqrt(F(0.0625 + 0.25) + F(0.015625))
    # a point at the origin of the scanner, an overflowing difference and a NaN have no pixel
    ok, _, _ = er.pixels(np.array([[1, 2, 3], [3e38, 0, 0], [np.nan, 0, 0]], F), np.array([1, 2, 3], F), N)
    ok2, _, _ = er.pixels(np.array([[3e38, 0, 0]], F), np.array([-3e38, 0, 0], F), N)
    assert ok.tolist() == [False, True, False] and ok2.tolist() == [False]


def test_range_plus_tolerance_equal_to_the_minimum_is_not_free():
    scan = np.array([[2, 0, 0], [2.5, 0.001, 0]], F)               # one pixel, its minimum is 2
    rec = np.array([[1.5, 0, 0], [1.75, 0, 0], [1.4375, 0, 0], [2, 0, 0]], F)
    t = np.array([0.0625, 0.25, 0.5], F)
    free = er.free_classes(rec, [scan], np.zeros((1, 3), F), t, 8)
    assert free.tolist() == [2, 1, 3, 0]                              # 1.5 + 0.5 == 2 and 1.75 + 0.25 == 2 are not below it
    # the maximum over the scans
    free2 = er.free_classes(rec, [scan, np.array([[3, 0, 0]], F)], np.zeros((2, 3), F), t, 8)
    assert free2.tolist() == [3, 3, 3, 3]


def test_nan_points_are_ignored():
    scan = wall()[::7]
    rng = np.random.default_rng(0)
    rec = (scan[::3] + rng.normal(0, 0.004, scan[::3].shape)).astype(F)
    A = er.evaluate(rec, [scan], [[0, 0, 0]], (0.005, 0.01), 0.05, 64)
    bad = np.array([[np.nan, 0, 0], [2, np.inf, 0], [2, 0, -np.inf]], F)
    rec2 = np.insert(rec, [0, 5, 5], bad, axis=0)
    scan2 = np.insert(scan, [3, 9, 200], bad, axis=0)
    B = er.evaluate(rec2, [scan2], [[0, 0, 0]], (0.005, 0.01), 0.05, 64)
    keep_r, keep_s = er.finite_rows(rec2), er.finite_rows(scan2)
    assert (B["near_rec"][~keep_r] == 255).all() and (B["free"][~keep_r] == 255).all() and (B["near_scan"][~keep_s] == 255).all()
    assert np.array_equal(B["near_rec"][keep_r], A["near_rec"]) and np.array_equal(B["free"][keep_r], A["free"])
    assert np.array_equal(B["near_scan"][keep_s], A["near_scan"])
    for key in ("completeness", "accuracy", "f1", "evaluated_voxels"):
        assert np.array_equal(A[key], B[key])
    for kind in ("scan_voxels", "rec_voxels"):
        for key in ("ijk", "n_points", "count_a", "count_b"):
            assert np.array_equal(A[kind][key], B[kind][key])


def test_voxels_and_zero_denominators():
    scan = np.array([[2, 0, 0], [2, 0.3, 0]], F)
    # voxel (19, 0, 0): one accurate and one inaccurate point; voxel (15, 0, 0): inaccurate; voxel (25, 0, 0) and (0, 50, 0): unobserved
    rec = np.array([[1.999, 0.001, 0.001], [1.95, 0.001, 0.001], [1.5, 0.01, 0.02], [2.5, 0.001, 0], [0, 5, 0]], F)
    E = er.evaluate(rec, [scan], [[0, 0, 0]], (0.01,), 0.1, 4)
    assert E["rec_voxels"]["ijk"].tolist() == [[15, 0, 0], [19, 0, 0], [25, 0, 0], [0, 50, 0]]
    assert E["rec_voxels"]["n_points"].tolist() == [1, 2, 1, 1]
    assert E["rec_voxels"]["count_a"].ravel().tolist() == [0, 1, 0, 0] and E["rec_voxels"]["count_b"].ravel().tolist() == [1, 1, 0, 0]
    assert E["evaluated_voxels"].tolist() == [2] and E["accuracy"].tolist() == [0.25]
    assert E["scan_voxels"]["ijk"].tolist() == [[20, 0, 0], [20, 3, 0]] and E["completeness"].tolist() == [0.5]
    assert E["f1"][0] == (2.0 * 0.25) * 0.5 / 0.75
    # negative coordinates floor downwards; the order is (k, j, i)
    ijk, _, _ = er.voxel_table(np.array([[-0.05, 0, 0.15], [0.05, -0.15, 0], [0.05, 0.15, 0]], F), 0.1)
    assert ijk.tolist() == [[0, -2, 0], [0, 1, 0], [-1, 0, 1]]
    # nothing to judge: every score is 0
    for r, s in ((np.zeros((0, 3), F), scan), (rec, np.zeros((0, 3), F)), (rec[3:], scan)):
        E = er.evaluate(r, [s], [[0, 0, 0]], (0.01, 0.02), 0.1, 4)
        assert E["accuracy"].tolist() == [0, 0] and E["f1"].tolist() == [0, 0] and E["evaluated_voxels"].tolist() == [0, 0]
        assert E["completeness"].tolist() == [0, 0]


def test_the_scans_against_themselves_score_one():
    rng = np.random.default_rng(3)
    scans = [rng.uniform(-2, 2, (300, 3)).astype(F), rng.uniform(-2, 2, (200, 3)).astype(F)]
    E = er.evaluate(np.concatenate(scans), scans, [[0, 0, 0], [0.5, 0.5, 0.5]], er.DEFAULT_TOLERANCES, 0.37, 64)
    assert (E["near_rec"] == 0).all() and (E["near_scan"] == 0).all()
    assert E["completeness"].tolist() == [1.0] * 6 and E["accuracy"].tolist() == [1.0] * 6 and E["f1"].tolist() == [1.0] * 6


def test_refusals():
    rec = np.zeros((1, 3), F)
    for tol in ((), (0.02, 0.01), (0.01, 0.01), (0.0,), (-1.0,), (np.nan,), (np.inf,), tuple(0.01 * k for k in range(1, 10))):
        with pytest.raises(ValueError):
            er.evaluate(rec, [rec], [[0, 0, 1]], tol, 0.01, 64)
    for h, N, scans in ((0.0, 64, [rec]), (np.nan, 64, [rec]), (0.01, 63, [rec]), (0.01, 0, [rec]), (0.01, 8194, [rec]), (0.01, 64, [])):
        with pytest.raises(ValueError):
            er.evaluate(rec, scans, [[0, 0, 1]] * len(scans), (0.01,), h, N)
    far = np.array([[0, F(2 ** 20) * F(0.01), 0]], F)
    with pytest.raises(ValueError):
        er.evaluate(far, [rec], [[0, 0, 1]], (0.01,), 0.01, 64)
    with pytest.raises(ValueError):
        er.evaluate(rec, [far], [[0, 0, 1]], (0.01,), 0.01, 64)
    er.evaluate(np.concatenate([rec, [[np.nan, 1e30, 0]]]).astype(F), [rec], [[0, 0, 1]], (0.01,), 0.01, 64)      # an ignored point is not refused


# ---- the tool -------------------------------------------------------------------------------------------------------------------------
def _run(args):
    if not os.path.exists(TOOL):
        pytest.fail("bin/ReconstructionEvaluator missing: build() makes it")
    return subprocess.run([TOOL] + args, capture_output=True, text=True, timeout=60)


@pytest.fixture()
def project(tmp_path):
    write_ply_xyz(str(tmp_path / "rec.ply"), np.zeros((4, 3), F))
    write_mlp(str(tmp_path / "scans.mlp"), [("scan", "scan.ply", np.eye(4))])
    write_mlp(str(tmp_path / "empty.mlp"), [])
    return tmp_path


def test_tool_missing_paths(project):
    for args in ([], ["--reconstruction_ply_path", str(project / "rec.ply")], ["--ground_truth_mlp_path", str(project / "scans.mlp")], ["--voxel_size", "0.02"]):
        r = _run(args)
        assert r.returncode == 1 and "please provide --reconstruction_ply_path and --ground_truth_mlp_path" in r.stderr and r.stdout == ""


@pytest.mark.parametrize("flag,value,message", [
    ("--tolerances", "0.02,0.01", "--tolerances must be 1 to 8 positive numbers in strictly ascending order"),
    ("--tolerances", "0.01,0.01", "--tolerances must be 1 to 8 positive numbers in strictly ascending order"),
    ("--tolerances", "0,0.01", "--tolerances must be 1 to 8 positive numbers in strictly ascending order"),
    ("--tolerances", "-0.01", "--tolerances must be 1 to 8 positive numbers in strictly ascending order"),
    ("--tolerances", "0.01,,0.02", "--tolerances must be 1 to 8 positive numbers in strictly ascending order"),
    ("--tolerances", "0.01,abc", "--tolerances must be 1 to 8 positive numbers in strictly ascending order"),
    ("--tolerances", "1,2,3,4,5,6,7,8,9", "--tolerances must be 1 to 8 positive numbers in strictly ascending order"),
    ("--cube_map_size", "2047", "--cube_map_size must be even, from 2 to 8192"),
    ("--cube_map_size", "0", "--cube_map_size must be even, from 2 to 8192"),
    ("--cube_map_size", "8194", "--cube_map_size must be even, from 2 to 8192"),
    ("--voxel_size", "0", "--voxel_size must be positive"),
    ("--cloud_tolerance", "0.03", "--cloud_tolerance must be one of --tolerances"),
])
def test_tool_refuses_bad_arguments_before_loading(project, flag, value, message):
    # scans.mlp names a scan file that does not exist: a tool that loaded anything first would complain about that instead
    r = _run(["--reconstruction_ply_path", str(project / "none.ply"), "--ground_truth_mlp_path", str(project / "scans.mlp"), flag, value])
    assert r.returncode == 1 and message in r.stderr and "cannot open" not in r.stderr and r.stdout == ""


def test_tool_project_without_scans_and_missing_files(project):
    r = _run(["--reconstruction_ply_path", str(project / "none.ply"), "--ground_truth_mlp_path", str(project / "empty.mlp")])
    assert r.returncode == 1 and "cannot read scan poses from" in r.stderr and "cannot open" not in r.stderr
    r = _run(["--reconstruction_ply_path", str(project / "rec.ply"), "--ground_truth_mlp_path", str(project / "none.mlp")])
    assert r.returncode == 1 and "cannot read scan poses from" in r.stderr
    r = _run(["--reconstruction_ply_path", str(project / "none.ply"), "--ground_truth_mlp_path", str(project / "scans.mlp")])
    assert r.returncode == 1 and "cannot open" in r.stderr and r.stdout == ""
