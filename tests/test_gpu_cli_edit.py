"""bin/PointCloudEditor end to end: scripted clean-up sessions whose expected files come from tests/edit_ref.py (coordinates and
colours byte for byte), labels, a mesh with the depth-image visibility test, the look-at camera, and the GUI's message boxes as
errors."""
import os
import re
import subprocess

import numpy as np
import pytest

import cli_util
import edit_ref as er

pytestmark = pytest.mark.gpu

TOOL = os.path.join(cli_util.BIN, "PointCloudEditor")


def run_tool(args, cwd):
    return subprocess.run([TOOL] + args, cwd=str(cwd), capture_output=True, text=True, timeout=300)


def read_cloud(path):
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    n = int(re.search(rb"element vertex (\d+)", data[:end]).group(1))
    rec = np.frombuffer(data, dtype=[("p", "<f4", 3), ("c", "u1", 3)], count=n, offset=end)
    return rec["p"].copy(), rec["c"].copy()


def read_mesh(path):
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    n = int(re.search(rb"element vertex (\d+)", data[:end]).group(1))
    m = int(re.search(rb"element face (\d+)", data[:end]).group(1))
    v = np.frombuffer(data, "<f4", 3 * n, end).reshape(n, 3)
    f = np.frombuffer(data, dtype=[("c", "u1"), ("i", "<i4", 3)], count=m, offset=end + 12 * n)
    assert len(data) == end + 12 * n + 13 * m and (f["c"] == 3).all()
    return v.copy(), f["i"].copy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# a pose of exactly representable numbers: a quarter turn about z, then about x; the translation in eighths
POSE = np.array([[0, -1, 0, 0.5], [0, 0, -1, -0.25], [1, 0, 0, 2.0]], np.float32)


def pose_words(T):
    return " ".join("%.9g" % v for v in np.concatenate([T[:, :3].ravel(), T[:, 3]]))


def cloud_in_view(n, seed, T):
    """Points in front of the camera of pose T (camera = R p + t), spread over and around a 4 : 3 window."""
    rng = np.random.RandomState(seed)
    z = rng.uniform(0.5, 12.0, n)
    cam = np.stack([rng.uniform(-0.9, 0.9, n) * z, rng.uniform(-0.7, 0.7, n) * z, z], 1)
    R, t = T[:, :3].astype(np.float64), T[:, 3].astype(np.float64)
    return ((cam - t) @ R).astype(np.float32), rng.randint(0, 256, (n, 3)).astype(np.uint8)


def camera_position(T):
    """-R^T t in f32, in the order the tool uses"""
    T = np.asarray(T, np.float32)
    return np.array([-((T[0, i] * T[0, 3] + T[1, i] * T[1, 3]) + T[2, i] * T[2, 3]) for i in range(3)], np.float32)


def test_clean_up_session(tmp_path):
    W, H = 160, 120
    xyz0, rgb0 = cloud_in_view(4000, 1, POSE)
    xyz1, rgb1 = cloud_in_view(700, 2, POSE)
    cli_util.write_ply_xyz(str(tmp_path / "scan.ply"), xyz0, rgb0)
    cli_util.write_ply_xyz(str(tmp_path / "scan.outliers.ply"), xyz1, rgb1)
    view = er.make_view(W, H, POSE, 1.0, 10.0)
    polygon = [(20, 10), (90.5, 5.25), (70, 60), (120, 110), (15.5, 100)]
    clicks = [(30, 30), (130, 40), (80, 100)]
    # what every step has to give
    moved = er.lasso(view, xyz0, polygon)
    left_xyz, left_rgb = xyz0[~moved], rgb0[~moved]
    idx = [int(er.pick(view, left_xyz, [c])[0][0]) for c in clicks]
    assert min(idx) >= 0 and len(set(idx)) == 3
    plane_points = left_xyz[idx]
    beyond = er.beyond_plane(view, left_xyz, plane_points, camera_position(POSE), True)
    assert 100 < moved.sum() < 3000 and 50 < beyond.sum() < len(left_xyz) - 50

    script = ["# clean-up of scan.ply: outliers to the outlier file, then everything behind the far wall",
              "object 0", "view %d %d" % (W, H), "depth_range 1 10", "camera pose " + pose_words(POSE), "print_view",
              "lasso replace " + " ".join("%g %g" % p for p in polygon), "print_selection", "move", "print_selection",
              "save 0 mid0.ply", "save 1 mid1.ply"]
    script += ["pick %g %g" % c for c in clicks]
    script += ["beyond_plane visible_only", "print_selection", "delete", "save 0 out0.ply", "save 1 out1.ply"]
    (tmp_path / "edits.txt").write_text("\n".join(script) + "\n")
    r = run_tool(["--in", "scan.ply", "--in", "scan.outliers.ply", "--script", "edits.txt", "--timings"], tmp_path)
    assert r.returncode == 0, r.stderr
    counts = [int(c) for c in re.findall(r"selection: (\d+) of", r.stdout)]
    assert counts == [moved.sum(), 0, beyond.sum()]
    printed = np.array([l.split() for l in r.stdout.split("\n")[:3]], np.float64)
    assert np.array_equal(printed.astype(np.float32), POSE)
    assert len(re.findall(r"timing (lasso|pick|beyond_plane|delete|move \(extract\)) [0-9.]+ ms", r.stdout)) == 8

    m0, c0 = read_cloud(tmp_path / "mid0.ply")
    m1, c1 = read_cloud(tmp_path / "mid1.ply")
    assert same_bits(m0, left_xyz) and np.array_equal(c0, left_rgb)
    assert same_bits(m1, np.vstack([xyz1, xyz0[moved]])) and np.array_equal(c1, np.vstack([rgb1, rgb0[moved]]))
    assert len(m0) + len(m1) == len(xyz0) + len(xyz1)
    o0, k0 = read_cloud(tmp_path / "out0.ply")
    o1, k1 = read_cloud(tmp_path / "out1.ply")
    assert same_bits(o0, left_xyz[~beyond]) and np.array_equal(k0, left_rgb[~beyond])
    assert same_bits(o1, m1) and np.array_equal(k1, c1)
    assert len(o0) + len(o1) == len(xyz0) + len(xyz1) - beyond.sum()
    assert not (tmp_path / "out0.labels").exists()


def test_labels(tmp_path):
    W, H = 64, 48
    xyz, rgb = cloud_in_view(3000, 3, POSE)
    cli_util.write_ply_xyz(str(tmp_path / "scan.ply"), xyz, rgb)
    (tmp_path / "labels.txt").write_text("# Index Name R G B\n1 wall 200 0 0\n4 floor 0 200 0\n9 clutter 0 0 200\n")
    view = er.make_view(W, H, POSE)
    first, second = [(5, 5), (40, 8), (30, 40)], [(20, 2), (60, 20), (25, 44), (10, 20)]
    a = er.lasso(view, xyz, first)
    b = er.lasso(view, xyz, second)
    labels = np.full(len(xyz), 1, np.uint8)
    labels[a] = 4
    labels[b] = 9
    assert a.sum() > 50 and b.sum() > 50 and (a & b).sum() > 10
    script = ["view %d %d" % (W, H), "camera pose " + pose_words(POSE), "assign_label_to_cloud 1",
              "lasso replace " + " ".join("%g %g" % p for p in first), "label 4", "print_selection",
              "lasso replace " + " ".join("%g %g" % p for p in second), "label 9",
              "select_label 4", "print_selection", "select_label 9", "print_selection", "select_label 1", "print_selection", "save 0 out.ply"]
    (tmp_path / "edits.txt").write_text("\n".join(script) + "\n")
    r = run_tool(["--in", "scan.ply", "--label_definitions", "labels.txt", "--script", "edits.txt"], tmp_path)
    assert r.returncode == 0, r.stderr
    counts = [int(c) for c in re.findall(r"selection: (\d+) of 3000", r.stdout)]
    assert counts == [0, (labels == 4).sum(), (labels == 9).sum(), (labels == 1).sum()]
    assert (tmp_path / "out.labels").read_bytes() == labels.tobytes()
    p, c = read_cloud(tmp_path / "out.ply")
    assert same_bits(p, xyz) and np.array_equal(c, rgb)
    # deleting a label's points takes their labels along
    (tmp_path / "again.txt").write_text("select_label 9\ndelete\nsave\n")
    r = run_tool(["--in", "out.ply", "--label_definitions", "labels.txt", "--script", "again.txt"], tmp_path)
    assert r.returncode == 0, r.stderr
    p, c = read_cloud(tmp_path / "out.ply")
    assert same_bits(p, xyz[labels != 9]) and np.array_equal(c, rgb[labels != 9])
    assert (tmp_path / "out.labels").read_bytes() == labels[labels != 9].tobytes()


def _square(half, z, cells):
    g = np.linspace(-half, half, cells + 1)
    x, y = np.meshgrid(g, g, indexing="xy")
    v = np.stack([x.ravel(), y.ravel(), np.full(x.size, z)], 1).astype(np.float32)
    i = np.arange(cells)[:, None] * (cells + 1) + np.arange(cells)[None, :]
    i = i.ravel()
    f = np.concatenate([np.stack([i, i + 1, i + cells + 2], 1), np.stack([i, i + cells + 2, i + cells + 1], 1)])
    return v, f.astype(np.int32)


def test_mesh_lasso_takes_only_visible_vertices(tmp_path):
    """Identity pose, a 128 x 96 window (fx = 96).  The front square (z = 2, half size 0.5) projects to +-24 px about the centre, the
    back one (z = 4, half size 0.8) to +-19.2 px: every back vertex lies at least 4 px inside the front square's image and is
    hidden (2 < 0.99 * 4); every front vertex sees itself (2 is not < 1.98) or, on the outline, at most nothing."""
    fv, ff = _square(0.5, 2.0, 8)
    bv, bf = _square(0.8, 4.0, 6)
    cli_util.write_ply_mesh(str(tmp_path / "mesh.ply"), np.vstack([fv, bv]), np.vstack([ff, bf + len(fv)]))
    (tmp_path / "edits.txt").write_text("view 128 96\ndepth_range 0.5 50\nlasso replace 2 2 126 2 126 94 2 94\nprint_selection\ndelete\nsave 0 out.ply\n")
    r = run_tool(["--in", "mesh.ply", "--script", "edits.txt"], tmp_path)
    assert r.returncode == 0, r.stderr
    assert "selection: %d of %d" % (len(fv), len(fv) + len(bv)) in r.stdout
    v, f = read_mesh(tmp_path / "out.ply")
    assert same_bits(v, bv) and np.array_equal(f, bf)
    # a cloud of the same vertices has no such test: everything is taken
    cli_util.write_ply_xyz(str(tmp_path / "cloud.ply"), np.vstack([fv, bv]), np.zeros((len(fv) + len(bv), 3), np.uint8))
    (tmp_path / "cloud.txt").write_text("view 128 96\ndepth_range 0.5 50\nlasso replace 2 2 126 2 126 94 2 94\nprint_selection\n")
    r = run_tool(["--in", "cloud.ply", "--script", "cloud.txt"], tmp_path)
    assert r.returncode == 0 and "selection: %d of" % (len(fv) + len(bv)) in r.stdout


def test_camera_look_at(tmp_path):
    W, H = 200, 150
    look_from, look_at = (3.0, 1.0, 2.0), (0.0, 0.5, 0.25)
    T = er.look_at_pose(look_from, look_at)
    rng = np.random.RandomState(7)
    xyz = rng.uniform(-1.5, 1.5, (2000, 3)).astype(np.float32)
    # the analytic projection in f64, and a rectangle that no point comes closer to than 2 px
    cam = xyz.astype(np.float64) @ T[:, :3].astype(np.float64).T + T[:, 3].astype(np.float64)
    px = H * cam[:, 0] / cam[:, 2] + 0.5 * W
    py = H * cam[:, 1] / cam[:, 2] + 0.5 * H
    x0, y0, x1, y1 = 40.0, 30.0, 110.0, 140.0
    near = ((np.abs(px - x0) < 2) | (np.abs(px - x1) < 2)) & (py > y0 - 2) & (py < y1 + 2) | ((np.abs(py - y0) < 2) | (np.abs(py - y1) < 2)) & (px > x0 - 2) & (px < x1 + 2)
    keep = ~near & (np.abs(cam[:, 2] - 0.1) > 1e-3)
    xyz, cam, px, py = xyz[keep], cam[keep], px[keep], py[keep]
    expect = (cam[:, 2] >= 0.1) & (cam[:, 2] <= 100) & (px > x0) & (px < x1) & (py > y0) & (py < y1)
    assert 100 < expect.sum() < len(xyz) - 100
    cli_util.write_ply_xyz(str(tmp_path / "scan.ply"), xyz, np.zeros((len(xyz), 3), np.uint8))
    (tmp_path / "edits.txt").write_text("view %d %d\ncamera look_from %g %g %g look_at %g %g %g\nprint_view\nlasso replace %g %g %g %g %g %g %g %g\n"
                                        "print_selection\ndelete\nsave 0 out.ply\n" % ((W, H) + look_from + look_at + (x0, y0, x1, y0, x1, y1, x0, y1)))
    r = run_tool(["--in", "scan.ply", "--script", "edits.txt"], tmp_path)
    assert r.returncode == 0, r.stderr
    printed = np.array([l.split() for l in r.stdout.split("\n")[:3]], np.float64)
    assert printed.shape == (3, 4) and np.abs(printed - T).max() < 1e-6
    assert "selection: %d of %d" % (expect.sum(), len(xyz)) in r.stdout
    p, _ = read_cloud(tmp_path / "out.ply")
    assert same_bits(p, xyz[~expect])


def test_select_outliers(tmp_path, e3d):
    """The selection becomes the points PointCloudCleaner's filter removes; deleting them leaves its inliers."""
    rng = np.random.RandomState(4)
    xyz = np.vstack([rng.uniform(-1, 1, (3000, 3)), rng.uniform(-6, 6, (40, 3))]).astype(np.float32)
    xyz = xyz[rng.permutation(len(xyz))]
    rgb = rng.randint(0, 256, (len(xyz), 3)).astype(np.uint8)
    cli_util.write_ply_xyz(str(tmp_path / "scan.ply"), xyz, rgb)
    inlier = e3d.local_outlier_removal(xyz, 8, 1.5)
    assert 10 < (~inlier).sum() < 1000
    (tmp_path / "edits.txt").write_text("select_outliers 8 1.5\nprint_selection\ndelete\nprint_selection\nsave 0 out.ply\n")
    r = run_tool(["--in", "scan.ply", "--script", "edits.txt"], tmp_path)
    assert r.returncode == 0, r.stderr
    assert "selection: %d of %d" % ((~inlier).sum(), len(xyz)) in r.stdout and "selection: 0 of %d" % inlier.sum() in r.stdout
    p, c = read_cloud(tmp_path / "out.ply")
    assert same_bits(p, xyz[inlier]) and np.array_equal(c, rgb[inlier])


@pytest.mark.parametrize("script, inputs, message", [
    ("lasso replace 0 0 64 0 64 48 0 48\nmove\n", ["scan.ply"], "exactly 2 objects"),
    ("lasso replace 0 0 64 0 64 48 0 48\nlabel 1\n", ["scan.ply"], "does not have labels"),
    ("select_label 7\n", ["scan.ply"], "no definition"),
    ("object 1\nassign_label_to_cloud 1\nobject 0\nlasso replace 0 0 64 0 64 48 0 48\nmove\n", ["scan.ply", "other.ply"], "objects with labels"),
    ("point 0 0 1\npoint 1 1 2\npoint 2 2 3\nbeyond_plane\n", ["scan.ply"], "one line"),
    ("depth_range 500 600\npick 3 3\n", ["scan.ply"], "depth range"),
], ids=["move_one_object", "label_without_labels", "select_undefined_label", "move_with_labels", "collinear_plane", "pick_nothing_in_range"])
def test_message_boxes_are_errors(tmp_path, script, inputs, message):
    xyz, rgb = cloud_in_view(500, 11, np.eye(4, dtype=np.float32)[:3])
    for name in inputs:
        cli_util.write_ply_xyz(str(tmp_path / name), xyz, rgb)
    (tmp_path / "labels.txt").write_text("1 wall 200 0 0\n")
    (tmp_path / "edits.txt").write_text("view 64 48\n" + script)
    args = []
    for name in inputs:
        args += ["--in", name]
    r = run_tool(args + ["--label_definitions", "labels.txt", "--script", "edits.txt"], tmp_path)
    assert r.returncode != 0
    assert message in r.stderr and "edits.txt:%d:" % (script.count("\n") + 1) in r.stderr, r.stderr
