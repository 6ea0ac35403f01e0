"""The numpy restatement of the PointCloudEditor operations (tests/edit_ref.py) against hand-worked cases, and the parts of the
PointCloudEditor tool that need no GPU: the script parser, the label definitions and the .labels files."""
import os
import subprocess

import numpy as np
import pytest

import cli_util
import edit_ref as er

TOOL = os.path.join(cli_util.BIN, "PointCloudEditor")
SQUARE = [(10, 10), (20, 10), (20, 20), (10, 20)]


def _inside(polygon, x, y):
    return bool(er.points_in_polygon(np.array([x], np.float32), np.array([y], np.float32), polygon)[0])


def test_points_on_vertices():
    # the rule `y >= y1 && y < y2 && x_edge <= x` takes the top-left vertex only: at (20, 10) both vertical edges count, and
    # y == 20 is below every edge's half-open range
    assert _inside(SQUARE, 10, 10)
    assert not _inside(SQUARE, 20, 10)
    assert not _inside(SQUARE, 10, 20)
    assert not _inside(SQUARE, 20, 20)


def test_points_on_left_and_right_edges():
    assert _inside(SQUARE, 10, 15)               # on the left edge: x_edge == x counts once
    assert not _inside(SQUARE, 20, 15)           # on the right edge: both edges count
    assert _inside(SQUARE, 19.999, 15) and not _inside(SQUARE, 9.999, 15)
    # a slanted edge met exactly: (0, 0) - (8, 16) at y = 4 is x = 2
    tri = [(0, 0), (8, 16), (-8, 16)]
    assert _inside(tri, 2, 4) is False           # right side of the triangle: the edge and the left edge both count
    assert _inside(tri, -2, 4) is True           # left side


def test_points_on_horizontal_edges():
    assert _inside(SQUARE, 15, 10)               # top edge (y1 of the vertical edges): inside
    assert not _inside(SQUARE, 15, 20)           # bottom edge: outside
    assert er.polygon_edges(SQUARE) == [(20.0, 10.0, 20.0, 20.0), (10.0, 10.0, 10.0, 20.0)]       # the horizontal ones are gone


def test_bow_tie_under_odd_even():
    bow = [(0, 0), (10, 10), (10, 0), (0, 10)]
    assert _inside(bow, 2, 5) and _inside(bow, 8, 5)              # the two lobes
    assert not _inside(bow, 5, 2) and not _inside(bow, 5, 8)      # between the crossing edges
    assert not _inside(bow, 11, 5) and not _inside(bow, -1, 5)


def test_on_boundary_helper():
    on = er.points_on_boundary(np.array([10, 15, 20, 15, 12], np.float32), np.array([10, 10, 15, 15, 20], np.float32), SQUARE)
    assert on.tolist() == [True, True, True, False, True]


def test_projection_gives_integer_pixels_and_inclusive_depth_range():
    view = er.make_view(48, 64, min_depth=1.0, max_depth=4.0)       # fx = fy = 64: pixel = (k + 24, m + 32) for x = k z / 64, y = m z / 64
    z = np.array([1, 2, 4, 4, 1], np.float32)
    k = np.array([-24, 0, 5, 23, 7], np.float32)
    m = np.array([-32, 0, -3, 31, 7], np.float32)
    xyz = np.stack([k * z / 64, m * z / 64, z], 1)
    in_range, px, py, cz = er.project(view, xyz)
    assert in_range.all()                                         # z == min_depth and z == max_depth are in range
    assert px.tolist() == (k + 24).tolist() and py.tolist() == (m + 32).tolist()
    just_out = np.array([[0, 0, np.nextafter(np.float32(1), np.float32(0))], [0, 0, np.nextafter(np.float32(4), np.float32(5))],
                         [0, 0, np.nan], [0, 0, -2]], np.float32)
    assert not er.project(view, just_out)[0].any()
    whole = [(-100, -100), (200, -100), (200, 200), (-100, 200)]
    assert er.lasso(view, np.vstack([xyz, just_out]), whole).tolist() == [True] * 5 + [False] * 4


def test_lasso_modes_and_small_polygons():
    view = er.make_view(48, 64, min_depth=1.0, max_depth=4.0)
    xyz = np.array([[0, 0, 1], [10 / 64, 0, 1], [-10 / 64, 0, 1]], np.float32)     # pixels (24, 32), (34, 32), (14, 32)
    right = [(20, 0), (40, 0), (40, 64), (20, 64)]
    old = np.array([False, False, True])
    assert er.lasso(view, xyz, right).tolist() == [True, True, False]
    assert er.lasso(view, xyz, right, "add", old).tolist() == [True, True, True]
    assert er.lasso(view, xyz, right, "remove", np.array([True, False, True])).tolist() == [False, False, True]
    assert er.lasso(view, xyz, right[:2], "replace", old).tolist() == old.tolist()     # two vertices: nothing happens


def test_depth_gate():
    view = er.make_view(4, 4, min_depth=1.0, max_depth=200.0)
    # all at pixel (2, 2): z = 100 makes 0.99f * z = 99 exactly
    xyz = np.array([[0, 0, 100]] * 5, np.float32)
    whole = [(-1, -1), (5, -1), (5, 5), (-1, 5)]
    assert np.float32(0.99) * np.float32(100) == np.float32(99)
    for value, expect in [(98.5, False), (99.0, True), (99.5, True), (np.inf, True), (-np.inf, True), (np.nan, True)]:
        depth = np.full((4, 4), value, np.float32)
        assert er.lasso(view, xyz, whole, depth=depth).tolist() == [expect] * 5, value


def test_plane_and_points_on_it():
    view = er.make_view(64, 48)
    pts = np.array([[0, 0, 2], [1, 0, 2], [0, 1, 2]], np.float32)
    n, offset = er.plane_through(pts)
    assert n.tolist() == [0, 0, -1] and offset == 2               # (p2 - p0) x (p1 - p0)
    xyz = np.array([[0, 0, 1], [0, 0, 2], [5, 5, 2], [0, 0, 3], [np.nan, 0, 3]], np.float32)
    assert er.beyond_plane(view, xyz, pts, [0, 0, 0]).tolist() == [False, False, False, True, False]      # on the plane: not selected
    assert er.beyond_plane(view, xyz, pts, [0, 0, 9]).tolist() == [True, False, False, False, False]      # the camera on the other side
    assert er.beyond_plane(view, xyz, pts, [0, 0, 0], True).tolist() == [False, False, False, True, False]
    with pytest.raises(ValueError):
        er.plane_through([[0, 0, 0], [1, 1, 1], [2, 2, 2]])


def test_pick_tie_takes_the_lowest_index():
    view = er.make_view(48, 64, min_depth=1.0, max_depth=4.0)
    # points 1, 2 and 4 share pixel (29, 32) at different depths; point 0 is out of range at the same pixel; 3 is NaN
    xyz = np.array([[5 * 8 / 64, 0, 8], [5 / 64, 0, 1], [10 / 64, 0, 2], [np.nan, 0, 1], [20 / 64, 0, 4]], np.float32)
    idx, dist = er.pick(view, xyz, [(29, 32), (32, 36), (29.5, 32)])
    assert idx.tolist() == [1, 1, 1] and dist.tolist() == [0.0, 25.0, 0.25]
    idx, dist = er.pick(view, xyz[:1], [(29, 32)])
    assert idx.tolist() == [-1] and np.isinf(dist[0])


def test_look_at_pose():
    T = er.look_at_pose([3, 0, 0], [0, 0, 0])
    # forward = -x, right = forward x z = +y, -up = -z: a point in front of the camera on its axis
    assert np.allclose(T @ np.array([0, 0, 0, 1.0]), [0, 0, 3], atol=1e-6)
    assert np.allclose(T @ np.array([0, 1, 0, 1.0]), [1, 0, 3], atol=1e-6)
    assert np.allclose(T @ np.array([0, 0, 1, 1.0]), [0, -1, 3], atol=1e-6)


# ---- the tool, as far as it runs without a GPU -----------------------------------------------------------------------------------------
def _run(args, cwd):
    return subprocess.run([TOOL] + args, cwd=cwd, capture_output=True, text=True, timeout=60)


def _cloud(tmp_path, n=7):
    xyz = np.arange(3 * n, dtype=np.float32).reshape(n, 3)
    rgb = (np.arange(3 * n) % 251).astype(np.uint8).reshape(n, 3)
    cli_util.write_ply_xyz(str(tmp_path / "scan.ply"), xyz, rgb)
    (tmp_path / "labels.txt").write_text("# Index Name R G B\n0 unlabeled 0 0 0\n1 wall 200 10 10\n\n4 floor 10 200 10\n")
    return xyz, rgb


def test_labels_round_trip_through_the_tool(tmp_path):
    xyz, rgb = _cloud(tmp_path)
    (tmp_path / "edits.txt").write_text("# label everything, then move label 1 to 4\nobject 0\nassign_label_to_cloud 1\nselect_label 1   # all\n"
                                        "print_selection\nlabel 4\nprint_selection\nsave 0 out.ply\n")
    r = _run(["--in", "scan.ply", "--label_definitions", "labels.txt", "--script", "edits.txt"], tmp_path)
    assert r.returncode == 0, r.stderr
    assert "selection: 7 of 7" in r.stdout and "selection: 0 of 7" in r.stdout
    assert (tmp_path / "out.labels").read_bytes() == bytes([4] * 7)
    data = (tmp_path / "out.ply").read_bytes()
    body = data[data.index(b"end_header\n") + 11:]
    rec = np.frombuffer(body, dtype=[("p", "<f4", 3), ("c", "u1", 3)], count=7)
    assert np.array_equal(rec["p"], xyz) and np.array_equal(rec["c"], rgb)
    # read back: the .labels file next to out.ply is picked up and checked against the definitions
    (tmp_path / "again.txt").write_text("select_label 4\nprint_selection\nselect_label 1\nprint_selection\n")
    r = _run(["--in", "out.ply", "--label_definitions", "labels.txt", "--script", "again.txt"], tmp_path)
    assert r.returncode == 0, r.stderr
    assert r.stdout.count("selection: 7 of 7") == 1 and r.stdout.count("selection: 0 of 7") == 1


def test_label_files_are_checked(tmp_path):
    _cloud(tmp_path)
    (tmp_path / "edits.txt").write_text("print_selection\n")
    args = ["--in", "scan.ply", "--label_definitions", "labels.txt", "--script", "edits.txt"]
    (tmp_path / "scan.labels").write_bytes(bytes([1] * 6))
    r = _run(args, tmp_path)
    assert r.returncode != 0 and "inconsistent" in r.stderr
    (tmp_path / "scan.labels").write_bytes(bytes([1] * 8))
    assert _run(args, tmp_path).returncode != 0
    (tmp_path / "scan.labels").write_bytes(bytes([1, 1, 1, 2, 1, 1, 1]))           # 2 has no definition (the list has a hole there)
    r = _run(args, tmp_path)
    assert r.returncode != 0 and "no definition" in r.stderr
    (tmp_path / "scan.labels").write_bytes(bytes([1, 0, 4, 4, 1, 0, 1]))
    assert _run(args, tmp_path).returncode == 0
    (tmp_path / "twice.txt").write_text("1 a 0 0 0\n1 b 0 0 0\n")
    assert _run(["--in", "scan.ply", "--label_definitions", "twice.txt", "--script", "edits.txt"], tmp_path).returncode != 0
    (tmp_path / "big.txt").write_text("1 a 0 0 256\n")
    assert _run(["--in", "scan.ply", "--label_definitions", "big.txt", "--script", "edits.txt"], tmp_path).returncode != 0


@pytest.mark.parametrize("bad, line", [
    ("object 0\nview 64 48\nlasso replac 0 0 1 1 2 2\n", 3),
    ("object 0\n\n# comment\nlasso add 0 0 1 1 2\n", 4),
    ("frobnicate\n", 1),
    ("view 64\n", 1),
    ("depth_range 2 1\n", 1),
    ("view 64 48\ncamera pose 1 0 0 0 1 0 0 0 1 0 0\n", 2),
    ("camera look_from 0 0 0 look_at 1 1\n", 1),
    ("pick 1 x\n", 1),
    ("beyond_plane hidden_only\n", 1),
    ("select_label 256\n", 1),
    ("select_none\nselect_outliers 0 1.5\n", 2),
], ids=["lasso_mode", "lasso_odd", "unknown", "view_arity", "depth_range_order", "pose_arity", "look_at_arity", "pick_number", "beyond_plane_word",
        "label_range", "outliers_k"])
def test_script_parse_errors_name_the_line(tmp_path, bad, line):
    _cloud(tmp_path)
    (tmp_path / "edits.txt").write_text(bad)
    r = _run(["--in", "scan.ply", "--script", "edits.txt"], tmp_path)
    assert r.returncode != 0
    assert "edits.txt:%d:" % line in r.stderr, r.stderr


def test_run_time_errors_name_the_line(tmp_path):
    _cloud(tmp_path)
    for script, line, text in [("object 0\nobject 1\n", 2, "out of range"),
                               ("select_none\nselect_label 3\n", 2, "no definition"),
                               ("camera look_from 0 0 5 look_at 0 0 0\n", 1, "parallel to z"),
                               ("camera pose 2 0 0 0 1 0 0 0 1 0 0 0\n", 1, "not a rotation"),
                               ("point 0 0 0\npoint 1 0 0\nbeyond_plane\n", 3, "three points")]:
        (tmp_path / "edits.txt").write_text(script)
        r = _run(["--in", "scan.ply", "--label_definitions", "labels.txt", "--script", "edits.txt"], tmp_path)
        assert r.returncode != 0 and "edits.txt:%d:" % line in r.stderr and text in r.stderr, (script, r.stderr)


def test_usage_without_script(tmp_path):
    r = _run(["--in", "scan.ply"], tmp_path)
    assert r.returncode != 0 and "Usage" in r.stderr
