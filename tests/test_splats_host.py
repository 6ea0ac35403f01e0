"""SplatCreator without a GPU: the tool's argument handling and the CPU restatement (tests/splat_ref.py) checked against
itself -- the f32 Ericson value against an f64 projection, Eigen's unitOrthogonal selector."""
import os
import subprocess

import numpy as np
import pytest

import splat_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "dataset-pipeline_amd", "bin", "SplatCreator")


def _tool():
    if not os.path.exists(TOOL):
        pytest.fail("bin/SplatCreator missing: build() makes it")
    return TOOL


def test_missing_paths_message_and_failure():
    for args in ([], ["--mesh_path", "m.ply", "--output_path", "o.ply"], ["--point_normal_cloud_path", "p.ply", "--mesh_path", "m.ply"]):
        r = subprocess.run([_tool()] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0
        assert "Please provide input / output paths." in r.stdout


def test_missing_input_file_fails_cleanly(tmp_path):
    out = tmp_path / "splats.ply"
    r = subprocess.run([_tool(), "--point_normal_cloud_path", str(tmp_path / "none.ply"), "--mesh_path", str(tmp_path / "none_mesh.ply"),
                        "--output_path", str(out)], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "cannot open" in r.stderr
    assert not out.exists()


def _closest_f64(p, a, b, c):
    """Exact (f64) squared distance from p to triangle abc: the plane projection if it falls inside, else the nearest edge."""
    p, a, b, c = (np.asarray(x, np.float64) for x in (p, a, b, c))
    n = np.cross(b - a, c - a)
    nn = n @ n
    q = p - ((p - a) @ n) / nn * n
    # barycentrics of q
    def inside(q):
        return all(np.cross(y - x, q - x) @ n >= 0 for x, y in ((a, b), (b, c), (c, a)))
    best = np.inf
    if inside(q):
        best = (p - q) @ (p - q)
    for x, y in ((a, b), (b, c), (c, a)):
        e = y - x
        t = min(1.0, max(0.0, ((p - x) @ e) / (e @ e)))
        d = p - (x + t * e)
        best = min(best, d @ d)
    return best


def test_ericson_f32_agrees_with_f64_projection():
    rng = np.random.default_rng(5)
    m = 4000
    a = rng.uniform(-1, 1, (m, 3)).astype(np.float32)
    b = (a + rng.uniform(-0.5, 0.5, (m, 3))).astype(np.float32)
    c = (a + rng.uniform(-0.5, 0.5, (m, 3))).astype(np.float32)
    p = rng.uniform(-2, 2, (m, 3)).astype(np.float32)
    # well-conditioned: no angle below ~15 degrees, edges not tiny
    e1, e2, e3 = b - a, c - a, c - b
    def ang(u, v):
        return np.degrees(np.arccos(np.clip((u * v).sum(1) / np.linalg.norm(u, axis=1) / np.linalg.norm(v, axis=1), -1, 1)))
    ok = (ang(e1, e2) > 15) & (ang(-e1, e3) > 15) & (ang(-e2, -e3) > 15) & (np.linalg.norm(e1, axis=1) > 0.05)
    got = sr.ericson_sq(p[ok], a[ok], b[ok], c[ok])
    regions = set()
    for i, k in enumerate(np.nonzero(ok)[0]):
        ref = _closest_f64(p[k], a[k], b[k], c[k])
        assert abs(float(got[i]) - ref) <= 1e-5 * max(ref, 1e-3), (k, float(got[i]), ref)
        regions.add(sr.ericson_region(p[k], a[k], b[k], c[k]))
    assert regions == set(range(7))                     # every region of the routine was exercised


def test_brute_force_minimum_ties_and_nan():
    V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5], [6, 6, 6], [7, 7, 7]], np.float32)
    T = np.array([[6, 7, 8], [0, 1, 2], [3, 4, 5]], np.int64)         # a collinear triangle, then the same triangle twice
    d, i = sr.mesh_min_sq(np.array([[0.2, 0.2, 1.0], [np.nan, 0, 0]], np.float32), V, T)
    assert d[0] == np.float32(1.0) and i[0] == 1                       # the lower id of the two equal minima
    assert d[1] == np.inf and i[1] == -1
    d, i = sr.mesh_min_sq(np.array([[0.2, 0.2, 1.0]], np.float32), V, T, max_sq=0.5)
    assert d[0] == np.inf and i[0] == -1


def test_unit_orthogonal_unit_orthogonal_both_branches():
    rng = np.random.default_rng(7)
    n = rng.normal(size=(5000, 3)).astype(np.float32)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    n[:50, :2] *= np.float32(1e-7)                                       # (almost) along z: the second branch
    n[50:60] = np.array([0, 0, 1], np.float32)
    r, first = sr.unit_orthogonal(n)
    assert first.any() and (~first).any()
    assert np.allclose(np.linalg.norm(r.astype(np.float64), axis=1), 1.0, atol=1e-6)
    assert np.abs((r.astype(np.float64) * n).sum(1)).max() < 1e-6
    up = sr.cross(n, r)
    assert np.abs((up.astype(np.float64) * r).sum(1)).max() < 1e-6
    C = sr.corners(np.zeros((5000, 3), np.float32), n, np.full(5000, 0.5, np.float32))
    assert C.shape == (5000, 4, 3)
    np.testing.assert_array_equal(C[:, 0], np.float32(0.5) * (r + up))    # TR = p + r (right + up)
