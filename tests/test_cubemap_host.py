"""CubeMapRenderer / SfMScaleEstimator, the parts that need no GPU: the numpy restatement (tests/cubemap_ref.py) against cases
computed by hand and against a naive loop implementation, the tools' argument handling, and SfMScaleEstimator end to end."""
import os
import subprocess

import numpy as np
import pytest

import cubemap_ref as cr
import sfm_case
from cli_util import BIN, read_mlp, write_ply_xyz

F = np.float32
INF = np.inf
SIX = 5.5e-6        # a value printed with six significant digits: half a unit of the sixth, plus the f32 roundings before it


def _u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _pt(size, face, ix, iy, z, fx_off=0.5, fy_off=0.5):
    """a point that lands at pixel (ix + fx_off, iy + fy_off) of `face` at depth z (size a power of two: exact in f32)"""
    h = size // 2
    rx, ry = (ix + fx_off - h) / h * z, (iy + fy_off - h) / h * z
    inv = {0: (rx, ry, z), 1: (-z, ry, rx), 2: (-rx, ry, -z), 3: (z, ry, -rx), 4: (rx, z, -ry), 5: (rx, -z, ry)}[face]
    return list(inv)


# ---- 1. hand-computed cases ----------------------------------------------------------------------------------------------
def test_equal_depth_lowest_index_wins():
    xyz = np.array([_pt(8, 0, 3, 2, 2.0, 0.25), _pt(8, 0, 3, 2, 1.0, 0.5), _pt(8, 0, 3, 2, 1.0, 0.75)], F)
    rgb = np.array([[10, 0, 0], [0, 20, 0], [0, 0, 30]], np.uint8)
    c, d, _ = cr.render(xyz, rgb, 8, fill=False)
    assert d[0, 2, 3] == 1.0 and tuple(c[0, 2, 3]) == (0, 20, 0)
    assert np.isinf(d).sum() == d.size - 1
    c, d, _ = cr.render(xyz[::-1], rgb[::-1], 8, fill=False)            # file order decides, not position
    assert tuple(c[0, 2, 3]) == (0, 0, 30)


def test_truncation_toward_zero_and_right_edge():
    # x = (4 * rx) / 1 + 4: rx = -1.125 -> x = -0.5 -> column 0; rx = 1 -> x = 8 = size: rejected; rx = -1.25 -> x = -1: rejected
    xyz = np.array([[-1.125, 0, 1], [1.0, 0, 1], [-1.25, 0, 1], [0, -1.125, 1]], F)
    rgb = np.full((4, 3), 9, np.uint8)
    _, d, _ = cr.render(xyz, rgb, 8, fill=False)
    assert d[0, 4, 0] == 1.0 and d[0, 0, 4] == 1.0
    assert np.isfinite(d[0]).sum() == 2
    # the point (1, 0, 1) is on the ray x = z: front rejects it (x = size), right (r = (-z, y, x)) sees it at x = 0
    assert d[3, 4, 0] == 1.0
    faces_with_point1 = [f for f in range(6) if np.isfinite(cr.render(xyz[1:2], rgb[1:2], 8, fill=False)[1][f]).any()]
    assert faces_with_point1 == [3]


def test_nonfinite_points_land_nowhere():
    xyz = np.array([[np.nan, 0, 1], [0, np.inf, 1], [0, 0, np.inf], [-np.inf, 0, 0], [0, 0, np.nan], [0.1, 0.1, 1]], F)
    rgb = np.full((6, 3), 200, np.uint8)
    c, d, _ = cr.render(xyz, rgb, 8, fill=False)
    assert np.isfinite(d).sum() == 1 and d[0, 4, 4] == 1.0 and (c.reshape(-1, 3).sum(1) > 0).sum() == 1


def test_median_of_first_three_ignores_the_fourth():
    # hole at (3, 3) of the front face; valid neighbours in row-major order: (2,2) 5.0, (2,3) 7.0, (3,2) 6.0, (4,4) 1.0
    cells = [((2, 2), 5.0, 40), ((3, 2), 7.0, 80), ((2, 3), 6.0, 120), ((4, 4), 1.0, 201)]        # ((x, y), depth, red)
    xyz = np.array([_pt(8, 0, x, y, z) for (x, y), z, _ in cells], F)
    rgb = np.array([[r, 0, 0] for _, _, r in cells], np.uint8)
    c, d, s = cr.render(xyz, rgb, 8)
    assert d[0, 3, 3] == 6.0                                            # median(5, 7, 6); the 1.0 is not used
    assert c[0, 3, 3, 0] == int(F(441) / F(4) + F(0.5))                 # colour: all four, 110.25 + 0.5 -> 110
    assert d[0, 2, 2] == 5.0


def test_single_neighbour_fills_colour_not_depth_and_border_is_inf():
    xyz = np.array([_pt(8, 0, 3, 3, 2.0), _pt(8, 0, 0, 5, 1.5)], F)     # the second is on the border column
    rgb = np.array([[100, 150, 200], [50, 60, 70]], np.uint8)
    c0, d0, _ = cr.render(xyz, rgb, 8, fill=False)
    assert d0[0, 5, 0] == 1.5                                           # rendered ...
    fc, fd, flag = cr.fill_pass1(c0[0], d0[0])
    assert np.isinf(fd[5, 0]) and tuple(fc[5, 0]) == (0, 0, 0)          # ... but a border pixel: depth inf
    assert fd[3, 3] == 2.0 and np.isinf(fd[2, 2]) and tuple(fc[2, 2]) == (100, 150, 200)      # m == 1
    # (1, 4) has the border point as its only neighbour: colour from it, depth stays inf
    assert np.isinf(fd[4, 1]) and tuple(fc[4, 1]) == (50, 60, 70)
    assert flag
    assert np.isfinite(fd).sum() == 1


def test_sweep_count_is_chebyshev_distance_and_empty_face_terminates():
    size = 16
    xyz = np.array([_pt(size, 0, 4, 6, 1.0)], F)
    rgb = np.array([[90, 91, 92]], np.uint8)
    c, d, s = cr.render(xyz, rgb, size)
    assert s[0] == max(4, size - 1 - 4, 6, size - 1 - 6)                # farthest corner (15, 15): 11
    assert (c[0] == [90, 91, 92]).all() and np.isfinite(d[0]).sum() == 1
    assert (s[1:] == 0).all() and (c[1:] == 0).all() and np.isinf(d[1:]).all()       # empty faces: black, inf, and they end


# ---- 2. against a naive implementation -----------------------------------------------------------------------------------
def _naive(xyz, rgb, size, fill=True):
    """plain loops in file order"""
    xyz = np.asarray(xyz, F); n = len(xyz)
    h = F(size // 2)
    out_c = np.zeros((6, size, size, 3), np.uint8); out_d = np.full((6, size, size), INF, F); sweeps = [0] * 6
    for face in range(6):
        col = np.zeros((size, size, 3), np.uint8); dep = np.full((size, size), INF, F)
        for i in range(n):
            x, y, z = xyz[i]
            if not (np.isfinite(x) and np.isfinite(y) and np.isfinite(z)):
                continue
            rx, ry, rz = [(x, y, z), (z, y, -x), (-x, y, -z), (-z, y, x), (x, -z, y), (x, z, -y)][face]
            if rz <= 0:
                continue
            with np.errstate(all="ignore"):
                px = F(F(h * rx) / rz) + h
                py = F(F(h * ry) / rz) + h
            if not (np.isfinite(px) and np.isfinite(py)):
                continue
            ix, iy = int(px), int(py)                                   # toward zero
            if 0 <= ix < size and 0 <= iy < size and rz < dep[iy, ix]:
                dep[iy, ix] = rz; col[iy, ix] = rgb[i]
        if not fill:
            out_c[face], out_d[face] = col, dep
            continue
        fcol = np.zeros_like(col); fdep = np.full((size, size), INF, F); flag = False

        def mean(vals):
            m = len(vals)
            return [int(F(F(sum(int(v[ch]) for v in vals)) / F(F(1) * F(m))) + F(0.5)) for ch in range(3)]
        for y in range(1, size - 1):
            for x in range(1, size - 1):
                if not np.isinf(dep[y, x]):
                    fdep[y, x] = dep[y, x]; fcol[y, x] = col[y, x]
                    continue
                nb = [(dep[y + dy, x + dx], col[y + dy, x + dx]) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
                      if (dx or dy) and not np.isinf(dep[y + dy, x + dx])]
                m = len(nb)
                if m == 2:
                    fdep[y, x] = min(nb[0][0], nb[1][0])
                elif m >= 3:
                    k = 3 if m <= 4 else (5 if m <= 6 else 7)
                    fdep[y, x] = sorted(v[0] for v in nb[:k])[k // 2]
                if m > 0:
                    fcol[y, x] = mean([v[1] for v in nb])
                else:
                    flag = True; fcol[y, x] = col[y, x]
        valid = ~np.isinf(fdep)
        while flag:
            src_c, src_v = fcol.copy(), valid.copy()
            flag = False; changed = False
            for y in range(size):
                for x in range(size):
                    if src_v[y, x]:
                        continue
                    nb = [src_c[yy, xx] for yy in range(max(0, y - 1), min(size - 1, y + 1) + 1)
                          for xx in range(max(0, x - 1), min(size - 1, x + 1) + 1) if (yy, xx) != (y, x) and src_v[yy, xx]]
                    if nb:
                        fcol[y, x] = mean(nb); valid[y, x] = True; changed = True
                    else:
                        flag = True
            if not changed:
                break                                                   # empty face
            sweeps[face] += 1
        out_c[face], out_d[face] = fcol, fdep
    return out_c, out_d, np.array(sweeps, np.int32)


def tie_cloud(seed, n, with_nonfinite=True):
    """coordinates quantised to 1/4 so that many points share rays and depths"""
    rng = np.random.default_rng(seed)
    xyz = (np.round(rng.uniform(-4, 4, (n, 3)) * 4) / 4).astype(F)
    rgb = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    if with_nonfinite and n >= 8:
        xyz[rng.integers(0, n, 4), rng.integers(0, 3, 4)] = [np.nan, np.inf, -np.inf, np.nan]
    return xyz, rgb


@pytest.mark.parametrize("size,n,seed", [(8, 60, 1), (9, 150, 2), (16, 40, 3), (17, 700, 4), (32, 300, 5), (32, 3, 6)])
@pytest.mark.parametrize("fill", [False, True])
def test_restatement_equals_naive_loops(size, n, seed, fill):
    xyz, rgb = tie_cloud(seed, n)
    if seed == 5:
        xyz = xyz[xyz[:, 1] < 1.0]; rgb = rgb[:len(xyz)]                # an empty cone: the down face needs sweeps
    a = cr.render(xyz, rgb, size, fill)
    b = _naive(xyz, rgb, size, fill)
    assert np.array_equal(a[0], b[0])
    assert np.array_equal(_u32(a[1]), _u32(b[1]))
    assert np.array_equal(a[2], b[2])
    if fill and seed in (3, 5, 6):
        assert a[2].max() >= 2


# ---- 3. bin/CubeMapRenderer without a GPU ---------------------------------------------------------------------------------
def _run(args, **kw):
    return subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, **kw)


def test_cube_map_renderer_arguments(tmp_path):
    exe = os.path.join(BIN, "CubeMapRenderer")
    r = _run([exe])
    assert r.returncode != 0 and "Please provide the input path and the image side length." in r.stdout
    r = _run([exe, "-c", "x.ply", "-o", str(tmp_path / "o")])
    assert r.returncode != 0 and "Please provide the input path and the image side length." in r.stdout
    r = _run([exe, "-c", str(tmp_path / "missing.ply"), "-o", str(tmp_path / "o"), "--size", "8"])
    assert r.returncode != 0 and "Cannot read cloud file: %s!" % (tmp_path / "missing.ply") in r.stdout
    xyz, rgb = tie_cloud(1, 50, False)
    write_ply_xyz(str(tmp_path / "c.ply"), xyz, rgb)
    r = _run([exe, "-c", str(tmp_path / "c.ply"), "--size", "8"])
    assert r.returncode != 0 and "-o" in r.stdout


def test_cube_map_renderer_fails_loudly_without_gpu(e3d, tmp_path):
    if e3d.lib().e3d_init(0) > 0:
        return                                                          # a GPU is visible: tests/test_gpu_cubemap.py runs the tool
    xyz, rgb = tie_cloud(1, 50, False)
    write_ply_xyz(str(tmp_path / "c.ply"), xyz, rgb)
    r = _run([os.path.join(BIN, "CubeMapRenderer"), "-c", str(tmp_path / "c.ply"), "-o", str(tmp_path / "o"), "--size", "8"])
    assert r.returncode != 0 and "FATAL" in r.stderr
    assert not os.path.exists(str(tmp_path / "o.front.png"))
    with pytest.raises(e3d.E3DError):
        e3d.render_cube_map(xyz, rgb, 8)


def test_render_cube_map_argument_errors(e3d):
    xyz, rgb = tie_cloud(1, 50, False)
    with pytest.raises(e3d.E3DError, match="size"):
        e3d.render_cube_map(xyz, rgb, 2)


# ---- 4. bin/SfMScaleEstimator end to end -----------------------------------------------------------------------------------
def run_scale_estimator(case):
    return _run([os.path.join(BIN, "SfMScaleEstimator"), "-s", case["model"], "-si", case["images"], "-i", case["scans"], "-o", case["out"]])


def check_scale_estimator_outputs(case, r):
    k = case["k"]
    want, bound, n = sfm_case.expected_factor(case)
    got, n_tool = sfm_case.tool_factor(r.stdout)
    err = abs(got - want) / want
    print("factor tool %.9g float64 %.12g relative difference %.3g bound %.3g (n = %d)" % (got, want, err, bound, n))
    assert n_tool == n == 2 * 6 * 40
    assert err <= bound + 5e-9                                          # (+ the nine printed digits)
    assert abs(want / k - 1) < 0.01                                     # the construction: k up to the 2 % noise
    # the MeshLab project: one pose per scan, rotation = the truth, translation = factor * the model's
    mlp = read_mlp(os.path.join(case["out"], "meshlab_project.mlp"))
    assert [m[0] for m in mlp] == ["scan1.ply", "scan2.ply"]
    for label, fn, M, text in mlp:
        Rs, ts = case["poses"][label]
        assert fn == "../scans/" + label
        assert np.abs(M[:3, :3] - Rs).max() < SIX
        assert np.allclose(M[:3, 3], got * (ts / k), rtol=SIX, atol=1e-6)
        assert (M[3] == [0, 0, 0, 1]).all()
        lines = text.split("\n")
        assert lines[0] == "" and all(ln.endswith(" ") for ln in lines[1:5]) and lines[4] == "0 0 0 1 "
    # the scaled model
    cm = os.path.join(case["out"], "colmap_model")
    assert open(os.path.join(cm, "cameras.txt")).read() == open(os.path.join(case["model"], "cameras.txt")).read()
    assert open(os.path.join(cm, "rigs.json")).read() == "[]"
    lines = [ln for ln in open(os.path.join(cm, "images.txt")).read().split("\n") if not ln.startswith("#")]
    src = sorted(case["image_lines"], key=lambda ab: int(ab[0].split()[0]))
    assert len(lines) == 2 * len(src) + 1 and lines[-1] == ""
    for i, (head, obs) in enumerate(src):
        w, v = lines[2 * i].split(), head.split()
        assert w[0] == v[0] and w[8:] == v[8:]
        assert np.allclose([float(x) for x in w[1:5]], [float(x) for x in v[1:5]], rtol=SIX, atol=1e-6)
        assert np.allclose([float(x) for x in w[5:8]], [got * float(x) for x in v[5:8]], rtol=SIX, atol=1e-6)
        assert lines[2 * i + 1].startswith(" ")
        assert [float(x) for x in lines[2 * i + 1].split()] == [float(x) for x in obs.split()]
    plines = open(os.path.join(cm, "points3D.txt")).read().split("\n")
    assert len(plines) == len(case["point_lines"]) + 1
    for a, b in zip(plines, case["point_lines"]):
        w, v = a.split(), b.split()
        assert w[0] == v[0] and w[4:] == v[4:]                          # colour, error and track words untouched
        assert np.allclose([float(x) for x in w[1:4]], [got * float(x) for x in v[1:4]], rtol=SIX, atol=1e-6)
    return got


def test_sfm_scale_estimator_end_to_end(tmp_path):
    case = sfm_case.build(str(tmp_path), k=3.7, with_scan3=True)
    r = run_scale_estimator(case)
    assert r.returncode != 0, r.stdout                                  # scan3.ply got no pose
    assert "WARNING: SfM did not provide initial estimates for all scan poses." in r.stdout
    assert "\n  scan3.ply\n" in r.stdout and "scanner_notes" not in r.stdout and "scan1.ply\n  " not in r.stdout
    assert r.stdout.count("Found cube map face:") == 12
    check_scale_estimator_outputs(case, r)


def test_sfm_scale_estimator_all_scans_aligned(tmp_path):
    case = sfm_case.build(str(tmp_path), k=0.21, with_scan3=False)
    r = run_scale_estimator(case)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.rstrip().endswith("Finished!") and "WARNING" not in r.stdout
    check_scale_estimator_outputs(case, r)


def test_sfm_scale_estimator_messages_and_no_gpu_library(tmp_path):
    exe = os.path.join(BIN, "SfMScaleEstimator")
    r = _run([exe, "-s", "a", "-si", "b"])
    assert r.returncode != 0 and "Please provide input paths." in r.stdout
    r = _run([exe, "-s", str(tmp_path), "-si", str(tmp_path), "-i", str(tmp_path), "-o", str(tmp_path / "o")])
    assert r.returncode != 0 and "Cannot read file " + str(tmp_path / "images.txt") in r.stdout
    ldd = subprocess.check_output(["ldd", exe]).decode()
    assert "hip" not in ldd.lower() and "libdl" not in ldd
