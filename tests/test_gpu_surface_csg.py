"""Box union and subtraction of the SurfaceReconstructor on the GPU (e3d_surface_reconstruct_csg, bin/SurfaceReconstructor
--csg_script) against the numpy restatement tests/surface_csg_ref.py, which applies the operation list to the scan field of
tests/surface_ref.py and hands the result to its unchanged extraction.

A solid's function g is bit-defined (f64, fixed order, no contraction), so everything made of solids alone is compared with
np.array_equal: corner set, f, count == 0, vertices, cells, triangles.  Where a cloud takes part the condition and the tolerances are
those of tests/test_gpu_surface.py, asserted in every case: the SCAN field has zero ambiguous corners (0 < |S| <= 1e-6 T) and at
most 4096 contributors per corner; then corner set, counts, cells and triangles are exact, f is exact where count == 0 and within
1e-9 T / W elsewhere, W within 1e-9 W, vertices within 1e-5 h plus one f32 ulp of the largest coordinate.  The cases' seeds are
those of the existing file, for which the restatement satisfies the condition (checked without a GPU)."""
import functools
import os
import subprocess

import numpy as np
import pytest

import surface_csg_ref as cr
import surface_ref as sr
from cli_util import BIN
from test_gpu_surface import _write_ply_27, oriented_cloud

pytestmark = pytest.mark.gpu

F = np.float32
H = sr.H
H13 = F(0.013)
MAX_CONTRIBUTORS = 4096
I3 = np.eye(3)
GENERIC = cr.quat_to_rotation(0.8, 0.2, -0.4, 0.4)
DIAGONAL = cr.quat_to_rotation(0.5, 0.5, 0.5, 0.5)                     # 120 degrees about (1, 1, 1): a permutation matrix
NO_XYZ = np.zeros((0, 3), F)


def _box(kind, centre, rotation, half):
    return (kind, np.asarray(centre, np.float64), np.asarray(rotation, np.float64), np.asarray(half, np.float64))


def _compare(e3d, xyz, nrm, h, R, solids, scan=None, exact=False, timings=None):
    """One call against the restatement; returns (vertices, triangles, corners, restatement)."""
    scan = sr.field(xyz, nrm, h, R) if scan is None else scan
    assert int(sr.ambiguous(scan).sum()) == 0
    assert int(scan["count"].max(initial=0)) <= MAX_CONTRIBUTORS
    M = cr.apply_solids(scan, solids, h)
    M.update(sr.extract(M, h))
    v, t, c = e3d.reconstruct_surface(xyz, nrm, h, R, return_corners=True, solids=solids, timings=timings)
    assert v.dtype == F and t.dtype == np.uint32 and c["ijk"].dtype == np.int32 and c["f"].dtype == np.float64
    assert np.array_equal(c["ijk"], M["ijk"]), (len(c["ijk"]), len(M["ijk"]))
    assert np.array_equal(c["count"], M["count"])
    lone = M["count"] == 0
    assert np.array_equal(c["f"][lone], M["f"][lone]) and (c["weight"][lone] == 0).all()
    seen = ~lone
    df = np.abs(c["f"] - M["f"])[seen]; dw = np.abs(c["weight"] - M["W"])[seen]
    if len(df):
        print("max |df| / (T / W) = %.3g, max |dW| / W = %.3g" % ((df / np.maximum(M["T"][seen] / M["W"][seen], 1e-300)).max(), (dw / M["W"][seen]).max()))
    assert (df <= 1e-9 * M["T"][seen] / M["W"][seen]).all()
    assert (dw <= 1e-9 * M["W"][seen]).all()
    assert np.array_equal(c["cell_ijk"], M["cell_ijk"]), (len(c["cell_ijk"]), len(M["cell_ijk"]))
    assert np.array_equal(t, M["triangles"])
    if exact:
        assert np.array_equal(c["f"], M["f"])
        assert np.array_equal(v.view(np.uint32), M["vertices"].view(np.uint32))
    elif len(v):
        bound = 1e-5 * float(h) + float(np.spacing(F(np.abs(M["vertices"]).max())))
        dv = np.abs(v.astype(np.float64) - M["vertices"].astype(np.float64)).max()
        print("max vertex deviation %.3g (bound %.3g)" % (dv, bound))
        assert dv <= bound
    return v, t, c, M


# ---- solids only: everything exact -------------------------------------------------------------------------------------------------
def _many_boxes(h, count=256):
    """`count` boxes of 1 to 4 cells per side in a region 24 cells wide, every third one subtracted, every rotation in turn."""
    rng = np.random.default_rng(256)
    ops = []
    for i in range(count):
        centre = np.array([-0.31, 0.17, -0.23]) + rng.uniform(-12, 12, 3) * float(h)
        half = rng.uniform(0.5, 2.0, 3) * float(h)
        ops.append(_box("subtract" if i % 3 == 2 else "union", centre, (I3, GENERIC, DIAGONAL)[i % 3], half))
    return ops


S19 = float(2 ** 19) * float(H)
SOLID_CASES = {
    # name: (h, solids, minimum number of triangles)
    "axis_aligned": (H, [_box("union", (0.013, -0.021, 0.007), I3, (0.12, 0.16, 0.09))], 100),
    "generic_20_cells_negative": (H13, [_box("union", (-1.3, -0.7, -2.1), GENERIC, (10 * 0.013, 4.5 * 0.013, 0.25 * 0.013))], 400),
    "diagonal": (H, [_box("union", (0.21, 0.33, -0.12), DIAGONAL, (0.31, 0.07, 0.18))], 100),
    "two_ops": (H, [_box("union", (0.21, 0.33, -0.12), DIAGONAL, (0.31, 0.17, 0.18)), _box("subtract", (0.3, 0.4, 0.0), GENERIC, (0.11, 0.5, 0.09))], 100),
    "subtract_first": (H, [_box("subtract", (0.3, 0.4, 0.0), GENERIC, (0.11, 0.5, 0.09)), _box("union", (0.21, 0.33, -0.12), DIAGONAL, (0.31, 0.17, 0.18))], 100),
    "half_a_cell_around_a_corner": (H, [_box("union", (0.1 * 0.05, 0.05 + 0.004, -0.05), I3, (0.0125, 0.0125, 0.0125))], 8),
    "half_a_cell_between_corners": (H, [_box("union", (0.025, 0.025, 0.025), GENERIC, (0.0125, 0.0125, 0.0125))], 0),
    "near_plus_2_19": (H, [_box("union", (S19 - 3.0, S19 - 2.0, S19 - 1.0), GENERIC, (0.21, 0.16, 0.11))], 100),
    "near_minus_2_19": (H, [_box("union", (-(S19 - 3.0), -(S19 - 2.0), -(S19 - 1.0)), DIAGONAL, (0.21, 0.16, 0.11)),
                            _box("subtract", (-(S19 - 3.0), -(S19 - 2.0), -(S19 - 1.2)), I3, (0.1, 0.4, 0.1))], 100),
    "many_256": (H13, _many_boxes(H13), 1000),
    "subtract_alone": (H, [_box("subtract", (0, 0, 0), I3, (0.2, 0.2, 0.2))], 0),
}


@pytest.mark.parametrize("cloud", ["empty", "nan"])
@pytest.mark.parametrize("name", list(SOLID_CASES))
def test_solids_only_exact(e3d, name, cloud):
    h, solids, least = SOLID_CASES[name]
    if cloud == "empty":
        xyz, nrm = NO_XYZ, NO_XYZ
    else:                                                             # points that do not contribute: the same as none
        xyz = np.array([[np.nan, 0, 0], [0.1, 0.1, 0.1], [0, np.inf, 0]], F)
        nrm = np.array([[0, 0, 1], [0, 0, 0], [0, 0, 1]], F)
    v, t, c, M = _compare(e3d, xyz, nrm, h, F(2) * h, solids, exact=True)
    assert (c["count"] == 0).all() and (c["weight"] == 0).all()
    assert len(t) >= least and (least > 0 or len(t) == 0)
    if name == "subtract_alone":
        assert len(c["ijk"]) == 0
    if name in ("axis_aligned", "diagonal", "near_plus_2_19"):
        closed, euler, _ = sr.mesh_stats(v, t)
        assert closed and euler == 2
    if name.startswith("near_"):
        assert np.abs(c["ijk"]).max() > 2 ** 19 - 100


# ---- cloud plus solids ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cloud(name):
    if name == "sphere":
        xyz, nrm = sr.fibonacci_sphere()
        return xyz, nrm
    return oriented_cloud(int(name), seed=100 + int(name))


@functools.lru_cache(maxsize=None)
def _scan(name, ratio):
    xyz, nrm = _cloud(name)
    return sr.field(xyz, nrm, H, F(ratio) * H)


def _cloud_solids(radius):
    """Operation lists around a sphere of the given radius at the origin (the clouds' centres are within 0.03 of it)."""
    r = radius
    overlap = _box("union", (r, 0.02, -0.03), GENERIC, (0.4 * r, 0.3 * r, 0.25 * r))
    cap = _box("subtract", (0.01, -0.02, r), I3, (0.8 * r, 0.8 * r, 0.3 * r))
    return {
        "union_overlapping": [overlap],
        "subtract_cap": [cap],
        "subtract_everything": [_box("subtract", (0, 0, 0), DIAGONAL, (4 * r, 4 * r, 4 * r))],
        "touches_nothing": [_box("subtract", (5.0, 5.0, 5.0), GENERIC, (0.2, 0.2, 0.2))],
        "union_far_away": [_box("union", (-3.0, -2.0, -1.5), GENERIC, (0.17, 0.12, 0.21))],
        "union_then_subtract": [overlap, cap, _box("subtract", (r, 0.0, 0.0), I3, (0.15 * r, 0.6 * r, 0.1 * r))],
        "subtract_then_union": [_box("subtract", (r, 0.0, 0.0), I3, (0.15 * r, 0.6 * r, 0.1 * r)), cap, overlap],
    }


CLOUD_CASES = [("sphere", 1.0), ("sphere", 2.0), ("sphere", 3.5)] + [(str(n), ratio) for n in (1, 63, 64, 65, 4000) for ratio in (1.0, 2.0, 3.5)] + [("20000", 2.0)]


@pytest.mark.parametrize("name,ratio", CLOUD_CASES)
def test_cloud_with_solids(e3d, name, ratio):
    xyz, nrm = _cloud(name)
    scan = _scan(name, ratio)
    plain = e3d.reconstruct_surface(xyz, nrm, H, F(ratio) * H, return_corners=True)
    results = {}
    for what, solids in _cloud_solids(0.3 if name == "sphere" else 0.5).items():
        v, t, c, M = _compare(e3d, xyz, nrm, H, F(ratio) * H, solids, scan=scan)
        results[what] = (v, t, c)
        if what == "subtract_everything":
            assert len(t) == 0 and np.array_equal(c["ijk"], plain[2]["ijk"]) and (c["f"] > 0).all()
        if what == "touches_nothing":
            assert v.tobytes() == plain[0].tobytes() and t.tobytes() == plain[1].tobytes() and c["f"].tobytes() == plain[2]["f"].tobytes()
        if what == "union_far_away":
            assert (c["count"] == 0).sum() > 500 and c["ijk"].min() < -50 and len(t) > len(plain[1])
            seen = c["count"] > 0
            assert c["f"][seen].tobytes() == plain[2]["f"].tobytes()                   # the cloud's part does not notice the enlarged origin
        if what == "union_overlapping":
            assert (c["count"] == 0).any() and len(c["ijk"]) > len(plain[2]["ijk"])
        if what == "subtract_cap":
            assert np.array_equal(c["ijk"], plain[2]["ijk"]) and (c["f"] >= plain[2]["f"]).all()
    if name in ("sphere", "4000", "20000"):
        assert not np.array_equal(results["union_then_subtract"][1], results["subtract_then_union"][1])       # the order shows
        assert (results["subtract_cap"][2]["f"] > plain[2]["f"]).any()


def test_two_walls_with_a_window_through_both(e3d):
    """The two sheets 3 h apart of tests/test_gpu_surface.py (a slab seen from both sides) and a subtracted box through both."""
    rng = np.random.default_rng(3 + 20)
    g = (np.stack(np.meshgrid(np.arange(40), np.arange(40), indexing="ij"), -1).reshape(-1, 2) * 0.0125 + rng.normal(0, 0.002, (1600, 2)))
    z0 = 0.0131
    lower = np.concatenate([g, np.full((1600, 1), z0) + rng.normal(0, 0.0005, (1600, 1))], 1)
    upper = np.concatenate([g, np.full((1600, 1), z0 + 3.0 * float(H)) + rng.normal(0, 0.0005, (1600, 1))], 1)
    xyz = np.concatenate([lower, upper]).astype(F)
    nrm = np.concatenate([np.tile([[0, 0, -1]], (1600, 1)), np.tile([[0, 0, 1]], (1600, 1))]).astype(F)
    window = [_box("subtract", (0.25, 0.24, z0 + 1.5 * float(H)), I3, (0.08, 0.11, 0.4))]
    plain = e3d.reconstruct_surface(xyz, nrm, H, F(2) * H)
    v, t, c, M = _compare(e3d, xyz, nrm, H, F(2) * H, window)
    assert len(t) > 0 and len(t) != len(plain[1])                      # two holes in the sheets, a rim through the slab
    # no vertex is left well inside the window, on either sheet
    inside = (np.abs(v[:, 0] - 0.25) < 0.08 - float(H)) & (np.abs(v[:, 1] - 0.24) < 0.11 - float(H))
    assert not inside.any()
    pv = plain[0]
    assert ((np.abs(pv[:, 0] - 0.25) < 0.08 - float(H)) & (np.abs(pv[:, 1] - 0.24) < 0.11 - float(H))).sum() >= 4


# ---- identity, repeatability, kernel groups ------------------------------------------------------------------------------------------
FIVE = ("grid", "candidates", "field", "corners", "extract")


def test_no_operations_is_the_plain_call(e3d):
    xyz, nrm = _cloud("4000")
    ta, tb = {}, {}
    a = e3d.reconstruct_surface(xyz, nrm, H, F(2) * H, return_corners=True, timings=ta)
    b = e3d.reconstruct_surface(xyz, nrm, H, F(2) * H, return_corners=True, timings=tb, solids=[])
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and len(a[1]) > 0
    for key in ("ijk", "f", "weight", "count", "cell_ijk"):
        assert a[2][key].tobytes() == b[2][key].tobytes()
    assert list(ta) == list(tb) == [g + "_ms" for g in FIVE]
    v, t, c = e3d.reconstruct_surface(NO_XYZ, NO_XYZ, H, F(2) * H, return_corners=True, solids=[])
    assert v.shape == (0, 3) and t.shape == (0, 3) and len(c["ijk"]) == 0


def test_two_calls_identical_bytes_and_six_kernel_groups(e3d):
    xyz, nrm = _cloud("20000")
    solids = _cloud_solids(0.5)["union_then_subtract"] + _cloud_solids(0.5)["union_far_away"]
    tm = {}
    a = e3d.reconstruct_surface(xyz, nrm, H, F(2) * H, return_corners=True, timings=tm, solids=solids)
    b = e3d.reconstruct_surface(xyz, nrm, H, F(2) * H, return_corners=True, solids=solids)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and len(a[1]) > 1000
    for key in ("ijk", "f", "weight", "count", "cell_ijk"):
        assert a[2][key].tobytes() == b[2][key].tobytes()
    assert list(tm) == [g + "_ms" for g in FIVE + ("solids",)]
    assert all(np.isfinite(x) and x >= 0 for x in tm.values()) and tm["solids_ms"] > 0 and tm["field_ms"] > 0
    # a subtract alone ends early on an empty cloud and still names six groups
    tm = {}
    e3d.reconstruct_surface(NO_XYZ, NO_XYZ, H, F(2) * H, timings=tm, solids=[_box("subtract", (0, 0, 0), I3, (1, 1, 1))])
    assert list(tm)[-1] == "solids_ms" and len(tm) == 6


# ---- refusals, each followed by a call that works ------------------------------------------------------------------------------------
def test_refusals_and_recovery(e3d):
    xyz, nrm, h, R = sr.one_point_case()
    good = _box("union", (0.3, 0.3, 0.3), GENERIC, (0.1, 0.1, 0.1))
    sheared = I3.copy(); sheared[0, 1] = 1e-6
    mirrored = np.diag([1.0, 1.0, -1.0])
    scaled = I3 * (1.0 + 1e-8)
    two20 = float(2 ** 20) * float(h)
    bad_lists = {
        "257 operations": [good] * 257,
        "kind 7": [good, (7,) + good[1:]],
        "zero extent": [_box("union", (0, 0, 0), I3, (0.1, 0.0, 0.1))],
        "negative extent": [_box("subtract", (0, 0, 0), I3, (0.1, 0.1, -0.1))],
        "NaN extent": [_box("union", (0, 0, 0), I3, (np.nan, 0.1, 0.1))],
        "infinite extent": [_box("union", (0, 0, 0), I3, (0.1, np.inf, 0.1))],
        "NaN centre": [_box("subtract", (0, np.nan, 0), I3, (0.1, 0.1, 0.1))],
        "infinite rotation": [_box("union", (0, 0, 0), np.where(I3 > 0, np.inf, 0.0), (0.1, 0.1, 0.1))],
        "sheared": [_box("union", (0, 0, 0), sheared, (0.1, 0.1, 0.1))],
        "scaled": [_box("union", (0, 0, 0), scaled, (0.1, 0.1, 0.1))],
        "mirrored": [_box("union", (0, 0, 0), mirrored, (0.1, 0.1, 0.1))],
        "box at 2^20 h": [_box("union", (0, two20, 0), I3, (0.1, 0.1, 0.1))],
        "subtract box at -2^20 h": [_box("subtract", (-two20, 0, 0), I3, (0.1, 0.1, 0.1))],
        "band reaches 2^20 h": [_box("union", (0, 0, two20 - 4.5 * float(h)), I3, (float(h), float(h), float(h)))],
    }
    for what, solids in bad_lists.items():
        with pytest.raises(e3d.E3DError):
            e3d.reconstruct_surface(xyz, nrm, h, R, solids=solids)
        v, t = e3d.reconstruct_surface(xyz, nrm, h, R, solids=[good])
        assert len(v) > 21 and len(t) > 24, what
    # 256 operations, a rotation off by 1e-10 and a box whose band ends just below 2^20 h are accepted
    e3d.reconstruct_surface(xyz, nrm, h, R, solids=[good] * 256)
    e3d.reconstruct_surface(xyz, nrm, h, R, solids=[_box("union", (0, 0, 0), I3 * (1.0 + 1e-11), (0.1, 0.1, 0.1))])
    v, t = e3d.reconstruct_surface(NO_XYZ, NO_XYZ, h, R, solids=[_box("union", (0, 0, two20 - 8.0 * float(h)), I3, (float(h), float(h), float(h)))])
    assert len(t) > 0


def test_span_of_cloud_and_solids(e3d):
    """The key holds 21 bits per axis relative to the lowest lattice coordinate: a cloud and a solid 2^21 - 36 steps apart or more are
    refused together though each alone is fine.  A cloud at -2^19 h with a box at 2^20 h - 8 h spans 1.5 * 2^20 steps: that fits."""
    _, nrm, h, R = sr.one_point_case()
    hh = float(h)
    box = [_box("union", (0.0, 0.0, float(2 ** 20) * hh - 8.0 * hh), I3, (hh, hh, hh))]
    low = np.array([[0.5 * hh, 0.5 * hh, -(float(2 ** 20) - 8.5) * hh]], F)
    assert abs(float(low[0, 2])) / hh < 2 ** 20
    assert len(e3d.reconstruct_surface(low, nrm, h, R)[1]) > 0          # each alone works
    assert len(e3d.reconstruct_surface(NO_XYZ, NO_XYZ, h, R, solids=box)[1]) > 0
    with pytest.raises(e3d.E3DError, match="span"):
        e3d.reconstruct_surface(low, nrm, h, R, solids=box)
    with pytest.raises(e3d.E3DError, match="span"):                     # a subtract counts for the span too
        e3d.reconstruct_surface(low, nrm, h, R, solids=[("subtract",) + box[0][1:]])
    mid = np.array([[0.5 * hh, 0.5 * hh, -(float(2 ** 19) - 0.5) * hh]], F)
    v, t, c, M = _compare(e3d, mid, nrm, h, R, box)
    assert len(t) > 24 and int(c["ijk"][:, 2].max()) - int(c["ijk"][:, 2].min()) > 3 * 2 ** 19 - 16


# ---- end to end: the tool, then the mesh as occlusion geometry -------------------------------------------------------------------
def _wall():
    """Points on the lattice corners of the plane y = 16 h (exact in f32), normals -y: f == 0 on that plane and t == 0 on every
    crossing edge, so the wall's vertices do not depend on the order of the sums."""
    i = np.arange(-12, 13)
    xz = np.stack(np.meshgrid(i, i, indexing="ij"), -1).reshape(-1, 2).astype(F) * H
    xyz = np.stack([xz[:, 0], np.full(len(xz), F(16) * H, F), xz[:, 1]], 1).astype(F)
    return xyz, np.tile(np.array([[0, -1, 0]], F), (len(xyz), 1))


BOX_LINE = "union box 0.013 0.313 -0.021  %s  0.3 0.3 0.3\n"


def _run_tool(tmp_path, cloud, script_text, tag):
    mesh = str(tmp_path / ("surface_%s.ply" % tag))
    args = [os.path.join(BIN, "SurfaceReconstructor"), "--point_normal_cloud_path", cloud, "--output_path", mesh, "--voxel_size", "0.05",
            "--support_radius", "0.1", "--timings"]
    if script_text is not None:
        script = tmp_path / ("boxes_%s.txt" % tag)
        script.write_text(script_text)
        args += ["--csg_script", str(script)]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert ("[timings] solids" in r.stderr) == (script_text is not None)
    return mesh


def test_tool_with_script_and_occlusion_depth(e3d, tmp_path):
    from reg_util import camera_params, look_at_pose, pyramid_u8, quat_from_R
    xyz, nrm = _wall()
    scan = sr.field(xyz, nrm, H, F(0.1))
    assert int(sr.ambiguous(scan).sum()) == 0
    cloud = str(tmp_path / "wall.ply")
    _write_ply_27(cloud, xyz, nrm)
    meshes = {}
    for tag, quat in (("identity", "1 0 0 0"), ("diagonal", "0.5 0.5 0.5 0.5"), ("generic", "0.8 0.2 -0.4 0.4")):
        text = "# a box the scanner did not see\n" + BOX_LINE % quat
        mesh = _run_tool(tmp_path, cloud, text, tag)
        M = cr.apply_solids(scan, cr.parse_script(text), H)
        M.update(sr.extract(M, H))
        nv, nf, body = cr.read_ply_body(mesh)
        assert nv == len(M["vertices"]) and nf == len(M["triangles"]) and nf > 500
        if tag == "generic":
            V = np.frombuffer(body, "<f4", 3 * nv).reshape(-1, 3)
            bound = 1e-5 * float(H) + float(np.spacing(F(np.abs(M["vertices"]).max())))
            assert np.abs(V.astype(np.float64) - M["vertices"].astype(np.float64)).max() <= bound
            assert body[12 * nv:] == cr.ply_mesh_body(M["vertices"], M["triangles"])[12 * nv:]
        else:
            assert body == cr.ply_mesh_body(M["vertices"], M["triangles"])            # byte for byte
        V = np.frombuffer(body, "<f4", 3 * nv).reshape(-1, 3).copy()
        T = np.frombuffer(body, np.dtype([("c", "u1"), ("i", "<i4", 3)]), nf, 12 * nv)["i"].astype(np.uint32)
        meshes[tag] = (V, T)
    plain = _run_tool(tmp_path, cloud, None, "plain")
    nv, nf, body = cr.read_ply_body(plain)
    gv, gt = e3d.reconstruct_surface(xyz, nrm, H, F(0.1))
    assert body == cr.ply_mesh_body(gv, gt)
    meshes["plain"] = (gv, gt)
    # a cloud file with zero points: the box alone
    empty = str(tmp_path / "empty.ply")
    _write_ply_27(empty, NO_XYZ, NO_XYZ)
    text = BOX_LINE % "0.5 0.5 0.5 0.5"
    nv, nf, body = cr.read_ply_body(_run_tool(tmp_path, empty, text, "empty"))
    M = cr.reconstruct(NO_XYZ, NO_XYZ, H, F(0.1), cr.parse_script(text))
    assert nf > 100 and body == cr.ply_mesh_body(M["vertices"], M["triangles"])

    # the meshes as occlusion geometry of a pinhole view from y = -1.2 along +y: the wall is 2.0 away, the box's face at
    # y = 0.313 - 0.15 is 1.363 away; 1e-3 is the depth renderer's own test tolerance (tests/test_gpu_reg.py)
    W, Hh, fx = 160, 120, 150.0
    params = camera_params(0, fx, fx, W / 2, Hh / 2)
    R0, t = look_at_pose((0.013, -1.2, -0.021), (0.013, 0.8, -0.021))
    q = quat_from_R(R0)
    depth = {}
    for tag in ("identity", "diagonal", "plain"):
        V, T = meshes[tag]
        P = e3d.RegProblem(e3d.default_reg_params(image_scale_count=1, point_neighbor_count=5))
        P.set_intrinsics(0, W, Hh, params, 0, 1, camera_type=0)
        P.set_image(0, 0, pyramid_u8(np.zeros((Hh, W), np.uint8), 1)); P.set_image_pose(0, q, t)
        assert P.add_occlusion_mesh(V, T) == 1
        P.set_occlusion_options(0.05, 100.0, False)
        depth[tag] = float(P.render_depth(0, 0, (Hh, W))[Hh // 2, W // 2])
    print("centre depths", depth)
    assert abs(depth["identity"] - 1.363) < 1e-3 and abs(depth["diagonal"] - 1.363) < 1e-3
    assert abs(depth["plain"] - 2.0) < 1e-3
