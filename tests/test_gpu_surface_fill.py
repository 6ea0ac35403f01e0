"""Hole filling of the SurfaceReconstructor on the GPU (e3d_surface_reconstruct_filled, bin/SurfaceReconstructor --fill_holes) against
the numpy restatement tests/surface_fill_ref.py.

The rules are bit-defined (f64, fixed neighbour order, sums that start at +0.0), so the comparison starts from the library's own scan
field: a call with N = 0 and return_corners gives ijk and f; fill() of the restatement runs on those bits, the solids and the
extraction of tests/surface_csg_ref.py / tests/surface_ref.py follow, and the call with N must give the same corner set, f,
corner_filled, vertex cells, triangles and vertex_filled (np.array_equal) and vertices within the existing vertex tolerance (1e-5 h
plus one f32 ulp of the largest coordinate).  Without solids the sources of the N call equal the N = 0 call byte for byte."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import surface_csg_ref as cr
import surface_fill_ref as fr
import surface_ref as sr
from cli_util import BIN
from test_gpu_surface import _write_ply_27, oriented_cloud

pytestmark = pytest.mark.gpu

F = np.float32
H = sr.H
h = float(H)
I3 = np.eye(3)
NO_XYZ = np.zeros((0, 3), F)
NS = (1, 2, 3, 4, 5, 8, 9, 17, 32)                  # growth crosses one, two and several brick faces
S19 = float(2 ** 19) * h
FIVE = ("grid", "candidates", "field", "corners", "extract")
CORNER_KEYS = ("ijk", "f", "weight", "count", "cell_ijk")


def _scan_of(corners):
    return {"ijk": corners["ijk"], "f": corners["f"], "count": corners["count"], "W": corners["weight"]}


def _compare(e3d, cloud, N, plain, G, solids=None, timings=None):
    """The call with N against the restatement G = fill(scan of the N = 0 call, N); returns (vertices, triangles, corners, M)."""
    xyz, nrm, hh, R = cloud
    M = fr.finish(_scan_of(plain[2]), N, list(solids or ()), hh, G=G)
    v, t, c = e3d.reconstruct_surface(xyz, nrm, hh, R, return_corners=True, solids=solids, fill_iterations=N, timings=timings)
    assert v.dtype == F and t.dtype == np.uint32 and c["corner_filled"].dtype == bool and c["vertex_filled"].dtype == bool
    assert np.array_equal(c["ijk"], M["ijk"]), (len(c["ijk"]), len(M["ijk"]))
    assert np.array_equal(c["corner_filled"], M["filled"]), (int(c["corner_filled"].sum()), int(M["filled"].sum()))
    assert np.array_equal(c["f"], M["f"]), int((c["f"] != M["f"]).sum())
    assert np.array_equal(c["count"], M["count"]) and np.array_equal(c["weight"], M["W"])
    assert (c["count"][c["corner_filled"]] == 0).all() and (c["weight"][c["corner_filled"]] == 0).all()
    assert np.array_equal(c["cell_ijk"], M["cell_ijk"]), (len(c["cell_ijk"]), len(M["cell_ijk"]))
    assert np.array_equal(t, M["triangles"])
    assert np.array_equal(c["vertex_filled"], M["vertex_filled"])
    if len(v):
        bound = 1e-5 * float(hh) + float(np.spacing(F(np.abs(M["vertices"]).max())))
        assert np.abs(v.astype(np.float64) - M["vertices"].astype(np.float64)).max() <= bound
    if not solids:
        src = ~c["corner_filled"]
        assert np.array_equal(c["ijk"][src], plain[2]["ijk"])
        for key in ("f", "weight", "count"):
            assert c[key][src].tobytes() == plain[2][key].tobytes()
    return v, t, c, M


# ---- the clouds, their N = 0 call and the restatement's iterations: computed once ------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cloud(name):
    if name == "sphere":
        return fr.capped_sphere_case()
    if name == "wall":
        return fr.wall_with_hole_case()
    if name == "wall_ratio_1":
        return fr.wall_with_hole_case(ratio=1.0)
    if name == "wall_ratio_3.5":
        return fr.wall_with_hole_case(ratio=3.5)
    if name == "wall_brick_corner":                                     # the hole's centre on a brick corner: (8, -4, 4) cells
        return fr.wall_with_hole_case(shift=np.array([0.4, -0.2, 0.2]) - fr.WALL_OFFSET)
    if name == "wall_negative":
        return fr.wall_with_hole_case(shift=(-3.0, -2.0, -1.5))
    if name == "wall_plus_2_19":
        return fr.wall_with_hole_case(n=10000, size=0.8, hole=0.3, shift=(S19 - 3.0, S19 - 2.0, S19 - 1.0))
    if name == "wall_minus_2_19":
        return fr.wall_with_hole_case(n=10000, size=0.8, hole=0.3, shift=(-(S19 - 3.0), -(S19 - 2.0), -(S19 - 1.0)))
    if name == "two_walls":                                              # the two sheets 3 h apart of tests/test_gpu_surface_csg.py
        rng = np.random.default_rng(3 + 20)
        g = (np.stack(np.meshgrid(np.arange(40), np.arange(40), indexing="ij"), -1).reshape(-1, 2) * 0.0125 + rng.normal(0, 0.002, (1600, 2)))
        z0 = 0.0131
        lower = np.concatenate([g, np.full((1600, 1), z0) + rng.normal(0, 0.0005, (1600, 1))], 1)
        upper = np.concatenate([g, np.full((1600, 1), z0 + 3.0 * h) + rng.normal(0, 0.0005, (1600, 1))], 1)
        nrm = np.concatenate([np.tile([[0, 0, -1]], (1600, 1)), np.tile([[0, 0, 1]], (1600, 1))]).astype(F)
        return np.concatenate([lower, upper]).astype(F), nrm, H, F(2) * H
    if name == "wall_nan":                                               # every seventh point or normal spoilt: they contribute nothing
        xyz, nrm, hh, R = fr.wall_with_hole_case(n=12000)
        xyz, nrm = xyz.copy(), nrm.copy()
        xyz[0::28, 1] = np.nan; nrm[7::28] = 0; nrm[14::28, 2] = np.nan; xyz[21::28, 0] = np.inf
        return xyz, nrm, hh, R
    xyz, nrm = oriented_cloud(int(name), seed=100 + int(name)) if int(name) else (NO_XYZ, NO_XYZ)
    return xyz, nrm, H, F(2) * H


_PLAIN = {}


def _plain(e3d, name):
    """(N = 0 call with corners, {N: fill of its scan field for every N of NS})"""
    if name not in _PLAIN:
        xyz, nrm, hh, R = _cloud(name)
        plain = e3d.reconstruct_surface(xyz, nrm, hh, R, return_corners=True)
        _PLAIN[name] = (plain, fr.fill_all(_scan_of(plain[2]), NS))
    return _PLAIN[name]


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("name", ["sphere", "wall"])
def test_exact_against_the_restatement(e3d, name, N):
    plain, G = _plain(e3d, name)
    v, t, c, M = _compare(e3d, _cloud(name), N, plain, G[N])
    assert c["corner_filled"].any() and c["vertex_filled"].any() and len(t) > len(plain[1])
    # the closure properties of tests/test_surface_fill_host.py, on the library's result
    if name == "sphere":
        assert len(fr.boundary_edges(plain[1])) == 24
        closed, euler, volume = sr.mesh_stats(v, t)
        assert (closed and euler == 2) == (N >= 6)
        assert fr.components(len(v), t) == 1
        if N >= 6:
            assert abs(volume - 0.1158) < 5e-4 and 589 <= int(c["corner_filled"].sum()) <= 592
    else:
        w = fr.to_wall_frame(v)
        near = np.hypot(w[:, 0], w[:, 1]) < 0.4
        be = fr.boundary_edges(t)
        around = int((near[be[:, 0]] & near[be[:, 1]]).sum())
        assert around == (12 if N == 3 else 0) or N < 3
        assert fr.components(len(v), t) == 1
        grown = float(plain[0][:, 0].min()) - float(v[:, 0].min())
        assert abs(grown - N * h) < 1e-5                                # the extent along the tilt axis: h per iteration


@pytest.mark.parametrize("name,N", [("wall_ratio_1", 3), ("wall_ratio_1", 9), ("wall_ratio_3.5", 3), ("wall_ratio_3.5", 9), ("wall_brick_corner", 5),
                                    ("wall_brick_corner", 9), ("wall_negative", 5), ("wall_plus_2_19", 5), ("wall_minus_2_19", 9), ("two_walls", 4),
                                    ("two_walls", 17), ("wall_nan", 6), ("0", 4), ("1", 4), ("63", 5), ("64", 5), ("65", 5), ("65", 32)])
def test_exact_on_the_edge_cases(e3d, name, N):
    cloud = _cloud(name)
    xyz, nrm, hh, R = cloud
    plain = e3d.reconstruct_surface(xyz, nrm, hh, R, return_corners=True)
    v, t, c, M = _compare(e3d, cloud, N, plain, fr.fill(_scan_of(plain[2]), N))
    if name == "0":
        assert len(c["ijk"]) == 0 and len(v) == 0 and len(t) == 0 and len(c["corner_filled"]) == 0       # no error
    else:
        assert len(t) > 0 and c["corner_filled"].any()
    if name.startswith("wall_") and "2_19" in name:
        assert np.abs(c["ijk"]).max() > 2 ** 19 - 100
    if name == "wall_negative":
        assert c["ijk"].max() < 0
    if name == "wall_brick_corner":
        lo, hi = c["ijk"][c["corner_filled"]].min(0), c["ijk"][c["corner_filled"]].max(0)
        assert (lo < np.array([8, -4, 4])).all() and (hi > np.array([8, -4, 4])).all()      # filled corners in all eight bricks around it


# ---- fill, then the solids ----------------------------------------------------------------------------------------------------------------
def _many_boxes(count=256):
    """`count` boxes of 1 to 4 cells per side around the wall's hole, every third one subtracted, three rotations in turn."""
    rng = np.random.default_rng(256)
    generic, diagonal = cr.quat_to_rotation(0.8, 0.2, -0.4, 0.4), cr.quat_to_rotation(0.5, 0.5, 0.5, 0.5)
    ops = []
    for i in range(count):
        centre = fr.WALL_OFFSET + rng.uniform(-9, 9, 3) * np.array([h, h, 0.3 * h])
        ops.append(("subtract" if i % 3 == 2 else "union", centre, (I3, generic, diagonal)[i % 3], rng.uniform(0.5, 2.0, 3) * h))
    return ops


def _solid_lists():
    Q = fr.wall_frame()
    through = ("subtract", fr.WALL_OFFSET, Q, np.array([0.15, 0.15, 0.5]))
    inside = ("union", fr.WALL_OFFSET + 0.1 * Q[:, 2], Q, np.array([0.12, 0.12, 0.1]))
    return {"subtract_through": [through], "union_inside": [inside], "union_then_subtract": [inside, through], "subtract_then_union": [through, inside],
            "many_256": _many_boxes()}


@pytest.mark.parametrize("what", list(_solid_lists()))
def test_fill_then_solids(e3d, what):
    solids = _solid_lists()[what]
    plain, G = _plain(e3d, "wall")
    tm = {}
    v, t, c, M = _compare(e3d, _cloud("wall"), 8, plain, G[8], solids=solids, timings=tm)
    assert list(tm) == [g + "_ms" for g in FIVE + ("solids", "fill")] and tm["fill_ms"] > 0 and tm["solids_ms"] > 0
    w = fr.to_wall_frame(v)
    window = (np.abs(w[:, 0]) < 0.15 - h) & (np.abs(w[:, 1]) < 0.15 - h)
    if what in ("subtract_through", "union_then_subtract"):
        assert not window.any()                                        # the script re-opens what the fill closed
    if what in ("union_inside", "subtract_then_union"):
        assert (window & (np.abs(w[:, 2] - 0.2) < h)).sum() >= 9        # the box's top
    if what == "subtract_then_union":
        other = _compare(e3d, _cloud("wall"), 8, plain, G[8], solids=_solid_lists()["union_then_subtract"])
        assert not np.array_equal(other[1], t)                         # the order shows
    if what == "many_256":
        assert ((c["count"] == 0) & ~c["corner_filled"]).any() and c["corner_filled"].any()


# ---- identity, kernel groups, repeatability -------------------------------------------------------------------------------------------------
def _raw_filled_call(e3d, xyz, nrm, hh, R, N):
    """e3d_surface_reconstruct_filled itself, without operations: (vertices, cells, triangles, ijk, f, weight, count, group names)."""
    lib = e3d.lib()
    xyz = np.ascontiguousarray(xyz, F); nrm = np.ascontiguousarray(nrm, F)
    handle = lib.e3d_surface_reconstruct_filled(C.c_void_p(xyz.ctypes.data), C.c_void_p(nrm.ctypes.data), len(xyz), float(hh), float(R), int(N), None, 0)
    assert handle
    try:
        nc, nv, nt = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        lib.e3d_surface_counts(handle, C.byref(nc), C.byref(nv), C.byref(nt))
        v = np.zeros((nv.value, 3), F); cells = np.zeros((nv.value, 3), np.int32); t = np.zeros((nt.value, 3), np.uint32)
        assert lib.e3d_surface_get_mesh(handle, C.c_void_p(v.ctypes.data), C.c_void_p(cells.ctypes.data), C.c_void_p(t.ctypes.data)) == 0
        ijk = np.zeros((nc.value, 3), np.int32); f = np.zeros(nc.value); wgt = np.zeros(nc.value); cnt = np.zeros(nc.value, np.int32)
        assert lib.e3d_surface_get_corners(handle, *(C.c_void_p(a.ctypes.data) for a in (ijk, f, wgt, cnt))) == 0
        cf = np.ones(nc.value, np.uint8); vf = np.ones(nv.value, np.uint8)
        assert lib.e3d_surface_get_fill(handle, C.c_void_p(cf.ctypes.data), C.c_void_p(vf.ctypes.data)) == 0
        ms = (C.c_float * 16)(); names = (C.c_char_p * 16)()
        g = lib.e3d_surface_kernel_ms(handle, ms, names, 16)
        return v, cells, t, ijk, f, wgt, cnt, cf, vf, [names[i].decode() for i in range(g)]
    finally:
        lib.e3d_surface_destroy(handle)


def test_zero_iterations_through_the_new_entry_point_is_the_plain_call(e3d):
    xyz, nrm, hh, R = _cloud("sphere")
    tm = {}
    a = e3d.reconstruct_surface(xyz, nrm, hh, R, return_corners=True, timings=tm)
    v, cells, t, ijk, f, wgt, cnt, cf, vf, names = _raw_filled_call(e3d, xyz, nrm, hh, R, 0)
    assert v.tobytes() == a[0].tobytes() and t.tobytes() == a[1].tobytes() and len(t) > 0
    for got, key in ((ijk, "ijk"), (f, "f"), (wgt, "weight"), (cnt, "count"), (cells, "cell_ijk")):
        assert got.tobytes() == a[2][key].tobytes()
    assert tuple(names) == FIVE and list(tm) == [g + "_ms" for g in FIVE]
    assert not cf.any() and not vf.any()
    assert "corner_filled" not in a[2]


def test_six_groups_with_fill_last_and_two_calls_identical(e3d):
    xyz, nrm, hh, R = _cloud("wall")
    ta = {}
    a = e3d.reconstruct_surface(xyz, nrm, hh, R, return_corners=True, fill_iterations=9, timings=ta)
    b = e3d.reconstruct_surface(xyz, nrm, hh, R, return_corners=True, fill_iterations=9)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and len(a[1]) > 1000
    for key in CORNER_KEYS + ("corner_filled", "vertex_filled"):
        assert a[2][key].tobytes() == b[2][key].tobytes()
    assert list(ta) == [g + "_ms" for g in FIVE + ("fill",)]
    assert all(np.isfinite(x) and x >= 0 for x in ta.values()) and ta["fill_ms"] > 0
    # an empty cloud ends early and still names the groups of its call
    tm = {}
    v, t, c = e3d.reconstruct_surface(NO_XYZ, NO_XYZ, hh, R, return_corners=True, fill_iterations=3, timings=tm)
    assert len(v) == 0 and len(t) == 0 and list(tm) == [g + "_ms" for g in FIVE + ("fill",)]
    tm = {}
    box = [("union", np.zeros(3), I3, np.array([0.1, 0.1, 0.1]))]
    v, t, c = e3d.reconstruct_surface(NO_XYZ, NO_XYZ, hh, R, return_corners=True, fill_iterations=3, solids=box, timings=tm)
    assert list(tm) == [g + "_ms" for g in FIVE + ("solids", "fill")] and len(t) > 0 and not c["corner_filled"].any()
    alone = e3d.reconstruct_surface(NO_XYZ, NO_XYZ, hh, R, solids=box)
    assert alone[0].tobytes() == v.tobytes() and alone[1].tobytes() == t.tobytes()


# ---- refusals, each followed by a call that works ------------------------------------------------------------------------------------
def test_refusals_and_recovery(e3d):
    xyz, nrm, hh, R = sr.one_point_case()

    def works():
        v, t, c = e3d.reconstruct_surface(xyz, nrm, hh, R, return_corners=True, fill_iterations=2)
        assert len(t) > 0 and c["corner_filled"].any()

    for N in (-1, 33):
        with pytest.raises(e3d.E3DError, match="fill_iterations"):
            e3d.reconstruct_surface(xyz, nrm, hh, R, fill_iterations=N)
        works()
    e3d.reconstruct_surface(xyz, nrm, hh, R, fill_iterations=32)
    # a source within N + 4 steps of the range: the point's voxel is 2^20 - 11, so N + 4 = 11 steps reach 2^20 and 10 do not
    q = float(hh)
    high = np.array([[0.5 * q, 0.5 * q, (float(2 ** 20) - 10.5) * q]], F)
    assert int(np.floor(float(high[0, 2]) / q)) == 2 ** 20 - 11
    assert len(e3d.reconstruct_surface(high, nrm, hh, R)[1]) > 0
    with pytest.raises(e3d.E3DError, match=r"2\^20"):
        e3d.reconstruct_surface(high, nrm, hh, R, fill_iterations=7)
    works()
    assert len(e3d.reconstruct_surface(high, nrm, hh, R, fill_iterations=6)[1]) > 0
    with pytest.raises(e3d.E3DError, match=r"2\^20"):
        e3d.reconstruct_surface(-high, nrm, hh, R, fill_iterations=8)
    works()
    # a span too large only once grown: voxels -2^20 + 38 and 2^20 - 42 span 2^21 - 80; both ends stay in range for N = 32, the
    # grown box spans 2^21 - 8 and does not leave the 36 steps the keys need
    two = np.array([[0.5 * q, 0.5 * q, (-float(2 ** 20) + 38.5) * q], [0.5 * q, 0.5 * q, (float(2 ** 20) - 41.5) * q]], F)
    vox = np.floor(two[:, 2].astype(np.float64) / q).astype(np.int64)
    assert vox[0] == -2 ** 20 + 38 and vox[1] == 2 ** 20 - 42
    both = np.tile(nrm, (2, 1))
    assert len(e3d.reconstruct_surface(two, both, hh, R)[1]) > 0
    with pytest.raises(e3d.E3DError, match="span"):
        e3d.reconstruct_surface(two, both, hh, R, fill_iterations=32)
    works()
    assert len(e3d.reconstruct_surface(two, both, hh, R, fill_iterations=8)[1]) > 0


# ---- end to end: the tool, then the mesh as occlusion geometry -------------------------------------------------------------------
def _ray_hit(V, T, origin, direction):
    """The nearest intersection of a ray with a triangle mesh (Moeller-Trumbore in f64): the distance along the ray."""
    V = V.astype(np.float64); T = T.astype(np.int64)
    a, e1, e2 = V[T[:, 0]], V[T[:, 1]] - V[T[:, 0]], V[T[:, 2]] - V[T[:, 0]]
    p = np.cross(direction, e2)
    det = (e1 * p).sum(1)
    ok = np.abs(det) > 1e-14
    inv = 1.0 / np.where(ok, det, 1.0)
    tv = origin - a
    u = (tv * p).sum(1) * inv
    q = np.cross(tv, e1)
    w = (q @ direction) * inv
    d = (e2 * q).sum(1) * inv
    return float(d[ok & (u >= 0) & (w >= 0) & (u + w <= 1) & (d > 0)].min())


def test_tool_with_fill_and_occlusion_depth(e3d, tmp_path):
    from reg_util import camera_params, look_at_pose, pyramid_u8, quat_from_R
    xyz, nrm, hh, R = _cloud("wall")
    Q = fr.wall_frame()
    rear, rear_n, _, _ = fr.wall_with_hole_case(n=20000, hole=0.0, seed=8, shift=-1.0 * Q[:, 2])      # a whole wall 1 m behind
    xyz = np.concatenate([xyz, rear]); nrm = np.concatenate([nrm, rear_n])
    cloud = str(tmp_path / "walls.ply")
    _write_ply_27(cloud, xyz, nrm)
    mesh, filled_mesh = str(tmp_path / "surface.ply"), str(tmp_path / "filled.ply")
    r = subprocess.run([os.path.join(BIN, "SurfaceReconstructor"), "--point_normal_cloud_path", cloud, "--output_path", mesh, "--voxel_size", "0.05",
                        "--support_radius", "0.1", "--fill_holes", "6", "--filled_mesh_path", filled_mesh, "--timings"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    gv, gt, gc = e3d.reconstruct_surface(xyz, nrm, hh, R, return_corners=True, fill_iterations=6)
    nv, nf, body = cr.read_ply_body(mesh)
    assert body == cr.ply_mesh_body(gv, gt) and nf > 5000                # byte for byte
    flagged = gc["vertex_filled"][gt.astype(np.int64)].any(1)
    nv2, nf2, body2 = cr.read_ply_body(filled_mesh)
    assert nv2 == nv and nf2 == int(flagged.sum()) and 0 < nf2 < nf
    assert body2 == cr.ply_mesh_body(gv, gt[flagged])                    # exactly the flagged triangles, in order
    line = "Filled: %d lattice corners, %d vertices, %d triangles." % (int(gc["corner_filled"].sum()), int(gc["vertex_filled"].sum()), nf2)
    assert line in r.stderr and "[timings] fill" in r.stderr
    pv, pt = e3d.reconstruct_surface(xyz, nrm, hh, R)

    # The meshes as occlusion geometry of a pinhole view from 1.2 in front of the hole's centre along the wall's normal.  1e-3 is the
    # depth renderer's own test tolerance (tests/test_gpu_reg.py) against the mesh it is given; the patch itself lies within a cell
    # of the wall's plane (the extension runs along lattice directions), the rear wall is 1 m behind
    W, Hh, fx = 160, 120, 150.0
    params = camera_params(0, fx, fx, W / 2, Hh / 2)
    eye = fr.WALL_OFFSET + 1.2 * Q[:, 2]
    R0, tr = look_at_pose(tuple(eye), tuple(fr.WALL_OFFSET - 1.0 * Q[:, 2]))
    depth, want = {}, {}
    for tag, (V, T) in (("filled", (gv, gt)), ("plain", (pv, pt))):
        P = e3d.RegProblem(e3d.default_reg_params(image_scale_count=1, point_neighbor_count=5))
        P.set_intrinsics(0, W, Hh, params, 0, 1, camera_type=0)
        P.set_image(0, 0, pyramid_u8(np.zeros((Hh, W), np.uint8), 1)); P.set_image_pose(0, quat_from_R(R0), tr)
        assert P.add_occlusion_mesh(V, T) == 1
        P.set_occlusion_options(0.05, 100.0, False)
        depth[tag] = float(P.render_depth(0, 0, (Hh, W))[Hh // 2, W // 2])
        want[tag] = _ray_hit(V, T, eye, -Q[:, 2])
    print("centre depths", depth, "ray", want)
    assert abs(want["filled"] - 1.2) < h and abs(want["plain"] - 2.2) < 1e-3
    assert abs(depth["filled"] - want["filled"]) < 1e-3 and abs(depth["plain"] - want["plain"]) < 1e-3
