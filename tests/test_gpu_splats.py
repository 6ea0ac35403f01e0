"""SplatCreator on the GPU (e3d_mesh_squared_distance, e3d_create_splats, bin/SplatCreator) against the CPU restatement of
tests/splat_ref.py: distances, triangle ids, flags, radii and splat corners bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import splat_ref as sr
from cli_util import BIN, write_ply_mesh

pytestmark = pytest.mark.gpu

F = np.float32


def _u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- 1. bounded minimum ---------------------------------------------------------------------------------------------
def _soup(seed):
    rng = np.random.default_rng(seed)
    nt = 300
    a = rng.uniform(0, 1, (nt, 3)).astype(F)
    b = (a + rng.normal(0, 0.15, (nt, 3))).astype(F)
    c = (a + rng.normal(0, 0.15, (nt, 3))).astype(F)
    b[:10] = a[:10]                                                   # a == b
    c[10:20] = a[10:20] + F(2) * (b[10:20] - a[10:20])                 # collinear (up to f32 rounding)
    b[20:30] = a[20:30]; c[20:30] = a[20:30]                           # a point
    c[30:40] = b[30:40]                                                # b == c
    c[40:50] = (a[40:50] + b[40:50]) * F(0.5)                          # zero area, midpoint
    # one well-shaped triangle with points in each of Ericson's seven regions
    a[50], b[50], c[50] = (0.4, 0.4, 0.5), (0.8, 0.4, 0.5), (0.4, 0.8, 0.5)
    V = np.stack([a, b, c], 1).reshape(-1, 3)
    T = np.arange(3 * nt, dtype=np.uint32).reshape(nt, 3)
    # shared vertices too: a few triangles index vertices of others
    T[60:70, 1] = T[70:80, 0]
    P = [rng.uniform(-0.2, 1.2, (3000, 3)).astype(F)]
    P.append(V[rng.integers(0, V.shape[0], 300)])                      # exactly on vertices
    e = rng.integers(0, nt, 300)
    t = rng.uniform(0, 1, (300, 1)).astype(F)
    P.append((V[T[e, 0]] + t * (V[T[e, 1]] - V[T[e, 0]])).astype(F))   # on (or next to, by rounding) edges
    P.append(np.array([[0.3, 0.3, 0.6], [0.9, 0.35, 0.55], [0.35, 0.9, 0.45], [0.6, 0.3, 0.52], [0.3, 0.6, 0.48],
                       [0.7, 0.7, 0.6], [0.5, 0.5, 0.51]], F))       # regions A, B, C, AB, AC, BC, face of triangle 50
    return V, T, np.concatenate(P)


@pytest.mark.parametrize("offset", [0.0, 1000.0])
@pytest.mark.parametrize("max_sq", [np.inf, 0.004])
def test_mesh_squared_distance_bit_exact(e3d, offset, max_sq):
    for seed in (1, 2):
        V, T, P = _soup(seed)
        V = (V + F(offset)).astype(F); P = (P + F(offset)).astype(F)
        if seed == 1:
            regions = {sr.ericson_region(p, V[150], V[151], V[152]) for p in P[-7:]}
            assert regions == set(range(7)) or offset != 0.0
        d, i = e3d.mesh_squared_distance(P, V, T, max_sq)
        rd, ri = sr.mesh_min_sq(P, V, T, max_sq)
        assert np.array_equal(_u32(d), _u32(rd)), (np.nonzero(_u32(d) != _u32(rd))[0][:10])
        assert np.array_equal(i, ri)
        if max_sq < np.inf:
            assert np.isinf(d).any() and (d[np.isfinite(d)] <= F(max_sq)).all()


def test_mesh_squared_distance_nonfinite_points_and_vertices(e3d):
    V, T, P = _soup(3)
    V[5] = np.nan                                                     # triangle 1 has a NaN vertex
    P[:4] = [[np.nan, 0, 0], [np.inf, 0, 0], [0, -np.inf, 0], [0, 0, np.nan]]
    d, i = e3d.mesh_squared_distance(P, V, T)
    rd, ri = sr.mesh_min_sq(P, V, T)
    assert np.array_equal(_u32(d), _u32(rd)) and np.array_equal(i, ri)
    assert np.isinf(d[:4]).all() and (i[:4] == -1).all()
    with pytest.raises(e3d.E3DError):
        e3d.mesh_squared_distance(P, V, np.array([[0, 1, V.shape[0]]], np.uint32))


# ---- 2. splats on a synthetic room ----------------------------------------------------------------------------------
def _grid(axes, w_val, u0, u1, v0, v1, nu, nv, base):
    """grid in the plane axis[2] = w_val, u along axes[0], v along axes[1]: vertices, triangles (indices from base)"""
    us = np.linspace(u0, u1, nu, dtype=F); vs = np.linspace(v0, v1, nv, dtype=F)
    Vg = np.empty((nv, nu, 3), F)
    Vg[..., axes[0]] = us[None, :]; Vg[..., axes[1]] = vs[:, None]; Vg[..., axes[2]] = F(w_val)
    idx = np.arange(nv - 1)[:, None] * nu + np.arange(nu - 1)[None, :] + base
    Tg = np.stack([np.stack([idx, idx + 1, idx + nu], -1), np.stack([idx + 1, idx + nu + 1, idx + nu], -1)], 2).reshape(-1, 3)
    return Vg.reshape(-1, 3), Tg


HOLE = (-1.0, 1.0, -0.5, 0.5)          # x and z range of the hole in the wall y = +5 (local frame)


def _room_mesh(res=0.25):
    """the synthetic room's floor and walls in the scan's local frame (origin (5, 5, 1.5), yaw 0) without the cylinders, with
    a hole in the wall y = +5"""
    parts = []
    base = 0
    n10, n3 = int(round(10 / res)) + 1, int(round(3 / res)) + 1
    for axes, w, (u0, u1, v0, v1, nu, nv) in [((0, 1, 2), -1.5, (-5, 5, -5, 5, n10, n10)), ((1, 2, 0), -5, (-5, 5, -1.5, 1.5, n10, n3)),
                                              ((1, 2, 0), 5, (-5, 5, -1.5, 1.5, n10, n3)), ((0, 2, 1), -5, (-5, 5, -1.5, 1.5, n10, n3)),
                                              ((0, 2, 1), 5, (-5, 5, -1.5, 1.5, n10, n3))]:
        Vg, Tg = _grid(axes, w, u0, u1, v0, v1, nu, nv, base)
        if axes == (0, 2, 1) and w == 5:
            cen = Vg[Tg - base].mean(1)
            keep = ~((cen[:, 0] > HOLE[0]) & (cen[:, 0] < HOLE[1]) & (cen[:, 2] > HOLE[2]) & (cen[:, 2] < HOLE[3]))
            Tg = Tg[keep]
        parts.append((Vg, Tg))
        base += Vg.shape[0]
    V = np.concatenate([p[0] for p in parts]); T = np.concatenate([p[1] for p in parts]).astype(np.uint32)
    return V, T


@pytest.fixture(scope="module")
def room(synth):
    xyz, nrm, _ = synth.make_scan(200_000, (5.0, 5.0, 1.5), 0.0, seed=11)
    xyz = xyz.numpy().copy(); nrm = nrm.numpy().copy()
    nrm[[7, 70, 700, 7000]] = np.nan                                  # skipped points
    nrm[[8, 80]] = [np.nan, 0, 1]
    V, T = _room_mesh()
    return xyz, nrm, V, T


def _check_splats(e3d, xyz, nrm, V, T, thr, max_splat):
    gv, gf, ga, gr = e3d.create_splats(xyz, nrm, V, T, thr, max_splat)
    rv, rf, ra, rr = sr.splats(xyz, nrm, V, T, thr, max_splat)
    assert np.array_equal(ga, ra), ("flags differ", np.nonzero(ga != ra)[0][:10])
    assert np.array_equal(_u32(gr), _u32(rr)), "radii differ"
    assert np.array_equal(_u32(gv), _u32(rv)), "splat vertices differ"
    m = int(ga.sum())
    s = np.arange(m)[:, None] * 4
    assert np.array_equal(gf, np.concatenate([s + 2, s + 1, s, s, s + 3, s + 2], 1).reshape(-1, 3))
    assert np.array_equal(gf, rf) and gv.shape == (4 * m, 3)
    return ga, gr


@pytest.mark.parametrize("thr,max_splat", [(0.02, np.inf), (0.01, np.inf), (0.05, np.inf), (0.02, 0.015)])
def test_splats_room(e3d, room, thr, max_splat):
    xyz, nrm, V, T = room
    ga, gr = _check_splats(e3d, xyz, nrm, V, T, thr, max_splat)
    assert not ga[[7, 70, 700, 7000, 8, 80]].any() and np.isnan(gr[[7, 70, 700, 7000, 8, 80]]).all()
    live = ~np.isnan(nrm).any(1)
    # cylinders (radius 0.4 about (cx - 5, cy - 5)), away from the floor: splatted
    on_cyl = np.zeros(len(xyz), bool)
    for cx, cy in ((3.0, 3.0), (7.0, 4.0), (5.0, 7.5)):
        on_cyl |= np.abs(np.hypot(xyz[:, 0] - (cx - 5), xyz[:, 1] - (cy - 5)) - 0.4) < 0.02
    sel = on_cyl & (xyz[:, 2] > -1.4) & live
    assert sel.sum() > 1000 and ga[sel].all()
    # in the hole: splatted
    hole = (np.abs(xyz[:, 1] - 5) < 0.02) & (xyz[:, 0] > HOLE[0] + 0.1) & (xyz[:, 0] < HOLE[1] - 0.1) & (xyz[:, 2] > HOLE[2] + 0.1) & (xyz[:, 2] < HOLE[3] - 0.1) & live
    assert hole.sum() > 50 and ga[hole].all()
    # meshed wall x = +5, away from its edges: not splatted
    wall = (np.abs(xyz[:, 0] - 5) < 0.02) & (np.abs(xyz[:, 1]) < 4.6) & (np.abs(xyz[:, 2]) < 1.1) & ~on_cyl & live
    assert wall.sum() > 1000 and not ga[wall].any()


# ---- 3. small / non-finite clouds -----------------------------------------------------------------------------------
def test_too_few_points_is_an_error(e3d, room):
    _, _, V, T = room
    xyz = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.nan, 0, 0], [0, 0, 1]], F)
    with pytest.raises(e3d.E3DError):
        e3d.create_splats(xyz, np.tile(np.array([[0, 0, 1]], F), (5, 1)), V, T)


def test_nonfinite_points_never_splatted(e3d, room):
    xyz, nrm, V, T = room
    xyz = xyz[:20000].copy(); nrm = nrm[:20000].copy()
    xyz[[3, 30, 300]] = [[np.nan, 0, 0], [np.inf, 1, 1], [0, 0, -np.inf]]
    ga, gr = _check_splats(e3d, xyz, nrm, V, T, 0.02, np.inf)
    assert not ga[[3, 30, 300]].any()


# ---- 4. the tool end to end -----------------------------------------------------------------------------------------
def _write_ply_xyz_normals(path, xyz, nrm):
    with open(path, "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                 "property float normal_x\nproperty float normal_y\nproperty float normal_z\nend_header\n" % len(xyz)).encode())
        f.write(np.concatenate([xyz, nrm], 1).astype("<f4").tobytes())


def test_cli_end_to_end(e3d, room, tmp_path):
    xyz, nrm, V, T = room
    xyz = xyz[:50000]; nrm = nrm[:50000]
    _write_ply_xyz_normals(str(tmp_path / "cloud.ply"), xyz, nrm)
    write_ply_mesh(str(tmp_path / "mesh.ply"), V, T)
    out = tmp_path / "splats.ply"
    r = subprocess.run([os.path.join(BIN, "SplatCreator"), "--point_normal_cloud_path", str(tmp_path / "cloud.ply"), "--mesh_path",
                        str(tmp_path / "mesh.ply"), "--output_path", str(out), "--distance_threshold", "0.02"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    gv, gf, ga, _ = e3d.create_splats(xyz, nrm, V, T, 0.02)
    m = int(ga.sum())
    assert m > 0
    assert "Finished!" in r.stdout
    assert ("Added %d splats." % m) in r.stderr
    data = out.read_bytes()
    hdr = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
           "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (4 * m, 2 * m)).encode()
    assert data[:len(hdr)] == hdr
    body = data[len(hdr):]
    assert len(body) == 4 * m * 12 + 2 * m * 13
    verts = np.frombuffer(body[:48 * m], "<f4").reshape(-1, 3)
    assert np.array_equal(_u32(verts), _u32(gv))
    rec = np.frombuffer(body[48 * m:], dtype=[("c", "u1"), ("i", "<i4", 3)])
    assert (rec["c"] == 3).all() and np.array_equal(rec["i"], gf)
    P = e3d.RegProblem(e3d.default_reg_params())
    P.add_occlusion_mesh(verts, rec["i"].astype(np.uint32))
    # zero splats: a valid empty mesh
    out0 = tmp_path / "none.ply"
    r = subprocess.run([os.path.join(BIN, "SplatCreator"), "--point_normal_cloud_path", str(tmp_path / "cloud.ply"), "--mesh_path",
                        str(tmp_path / "mesh.ply"), "--output_path", str(out0), "--distance_threshold", "1e30"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Added 0 splats." in r.stderr
    assert out0.read_bytes() == (b"ply\nformat binary_little_endian 1.0\nelement vertex 0\nproperty float x\nproperty float y\nproperty float z\n"
                                 b"element face 0\nproperty list uchar int vertex_indices\nend_header\n")


# ---- 5. at size -----------------------------------------------------------------------------------------------------
def test_splats_at_size(e3d, synth):
    import torch
    n = 20_000_000
    xyz, _, _ = synth.make_scan(n, (5.0, 5.0, 1.5), 0.0, seed=5, device="cuda")
    nrm, _ = e3d.normals_knn(xyz, 8)
    xyz = xyz.cpu().numpy()
    V, T = _room_mesh(res=0.006)
    assert T.shape[0] >= 10_000_000
    tm = {}
    gv, gf, ga, gr = e3d.create_splats(xyz, nrm, V, T, 0.02, np.inf, timings=tm)
    print("at size: %d points, %d triangles, %d splats, index %.1f ms, splat pass %.1f ms" % (n, T.shape[0], int(ga.sum()), tm["index_ms"], tm["splat_ms"]))
    rng = np.random.default_rng(0)
    samp = np.sort(rng.choice(n, 100_000, replace=False))
    thr2 = F(0.02) * F(0.02)
    # sampled distances: the bounded minimum (max_sq = thr^2) against the culled restatement
    d, i = e3d.mesh_squared_distance(xyz[samp], V, T, thr2)
    rd, ri = sr.culled_min_sq(xyz[samp], V, T, thr2)
    assert np.array_equal(_u32(d), _u32(rd)) and np.array_equal(i, ri)
    # sampled flags: the five queries of 20000 of them
    fs = samp[:20000]
    live = ~np.isnan(nrm[fs]).any(1)
    r = gr[fs]
    assert np.array_equal(np.isnan(r), ~live)
    C = sr.corners(xyz[fs[live]], nrm[fs[live]], r[live])
    far = np.zeros(live.sum(), bool)
    for q in [xyz[fs[live]]] + [C[:, k] for k in range(4)]:
        qd, _ = sr.culled_min_sq(q.astype(F), V, T, thr2)
        far |= ~(qd <= thr2)
    assert np.array_equal(ga[fs[live]], far)
