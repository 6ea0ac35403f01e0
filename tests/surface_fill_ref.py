"""numpy restatement of the hole filling of the SurfaceReconstructor (include/e3d_hip.h, e3d_surface_reconstruct_filled)
on top of tests/surface_ref.py (scan field, extraction) and tests/surface_csg_ref.py (solids), which stay the arbiters of their parts.

fill() works on a dense lattice around the corners of a field dict and applies the rules literally: per iteration the X and X1 bits,
then growth and smoothing from state t - 1 alone.  Sums are np.where chains in the neighbour order -x, +x, -y, +y, -z, +z that start
at +0.0, so every bit of f is defined and the GPU result is compared with np.array_equal."""
import numpy as np

import surface_csg_ref as cr
import surface_ref as sr

# the six face neighbours in the order of the rules: (axis, step)
NEIGHBOURS = ((0, -1), (0, 1), (1, -1), (1, 1), (2, -1), (2, 1))


def _at(A, axis, step):
    """A at the neighbour `step` along `axis` of every corner.  The lattice has a margin no defined corner reaches, so what np.roll
    wraps around is undefined and zero."""
    return np.roll(A, -step, axis)


def fill_all(F, Ns):
    """fill(F, N) for every N of Ns in one run of max(Ns) iterations: {N: dict}."""
    Ns = sorted({int(N) for N in Ns})
    assert Ns and 0 <= Ns[0] and Ns[-1] <= 32
    ijk = np.asarray(F["ijk"], np.int64).reshape(-1, 3)
    extras = [k for k in ("S", "W", "T", "count") if k in F]
    plain = {k: np.array(F[k]) for k in extras}
    plain.update(ijk=ijk.astype(np.int32), f=np.array(F["f"], np.float64), filled=np.zeros(len(ijk), bool))
    if len(ijk) == 0:
        return {N: plain for N in Ns}
    out = {0: plain} if Ns[0] == 0 else {}
    top = Ns[-1]
    lo = ijk.min(0) - (top + 2)
    shape = tuple(int(x) for x in ijk.max(0) - lo + top + 3)
    at = tuple((ijk - lo).T)
    D = np.zeros(shape, bool)
    f = np.zeros(shape, np.float64)
    D[at] = True
    f[at] = F["f"]
    source = D.copy()
    for t in range(1, top + 1):
        neg = f < 0
        X = np.zeros(shape, bool)
        for axis, step in NEIGHBOURS:
            X |= D & _at(D, axis, step) & (_at(neg, axis, step) != neg)
        X1 = X.copy()
        for axis, step in NEIGHBOURS:
            X1 |= _at(X, axis, step)
        X1 &= D
        near = np.zeros(shape, bool)
        s = np.zeros(shape, np.float64)                                  # +0.0
        c = np.zeros(shape, np.int64)
        for axis, step in NEIGHBOURS:
            near |= _at(X1, axis, step)
            Dn = _at(D, axis, step)
            s = np.where(Dn, s + _at(f, axis, step), s)
            c += Dn
        grow = ~D & near                                                 # a neighbour with X1 is defined: c >= 1
        smooth = D & ~source
        with np.errstate(invalid="ignore", divide="ignore"):
            grown = s / c.astype(np.float64)
            smoothed = (s + f) / (c + 1).astype(np.float64)
        f = np.where(grow, grown, np.where(smooth, smoothed, f))
        D = D | grow
        if t not in Ns:
            continue
        k, j, i = np.nonzero(D.transpose(2, 1, 0))                       # ascending (k, j, i)
        got = np.stack([i, j, k], 1) + lo
        filled = ~source[i, j, k]
        G = {"ijk": got.astype(np.int32), "f": f[i, j, k], "filled": filled}
        assert np.array_equal(got[~filled], ijk)                         # the sources, in the ascending (k, j, i) they came in
        for name in extras:
            v = np.zeros(len(got), np.asarray(F[name]).dtype)
            v[~filled] = F[name]
            G[name] = v
        out[t] = G
    for A in (D[0], D[-1], D[:, 0], D[:, -1], D[:, :, 0], D[:, :, -1]):  # the margin was wide enough
        assert not A.any()
    return out


def fill(F, N):
    """N iterations on the field F (dict with ijk[c, 3] in ascending (k, j, i) and f[c]: surface_ref.field or the library's corners).
    Returns a dict of the corners defined afterwards in ascending (k, j, i): ijk int32, f, filled (bool: defined by the fill), and
    S, W, T, count where F has them (0 at filled corners)."""
    return fill_all(F, [N])[int(N)]


def _with_filled(F, filled_ijk):
    """F with the flag `filled` for the corners listed in filled_ijk."""
    ijk = F["ijk"].astype(np.int64)
    both = np.concatenate([ijk, np.asarray(filled_ijk, np.int64).reshape(-1, 3)])
    origin = both.min(0, initial=0) - 2
    F["filled"] = np.isin(sr._pack(ijk, origin), sr._pack(np.asarray(filled_ijk, np.int64).reshape(-1, 3), origin))
    return F


def vertex_filled(F, M):
    """Per vertex of the extraction M of the field F (with F["filled"]): does a crossing edge of its cell have a filled endpoint."""
    edges = M["edges"].astype(np.int64)
    cells = M["cell_ijk"].astype(np.int64)
    out = np.zeros(len(cells), bool)
    if len(edges) == 0:
        return out
    ijk = F["ijk"].astype(np.int64)
    origin = np.minimum(ijk.min(0), cells.min(0)) - 2
    keys = sr._pack(ijk, origin)
    a = edges[:, :3]
    d = edges[:, 3]
    b = a.copy()
    b[np.arange(len(a)), d] += 1
    flag = F["filled"][np.searchsorted(keys, sr._pack(a, origin))] | F["filled"][np.searchsorted(keys, sr._pack(b, origin))]
    cell_keys = sr._pack(cells, origin)
    for ou, ov in sr._QUAD:
        c = a.copy()
        c[np.arange(len(a)), (d + 1) % 3] += ou
        c[np.arange(len(a)), (d + 2) % 3] += ov
        np.logical_or.at(out, np.searchsorted(cell_keys, sr._pack(c, origin)), flag)
    return out


def finish(F, N, solids, voxel_size, G=None):
    """Fill, then the solids, then the extraction, from a scan field F: dict of the extraction (vertices, cell_ijk, triangles, edges,
    t), the corners (ijk, f, filled, count, W, ...), vertex_filled[v] and triangle_filled[t].  G: fill(F, N) where it is at hand."""
    G = dict(fill(F, N) if G is None else G)
    for name in ("S", "W", "T", "count"):                                # surface_csg_ref.apply_solids carries all of them
        G.setdefault(name, np.zeros(len(G["ijk"]), np.int32 if name == "count" else np.float64))
    filled_ijk = G["ijk"][G["filled"]]
    H = cr.apply_solids(G, solids, voxel_size) if solids else G
    H = _with_filled(dict(H), filled_ijk)
    M = sr.extract(H, voxel_size)
    M.update(H)
    M["vertex_filled"] = vertex_filled(H, M)
    M["triangle_filled"] = M["vertex_filled"][M["triangles"].astype(np.int64)].any(1) if len(M["triangles"]) else np.zeros(0, bool)
    return M


def reconstruct(xyz, normals, voxel_size, support_radius, N, solids=()):
    scan = sr.field(xyz, normals, voxel_size, support_radius)
    M = finish(scan, N, list(solids), voxel_size)
    M["scan"] = scan
    return M


# ---- shared cases and mesh measures ------------------------------------------------------------------------------------------------
def capped_sphere_case():
    """The Fibonacci sphere of surface_ref without the cap z > centre + 0.22: 3467 points."""
    xyz, nrm, h, R = sr.sphere_case()
    keep = xyz[:, 2].astype(np.float64) <= 0.007 + 0.22
    return xyz[keep], nrm[keep], h, R


WALL_TILT = 0.2
WALL_OFFSET = np.array([0.011, 0.017, 0.023])


def wall_frame():
    """Rotation by WALL_TILT about x: columns are the wall's axes (u, v, normal) in world coordinates."""
    c, s = np.cos(WALL_TILT), np.sin(WALL_TILT)
    return np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])


def wall_with_hole_case(n=40000, size=1.6, hole=0.6, seed=7, shift=(0.0, 0.0, 0.0), ratio=2.0):
    """n seeded points on a size x size wall through WALL_OFFSET + shift, tilted 0.2 rad about x, normals along the wall's +normal,
    without those in the centred hole x hole square."""
    rng = np.random.default_rng(seed)
    uv = rng.uniform(-0.5 * size, 0.5 * size, (n, 2))
    uv = uv[(np.abs(uv[:, 0]) > 0.5 * hole) | (np.abs(uv[:, 1]) > 0.5 * hole)]
    Q = wall_frame()
    xyz = (np.concatenate([uv, np.zeros((len(uv), 1))], 1) @ Q.T + WALL_OFFSET + np.asarray(shift, np.float64)).astype(np.float32)
    nrm = np.tile(Q[:, 2].astype(np.float32), (len(xyz), 1))
    return xyz, nrm, sr.H, np.float32(ratio) * sr.H


def to_wall_frame(vertices, shift=(0.0, 0.0, 0.0)):
    return (np.asarray(vertices, np.float64) - WALL_OFFSET - np.asarray(shift, np.float64)) @ wall_frame()


def boundary_edges(triangles):
    """Undirected edges used by exactly one triangle: [e, 2] vertex indices."""
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    e = np.sort(np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]]), 1)
    if len(e) == 0:
        return e
    u, n = np.unique(e, axis=0, return_counts=True)
    return u[n == 1]


def components(n_vertices, triangles):
    """The number of connected components among the vertices that a triangle uses."""
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    parent = np.arange(n_vertices)
    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]]]):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[ra] = rb
    used = np.unique(tri)
    return len({find(x) for x in used})
