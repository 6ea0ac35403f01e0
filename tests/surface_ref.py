"""numpy restatement of the SurfaceReconstructor rules (include/e3d_hip.h, e3d_surface_reconstruct) -- the arbiter of
the GPU tests.  Brute force: every contributing point visits the lattice corners within ceil(R / h) + 1 of its voxel, and the terms
are accumulated per corner.  Besides S, W and the contributor count it reports T = sum |w n.(x - p)| per corner: a corner is
AMBIGUOUS iff 0 < |S| <= 1e-6 T, i.e. iff an f64 sum formed in another order could give f another sign.

Everything is f64 on f32 inputs; the per-term expressions are those of the header, only the order of the sums is free."""
import numpy as np


def _pack(ijk, origin):
    """(k, j, i) sort key of lattice coordinates relative to an origin below all of them: 21 bits per axis."""
    rel = np.asarray(ijk, np.int64) - origin
    assert rel.min(initial=0) >= 0 and rel.max(initial=0) < (1 << 21)
    return (rel[..., 2] << 42) | (rel[..., 1] << 21) | rel[..., 0]


def _unpack(keys, origin):
    m = (1 << 21) - 1
    return (np.stack([keys & m, (keys >> 21) & m, keys >> 42], 1) + origin).astype(np.int32)


def contributing(xyz, normals):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    normals = np.asarray(normals, np.float32).reshape(-1, 3)
    return np.isfinite(xyz).all(1) & np.isfinite(normals).all(1) & (normals != 0).any(1)


def field(xyz, normals, voxel_size, support_radius):
    """The defined corners in ascending (k, j, i): dict of ijk[c, 3], S, W, T, f, count."""
    h = float(np.float32(voxel_size))
    R = float(np.float32(support_radius))
    keep = contributing(xyz, normals)
    p = np.asarray(xyz, np.float32).reshape(-1, 3)[keep].astype(np.float64)
    nr = np.asarray(normals, np.float32).reshape(-1, 3)[keep].astype(np.float64)
    R2 = R * R
    reach = int(np.ceil(R / h)) + 1
    v = np.floor(p / h).astype(np.int64)
    origin = v.min(0, initial=0) - reach - 1
    keys, terms, weights = [], [], []
    for ok in range(-reach, reach + 2):
        for oj in range(-reach, reach + 2):
            for oi in range(-reach, reach + 2):
                c = v + np.array([oi, oj, ok], np.int64)
                x = h * c.astype(np.float64)
                d = x - p
                d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
                m = d2 < R2
                if not m.any():
                    continue
                om = 1.0 - d2[m] / R2
                w = om * om
                dot = (nr[m, 0] * d[m, 0] + nr[m, 1] * d[m, 1]) + nr[m, 2] * d[m, 2]
                keys.append(_pack(c[m], origin))
                terms.append(w * dot)
                weights.append(w)
    if not keys:
        z = np.zeros(0)
        return {"ijk": np.zeros((0, 3), np.int32), "S": z, "W": z, "T": z, "f": z, "count": np.zeros(0, np.int32)}
    keys = np.concatenate(keys); terms = np.concatenate(terms); weights = np.concatenate(weights)
    uniq, inv = np.unique(keys, return_inverse=True)
    S = np.bincount(inv, terms, len(uniq))
    W = np.bincount(inv, weights, len(uniq))
    T = np.bincount(inv, np.abs(terms), len(uniq))
    count = np.bincount(inv, minlength=len(uniq)).astype(np.int32)
    return {"ijk": _unpack(uniq, origin), "S": S, "W": W, "T": T, "f": S / W, "count": count}


def ambiguous(F):
    return (np.abs(F["S"]) > 0) & (np.abs(F["S"]) <= 1e-6 * F["T"])


def _lookup(sorted_keys, keys):
    pos = np.searchsorted(sorted_keys, keys)
    pos[pos >= len(sorted_keys)] = 0
    hit = sorted_keys[pos] == keys if len(sorted_keys) else np.zeros(len(keys), bool)
    return np.where(hit, pos, -1)


# quad cell q of edge (a, d): offsets in (u, v) = ((d + 1) % 3, (d + 2) % 3)
_QUAD = ((-1, -1), (0, -1), (0, 0), (-1, 0))


def extract(F, voxel_size):
    """Crossing edges, vertices and triangles from a field: dict of edges[e, 4] = (i, j, k, d), t[e], vertices[v, 3] f32,
    cell_ijk[v, 3], triangles[2 e, 3] uint32."""
    h = float(np.float32(voxel_size))
    ijk = F["ijk"].astype(np.int64)
    f = F["f"]
    origin = ijk.min(0, initial=0) - 2
    keys = _pack(ijk, origin)
    neg = f < 0
    cross = np.zeros((len(ijk), 3), bool)
    other = np.zeros((len(ijk), 3), np.int64)
    for d in range(3):
        b = ijk.copy()
        b[:, d] += 1
        idx = _lookup(keys, _pack(b, origin)) if len(ijk) else np.zeros(0, np.int64)
        cross[:, d] = (idx >= 0) & (neg != neg[idx])
        other[:, d] = idx
    ec, ed = np.nonzero(cross)                     # ascending corner (= (k, j, i)), then axis
    fa, fb = f[ec], f[other[ec, ed]]
    t = fa / (fa - fb)
    a = ijk[ec]
    point = h * a.astype(np.float64)
    point[np.arange(len(ec)), ed] = point[np.arange(len(ec)), ed] + t * h
    quad_cells = np.zeros((len(ec), 4, 3), np.int64)
    for q, (ou, ov) in enumerate(_QUAD):
        c = a.copy()
        c[np.arange(len(ec)), (ed + 1) % 3] += ou
        c[np.arange(len(ec)), (ed + 2) % 3] += ov
        quad_cells[:, q] = c
    quad_keys = _pack(quad_cells, origin)
    cells = np.unique(quad_keys)
    quad_idx = np.searchsorted(cells, quad_keys)
    # the mean of a cell's crossing points, summed by axis, then offset along v, then along u: cell = a - du e_u - dv e_v
    total = np.zeros((len(cells), 3))
    number = np.zeros(len(cells))
    which = {(1, 1): 0, (0, 1): 1, (0, 0): 2, (1, 0): 3}            # (du, dv) -> q
    for d in range(3):
        for dv in range(2):
            for du in range(2):
                sel = ed == d
                idx = quad_idx[sel, which[(du, dv)]]
                total[idx] += point[sel]
                number[idx] += 1
    vertices = (total / number[:, None]).astype(np.float32) if len(cells) else np.zeros((0, 3), np.float32)
    quads = np.where(neg[ec][:, None], quad_idx, quad_idx[:, ::-1])
    triangles = np.stack([quads[:, [0, 1, 2]], quads[:, [0, 2, 3]]], 1).reshape(-1, 3).astype(np.uint32)
    edges = np.concatenate([a, ed[:, None]], 1).astype(np.int32)
    return {"edges": edges, "t": t, "vertices": vertices, "cell_ijk": _unpack(cells, origin), "triangles": triangles}


def reconstruct(xyz, normals, voxel_size, support_radius):
    F = field(xyz, normals, voxel_size, support_radius)
    M = extract(F, voxel_size)
    M.update(F)
    M["ambiguous"] = ambiguous(F)
    return M


F = np.float32
H = F(0.05)


# ---- shared cases ------------------------------------------------------------------------------------------------------------------
def fibonacci_sphere(n=4000, radius=0.3, centre=(0.013, -0.021, 0.007)):
    """n Fibonacci-lattice points on a sphere with exact outward normals, f32."""
    i = np.arange(n, dtype=np.float64)
    z = (2.0 * i + 1.0) / n - 1.0
    r = np.sqrt(1.0 - z * z)
    phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
    nrm = np.stack([r * np.cos(phi), r * np.sin(phi), z], 1)
    xyz = np.asarray(centre, np.float64) + radius * nrm
    return xyz.astype(np.float32), nrm.astype(np.float32)


def one_point_case():
    """One point in the middle of cell (0, 0, 0), normal +z, R = 2 h."""
    return np.array([[0.5, 0.5, 0.5]], F) * H, np.array([[0, 0, 1]], F), H, F(2) * H


def lattice_plane_case():
    """A 7 x 7 grid of points exactly on lattice corners of the plane z = 0, normals +z, R = 2 h."""
    g = np.arange(-3, 4)
    xy = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    xyz = np.concatenate([xy, np.zeros((len(xy), 1))], 1).astype(F) * H
    return xyz, np.tile(np.array([[0, 0, 1]], F), (len(xyz), 1)), H, F(2) * H


def sphere_case():
    xyz, nrm = fibonacci_sphere()
    return xyz, nrm, H, F(0.1)


def mesh_stats(vertices, triangles):
    """(closed and consistently oriented, V - E + F, signed volume) of a triangle mesh."""
    tri = np.asarray(triangles, np.int64)
    directed = np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]])
    code = directed[:, 0] * (len(vertices) + 1) + directed[:, 1]
    rev = directed[:, 1] * (len(vertices) + 1) + directed[:, 0]
    once = len(np.unique(code)) == len(code)
    closed = once and np.array_equal(np.sort(code), np.sort(rev))
    n_edges = len(np.unique(np.minimum(code, rev)))
    v = np.asarray(vertices, np.float64)
    a, b, c = v[tri[:, 0]], v[tri[:, 1]], v[tri[:, 2]]
    volume = float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)
    return closed, len(vertices) - n_edges + len(tri), volume
