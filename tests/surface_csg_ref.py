"""numpy restatement of the box union / subtraction rules of the SurfaceReconstructor (include/e3d_hip.h,
e3d_surface_reconstruct_csg) on top of tests/surface_ref.py, which stays the arbiter of the scan field and of the
extraction.  A solid is (kind, centre[3], rotation[3, 3], half_extent[3]) with kind "union" or "subtract"; its function g is
evaluated in f64 in the header's order, so g is bit-defined and a field made of solids alone is compared exactly."""
import numpy as np

import surface_ref as sr


def box_g(solid, ijk, h):
    """g of one solid at lattice corners ijk[c, 3]: d = x - c, u_m = (Q[0][m] d_0 + Q[1][m] d_1) + Q[2][m] d_2, q_m = |u_m| - a_m,
    g = max(max(q_0, q_1), q_2)."""
    _, centre, rotation, half = solid
    c = np.asarray(centre, np.float64).reshape(3)
    Q = np.asarray(rotation, np.float64).reshape(3, 3)
    a = np.asarray(half, np.float64).reshape(3)
    x = h * np.asarray(ijk, np.int64).astype(np.float64)
    d = x - c
    q = [np.abs((Q[0, m] * d[:, 0] + Q[1, m] * d[:, 1]) + Q[2, m] * d[:, 2]) - a[m] for m in range(3)]
    return np.maximum(np.maximum(q[0], q[1]), q[2])


def band_corners(solid, h):
    """The lattice corners with |g| <= 2 h: all corners of the box's world bounding box grown by 2 h (and two steps), filtered."""
    _, centre, rotation, half = solid
    c = np.asarray(centre, np.float64).reshape(3)
    Q = np.asarray(rotation, np.float64).reshape(3, 3)
    a = np.asarray(half, np.float64).reshape(3)
    e = np.abs(Q) @ (a + 2.0 * h)
    lo = np.floor((c - e) / h).astype(np.int64) - 2
    hi = np.ceil((c + e) / h).astype(np.int64) + 2
    out = []
    ii, jj = np.meshgrid(np.arange(lo[0], hi[0] + 1), np.arange(lo[1], hi[1] + 1), indexing="ij")
    for k in range(int(lo[2]), int(hi[2]) + 1):                      # slab by slab: a 20-cell box needs no 3-D temporary
        ijk = np.stack([ii.ravel(), jj.ravel(), np.full(ii.size, k, np.int64)], 1)
        g = box_g(solid, ijk, h)
        out.append(ijk[np.abs(g) <= 2.0 * h])
    return np.concatenate(out) if out else np.zeros((0, 3), np.int64)


def apply_solids(F, solids, voxel_size):
    """The operation list applied to a scan field F of surface_ref.field: dict of ijk, f, count, W, T (and S) of the corners that are
    defined afterwards, in ascending (k, j, i).  A corner defined by solids alone has count = W = T = S = 0."""
    h = float(np.float32(voxel_size))
    solids = list(solids)
    parts = [F["ijk"].astype(np.int64)] + [band_corners(s, h) for s in solids if s[0] == "union"]
    allc = np.concatenate(parts)
    if len(allc) == 0:
        return {k: F[k] for k in ("ijk", "S", "W", "T", "f", "count")}
    origin = allc.min(0) - 2
    keys = np.unique(sr._pack(allc, origin))
    ijk = sr._unpack(keys, origin).astype(np.int64)
    at = np.searchsorted(keys, sr._pack(F["ijk"].astype(np.int64), origin))
    defined = np.zeros(len(keys), bool)
    out = {}
    for name, dtype in (("S", np.float64), ("W", np.float64), ("T", np.float64), ("f", np.float64), ("count", np.int32)):
        out[name] = np.zeros(len(keys), dtype)
        out[name][at] = F[name]
    defined[at] = True
    f = out["f"]
    for s in solids:
        assert s[0] in ("union", "subtract")
        g = box_g(s, ijk, h)
        if s[0] == "union":
            lower = defined & (g < f)                                  # min(f, g): the first argument on equality
            born = ~defined & (np.abs(g) <= 2.0 * h)
            f[lower] = g[lower]
            f[born] = g[born]
            defined |= born
        else:
            ng = -g
            higher = defined & (ng > f)                                # max(f, -g)
            f[higher] = ng[higher]
    out = {k: v[defined] for k, v in out.items()}
    out["ijk"] = ijk[defined].astype(np.int32)
    return out


def reconstruct(xyz, normals, voxel_size, support_radius, solids):
    """surface_ref.reconstruct with an operation list; "scan" holds the scan field alone (for the ambiguity condition)."""
    scan = sr.field(xyz, normals, voxel_size, support_radius)
    F = apply_solids(scan, solids, voxel_size)
    M = sr.extract(F, voxel_size)
    M.update(F)
    M["scan"] = scan
    return M


def quat_to_rotation(w, x, y, z):
    """The tool's conversion (surface_reconstructor.cc, header comment), in Python floats = f64, each entry as written there."""
    w, x, y, z = float(w), float(x), float(y), float(z)
    n = float(np.sqrt(((w * w + x * x) + y * y) + z * z))
    if not abs(n - 1.0) <= 1e-6:
        raise ValueError("not a unit quaternion")
    w /= n; x /= n; y /= n; z /= n
    return np.array([[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
                     [2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)],
                     [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]])


def parse_script(text):
    """The tool's script format -> solids (full extents halved)."""
    solids = []
    for line in text.split("\n"):
        tok = line.split("#")[0].split()
        if not tok:
            continue
        assert tok[0] in ("union", "subtract") and tok[1] == "box" and len(tok) == 12
        v = [float(t) for t in tok[2:]]
        solids.append((tok[0], np.array(v[0:3]), quat_to_rotation(*v[3:7]), 0.5 * np.array(v[7:10])))
    return solids


def ply_mesh_body(vertices, triangles):
    """The bytes behind end_header of the tool's PLY for a mesh: float x y z per vertex, then uchar 3 + three int32 per face."""
    rec = np.zeros(len(triangles), np.dtype([("c", "u1"), ("i", "<i4", 3)]))
    rec["c"] = 3
    rec["i"] = np.asarray(triangles, np.int64)
    return np.ascontiguousarray(vertices, "<f4").tobytes() + rec.tobytes()


def read_ply_body(path):
    """(vertex count, face count, bytes behind end_header) of a binary little-endian PLY."""
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode().split("\n")
    assert lines[1] == "format binary_little_endian 1.0"
    nv = int([x for x in lines if x.startswith("element vertex")][0].split()[2])
    nf = int([x for x in lines if x.startswith("element face")][0].split()[2])
    return nv, nf, data[end:]
