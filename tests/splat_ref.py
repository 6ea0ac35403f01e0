"""CPU restatement of SplatCreator (src/exe/splat_creator.cc:75-235) for the splat tests: numpy f32 arithmetic in the
reference's operation order, no FMA (numpy never contracts).

* ericson_sq: igl::point_simplex_squared_distance (thirdparty/igl/point_simplex_squared_distance.cpp, Ericson ch. 5) for
  arrays of (point, triangle) pairs, the regions tested in igl's order; dot products and squaredNorm as e0 + (e1 + e2);
* mesh_min_sq: igl::AABB::squared_distance as the brute-force minimum with `<` from +inf (ties: the lowest triangle id);
* unit_orthogonal / cross / corners: Eigen 3.3's unitOrthogonal, cross and the corner sums of :167-178;
* splats: the whole tool, with the splat radius from the oracle's kNN (FLANN f32 squared distances).
"""
import numpy as np

F = np.float32
MARGIN_SCALE = F(1.0 / 65536.0)      # the index's delta = 2^-16 * max|coordinate|


def _dot(a0, a1, a2, b0, b1, b2):
    return a0 * b0 + (a1 * b1 + a2 * b2)


def ericson_sq(p, a, b, c):
    """p, a, b, c: (m, 3) float32 -> (m,) float32 computed squared distances."""
    p = np.asarray(p, F); a = np.asarray(a, F); b = np.asarray(b, F); c = np.asarray(c, F)
    with np.errstate(all="ignore"):
        px, py, pz = p[:, 0], p[:, 1], p[:, 2]
        ax, ay, az = a[:, 0], a[:, 1], a[:, 2]
        bx, by, bz = b[:, 0], b[:, 1], b[:, 2]
        cx, cy, cz = c[:, 0], c[:, 1], c[:, 2]
        abx, aby, abz = bx - ax, by - ay, bz - az
        acx, acy, acz = cx - ax, cy - ay, cz - az
        apx, apy, apz = px - ax, py - ay, pz - az
        d1 = _dot(abx, aby, abz, apx, apy, apz)
        d2 = _dot(acx, acy, acz, apx, apy, apz)
        bpx, bpy, bpz = px - bx, py - by, pz - bz
        d3 = _dot(abx, aby, abz, bpx, bpy, bpz)
        d4 = _dot(acx, acy, acz, bpx, bpy, bpz)
        vc = d1 * d4 - d3 * d2
        cpx, cpy, cpz = px - cx, py - cy, pz - cz
        d5 = _dot(abx, aby, abz, cpx, cpy, cpz)
        d6 = _dot(acx, acy, acz, cpx, cpy, cpz)
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        e43 = d4 - d3
        e56 = d5 - d6
        ab_ne = (ax != bx) | (ay != by) | (az != bz)
        left = np.ones(p.shape[0], bool)

        def take(cond):
            nonlocal left
            sel = left & cond
            left = left & ~cond
            return sel

        r_a = take((d1 <= 0) & (d2 <= 0))
        r_b = take((d3 >= 0) & (d4 <= d3))
        r_ab = take(ab_ne & (vc <= 0) & (d1 >= 0) & (d3 <= 0))
        r_c = take((d6 >= 0) & (d5 <= d6))
        r_ac = take((vb <= 0) & (d2 >= 0) & (d6 <= 0))
        r_bc = take((va <= 0) & (e43 >= 0) & (e56 >= 0))
        face = left
        v_ab = d1 / (d1 - d3)
        w_ac = d2 / (d2 - d6)
        w_bc = e43 / (e43 + e56)
        denom = F(1.0) / ((va + vb) + vc)
        v_f = vb * denom
        w_f = vc * denom
        q = np.empty_like(p)
        for k, (A, B, Cc, AB, AC) in enumerate(((ax, bx, cx, abx, acx), (ay, by, cy, aby, acy), (az, bz, cz, abz, acz))):
            qk = np.where(r_a, A, 0).astype(F)
            qk = np.where(r_b, B, qk)
            qk = np.where(r_ab, A + v_ab * AB, qk)
            qk = np.where(r_c, Cc, qk)
            qk = np.where(r_ac, A + w_ac * AC, qk)
            qk = np.where(r_bc, B + w_bc * (Cc - B), qk)
            qk = np.where(face, (A + AB * v_f) + AC * w_f, qk)
            q[:, k] = qk
        dx, dy, dz = px - q[:, 0], py - q[:, 1], pz - q[:, 2]
        return _dot(dx, dy, dz, dx, dy, dz)


def ericson_region(p, a, b, c):
    """Index (0 A, 1 B, 2 AB, 3 C, 4 AC, 5 BC, 6 face) of the region igl's routine takes for one pair (test helper)."""
    p, a, b, c = (np.asarray(x, F) for x in (p, a, b, c))
    ab, ac, ap = b - a, c - a, p - a
    d1 = _dot(*ab, *ap); d2 = _dot(*ac, *ap)
    if d1 <= 0 and d2 <= 0:
        return 0
    bp = p - b
    d3 = _dot(*ab, *bp); d4 = _dot(*ac, *bp)
    if d3 >= 0 and d4 <= d3:
        return 1
    vc = d1 * d4 - d3 * d2
    if (a != b).any() and vc <= 0 and d1 >= 0 and d3 <= 0:
        return 2
    cp = p - c
    d5 = _dot(*ab, *cp); d6 = _dot(*ac, *cp)
    if d6 >= 0 and d5 <= d6:
        return 3
    vb = d5 * d2 - d1 * d6
    if vb <= 0 and d2 >= 0 and d6 <= 0:
        return 4
    va = d3 * d6 - d5 * d4
    if va <= 0 and (d4 - d3) >= 0 and (d5 - d6) >= 0:
        return 5
    return 6


def mesh_min_sq(points, V, T, max_sq=np.inf, chunk=1 << 20):
    """Brute force: per point the minimum over all triangles with `<` from +inf (ties: lowest id), +inf / -1 above max_sq."""
    points = np.asarray(points, F); V = np.asarray(V, F); T = np.asarray(T, np.int64)
    n, nt = points.shape[0], T.shape[0]
    best = np.full(n, np.inf, F)
    bid = np.full(n, -1, np.int32)
    if nt == 0:                                                        # an empty mesh: nothing is below +inf
        return best, bid
    per = max(1, chunk // max(nt, 1))
    for s in range(0, n, per):
        e = min(n, s + per)
        P = np.repeat(points[s:e], nt, axis=0)
        tt = np.tile(np.arange(nt), e - s)
        d = ericson_sq(P, V[T[tt, 0]], V[T[tt, 1]], V[T[tt, 2]]).reshape(e - s, nt)
        d = np.where(np.isnan(d), np.inf, d)                      # NaN never wins `<`
        j = np.argmin(d, axis=1)                                   # first (lowest id) of the minimum
        m = d[np.arange(e - s), j]
        ok = m < np.inf
        best[s:e] = np.where(ok, m, np.inf)
        bid[s:e] = np.where(ok, j, -1)
    over = ~(best <= F(max_sq))
    best[over] = np.inf
    bid[over] = -1
    return best, bid


def any_within(points, V, T, thr2):
    """Per point: is some triangle's computed value <= thr2?  Triangles are culled by box with the index's margin
    delta = 2^-16 max(max|mesh coordinate|, max|point coordinate|) (exact for triangles that are not nearly degenerate)."""
    points = np.asarray(points, F); V = np.asarray(V, F); T = np.asarray(T, np.int64)
    n = points.shape[0]
    hit = np.zeros(n, bool)
    if n == 0 or T.shape[0] == 0:
        return hit
    mag = F(np.abs(V[np.isfinite(V).all(1)]).max()) if np.isfinite(V).any() else F(0)
    delta = MARGIN_SCALE * np.maximum(mag, np.abs(points).max(1))
    reach = float(np.sqrt(np.float64(thr2))) + float(delta.max()) * 2 + 1e-6
    lo = V[T].min(1); hi = V[T].max(1)
    order = np.argsort(points[:, 0], kind="stable")
    xs = points[order, 0]
    for t in range(T.shape[0]):
        i0 = np.searchsorted(xs, lo[t, 0] - reach, "left"); i1 = np.searchsorted(xs, hi[t, 0] + reach, "right")
        cand = order[i0:i1]
        cand = cand[~hit[cand]]
        if cand.size == 0:
            continue
        q = points[cand]
        near = ((q[:, 1] >= lo[t, 1] - reach) & (q[:, 1] <= hi[t, 1] + reach) & (q[:, 2] >= lo[t, 2] - reach) & (q[:, 2] <= hi[t, 2] + reach))
        cand = cand[near]
        if cand.size == 0:
            continue
        k = cand.size
        d = ericson_sq(points[cand], np.repeat(V[T[t, 0]][None], k, 0), np.repeat(V[T[t, 1]][None], k, 0), np.repeat(V[T[t, 2]][None], k, 0))
        hit[cand[d <= F(thr2)]] = True
    return hit


def culled_min_sq(Q, V, T, max_sq):
    """restatement minimum (+inf above max_sq) over the triangles whose centroid cell is near the query: every triangle that
    can produce a value <= max_sq has its centroid within sqrt(max_sq) + its own extent of the query"""
    reach = float(np.sqrt(np.float64(max_sq))) + 1e-3
    cen = V[T].mean(1)
    ext = float(np.abs(V[T] - cen[:, None]).max()) + 1e-4
    h = reach + ext
    key = lambda c: (np.floor(c[:, 0] / h).astype(np.int64) * 1_000_003 + np.floor(c[:, 1] / h).astype(np.int64)) * 1_000_033 + np.floor(c[:, 2] / h).astype(np.int64)
    kt = key(cen)
    order = np.argsort(kt, kind="stable")
    ks = kt[order]
    best = np.full(len(Q), np.inf, F)
    bid = np.full(len(Q), -1, np.int64)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                kq = key(Q + np.array([dx, dy, dz], np.float64) * h)
                lo = np.searchsorted(ks, kq, "left"); hi = np.searchsorted(ks, kq, "right")
                cnt = hi - lo
                qi = np.repeat(np.arange(len(Q)), cnt)
                ti = order[np.repeat(lo - np.cumsum(cnt) + cnt, cnt) + np.arange(cnt.sum())]
                for s in range(0, len(qi), 1 << 22):
                    a, b = qi[s:s + (1 << 22)], ti[s:s + (1 << 22)]
                    d = ericson_sq(Q[a], V[T[b, 0]], V[T[b, 1]], V[T[b, 2]])
                    d = np.where(np.isnan(d), np.inf, d)
                    # per query: smaller value, or equal value with lower id
                    o = np.lexsort((b, d, a))
                    a, b, d = a[o], b[o], d[o]
                    first = np.ones(len(a), bool); first[1:] = a[1:] != a[:-1]
                    a, b, d = a[first], b[first], d[first]
                    better = (d < best[a]) | ((d == best[a]) & (d < np.inf) & (b < bid[a]))
                    best[a[better]] = d[better]; bid[a[better]] = b[better]
    over = ~(best <= F(max_sq))
    best[over] = np.inf; bid[over] = -1
    return best, bid


def near_feature_pairs(rng, m):
    """(p, a, b, c) float32 for the tests of the pruning margin: ordinary triangles with vertices in [-2, 2]^3 and a query a few
    tens of ulps -- 10^U(-7, -5) of the triangle's max |coordinate| -- from vertex b or from a point of edge ab, in a random
    direction (half of them perpendicular to ab).  This close the computed edge point a + t ab can land an ulp outside the
    triangle's box on the query's side, which is a visible part of the distance: the input class that needs delta."""
    a, b, c = (rng.uniform(-2, 2, (m, 3)).astype(F) for _ in range(3))
    ab = b.astype(np.float64) - a
    d = rng.normal(size=(m, 3))
    perp = d - (d * ab).sum(1, keepdims=True) * ab / np.maximum((ab * ab).sum(1, keepdims=True), 1e-300)
    d = np.where(rng.random((m, 1)) < 0.5, perp, d)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    ext = np.abs(np.stack([a, b, c], 1)).max((1, 2))[:, None]
    t = np.where(rng.random((m, 1)) < 0.5, 1.0, rng.uniform(0, 1, (m, 1)))
    p = (a + t * ab + 10.0 ** rng.uniform(-7, -5, (m, 1)) * ext * d).astype(F)
    return p, a, b, c


def unit_orthogonal(n):
    """Eigen 3.3 unitOrthogonal of (m, 3) float32 vectors (the 3-vector selector, precision 1e-5f)."""
    n = np.asarray(n, F)
    x, y, z = n[:, 0], n[:, 1], n[:, 2]
    prec = F(1e-5)
    with np.errstate(all="ignore"):
        first = ~(np.abs(x) <= np.abs(z) * prec) | ~(np.abs(y) <= np.abs(z) * prec)
        inv1 = F(1) / np.sqrt(x * x + y * y)
        inv2 = F(1) / np.sqrt(y * y + z * z)
        r = np.empty_like(n)
        r[:, 0] = np.where(first, -y * inv1, F(0))
        r[:, 1] = np.where(first, x * inv1, -z * inv2)
        r[:, 2] = np.where(first, F(0), y * inv2)
    return r, first


def cross(a, b):
    a = np.asarray(a, F); b = np.asarray(b, F)
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def corners(p, n, r):
    """(m, 4, 3) corners TR, BR, BL, TL of splat_creator.cc:170-178."""
    p = np.asarray(p, F); r = np.asarray(r, F)[:, None]
    right, _ = unit_orthogonal(n)
    up = cross(n, right)
    with np.errstate(all="ignore"):
        s = [right + up, right - up, -right - up, -right + up]
        return np.stack([p + r * sk for sk in s], 1)


def splat_radius(xyz, max_splat_size=np.inf):
    """min(sqrtf(d2[4]), max_splat_size) from the oracle's k = 5 search over the finite points (input order, NaN elsewhere)."""
    from oracle import binding as ob
    xyz = np.asarray(xyz, F)
    fin = np.isfinite(xyz).all(1)
    _, dist = ob.knn(xyz[fin], xyz[fin], 5)
    s = np.sqrt(dist[:, 4].astype(F))
    m = F(max_splat_size)
    r = np.full(xyz.shape[0], np.nan, F)
    r[fin] = np.where(m < s, m, s)
    return r


def splats(xyz, normals, V, T, distance_threshold=0.02, max_splat_size=np.inf, cull=True):
    """The tool: (vertices[4m,3], faces[2m,3], add_splat[n], radius[n]) in ascending point order.  cull=False: "within" is the
    full brute-force minimum (mesh_min_sq) <= thr2, with no box culling and no margin delta: nothing shared with the index."""
    xyz = np.asarray(xyz, F); normals = np.asarray(normals, F)
    thr = F(distance_threshold)
    thr2 = thr * thr
    r = splat_radius(xyz, max_splat_size)
    live = np.isfinite(xyz).all(1) & ~np.isnan(normals).any(1)
    r[~live] = np.nan
    add = np.zeros(xyz.shape[0], bool)
    idx = np.nonzero(live)[0]
    C = corners(xyz[idx], normals[idx], r[idx])
    if thr2 < np.inf:
        far = np.zeros(idx.size, bool)
        for q in [xyz[idx]] + [C[:, k] for k in range(4)]:
            fin = np.isfinite(q).all(1)
            within = np.zeros(idx.size, bool)
            within[fin] = any_within(q[fin], V, T, thr2) if cull else (mesh_min_sq(q[fin], V, T, thr2)[0] <= thr2)
            far |= ~within
        add[idx] = far
    verts = C[add[idx]].reshape(-1, 3)
    m = int(add.sum())
    s = np.arange(m, dtype=np.int32)[:, None] * 4
    faces = np.concatenate([s + 2, s + 1, s, s, s + 3, s + 2], 1).reshape(-1, 3)
    return verts, faces, add, r
