"""numpy restatement of the PointCloudEditor operations (include/e3d_hip.h, e3d_edit_*), written from the rules stated there:
every f32 step runs on float32 arrays and every f64 step on float64 arrays, in the stated order (numpy does not contract a
multiplication and an addition into one operation).  Test infrastructure only."""
from types import SimpleNamespace

import numpy as np

F = np.float32


def make_view(width, height, camera_T_object=None, min_depth=0.1, max_depth=100.0):
    """RenderWidget::SetFreeOrbitViewport's intrinsics for a width x height window."""
    T = np.eye(4, dtype=F)[:3] if camera_T_object is None else np.asarray(camera_T_object, F)[:3, :4].copy()
    return SimpleNamespace(width=int(width), height=int(height), fx=F(height), fy=F(height), cx=F(0.5 * width - 0.5), cy=F(0.5 * height - 0.5),
                           T=T, min_depth=F(min_depth), max_depth=F(max_depth))


def project(view, xyz):
    """-> (in depth range, pixel x, pixel y, camera z), all per point; pixels are meaningless where out of range."""
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    r = view.T
    with np.errstate(all="ignore"):
        cx = ((r[0, 0] * x + r[0, 1] * y) + r[0, 2] * z) + r[0, 3]
        cy = ((r[1, 0] * x + r[1, 1] * y) + r[1, 2] * z) + r[1, 3]
        cz = ((r[2, 0] * x + r[2, 1] * y) + r[2, 2] * z) + r[2, 3]
        in_range = (cz >= view.min_depth) & (cz <= view.max_depth)
        px = (view.fx * (cx / cz) + view.cx) + F(0.5)
        py = (view.fy * (cy / cz) + view.cy) + F(0.5)
    assert px.dtype == F and cz.dtype == F
    return in_range, px, py, cz


def polygon_edges(polygon):
    """The closed polygon's edges that can count: (x1, y1, x2, y2) with y1 < y2."""
    P = np.asarray(polygon, np.float64).reshape(-1, 2)
    out = []
    for i in range(len(P)):
        (x1, y1), (x2, y2) = P[i], P[(i + 1) % len(P)]
        if y1 == y2:
            continue
        if y2 < y1:
            x1, y1, x2, y2 = x2, y2, x1, y1
        out.append((np.float64(x1), np.float64(y1), np.float64(x2), np.float64(y2)))
    return out


def points_in_polygon(px, py, polygon):
    """Odd-even rule in f64; px, py may be f32 (promoted)."""
    x = np.asarray(px).astype(np.float64)
    y = np.asarray(py).astype(np.float64)
    parity = np.zeros(x.shape, bool)
    with np.errstate(all="ignore"):
        for x1, y1, x2, y2 in polygon_edges(polygon):
            rows = np.flatnonzero((y >= y1) & (y < y2))          # the crossing is only worked out where the edge's y range holds
            if rows.size:
                slope = (x2 - x1) / (y2 - y1)
                parity[rows[x1 + slope * (y[rows] - y1) <= x[rows]]] ^= True
    return parity


def points_on_boundary(px, py, polygon):
    """Exactly on an edge or vertex of the closed polygon (exact for the integer coordinates the tie clouds use)."""
    x = np.asarray(px).astype(np.float64)
    y = np.asarray(py).astype(np.float64)
    P = np.asarray(polygon, np.float64).reshape(-1, 2)
    on = np.zeros(x.shape, bool)
    with np.errstate(all="ignore"):
        for i in range(len(P)):
            (x1, y1), (x2, y2) = P[i], P[(i + 1) % len(P)]
            cross = (x2 - x1) * (y - y1) - (y2 - y1) * (x - x1)
            on |= (cross == 0) & (x >= min(x1, x2)) & (x <= max(x1, x2)) & (y >= min(y1, y2)) & (y <= max(y1, y2))
    return on


def lasso(view, xyz, polygon, mode="replace", selection=None, depth=None):
    """-> bool flags after the call.  selection: the flags before (add / remove)."""
    n = np.asarray(xyz).reshape(-1, 3).shape[0]
    old = np.zeros(n, bool) if selection is None else np.asarray(selection, bool).copy()
    if len(np.asarray(polygon).reshape(-1, 2)) < 3:
        return old
    in_range, px, py, cz = project(view, xyz)
    hit = in_range & points_in_polygon(px, py, polygon)
    if depth is not None:
        depth = np.asarray(depth, F)
        with np.errstate(all="ignore"):
            ix = np.clip(np.trunc(np.where(hit, px, 0)), 0, view.width - 1).astype(np.int64)
            iy = np.clip(np.trunc(np.where(hit, py, 0)), 0, view.height - 1).astype(np.int64)
            d = depth[iy, ix]
            hidden = np.isfinite(d) & (d < F(0.99) * cz)
        hit &= ~hidden
    if mode == "replace":
        return hit
    if mode == "add":
        return old | hit
    assert mode == "remove"
    return old & ~hit


def plane_through(points):
    """Eigen::Hyperplane<float, 3>::Through(p0, p1, p2) in f32 -> (normal[3], offset); ValueError where Eigen would go to its SVD."""
    p0, p1, p2 = [np.asarray(p, F) for p in np.asarray(points, F).reshape(3, 3)]
    v0, v1 = p2 - p0, p1 - p0
    n = np.array([v0[1] * v1[2] - v0[2] * v1[1], v0[2] * v1[0] - v0[0] * v1[2], v0[0] * v1[1] - v0[1] * v1[0]], F)
    norm3 = lambda a: np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
    norm = norm3(n)
    if not norm > norm3(v0) * norm3(v1) * np.finfo(F).eps:
        raise ValueError("collinear points")
    n = n / norm
    offset = -((p0[0] * n[0] + p0[1] * n[1]) + p0[2] * n[2])
    assert n.dtype == F and offset.dtype == F
    return n, offset


def beyond_plane(view, xyz, points, camera_position_object, limit_to_visible=False):
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    n, offset = plane_through(points)
    c = np.asarray(camera_position_object, F)
    if ((n[0] * c[0] + n[1] * c[1]) + n[2] * c[2]) + offset < 0:
        n, offset = -n, -offset
    with np.errstate(all="ignore"):
        dist = ((n[0] * xyz[:, 0] + n[1] * xyz[:, 1]) + n[2] * xyz[:, 2]) + offset
        sel = dist < 0
        if limit_to_visible:
            in_range, px, py, _ = project(view, xyz)
            sel &= in_range & (px >= 0) & (py >= 0) & (px < F(view.width)) & (py < F(view.height))
    return sel


def pick(view, xyz, clicks):
    """-> (index[m] int64 (-1: none), squared pixel distance[m] f32 (+inf: none))."""
    in_range, px, py, _ = project(view, xyz)
    clicks = np.asarray(clicks, np.float64).reshape(-1, 2)
    idx = np.full(len(clicks), -1, np.int64)
    dist = np.full(len(clicks), np.inf, F)
    for c, (kx, ky) in enumerate(clicks):
        with np.errstate(all="ignore"):
            dx = px.astype(np.float64) - kx
            dy = py.astype(np.float64) - ky
            d = (dx * dx + dy * dy).astype(F)
        d = np.where(in_range & (d < np.inf), d, F(np.inf))      # NaN and out of range never win
        if len(d) and d.min() < np.inf:
            idx[c] = int(np.argmin(d))                           # the first of equal minima: the lowest index
            dist[c] = d[idx[c]]
    return idx, dist


def look_at_pose(look_from, look_at):
    """camera_T_world of render_widget.cc:832-843 (up = +z) as a 3 x 4 f32 matrix."""
    look_from, look_at = np.asarray(look_from, F), np.asarray(look_at, F)
    forward = look_at - look_from
    forward = forward / np.linalg.norm(forward)
    right = np.cross(forward, np.array([0, 0, 1], F))
    right = right / np.linalg.norm(right)
    up = np.cross(right, forward)
    world_R_camera = np.stack([right, -up, forward], axis=1).astype(np.float64)
    R = world_R_camera.T
    t = -R @ look_from.astype(np.float64)
    return np.concatenate([R, t[:, None]], axis=1).astype(F)
