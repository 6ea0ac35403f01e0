"""CubeMapRenderer restated in numpy f32 (test infrastructure): the yardstick of tests/test_gpu_cubemap.py, itself checked
against hand-computed cases and a naive loop implementation in tests/test_cubemap_host.py.

Six pinhole faces (front, left, back, right, down, up) with fx = fy = cx = cy = size // 2.
  * point pass: r = R_face p (a signed permutation of p), skipped if r.z <= 0; x = (fx * r.x) / r.z + cx in f32, likewise y;
    ix = trunc(x), accepted iff 0 <= ix < size (so x in (-1, 0) is column 0); per pixel the lowest depth wins, among equal
    depths the lowest point index: a lexsort on (pixel, depth bits, index) that keeps the first of each pixel.  Points with a
    non-finite coordinate land nowhere.
  * pass 1 (interior pixels): a pixel with a depth keeps depth and colour; a hole with m valid neighbours (row-major order)
    gets depth inf (m <= 1), the smaller (m == 2) or the median of the first 3 / 5 / 7 (m in 3-4 / 5-6 / 7-8), and, if
    m > 0, per channel uint8(sum / (1.f * m) + 0.5f) over all m; m == 0 raises the face's flag.  Border pixels: depth inf,
    colour black.
  * dilation, only if the flag was raised: validity = filled-in depth finite; each sweep gives every invalid pixel with a
    valid pixel in its (clamped) 3 x 3 window their mean colour and makes it valid; repeated until a sweep validates nothing.
    The sweep count is the number of sweeps that validated at least one pixel.
"""
import numpy as np

F = np.float32
FACES = ("front", "left", "back", "right", "down", "up")
NEIGHBOURS = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0)]


def face_coords(face, xyz):
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    return [(x, y, z), (z, y, -x), (-x, y, -z), (-z, y, x), (x, -z, y), (x, z, -y)][face]


def intrinsics_text(size):
    h = size // 2
    return ("# Cube map face image intrinsics in the format: width height fx fy cx cy\n"
            "# For the principal point the convention having pixel coordinates (0, 0) at the top left corner of the image "
            "(instead of the center of the top left pixel) is used.\n"
            "%d %d %d %d %d %d" % (size, size, h, h, h, h))


def point_pass(xyz, rgb, size):
    xyz = np.ascontiguousarray(xyz, F).reshape(-1, 3)
    rgb = np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3)
    depth = np.full((6, size, size), np.inf, F)
    color = np.zeros((6, size, size, 3), np.uint8)
    finite = np.isfinite(xyz).all(1)
    half = F(size // 2)
    for face in range(6):
        rx, ry, rz = face_coords(face, xyz)
        idx = np.nonzero(finite & (rz > 0))[0]
        with np.errstate(all="ignore"):
            px = (half * rx[idx]) / rz[idx] + half
            py = (half * ry[idx]) / rz[idx] + half
        assert px.dtype == F and py.dtype == F
        tx, ty = np.trunc(px), np.trunc(py)                      # inf stays inf and fails the range test
        acc = (tx >= 0) & (tx < size) & (ty >= 0) & (ty < size)
        idx = idx[acc]
        pix = ty[acc].astype(np.int64) * size + tx[acc].astype(np.int64)
        bits = np.ascontiguousarray(rz[idx], F).view(np.uint32)
        order = np.lexsort((idx, bits, pix))                     # the last key is the primary one
        ps = pix[order]
        first = np.ones(len(ps), bool)
        first[1:] = ps[1:] != ps[:-1]
        w = order[first]
        depth[face].reshape(-1)[pix[w]] = rz[idx[w]]
        color[face].reshape(-1, 3)[pix[w]] = rgb[idx[w]]
    return color, depth


def _mean_color(sums, m):
    """sums (k, 3) integer, m (k,) > 0 -> uint8 (k, 3): (uint8)(sum / (1.f * m) + 0.5f)"""
    fm = F(1) * m.astype(F)
    return (sums.astype(F) / fm[:, None] + F(0.5)).astype(np.uint8)


def fill_pass1(color, depth):
    """one face -> (filled colour, filled depth, flag)"""
    S = depth.shape[0]
    fdepth = np.full((S, S), np.inf, F)
    fcolor = np.zeros((S, S, 3), np.uint8)
    fdepth[1:-1, 1:-1] = depth[1:-1, 1:-1]
    fcolor[1:-1, 1:-1] = color[1:-1, 1:-1]
    hole = np.zeros((S, S), bool)
    hole[1:-1, 1:-1] = np.isinf(depth[1:-1, 1:-1])
    ys, xs = np.nonzero(hole)
    if len(ys) == 0:
        return fcolor, fdepth, False
    nd = np.stack([depth[ys + dy, xs + dx] for dy, dx in NEIGHBOURS])             # (8, h)
    nc = np.stack([color[ys + dy, xs + dx] for dy, dx in NEIGHBOURS]).astype(np.int64)   # (8, h, 3)
    nv = ~np.isinf(nd)
    m = nv.sum(0)
    # the valid values first, in row-major order
    order = np.argsort(~nv, axis=0, kind="stable")
    vals = np.take_along_axis(nd, order, 0)[:7].copy()
    used = np.where(m == 2, 2, np.where(m <= 4, 3, np.where(m <= 6, 5, 7)))
    vals[np.arange(7)[:, None] >= used[None, :]] = np.inf
    vals.sort(axis=0)
    pick = np.where(m == 2, 0, used // 2)
    d = vals[pick, np.arange(len(ys))]
    d[m <= 1] = np.inf
    fdepth[ys, xs] = d
    has = m > 0
    sums = (nc * nv[:, :, None]).sum(0)
    fcolor[ys[has], xs[has]] = _mean_color(sums[has], m[has])
    return fcolor, fdepth, bool((m == 0).any())


def dilate(fcolor, valid):
    """Jacobi sweeps on one face, restricted to the bounding box of the pixels that are still invalid -> sweep count"""
    S = valid.shape[0]
    valid = valid.copy()
    sweeps = 0
    while True:
        inv_rows = np.nonzero(~valid.all(1))[0]
        if len(inv_rows) == 0:
            break
        inv_cols = np.nonzero(~valid.all(0))[0]
        y0, y1, x0, x1 = inv_rows[0], inv_rows[-1] + 1, inv_cols[0], inv_cols[-1] + 1
        # window with a one-pixel rim; pixels outside the image do not exist (zero weight)
        H, W = y1 - y0, x1 - x0
        v = np.zeros((H + 2, W + 2), np.int64)
        c = np.zeros((H + 2, W + 2, 3), np.int64)
        sy0, sy1, sx0, sx1 = max(y0 - 1, 0), min(y1 + 1, S), max(x0 - 1, 0), min(x1 + 1, S)
        v[sy0 - (y0 - 1):sy1 - (y0 - 1), sx0 - (x0 - 1):sx1 - (x0 - 1)] = valid[sy0:sy1, sx0:sx1]
        c[sy0 - (y0 - 1):sy1 - (y0 - 1), sx0 - (x0 - 1):sx1 - (x0 - 1)] = fcolor[sy0:sy1, sx0:sx1]
        c *= v[:, :, None]
        cnt = np.zeros((H, W), np.int64)
        sums = np.zeros((H, W, 3), np.int64)
        for dy, dx in NEIGHBOURS:
            cnt += v[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
            sums += c[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
        new = (~valid[y0:y1, x0:x1]) & (cnt > 0)
        if not new.any():
            break                                       # nothing valid anywhere (the reference would not terminate)
        ny, nx = np.nonzero(new)
        fcolor[y0 + ny, x0 + nx] = _mean_color(sums[ny, nx], cnt[ny, nx])
        valid[y0 + ny, x0 + nx] = True
        sweeps += 1
    return sweeps


def render(xyz, rgb, size, fill=True):
    """-> colour (6, S, S, 3) uint8 R, G, B; depth (6, S, S) f32; sweeps (6,) int32"""
    color, depth = point_pass(xyz, rgb, size)
    sweeps = np.zeros(6, np.int32)
    if not fill:
        return color, depth, sweeps
    out_c = np.zeros_like(color)
    out_d = np.zeros_like(depth)
    for face in range(6):
        fc, fd, flag = fill_pass1(color[face], depth[face])
        if flag:
            sweeps[face] = dilate(fc, ~np.isinf(fd))
        out_c[face], out_d[face] = fc, fd
    return out_c, out_d, sweeps


def write_depth_files(base, depth, size):
    """<base>.intrinsics.txt and <base>.<face>.depth as the tool writes them"""
    with open(base + ".intrinsics.txt", "w") as f:
        f.write(intrinsics_text(size))
    for i, name in enumerate(FACES):
        np.ascontiguousarray(depth[i], "<f4").tofile(base + "." + name + ".depth")
