"""Numpy restatement of the ReconstructionEvaluator rules (include/e3d_hip.h, e3d_evaluate_reconstruction), written from the rules
and not from the kernels: brute-force distances in blocks, f32 steps in the stated order, voxel tables from np.unique, serial f64
sums.  It is the arbiter of tests/test_evaluate_host.py, tests/test_gpu_evaluate.py and tests/test_gpu_cli_evaluate.py.

The block arithmetic of the brute-force search can run in torch on a device (`device=`): the same separately rounded f32 steps, so
the same bits (test_gpu_evaluate.py checks that), and 10^10 pairs take a second instead of minutes."""
import numpy as np

F = np.float32
IGNORED = 255
DEFAULT_TOLERANCES = (0.01, 0.02, 0.05, 0.1, 0.2, 0.5)


def check_arguments(tolerances, voxel_size, cube_map_size, n_scans):
    t = np.asarray(tolerances, F).reshape(-1)
    if n_scans < 1:
        raise ValueError("at least one scan")
    if not 1 <= len(t) <= 8 or not np.isfinite(t).all() or not (t > 0).all() or not (np.diff(t) > 0).all():
        raise ValueError("tolerances")
    h = F(voxel_size)
    if not np.isfinite(h) or not h > 0:
        raise ValueError("voxel size")
    if cube_map_size < 2 or cube_map_size > 8192 or cube_map_size % 2:
        raise ValueError("cube map size")
    return t, h


def finite_rows(p):
    return np.isfinite(p).all(axis=1)


def thresholds(t):
    return (t.astype(np.float64) * t.astype(np.float64)).astype(F)


def min_d2(a, b, device=None, pairs_per_block=1 << 24):
    """min over b of d2(a, b) = ((dx dx) + dy dy) + dz dz, dx = a.x - b.x, every step rounded to f32; +inf for an empty b."""
    out = np.full(len(a), np.inf, F)
    if len(a) == 0 or len(b) == 0:
        return out
    if device is not None:
        import torch
        A = torch.from_numpy(np.ascontiguousarray(a)).to(device); B = torch.from_numpy(np.ascontiguousarray(b)).to(device)
        pairs_per_block = 1 << 26
    else:
        A, B = a, b
    step = max(1, pairs_per_block // len(b))
    for s in range(0, len(a), step):
        blk = A[s:s + step]
        dx = blk[:, None, 0] - B[None, :, 0]
        dy = blk[:, None, 1] - B[None, :, 1]
        dz = blk[:, None, 2] - B[None, :, 2]
        acc = dx * dx
        acc = acc + dy * dy
        acc = acc + dz * dz
        m = acc.min(1) if device is None else acc.min(1).values.cpu().numpy()
        assert m.dtype == F
        out[s:s + step] = m
    return out


def near_classes(a, b, t, device=None):
    """near(a | b) per row of a (rule 2); 255 for an ignored row."""
    fa, fb = finite_rows(a), finite_rows(b)
    cls = np.full(len(a), IGNORED, np.uint8)
    d = min_d2(a[fa], b[fb], device)
    thr = thresholds(t)
    c = np.full(len(d), len(t), np.uint8)
    for i in range(len(t) - 1, -1, -1):
        c[d <= thr[i]] = i
    cls[fa] = c
    return cls


def pixels(p, o, N):
    """Rule 3 for the rows of p seen from o: (has a pixel, pixel index (face N + row) N + col, range)."""
    p = np.asarray(p, F); o = np.asarray(o, F)
    with np.errstate(all="ignore"):
        d = p - o[None, :]
        ad = np.abs(d)
        m = ad.max(axis=1) if len(p) else np.zeros(0, F)
        ok = np.isfinite(d).all(axis=1) & (m != 0)
        axis = np.where(ad[:, 0] == m, 0, np.where(ad[:, 1] == m, 1, 2))
        rows = np.arange(len(p))
        da = d[rows, axis]
        a = d[rows, (axis + 1) % 3]
        b = d[rows, (axis + 2) % 3]
        face = 2 * axis + (da < 0)
        half = F(N // 2)
        col = np.minimum(N - 1, np.floor((a / m + F(1.0)) * half).astype(np.int64, copy=False))
        row = np.minimum(N - 1, np.floor((b / m + F(1.0)) * half).astype(np.int64, copy=False))
        acc = d[:, 0] * d[:, 0]
        acc = acc + d[:, 1] * d[:, 1]
        acc = acc + d[:, 2] * d[:, 2]
        rng = np.sqrt(acc)
    assert rng.dtype == F and m.dtype == F
    pix = (face * N + row) * N + col
    pix[~ok] = 0
    return ok, pix, rng


def range_image(q, o, N):
    """The non-empty pixels of scan q seen from o, ascending, and their rmin (rule 3)."""
    ok, pix, rng = pixels(q[finite_rows(q)], o, N)
    order = np.argsort(pix[ok], kind="stable")
    pk, rk = pix[ok][order], rng[ok][order]
    if len(pk) == 0:
        return np.zeros(0, np.int64), np.zeros(0, F)
    first = np.flatnonzero(np.r_[True, pk[1:] != pk[:-1]])
    return pk[first], np.minimum.reduceat(rk, first)


def seen_ranges(rec, q, o, N):
    """Per row of rec: (its pixel of scan q is not empty, range(r), that pixel's rmin)."""
    upix, umin = range_image(q, o, N)
    okr, pixr, rngr = pixels(rec, o, N)
    if len(upix) == 0:
        return np.zeros(len(rec), bool), rngr, np.zeros(len(rec), F)
    at = np.searchsorted(upix, pixr)
    at[at >= len(upix)] = 0
    return okr & finite_rows(rec) & (upix[at] == pixr), rngr, umin[at]


def free_classes(rec, scans, origins, t, N):
    """Rule 4: free[r] = max over the scans of the number of tolerances with range(r) + t_i < rmin of r's pixel; 255 if r is ignored."""
    free = np.zeros(len(rec), np.uint8)
    for q, o in zip(scans, origins):
        seen, rngr, rmin = seen_ranges(rec, q, o, N)
        count = np.zeros(len(rec), np.uint8)
        with np.errstate(all="ignore"):
            for ti in t:
                count += (seen & ((rngr + F(ti)) < rmin)).astype(np.uint8)
        free = np.maximum(free, count)
    free[~finite_rows(rec)] = IGNORED
    return free


def voxel_table(p, h):
    """Rule 6 for the non-ignored rows of p: (ijk[v, 3] int32 in ascending (k, j, i), voxel index per kept row, kept mask).
    ValueError for a point with |c| / h >= 2^20."""
    keep = finite_rows(p)
    q = p[keep] / F(h)
    assert q.dtype == F
    if (np.abs(q) >= F(2 ** 20)).any():
        raise ValueError("a point at |coordinate| / voxel size >= 2^20")
    v = np.floor(q).astype(np.int64)
    key = ((v[:, 2] + 2 ** 20) << 42) | ((v[:, 1] + 2 ** 20) << 21) | (v[:, 0] + 2 ** 20)
    ukey, inverse = np.unique(key, return_inverse=True)
    ijk = np.stack([(ukey & 0x1FFFFF), (ukey >> 21) & 0x1FFFFF, (ukey >> 42) & 0x1FFFFF], 1) - 2 ** 20
    return ijk.astype(np.int32), inverse.reshape(-1), keep


def serial_sum(x):
    return float(np.cumsum(np.asarray(x, np.float64))[-1]) if len(x) else 0.0


def evaluate(rec, scans, origins, tolerances=DEFAULT_TOLERANCES, voxel_size=0.01, cube_map_size=2048, device=None):
    """Everything e3d.evaluate_reconstruction(..., return_classes=True, return_voxels=True) returns, under the same keys."""
    t, h = check_arguments(tolerances, voxel_size, cube_map_size, len(scans))
    T = len(t)
    rec = np.asarray(rec, F).reshape(-1, 3)
    scans = [np.asarray(s, F).reshape(-1, 3) for s in scans]
    origins = np.asarray(origins, F).reshape(-1, 3)
    assert len(origins) == len(scans)
    scan_all = np.concatenate(scans) if scans else np.zeros((0, 3), F)
    # the refusals come before any class
    sv_ijk, sv_of, s_keep = voxel_table(scan_all, h)
    rv_ijk, rv_of, r_keep = voxel_table(rec, h)
    near_rec = near_classes(rec, scan_all, t, device)
    near_scan = near_classes(scan_all, rec, t, device)
    free = free_classes(rec, scans, origins, t, cube_map_size)
    levels = np.arange(T)[None, :]
    # rule 5
    complete = near_scan[s_keep][:, None] <= levels
    accurate = near_rec[r_keep][:, None] <= levels
    inaccurate = ~accurate & (levels < free[r_keep][:, None])
    sv = {"ijk": sv_ijk, "n_points": np.bincount(sv_of, minlength=len(sv_ijk)).astype(np.int32), "count_a": np.zeros((len(sv_ijk), T), np.int32),
          "count_b": np.zeros((len(sv_ijk), T), np.int32)}
    rv = {"ijk": rv_ijk, "n_points": np.bincount(rv_of, minlength=len(rv_ijk)).astype(np.int32), "count_a": np.zeros((len(rv_ijk), T), np.int32),
          "count_b": np.zeros((len(rv_ijk), T), np.int32)}
    for i in range(T):
        sv["count_a"][:, i] = np.bincount(sv_of, weights=complete[:, i], minlength=len(sv_ijk))
        rv["count_a"][:, i] = np.bincount(rv_of, weights=accurate[:, i], minlength=len(rv_ijk))
        rv["count_b"][:, i] = np.bincount(rv_of, weights=inaccurate[:, i], minlength=len(rv_ijk))
    # rule 7
    completeness = np.zeros(T); accuracy = np.zeros(T); f1 = np.zeros(T)
    evaluated = np.zeros(T, np.int64)
    for i in range(T):
        if len(sv_ijk):
            completeness[i] = serial_sum(sv["count_a"][:, i].astype(np.float64) / sv["n_points"].astype(np.float64)) / float(len(sv_ijk))
        den = rv["count_a"][:, i].astype(np.int64) + rv["count_b"][:, i]
        use = den > 0
        evaluated[i] = int(use.sum())
        if evaluated[i]:
            accuracy[i] = serial_sum(rv["count_a"][use, i].astype(np.float64) / den[use].astype(np.float64)) / float(evaluated[i])
        a, c = accuracy[i], completeness[i]
        f1[i] = ((2.0 * a) * c) / (a + c) if a + c > 0 else 0.0
    return {"tolerances": t, "completeness": completeness, "accuracy": accuracy, "f1": f1, "n_scan_voxels": len(sv_ijk), "n_rec_voxels": len(rv_ijk),
            "evaluated_voxels": evaluated, "near_rec": near_rec, "free": free, "near_scan": near_scan, "scan_voxels": sv, "rec_voxels": rv}


# ---- the tool's coloured clouds -----------------------------------------------------------------------------------------------------
def colours(near, free, level):
    """(kept mask, rgb[kept, 3]) at tolerance index `level`: accurate / complete green, inaccurate / incomplete red, unobserved blue;
    free=None for the scan points, which are never unobserved."""
    keep = near != IGNORED
    good = near[keep] <= level
    bad = ~good if free is None else (~good & (level < free[keep]))
    rgb = np.zeros((int(keep.sum()), 3), np.uint8)
    rgb[good, 1] = 255
    rgb[bad, 0] = 255
    rgb[~good & ~bad, 2] = 255
    return keep, rgb


def pcl_ply_bytes(xyz, rgb):
    """The binary PLY of a pcl::PointXYZRGB cloud as the tools write it (x y z f32, red green blue u8, PCL's camera element)."""
    n = len(xyz)
    header = ("ply\nformat binary_little_endian 1.0\ncomment PCL generated\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\nelement camera 1\nproperty float view_px\nproperty float view_py\n"
              "property float view_pz\nproperty float x_axisx\nproperty float x_axisy\nproperty float x_axisz\nproperty float y_axisx\n"
              "property float y_axisy\nproperty float y_axisz\nproperty float z_axisx\nproperty float z_axisy\nproperty float z_axisz\n"
              "property float focal\nproperty float scalex\nproperty float scaley\nproperty float centerx\nproperty float centery\n"
              "property int viewportx\nproperty int viewporty\nproperty float k1\nproperty float k2\nend_header\n" % n)
    rec = np.zeros(n, dtype=[("p", "<f4", 3), ("c", "u1", 3)])
    rec["p"] = xyz; rec["c"] = rgb
    camera = np.array([0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0], "<f4").tobytes() + np.array([n, 1], "<i4").tobytes() + np.zeros(2, "<f4").tobytes()
    return header.encode() + rec.tobytes() + camera
