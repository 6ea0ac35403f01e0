"""Plain float64 numpy restatement of the per-observation arithmetic of the image-registration passes: neighbour flags, the
photometric cost, the normal equations of pass 2 and the colour (descriptor) update.  A second reference beside the CPU oracle,
written from the formulas and not from the oracle's code; everything is float64 and vectorised over the observation list.

Two index spaces meet in every formula and are kept apart by name here:
  i, row  -- position in the observation list of one image (0 .. n_obs-1); I, J and flags are indexed by it
  p       -- point index (0 .. n_pts-1); nbr, the descriptors and obs_counts are indexed by it
o_idx[i] = p maps the first to the second; row_of(p) is its inverse on the observed points and -1 elsewhere.
"""
import numpy as np


def _rows_of_points(n_pts, o_idx):
    row = np.full(n_pts, -1, np.int64)
    row[np.asarray(o_idx, np.int64)] = np.arange(len(o_idx), dtype=np.int64)
    return row


def flags(n_pts, o_idx, nbr):
    """1 where all K neighbours of the observed point are in the list themselves."""
    o_idx = np.asarray(o_idx, np.int64)
    nbr = np.asarray(nbr, np.int64)
    if len(o_idx) == 0:
        return np.zeros(0, np.uint8)
    seen = np.zeros(n_pts, bool)
    seen[o_idx] = True
    return seen[nbr[o_idx]].all(axis=1).astype(np.uint8)


def robust_residual(rtype, param, r):
    """rho(r): 0 none (r^2 / 2), 1 Huber, 2 Tukey's biweight (robust_weighting.h: CalculateRobustResidual)."""
    r = np.asarray(r, np.float64)
    a = np.abs(r)
    if rtype == 1:
        return np.where(a < param, 0.5 * r * r, param * (a - 0.5 * param))
    if rtype == 2:
        t = 1.0 - (r / param) ** 2
        return np.where(a < param, param * param / 6.0 * (1.0 - t ** 3), param * param / 6.0)
    return 0.5 * r * r


def robust_weight(rtype, param, r):
    """w(r) = rho'(r) / r (robust_weighting.h: CalculateWeight)."""
    r = np.asarray(r, np.float64)
    a = np.abs(r)
    if rtype == 1:
        return np.where(a < param, 1.0, param / np.maximum(a, 1e-300))
    if rtype == 2:
        t = 1.0 - (r / param) ** 2
        return np.where(a < param, t * t, 0.0)
    return np.ones_like(r)


def _residuals(I, o_idx, flg, nbr, fixed_desc, var_desc, obs_counts, w_fixed, w_var):
    """Per residual kind (0 fixed, 1 variable): the observation rows it applies to, their neighbours' rows [n, K] and the
    K residual components c_k = (I[row(nbr_k)] - I[i]) - desc[p, k]."""
    I = np.asarray(I, np.float64)
    o_idx = np.asarray(o_idx, np.int64)
    nbr = np.asarray(nbr, np.int64)
    row = _rows_of_points(len(nbr), o_idx)
    out = []
    for kind, (weight, desc) in enumerate(((w_fixed, fixed_desc), (w_var, var_desc))):
        use = np.asarray(flg).astype(bool).copy()
        if not weight > 0:
            use[:] = False
        if kind == 1:
            use &= np.asarray(obs_counts)[o_idx] >= 2
        rows = np.nonzero(use)[0]
        p = o_idx[rows]
        nrows = row[nbr[p]]
        assert (nrows >= 0).all()                 # a set flag means every neighbour has a row
        comp = (I[nrows] - I[rows, None]) - np.asarray(desc, np.float64)[p]
        out.append((rows, nrows, comp))
    return out


def cost(I, o_idx, flg, nbr, fixed_desc, var_desc, obs_counts, rtype, rparam, w_fixed, w_var):
    """-> (sums[2], counts[2]): sum of rho(||c||_2) and number of residuals per kind; a kind whose weight is not > 0 is skipped,
    the variable kind applies where obs_counts[p] >= 2."""
    sums = np.zeros(2)
    counts = np.zeros(2, np.int64)
    for kind, (rows, nrows, comp) in enumerate(_residuals(I, o_idx, flg, nbr, fixed_desc, var_desc, obs_counts, w_fixed, w_var)):
        pr = np.sqrt((comp * comp).sum(axis=1))
        sums[kind] = robust_residual(rtype, float(rparam), pr).sum()
        counts[kind] = len(rows)
    return sums, counts


def accumulate(I, J, o_idx, flg, nbr, fixed_desc, var_desc, obs_counts, rtype, rparam, w_fixed, w_var):
    """J = [JI | JP] per observation (pass 1).  -> (H, b, sums, counts): H = sum w (J_nbr - J_i)^T (J_nbr - J_i) with only its
    upper triangle kept, b = sum w c_k (J_nbr - J_i), over the residual kinds, their observations and the K neighbours, with
    w = kind weight * w(||c||_2)."""
    J = np.asarray(J, np.float64)
    V = J.shape[1]
    H = np.zeros((V, V))
    b = np.zeros(V)
    sums = np.zeros(2)
    counts = np.zeros(2, np.int64)
    kinds = _residuals(I, o_idx, flg, nbr, fixed_desc, var_desc, obs_counts, w_fixed, w_var)
    for kind, (rows, nrows, comp) in enumerate(kinds):
        pr = np.sqrt((comp * comp).sum(axis=1))
        sums[kind] = robust_residual(rtype, float(rparam), pr).sum()
        counts[kind] = len(rows)
        w = (w_fixed, w_var)[kind] * robust_weight(rtype, float(rparam), pr)
        for k in range(nrows.shape[1] if len(rows) else 0):
            D = J[nrows[:, k]] - J[rows]
            H += (D * w[:, None]).T @ D
            b += (D * (w * comp[:, k])[:, None]).sum(axis=0)
    return np.triu(H), b, sums, counts


def color_accumulate(I, o_idx, flg, nbr, descriptors, counts):
    """One image's share of the descriptor update, in place: descriptors[p] += I[row(nbr)] - I[i], counts[p] += 1 for every
    observation with its flag set.  descriptors is float64 [n_pts, K], counts an integer array [n_pts]."""
    I = np.asarray(I, np.float64)
    o_idx = np.asarray(o_idx, np.int64)
    nbr = np.asarray(nbr, np.int64)
    row = _rows_of_points(len(nbr), o_idx)
    rows = np.nonzero(np.asarray(flg))[0]
    p = o_idx[rows]                               # a point appears at most once in one image's list
    descriptors[p] += I[row[nbr[p]]] - I[rows, None]
    counts[p] += 1


def color_finish(descriptors, counts):
    """The mean over the images, only where a point was counted more than once (a single sample stays as it is)."""
    many = np.asarray(counts) > 1
    descriptors[many] /= np.asarray(counts, np.float64)[many, None]


def deviations(H, b, sums, Href, bref, sums_ref):
    """The three numbers the registration tests bound, in their normalisation: sums relative to the largest, H relative to
    sqrt(diag x diag), b / sqrt(diag) relative to its largest entry."""
    d = np.sqrt(np.diag(Href))
    e_s = np.abs(sums - sums_ref).max() / max(np.abs(sums_ref).max(), 1e-300)
    with np.errstate(invalid="ignore", divide="ignore"):
        e_h = np.nanmax(np.where(np.outer(d, d) > 0, np.abs(H - Href) / np.outer(d, d), 0.0))
        e_b = np.abs((b - bref) / d).max() / np.abs(bref / d).max()
    return float(e_s), float(e_h), float(e_b)
