"""MergeClosePoints restated in numpy, brute force (TEST INFRASTRUCTURE ONLY), and the inputs that tests/test_multires_host.py
and tests/test_gpu_multires.py share.

merge_close_points() follows the rules the HIP kernels (csrc/e3d_multires.hip) and the CPU oracle (oracle/oracle_multires.c)
share, without a search structure: O(n^2), every centre looks at every point.
  * r2 = float32(float64(float32(dist)) ** 2)                (pcl::KdTreeFLANN::radiusSearch)
  * f32 squared distance in FLANN's order ((dx*dx) + dy*dy) + dz*dz, every operation rounded to f32, compared with a strict <
  * greedy in index order: a point nobody absorbed becomes a centre and absorbs ALL points within the radius
  * neighbours are visited in increasing index; the f32 sums start at 0 and run sequentially in that order
  * majority scan: the first scan to reach the maximal count
Besides the four outputs it returns, per centre, what a derived error bound needs (f64 means, neighbourhood sizes, magnitudes).
The keyword switches select rule VARIANTS; they exist only so that the host tests can prove that an input tells the variants apart.
"""
import functools
import math

import numpy as np

F = np.float32
U = 2.0 ** -24            # unit round-off of f32
MERGE_LIST = 40           # kMergeList of k_merge_decide: lower-index neighbours kept per thread


def gamma(m):
    """g(m) = m u / (1 - m u): an f32 sum of m terms in ANY order followed by one division is within g(m) * max|x_j| of the exact
    mean (m - 1 additions and one division, each with relative error <= u; |sum_j x_j| / m <= max|x_j|)."""
    m = np.asarray(m, np.float64)
    return m * U / (1.0 - m * U)


def radius2(dist):
    return F(np.float64(F(dist)) ** 2)


def sqdist(P, q):
    """f32 squared distances of every row of P to q, ((dx*dx) + dy*dy) + dz*dz"""
    dx = q[0] - P[:, 0]; dy = q[1] - P[:, 1]; dz = q[2] - P[:, 2]
    return (dx * dx + dy * dy) + dz * dz


def _seq_sum(x):
    """0.f + x[0] + x[1] + ... in f32, left to right; returns every partial sum"""
    return np.cumsum(np.concatenate([np.zeros(1, F), x.astype(F)]), dtype=F)[1:]


def merge_close_points(dist, num_scans, P, col, sidx, mxr, closed_radius=False, tie="first_to_max", only_unabsorbed=False):
    P = np.ascontiguousarray(P, F).reshape(-1, 3); col = np.ascontiguousarray(col, F)
    sidx = np.ascontiguousarray(sidx, np.uint8); mxr = np.ascontiguousarray(mxr, F)
    n = len(P)
    assert len(col) == len(sidx) == len(mxr) == n and 1 <= num_scans <= 16
    assert np.isfinite(P).all() and (n == 0 or int(sidx.max()) < num_scans), "undefined input"
    assert tie in ("first_to_max", "lowest_scan")
    r2 = radius2(dist)
    done = np.zeros(n, bool)
    o_xyz, o_col, o_scan, o_mxr = [], [], [], []
    centre, m_, c_, mean64, col64, amax_x, amax_c, nbrs = [], [], [], [], [], [], [], []
    for i in range(n):
        if done[i]:
            continue
        d2 = sqdist(P, P[i])
        nb = np.nonzero(d2 <= r2 if closed_radius else d2 < r2)[0]           # increasing index
        if only_unabsorbed:
            nb = nb[~done[nb]]
        done[nb] = True
        X = P[nb]
        m = len(nb)
        o_xyz.append([_seq_sum(X[:, a])[-1] / F(m) for a in range(3)])
        count = [0] * num_scans
        best, best_count = -1, 0
        for s in sidx[nb].tolist():
            count[s] += 1
            if count[s] > best_count:
                best_count, best = count[s], s
        if tie == "lowest_scan":
            best = int(np.argmax(count))
        sel = nb[sidx[nb] == best]
        c = len(sel)
        o_col.append(_seq_sum(col[sel])[-1] / F(c))
        o_scan.append(best)
        o_mxr.append(max(F(-1), mxr[nb].max()))
        centre.append(i); m_.append(m); c_.append(c); nbrs.append(nb)
        mean64.append([math.fsum(X[:, a].astype(np.float64).tolist()) / m for a in range(3)])
        col64.append(math.fsum(col[sel].astype(np.float64).tolist()) / c)
        amax_x.append(np.abs(X).max(0)); amax_c.append(np.abs(col[nb]).max())
    k = len(centre)
    return dict(xyz=np.array(o_xyz, F).reshape(k, 3), col=np.array(o_col, F), scan=np.array(o_scan, np.uint8), mxr=np.array(o_mxr, F),
                centre=np.array(centre, np.int64), m=np.array(m_, np.int64), c=np.array(c_, np.int64),
                mean64=np.array(mean64, np.float64).reshape(k, 3), col64=np.array(col64, np.float64),
                absmax_x=np.array(amax_x, np.float64).reshape(k, 3), absmax_col=np.array(amax_c, np.float64), nbrs=nbrs)


def outputs(R):
    return R["xyz"], R["col"], R["scan"], R["mxr"]


def mean_deviation_ratios(xyz, col, R):
    """(largest |position - f64 mean| / (g(m) max|x_j|), the same for the colours with g(c) max|col_j|); a zero bound (all terms 0)
    admits only a zero deviation and then counts as ratio 0."""
    def ratio(dev, bound):
        assert (dev[bound == 0] == 0).all()
        return float((dev[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    rp = ratio(np.abs(xyz.astype(np.float64) - R["mean64"]), gamma(R["m"])[:, None] * R["absmax_x"])
    rc = ratio(np.abs(col.astype(np.float64) - R["col64"]), gamma(R["c"]) * R["absmax_col"])
    return rp, rc


# ---- inputs --------------------------------------------------------------------------------------------------------------------
# every generator returns the argument tuple (dist, num_scans, P, col, sidx, mxr)
SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 1000)      # wave (64) and block (256) boundaries of the ticket and of the compaction
STEP = 1.0 / 64                                         # lattice step: every lattice coordinate is an integer number of steps
LATTICE_SHIFTS = {"lattice": (0.0, 0.0, 0.0), "lattice_m64": (-64.0,) * 3, "lattice_p4096": (4096.0,) * 3,
                  "lattice_far": (2.0 ** 17, -2.0 ** 17, 2.0 ** 17 - 3)}
CHAIN_N = 5000


def sizes_case(n):
    """n uniform points in a cube whose side makes the mean neighbourhood (the point itself included) about 4; 3 scans"""
    rng = np.random.RandomState(1000 + n)
    dist = 0.05
    side = dist * (max(n, 1) * (4.0 / 3.0) * np.pi / 4.0) ** (1.0 / 3.0)
    P = rng.uniform(0, side, (n, 3)).astype(F)
    return (dist, 3, P, rng.uniform(0, 255, n).astype(F), rng.randint(0, 3, n).astype(np.uint8), rng.uniform(0.001, 0.1, n).astype(F))


def lattice_case(shift=(0.0, 0.0, 0.0)):
    """4000 sites k / 64, k in [-40, 40]^3, drawn with repetition; merge distance 5 / 64, so that pairs with |dk|^2 == 25 sit at exactly
    the merge distance; integer colours, max_radius in eighths, 4 scans.  Every coordinate, difference, square and (short) sum is exact."""
    rng = np.random.RandomState(7)
    k = rng.randint(-40, 41, (4000, 3))
    P = (k.astype(np.float64) * STEP + np.asarray(shift, np.float64)).astype(F)
    assert np.array_equal(P.astype(np.float64), k * STEP + np.asarray(shift, np.float64)), "not representable"
    return (5.0 / 64, 4, P, rng.randint(0, 256, 4000).astype(F), rng.randint(0, 4, 4000).astype(np.uint8), (rng.randint(1, 64, 4000) / 8.0).astype(F))


def chain_positions(order):
    """position along the line of the point with index i"""
    if order == "increasing":
        return np.arange(CHAIN_N)
    if order == "decreasing":
        return np.arange(CHAIN_N)[::-1].copy()
    return np.random.RandomState(11).permutation(CHAIN_N)


def chain_case(order):
    """a line of points 3 / 64 apart, merge distance 5 / 64: every point reaches exactly its two neighbours along the line, so every
    decision hangs on the one before it.  In increasing order the centres are the even positions (0 absorbs 1, 2 absorbs 1 and 3, ...)."""
    pos = chain_positions(order)
    P = np.stack([pos * (3.0 / 64) - 100.0, np.full(CHAIN_N, 0.25), np.full(CHAIN_N, -1.5)], 1).astype(F)
    rng = np.random.RandomState(12)
    return (5.0 / 64, 2, P, rng.randint(0, 256, CHAIN_N).astype(F), rng.randint(0, 2, CHAIN_N).astype(np.uint8), (rng.randint(1, 64, CHAIN_N) / 8.0).astype(F))


def dense_case():
    """300 exact duplicates of one point (indices with i mod 10 in {0, 3, 7}) between 700 points scattered around it: point 0 is a
    centre with hundreds of neighbours, and from about index 50 on a point has more than kMergeList lower-index neighbours, so that
    k_merge_decide walks the cells again while it waits -- for a centre in its own wave (index < 64) and in other blocks."""
    rng = np.random.RandomState(5)
    dist = 0.05
    dup = np.isin(np.arange(1000) % 10, (0, 3, 7))
    P = np.empty((1000, 3))
    P[dup] = (0.3, -0.2, 1.1)
    P[~dup] = np.array((0.3, -0.2, 1.1)) + rng.normal(0, 0.45 * dist, (700, 3))
    return (dist, 3, P.astype(F), rng.uniform(0, 255, 1000).astype(F), rng.randint(0, 3, 1000).astype(np.uint8), rng.uniform(0.001, 0.1, 1000).astype(F))


def scans16_case(all_15=False):
    """3000 uniform points, mean neighbourhood about 6, sixteen scans: most centres see every scan at most once or twice, so the
    majority is decided by the tie rule"""
    rng = np.random.RandomState(16)
    dist = 0.05
    side = dist * (3000 * (4.0 / 3.0) * np.pi / 6.0) ** (1.0 / 3.0)
    P = rng.uniform(0, side, (3000, 3)).astype(F)
    sidx = rng.randint(0, 16, 3000).astype(np.uint8)
    if all_15:
        sidx[:] = 15
    return (dist, 16, P, rng.uniform(0, 255, 3000).astype(F), sidx, rng.uniform(0.001, 0.1, 3000).astype(F))


def grid_cells(dist, P):
    """The integer cell of every point of P in the hashed grid e3d_merge_close_points builds (csrc/e3d_multires.hip: cell size and
    origin in f64 from the f32 bounding box; cell_coord of csrc/e3d_kernels.hpp: floor((v - origin) * inv_cell) in f32), restated
    operation by operation."""
    P = np.ascontiguousarray(P, F).reshape(-1, 3)
    lo, hi = P.min(0).astype(np.float64), P.max(0).astype(np.float64)
    md = float(F(dist))
    cell = md * (1.0 + 1e-4) + 16.0 * 2.0 ** -23 * (max(np.abs(lo).max(), np.abs(hi).max()) + 4.0 * md)
    while (hi - lo).max() / cell > (1 << 21) - 8:
        cell *= 2.0
    origin, inv_cell = (lo - 2.0 * cell).astype(F), F(1.0 / cell)
    return np.floor((P - origin) * inv_cell).astype(np.int64)


# occupied grid cells at which twice their number meets and crosses a power of two, the 64-slot floor of the hash table included
CELL_COUNTS = (1, 32, 33, 64, 65, 1024, 1025)


def cells_case(C):
    """C pairs, each alone in a grid cell of its own: the first C sites (x fastest) of a cubic lattice of pitch 3.35 cells (about 3.35
    merge distances: no two pairs interact), and dist / 16 further along x each site's partner -- the partner of point j is point
    C + j, decided in another wave or block.  3.35: the sites of the first eleven columns lie between 0.05 and 0.8 of a cell behind
    a cell boundary, the partner 0.06 further on.  Only the first column sits ON a boundary (the grid's origin is the bounding box's
    minimum less two cells), on whichever side the rounding puts it; the cloud is moved by eighths until grid_cells puts every pair
    in one cell.  Integer colours, max_radius in eighths, 3 scans: with two points per centre every sum is the same in any order."""
    dist = 1.0 / 16
    side = 1
    while side ** 3 < C:
        side += 1
    k = np.arange(C)
    site = np.stack([k % side, (k // side) % side, k // (side * side)], 1) * (3.35 * dist * (1.0 + 1e-4))
    for eighths in range(64):
        A = (site + eighths / 8.0).astype(F)
        B = A.copy()
        B[:, 0] += F(dist / 16)
        cells = grid_cells(dist, np.concatenate([A, B]))
        if np.array_equal(cells[:C], cells[C:]) and len(np.unique(cells[:C], axis=0)) == C:
            break
    else:
        raise AssertionError("no placement with %d pairs in %d cells" % (C, C))
    rng = np.random.RandomState(100 + C)
    return (dist, 3, np.concatenate([A, B]), rng.randint(0, 256, 2 * C).astype(F), rng.randint(0, 3, 2 * C).astype(np.uint8),
            (rng.randint(1, 64, 2 * C) / 8.0).astype(F))


CASES = {"size_%d" % n: functools.partial(sizes_case, n) for n in SIZES}
CASES.update({"cells_%d" % C: functools.partial(cells_case, C) for C in CELL_COUNTS})
CASES.update({name: functools.partial(lattice_case, shift) for name, shift in LATTICE_SHIFTS.items()})
CASES.update({"chain_" + o: functools.partial(chain_case, o) for o in ("increasing", "decreasing", "shuffled")})
CASES.update({"dense": dense_case, "scans16": scans16_case, "scans16_all15": functools.partial(scans16_case, True)})
# f32 sums are exact (order cannot matter, outputs compare bit for bit): lattice coordinates of at most 2^18 steps, m <= 32
EXACT = ("lattice", "lattice_m64", "lattice_p4096", "chain_increasing", "chain_decreasing", "chain_shuffled")
DUPLICATES = ("lattice", "lattice_m64", "lattice_p4096", "lattice_far", "dense")      # inputs with coincident points


@functools.lru_cache(maxsize=None)
def case(name):
    """the (read-only) arguments of a named input"""
    args = CASES[name]()
    for a in args[2:]:
        a.setflags(write=False)
    return args


@functools.lru_cache(maxsize=None)
def reference(name):
    """the restatement's result for a named input, computed once per process"""
    return merge_close_points(*case(name))
