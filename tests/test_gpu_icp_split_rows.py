"""Resident correspondence rows that hold the TARGET half only (R0 = {tp.xy}, R1 = {tp.z, tn.xyz}) while the source half of every
row comes from one view per source cloud (V0 = {sp.xyz, sn.x}, V1 = {sn.yz}), e3d_icp.hip / e3d_icp_rows.hip (written) / e3d_icp_lm.hip (read).

A query without a partner is a row with a NaN in tp.x, which the LM passes read as twelve zeros.  What can go wrong: a row that keeps
a stale target half or a stale mark when its query changes partners, a view written for another frame, pose or sorted order, a slice
that reads the view from row 0, a legitimate all-zero target half taken for "no partner".  The LM costs notice every one of them.

The yardstick of tests 1 - 3 is a FRESH handle started at the poses the handle under test had before the outer iteration: its
rows have never been written, so the update rewrites every one of them from the match list.  Same poses in, same matches, the same
twelve floats per row in the same places: poses, counts and costs have to be the same bits.

"In the same places" is a condition on the yardstick, not on the rows: a handle sorts a cloud by the cells of a grid whose cell size
carries a rounding slack computed from the pose the grid was built at (build_grid: ~1e-5 of the radius, varying in its second
digit with the pose), so a fresh handle at a later pose can put a point next to a cell boundary into the neighbouring cell, the
rows of that cloud's pairs then lie in another order and an f64 cost differs in its last bit -- with the rows' layout untouched
(measured on the three-plane rows before the split, scene 25 013 points, room_scale 0.5, d = 0.08, iteration 1: initial_cost
1.9151286150642708 against 1.9151286150642706 with every count equal).  The number of such points is about
3 n (extent / cell) (d cell / cell) with d cell / cell ~ 1e-6: the scenes below (but for the partial-overlap room, which exists at
full size only) keep the room small against the radius, at most ~20 cells per axis, so that it stays below one; the tolerance
stays zero.
"""
import threading

import numpy as np
import pytest

from conftest import pose_error
from test_gpu_distributed import _ThreadAllReduce
from test_gpu_icp import ROT_TOL, TRANS_TOL

pytestmark = pytest.mark.gpu

THR = 1e-9


@pytest.fixture
def nn_mode(e3d):
    def set_mode(m):
        assert e3d.lib().e3d_set_nn_mode(m) == 0
    yield set_mode
    e3d.lib().e3d_set_nn_mode(0)


def _scene(synth, n_scans, n, seed, **kw):
    """[(xyz, normals)], [T_init]: the first n points of each scan of a scene with a few more"""
    scans = synth.make_scene(n_scans, n + 8, seed=seed, **kw)
    data = [(np.ascontiguousarray(s["xyz"].numpy()[:n]), np.ascontiguousarray(s["normals"].numpy()[:n])) for s in scans]
    return data, [s["T_init"] for s in scans]


def _handle(e3d, data, poses, fixed, resident=True):
    g = e3d.PointToPlaneICP()
    g.set_resident_rows(resident)
    ids = [g.add_point_cloud(xyz, nrm, T, f) for (xyz, nrm), T, f in zip(data, poses, fixed)]
    return g, ids


def _poses(g, ids, poses):
    return [g.get_result_global_T_cloud(i) if i >= 0 else T for i, T in zip(ids, poses)]


def _one(g, d, it):
    """one outer iteration: (converged, [(src, tgt, count)], iteration record)"""
    g.clear_records()
    ret = g.run(d, it, 1, THR, False)
    (rec,) = g.iter_records()
    return ret, [(r[1], r[2], r[3]) for r in g.pair_records()], rec


def _resident(rec):
    """the LM passes of this iteration walked resident rows (whole 64-row groups), not rows compacted for it (one per correspondence)"""
    return rec["corr_rows_walked"] % 64 == 0 and rec["corr_rows_walked"] > rec["correspondences"] > 0


def _compacted(rec):
    return rec["corr_rows_walked"] == rec["correspondences"] > 0


def _same_bits(a, ga, ia, b, gb, ib, what):
    (ra, pa, ca), (rb, pb, cb) = a, b
    assert ra == rb and pa == pb, (what, pa, pb)
    assert ca["correspondences"] == cb["correspondences"], what
    assert ca["initial_cost"] == cb["initial_cost"] and ca["final_cost"] == cb["final_cost"], (what, ca["initial_cost"], cb["initial_cost"], ca["final_cost"], cb["final_cost"])
    assert np.isfinite(ca["initial_cost"]) and np.isfinite(ca["final_cost"]), what
    for i, k in zip(ia, ib):
        if i >= 0:
            assert np.array_equal(ga.get_result_global_T_cloud(i), gb.get_result_global_T_cloud(k)), (what, i)


def _iterations_equal_fresh(e3d, g, ids, data, poses, fixed, d, its):
    """Runs the outer iterations `its` on g one by one, each against a fresh handle at the same poses; returns g's results."""
    out = []
    for it in its:
        before = _poses(g, ids, poses)
        f, fids = _handle(e3d, data, before, fixed)
        a = _one(g, d, it)
        b = _one(f, d, it)
        assert b[2]["corr_rows_rewritten"] >= b[2]["correspondences"]            # the fresh handle wrote every row
        _same_bits(a, g, ids, b, f, fids, "iteration %d" % it)
        out.append(a)
    return out


# ---- 1: flips ---------------------------------------------------------------------------------------------------------------------
# (n, scene, d, nn mode, batches): the partial-overlap room at the forced certificate search (pair by pair kernels), and a room small
# enough to be dense at 20 000 points, where the default mode takes the one-launch batch kernels (k_corr_update_multi); n < 64: one
# group with a tail; n = 64 k + 1: a last group of one row
FLIPS = [(19997, dict(partial=True), 0.06, 5, False), (19997, dict(room_scale=0.25), 0.15, 0, True),
         (50, dict(room_scale=0.25), 0.5, 5, False), (64 * 37 + 1, dict(room_scale=0.25), 0.12, 5, False)]


@pytest.mark.parametrize("n,kw,d,mode,batches", FLIPS, ids=["partial-19997", "dense-19997-batch", "n50", "n64k+1"])
def test_rows_follow_partner_changes(e3d, synth, nn_mode, n, kw, d, mode, batches):
    """Eight outer iterations while two scans meet: queries gain, lose and change partners, so target halves and marks are rewritten
    next to rows that stay.  After every iteration: the same bits as a handle whose rows were all written in that iteration."""
    assert n % 16 != 0 and n % 64 != 0
    nn_mode(mode)
    data, poses = _scene(synth, 2, n, 78, **kw)
    fixed = [False, False]
    g, ids = _handle(e3d, data, poses, fixed)
    res = _iterations_equal_fresh(e3d, g, ids, data, poses, fixed, d, range(8))
    recs = [r[2] for r in res]
    assert all(_resident(r) for r in recs)
    assert (sum(r["nn_batches"] for r in recs) > 0) == batches
    if n > 1000:
        # partners changed after the first iteration, and some rows stayed as they were
        assert any(0 < r["corr_rows_rewritten"] < r["queries"] for r in recs[1:]), [(r["corr_rows_rewritten"], r["queries"]) for r in recs]
        assert len({r["correspondences"] for r in recs}) > 1


# ---- 2: one view, two pairs -------------------------------------------------------------------------------------------------------
def test_one_source_view_feeds_two_pairs(e3d, synth, nn_mode):
    """Three movable clouds, all six directed pairs: cloud 1 is the source of 1 -> 0 (one-sided) and 1 -> 2 (kModeTwoCross), cloud 2
    of 2 -> 0 and 2 -> 1 (kModeTwo), each from ONE view.  Bit for bit a fresh handle's results; and those of rows compacted afresh
    every iteration within the tolerances of test_resident_rows_equal_compacted_rows."""
    nn_mode(0)
    data, poses = _scene(synth, 3, 30011, 21, room_scale=0.25)
    fixed = [False] * 3
    d, iters = 0.15, 4
    g, ids = _handle(e3d, data, poses, fixed)
    res = _iterations_equal_fresh(e3d, g, ids, data, poses, fixed, d, range(iters))
    assert all(len(r[1]) == 6 for r in res), res[0][1]
    assert sum(r[2]["nn_batches"] for r in res) > 0
    c, cids = _handle(e3d, data, poses, fixed, resident=False)
    for it in range(iters):
        rc, pc, b = _one(c, d, it)
        ra, pa, a = res[it]
        assert ra == rc and pa == pc
        assert _resident(a) and _compacted(b)
        assert abs(a["initial_cost"] - b["initial_cost"]) <= 1e-11 * max(abs(b["initial_cost"]), 1e-300), (a, b)
        assert abs(a["final_cost"] - b["final_cost"]) <= 1e-9 * max(abs(b["final_cost"]), 1e-300), (a, b)
    for i, k in zip(ids, cids):
        ang, tr = pose_error(g.get_result_global_T_cloud(i), c.get_result_global_T_cloud(k))
        assert ang <= 2e-7 and tr <= 2e-6, (i, ang, tr)


# ---- 3: sources kept in the global frame ------------------------------------------------------------------------------------------
def test_global_frame_views_are_rebuilt(e3d, synth, nn_mode):
    """The gauge cloud (impl cloud 0) and the fixed cloud are sources whose view is held in the global frame.  The handle is run once
    per outer iteration (rows and views outlive Run); after two iterations a fixed cloud joins: it becomes impl cloud 0, and the
    former gauge cloud can move from then on -- its view changes frames and is written again, as are the rows of its pairs."""
    nn_mode(5)
    data, poses = _scene(synth, 3, 6011, 9, room_scale=0.25)
    d = 0.2
    g, ids = _handle(e3d, data[:2], poses[:2], [False, False])
    _iterations_equal_fresh(e3d, g, ids, data[:2], poses[:2], [False, False], d, range(2))
    T0 = g.get_result_global_T_cloud(ids[0])
    assert np.array_equal(T0, np.asarray(poses[0], np.float32))                   # the gauge cloud stood still
    ids.append(g.add_point_cloud(data[2][0], data[2][1], poses[2], True))
    fixed = [False, False, True]
    res = _iterations_equal_fresh(e3d, g, ids, data, poses, fixed, d, range(2, 6))
    assert all(len(r[1]) >= 4 for r in res), res[0][1]                            # the fixed cloud is source and target
    assert res[0][2]["corr_rows_rewritten"] >= res[0][2]["correspondences"]       # frames changed: every row again
    assert not np.array_equal(g.get_result_global_T_cloud(ids[0]), T0)            # the former gauge cloud moved


# ---- 4: the mark is not a value ---------------------------------------------------------------------------------------------------
def test_zero_partner_counts_and_nan_point_does_not(e3d, ob, nn_mode):
    """A partner at the origin of its cloud's frame with a zero normal is an all-zero target half and still a correspondence: its
    residual (the source normal times the offset) is in the cost.  A target point with a NaN coordinate is nobody's partner."""
    n = 8001

    def patch(seed, dz):
        r = np.random.RandomState(seed)
        xy = r.uniform(-0.5, 0.5, (n, 2))
        z = 0.05 * np.sin(4 * xy[:, 0]) * np.cos(3 * xy[:, 1]) + dz
        nrm = np.stack([-0.2 * np.cos(4 * xy[:, 0]) * np.cos(3 * xy[:, 1]), 0.15 * np.sin(4 * xy[:, 0]) * np.sin(3 * xy[:, 1]), np.ones(n)], 1)
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        return np.concatenate([xy, z[:, None]], 1).astype(np.float32), nrm.astype(np.float32)

    A, An = patch(1, 0.0)
    B, Bn = patch(2, 0.004)
    # cloud B: nothing else within 6 cm of its origin, where a point with a zero normal sits; and one point with a NaN coordinate
    keep = np.linalg.norm(B, axis=1) > 0.06
    B, Bn = B[keep], Bn[keep]
    B = np.concatenate([B, [[0, 0, 0], [np.nan, 0.1, 0.0]]]).astype(np.float32)
    Bn = np.concatenate([Bn, [[0, 0, 0], [0, 0, 1]]]).astype(np.float32)
    zero_pt = len(B) - 2
    T0 = np.eye(4, dtype=np.float32)
    T1 = np.eye(4, dtype=np.float32); T1[:3, 3] = [0.003, -0.002, 0.001]
    d = 0.03
    # the zero point is the nearest neighbour of the queries of A around it (checked on the inputs, before any library call)
    near = np.linalg.norm(A - (B[zero_pt] + T1[:3, 3]), axis=1) < 0.02
    assert near.sum() >= 3
    nn_mode(5)
    clouds = [(A, An, T0, False), (B, Bn, T1, False)]
    runs = []
    for resident in (True, False):
        g = e3d.PointToPlaneICP()
        g.set_resident_rows(resident)
        for c in clouds:
            g.add_point_cloud(*c)
        g.run(d, 0, 3, THR, False)
        runs.append(g)
    gr, gc = runs
    o = ob.OracleICP()
    for c in clouds:
        o.add_point_cloud(*c)
    o.run(d, 0, 3, THR, False)
    assert [r[:4] for r in gr.pair_records()] == [r[:4] for r in o.pair_records()]
    assert gr.pair_records() == gc.pair_records()
    assert all(_resident(r) for r in gr.iter_records()) and all(_compacted(r) for r in gc.iter_records())
    for a, b in zip(gr.iter_records(), gc.iter_records()):
        assert np.isfinite(a["initial_cost"]) and a["initial_cost"] > 0
        assert abs(a["initial_cost"] - b["initial_cost"]) <= 1e-11 * max(abs(b["initial_cost"]), 1e-300), (a, b)
        assert abs(a["final_cost"] - b["final_cost"]) <= 1e-9 * max(abs(b["final_cost"]), 1e-300), (a, b)
    # the zero-normal partner's residuals: without them the first cost is smaller by the sum over the queries matched to it of
    # (source normal . offset)^2, far above the tolerance -- estimated here from the inputs for the queries of A -> B
    q = np.nonzero(near)[0]               # (every other point of B is more than 4 cm from them)
    off = (B[zero_pt] + T1[:3, 3])[None, :].astype(np.float64) - A[q].astype(np.float64)
    part = float(np.sum(np.sum(An[q].astype(np.float64) * off, axis=1) ** 2))
    c0 = gr.iter_records()[0]["initial_cost"]
    assert part > 1e-6 * c0, (part, c0)


# ---- 5: slices --------------------------------------------------------------------------------------------------------------------
def test_two_ranks_read_their_slice_of_the_view(e3d, synth, nn_mode):
    """Two thread-sharded ranks: rank 1's rows start at j0 > 0 of the source's view.  Global counts equal the one-rank run's, poses
    equal it (different partial sums: to the tolerance of test_sharded_equals_single_rank), the ranks agree bit for bit."""
    nn_mode(0)
    data, poses = _scene(synth, 3, 20011, 11, room_scale=0.25)
    fixed = [False, False, True]
    d, iters, world = 0.15, 4, 2
    ref, ids = _handle(e3d, data, poses, fixed)
    ref.run(d, 0, iters, THR, False)
    assert all(_resident(r) for r in ref.iter_records())
    ar = _ThreadAllReduce(world)
    handles, errors = [], []
    for r in range(world):
        h, _ = _handle(e3d, data, poses, fixed)
        h.set_shard(r, world, ar.make(r))
        handles.append(h)

    def work(h):
        try:
            h.run(d, 0, iters, THR, False)
        except Exception as ex:  # noqa: BLE001
            errors.append(ex)
            ar.barrier.abort()

    th = [threading.Thread(target=work, args=(h,)) for h in handles]
    for t in th:
        t.start()
    for t in th:
        t.join(120)
    assert not errors, errors
    ref_counts = [r[:4] for r in ref.pair_records()]
    for h in handles:
        assert [r[:4] for r in h.pair_records()] == ref_counts
        assert all(_resident(r) for r in h.iter_records())
        for i in ids:
            if i >= 0:
                ang, tr = pose_error(h.get_result_global_T_cloud(i), ref.get_result_global_T_cloud(i))
                assert ang <= ROT_TOL and tr <= TRANS_TOL, (i, ang, tr)
    for i in ids:
        if i >= 0:
            assert np.array_equal(handles[0].get_result_global_T_cloud(i), handles[1].get_result_global_T_cloud(i))
