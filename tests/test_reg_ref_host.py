"""The CPU oracle of the registration passes against the float64 numpy restatement (tests/reg_ref.py) on observation lists with
partial visibility: thinned lists at every neighbour count the library accepts a range of, and short compact lists.  No GPU.

Both sides get the same intensities and Jacobian rows (the oracle's pass 1), so what is compared is everything after pass 1: which
row and which point each term reads, the flags, the residual kinds, the robust functions and the sums.  Flags and counts must be
equal.  The sums, H and b differ by the oracle's f32 rounding of residuals and products.  Measured over all the cases of this file
(scene of 3000 points, seed 7), in the normalisation of reg_ref.deviations:

    quantity   thinned lists (K = 1 .. 8, models 0 and 2, robust types 0 1 2)   compact lists (m = 2 .. 257)
    sums       5.8e-9                                                           1.2e-7  (m = 9: one residual, one f32 rounding)
    H          3.7e-8                                                           8.3e-8
    b          2.8e-7                                                           5.2e-8

The bounds (reg_lists.ORACLE_VS_REF) are 10 times the worst of each row: room for other seeds, and still far below an indexing
error, which shows at order 1.
"""
import functools

import numpy as np
import pytest

import reg_lists
import reg_ref

TOL_SUMS, TOL_H, TOL_B = reg_lists.ORACLE_VS_REF

KS = [1, 2, 3, 4, 5, 7, 8]
MODELS = [0, 2]


@functools.lru_cache(maxsize=None)
def _scene(K, model):
    from oracle import reg_binding as rb
    S = reg_lists.scene(K, model)
    levels, o = reg_lists.full_list(rb, S)
    I, JI, JP = rb.pass1(S["pts"], S["point_radius"], levels[0], 0, S["pyr"], S["R"], S["t"], o)
    return S, levels, o, I, np.concatenate([JI, JP], axis=1)


def _sub(full, part, *arrays):
    """Rows of per-observation arrays of the full list that belong to the sub-list `part` (both in point order)."""
    sel = np.searchsorted(full[0], part[0])
    assert np.array_equal(full[0][sel], part[0])
    return [a[sel] for a in arrays]


def _both(rb, K, model, o, rtype, w_fixed=1.0, w_var=1.0):
    S, levels, full, I, J = _scene(K, model)
    n = len(S["pts"])
    of = rb.neighbors_observed(n, o[0], S["nbr"], K)
    rparam = reg_lists.ROBUST[rtype]
    orc = rb.accumulate(S["pts"], S["point_radius"], S["nbr"], K, S["fixed_desc"], S["var_desc"], S["obs_counts"], levels[0], 0, S["pyr"],
                        S["R"], S["t"], o, of, rtype, rparam, w_fixed, w_var)
    orc_cost = rb.cost(n, S["nbr"], K, S["fixed_desc"], S["var_desc"], S["obs_counts"], 0, S["pyr"], o, of, rtype, rparam, w_fixed, w_var)
    Is, Js = _sub(full, o, I, J)
    fr = reg_ref.flags(n, o[0], S["nbr"])
    rparam32 = float(np.float32(rparam))
    ref = reg_ref.accumulate(Is, Js, o[0], fr, S["nbr"], S["fixed_desc"], S["var_desc"], S["obs_counts"], rtype, rparam32, w_fixed, w_var)
    ref_cost = reg_ref.cost(Is, o[0], fr, S["nbr"], S["fixed_desc"], S["var_desc"], S["obs_counts"], rtype, rparam32, w_fixed, w_var)
    return S, of, fr, orc, orc_cost, ref, ref_cost


def _check(orc, orc_cost, ref, ref_cost, what):
    Ho, bo, so, co = orc
    Hr, br, sr, cr = ref
    assert np.array_equal(co, cr) and np.array_equal(orc_cost[1], ref_cost[1]) and np.array_equal(co, orc_cost[1])
    assert np.array_equal(np.tril(Hr, -1), np.zeros_like(Hr)) and np.array_equal(np.tril(Ho, -1), np.zeros_like(Ho))
    if co.sum() == 0:
        assert not Ho.any() and not bo.any() and not so.any() and not Hr.any() and not br.any() and not sr.any()
        return
    e_s, e_h, e_b = reg_ref.deviations(Ho, bo, so, Hr, br, sr)
    e_c = np.abs(orc_cost[0] - ref_cost[0]).max() / np.abs(ref_cost[0]).max()
    print("oracle vs numpy %s: sums %.2e cost %.2e H %.2e b %.2e" % (what, e_s, e_c, e_h, e_b))
    assert e_s <= TOL_SUMS and e_c <= TOL_SUMS and e_h <= TOL_H and e_b <= TOL_B, (what, e_s, e_c, e_h, e_b)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("K", KS)
def test_flags_and_shares_of_thinned_lists(rb, K, model):
    S, levels, full, I, J = _scene(K, model)
    o = reg_lists.drop(full, 100 + K)
    of = rb.neighbors_observed(len(S["pts"]), o[0], S["nbr"], K)
    assert np.array_equal(of, reg_ref.flags(len(S["pts"]), o[0], S["nbr"]))
    print("K %d model %d: %d of %d observations kept, flag share %.3f" % (K, model, len(o[0]), len(full[0]), of.mean()))
    reg_lists.assert_partial(S, o, of)
    assert 2400 < len(o[0]) < len(full[0])
    # the full list of these scenes is the trivial case the partial lists are there to leave
    assert np.array_equal(full[0], np.arange(len(S["pts"])))


@pytest.mark.parametrize("rtype", [0, 1, 2])
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("K", KS)
def test_thinned_lists(rb, K, model, rtype):
    S, levels, full, I, J = _scene(K, model)
    o = reg_lists.drop(full, 100 + K)
    S, of, fr, orc, orc_cost, ref, ref_cost = _both(rb, K, model, o, rtype)
    assert np.array_equal(of, fr)
    reg_lists.assert_partial(S, o, of, orc[3])
    _check(orc, orc_cost, ref, ref_cost, "K %d model %d robust %d" % (K, model, rtype))


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("K,m", [(5, m) for m in (1, 2, 9, 63, 64, 65, 255, 256, 257)] + [(K, m) for K in (3, 8) for m in (1, 64, 65)])
def test_compact_lists(rb, K, m, model):
    S, levels, full, I, J = _scene(K, model)
    o = reg_lists.compact(S["pts"], full, m)
    assert len(o[0]) == m
    S, of, fr, orc, orc_cost, ref, ref_cost = _both(rb, K, model, o, 1)
    assert np.array_equal(of, fr)
    print("K %d model %d m %d: %d flags set" % (K, model, m, int(of.sum())))
    if m == 1:
        assert not of.any() and not orc[3].any()
    elif m >= 63:
        assert 0 < of.sum() < m
    _check(orc, orc_cost, ref, ref_cost, "K %d model %d m %d" % (K, model, m))


@pytest.mark.parametrize("K", [3, 5])
@pytest.mark.parametrize("off", ["fixed", "variable"])
def test_a_weight_of_zero_skips_its_kind(rb, K, off):
    S, levels, full, I, J = _scene(K, 0)
    o = reg_lists.drop(full, 100 + K)
    wf, wv = (0.0, 1.0) if off == "fixed" else (1.0, 0.0)
    kind = 0 if off == "fixed" else 1
    S, of, fr, orc, orc_cost, ref, ref_cost = _both(rb, K, 0, o, 1, wf, wv)
    _, _, _, both, both_cost, _, _ = _both(rb, K, 0, o, 1)
    for sums, counts in (orc[2:], orc_cost, ref[2:], ref_cost):
        assert sums[kind] == 0 and counts[kind] == 0 and counts[1 - kind] > 100
    assert orc[2][1 - kind] == both[2][1 - kind] and orc[3][1 - kind] == both[3][1 - kind]
    assert not np.array_equal(orc[0], both[0])
    _check(orc, orc_cost, ref, ref_cost, "K %d without the %s kind" % (K, off))


@pytest.mark.parametrize("K", [1, 3, 5, 8])
def test_color_update_on_two_thinned_lists(rb, K):
    """Two images' worth of observations (two thinnings of one list): counts 0, 1 and 2 all occur, and only 2 divides.  The oracle
    works in f32: every difference, the sum of two and the division round once each, so a descriptor is within 2^-23 of the largest
    single intensity difference of the float64 value."""
    S, levels, full, I, J = _scene(K, 0)
    n = len(S["pts"])
    do = np.zeros((n, K), np.float32); co = np.zeros(n, np.int32)
    dr = np.zeros((n, K)); cr = np.zeros(n, np.int64)
    largest = 0.0
    for seed in (100 + K, 200 + K):
        o = reg_lists.drop(full, seed)
        of = rb.neighbors_observed(n, o[0], S["nbr"], K)
        rb.color_accumulate(n, S["nbr"], K, 0, S["pyr"], o, of, do, co)
        Is, = _sub(full, o, I)
        reg_ref.color_accumulate(Is, o[0], reg_ref.flags(n, o[0], S["nbr"]), S["nbr"], dr, cr)
        one = np.zeros((n, K)); reg_ref.color_accumulate(Is, o[0], of, S["nbr"], one, np.zeros(n, np.int64))
        largest = max(largest, np.abs(one).max())
    rb.color_finish(K, do, co); reg_ref.color_finish(dr, cr)
    assert np.array_equal(co, cr)
    assert (co == 0).sum() > 50 and (co == 1).sum() > 50 and (co == 2).sum() > 50
    assert largest > 10 and np.abs(do - dr).max() <= 2.0 ** -23 * largest
