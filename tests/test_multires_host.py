"""MergeClosePoints without a GPU: the numpy restatement (tests/multires_ref.py) against the CPU oracle on every input the GPU
tests use, its own rounding against the derived bound, and proof that these inputs tell the rule variants apart (a closed radius,
another tie rule, absorbing only fresh points) -- no wrong kernel is ever run on a GPU, a broken wait rule could hang it."""
import numpy as np
import pytest

import multires_ref as ref

ALL = sorted(ref.CASES)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


@pytest.mark.parametrize("name", ALL)
def test_restatement_matches_oracle_bit_for_bit(name):
    from oracle import multires as mr
    R = ref.reference(name)
    o = mr.merge_close_points(*ref.case(name))
    for a, b in zip(ref.outputs(R), o):
        assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b))          # both sum in index order in f32


@pytest.mark.parametrize("name", ALL)
def test_restatement_means_within_derived_bound(name):
    R = ref.reference(name)
    rp, rc = ref.mean_deviation_ratios(R["xyz"], R["col"], R)
    print("%s: %d centres, m <= %d, deviation / bound: position %.3g, colour %.3g" % (name, len(R["m"]), R["m"].max() if len(R["m"]) else 0, rp, rc))
    assert rp <= 1.0 and rc <= 1.0
    # the bookkeeping the bound rests on
    assert int(R["m"].sum()) >= len(ref.case(name)[2]) and (R["c"] >= 1).all() and (R["c"] <= R["m"]).all()
    assert np.array_equal(R["m"], [len(nb) for nb in R["nbrs"]])


def test_gamma():
    assert ref.gamma(1) == 2.0 ** -24 / (1 - 2.0 ** -24) and 31.9 * ref.U < ref.gamma(32) < 32.1 * ref.U
    assert ref.radius2(5.0 / 64) == np.float32(25.0 / 4096)


@pytest.mark.parametrize("name", sorted(ref.LATTICE_SHIFTS))
def test_lattice_has_pairs_at_exactly_the_merge_distance(name):
    dist, scans, P, col, sidx, mxr = ref.case(name)
    r2 = ref.radius2(dist)
    at = sum(int((ref.sqdist(P, P[i]) == r2).sum()) for i in range(len(P))) // 2
    print("%s: %d pairs with d2 == r2" % (name, at))
    assert at >= 100
    strict = ref.reference(name)
    closed = ref.merge_close_points(dist, scans, P, col, sidx, mxr, closed_radius=True)
    assert not np.array_equal(strict["centre"], closed["centre"])              # <= instead of < : other centres
    assert not np.array_equal(_bits(strict["mxr"]), _bits(closed["mxr"]))      # ... and visible in an output compared exactly


def test_sixteen_scans_exercise_the_tie_rule():
    args = ref.case("scans16")
    R = ref.reference("scans16")
    tied = 0
    for nb in R["nbrs"]:
        cnt = np.bincount(args[4][nb], minlength=16)
        tied += int((cnt == cnt.max()).sum() >= 2)
    low = ref.merge_close_points(*args, tie="lowest_scan")
    changed = int((low["scan"] != R["scan"]).sum())
    print("scans16: %d of %d centres tied, lowest-scan rule differs at %d, scans used %d" % (tied, len(R["m"]), changed, len(set(R["scan"].tolist()))))
    assert tied >= 0.2 * len(R["m"]) and changed >= 50
    assert set(R["scan"].tolist()) == set(range(16))
    one = ref.reference("scans16_all15")
    assert (one["scan"] == 15).all() and np.array_equal(one["centre"], R["centre"]) and np.array_equal(one["c"], one["m"])


@pytest.mark.parametrize("name", ref.DUPLICATES)
def test_duplicates_and_absorbing_absorbed_points(name):
    args = ref.case(name)
    P = args[2]
    assert len(np.unique(P, axis=0)) < len(P)                                 # coincident points
    R = ref.reference(name)
    fresh = ref.merge_close_points(*args, only_unabsorbed=True)
    # a centre absorbs absorbed points too: the variant keeps the centres (a covered point stays covered) but changes means
    assert np.array_equal(fresh["centre"], R["centre"])
    assert (_bits(fresh["xyz"]) != _bits(R["xyz"])).any()
    assert int(R["m"].sum()) > len(P)


def test_dense_case_overflows_the_neighbour_list_within_a_wave_and_across_blocks():
    dist, scans, P, col, sidx, mxr = ref.case("dense")
    r2 = ref.radius2(dist)
    is_centre = np.zeros(len(P), bool); is_centre[ref.reference("dense")["centre"]] = True
    same_wave = other_block = most = 0
    for i in range(len(P)):
        low = np.nonzero(ref.sqdist(P[:i], P[i]) < r2)[0]
        most = max(most, len(low))
        if len(low) <= ref.MERGE_LIST or not is_centre[low].any():
            continue
        first = int(low[is_centre[low]][0])                                    # the centre whose decision this point waits for
        same_wave += int(first // 64 == i // 64)
        other_block += int(first // 256 != i // 256)
    print("dense: up to %d lower-index neighbours; list overflow with the centre in the own wave %d times, in another block %d times"
          % (most, same_wave, other_block))
    assert same_wave >= 1 and other_block >= 1
    assert ref.reference("dense")["m"].max() > 300


@pytest.mark.parametrize("name", ref.EXACT)
def test_exact_cases_sum_without_rounding(name):
    """every partial sum of the sequential f32 sums is an integer number of lattice steps below 2^24 (and every other summation
    order passes through subsets of the same terms, whose sums obey the same limit: bounded here by sum |x_j|)"""
    dist, scans, P, col, sidx, mxr = ref.case(name)
    R = ref.reference(name)
    steps = P.astype(np.float64) / ref.STEP
    assert np.array_equal(steps, np.rint(steps)) and np.array_equal(col, np.rint(col)) and (col >= 0).all()
    max_pos = max(float(np.abs(steps[nb]).sum(0).max()) for nb in R["nbrs"])
    max_col = max(float(col[nb].astype(np.float64).sum()) for nb in R["nbrs"])
    print("%s: m <= %d, largest sum |x_j| = %d steps (2^%.2f), largest colour sum %d" % (name, R["m"].max(), max_pos, np.log2(max_pos), max_col))
    assert max_pos < 2 ** 24 and max_col < 2 ** 24 and R["m"].max() <= 32
    for nb in R["nbrs"]:
        part = np.cumsum(steps[nb], 0)
        assert np.array_equal(part, np.rint(part)) and np.abs(part).max() < 2 ** 24
    assert np.array_equal(R["xyz"].astype(np.float64), (R["mean64"]).astype(np.float32).astype(np.float64))    # one rounding: the division


def test_library_refuses_undefined_input_before_it_needs_a_device(e3d):
    """the refusals are a host pass over the arrays: they come before the device is looked for, with or without a GPU"""
    dist, scans, P, col, sidx, mxr = ref.case("size_65")
    for value in (np.nan, np.inf, -np.inf):
        bad = P.copy(); bad[64, 2] = value
        with pytest.raises(e3d.E3DError, match="point 64 has a non-finite coordinate"):
            e3d.merge_close_points(dist, scans, bad, col, sidx, mxr)
    bad = sidx.copy(); bad[7] = scans
    with pytest.raises(e3d.E3DError, match="point 7 has scan index 3, but there are 3 scans"):
        e3d.merge_close_points(dist, scans, P, col, bad, mxr)
    for d in (np.nan, np.inf, -1.0, 0.0):
        with pytest.raises(e3d.E3DError, match="merge distance must be positive"):
            e3d.merge_close_points(d, scans, P, col, sidx, mxr)


@pytest.mark.parametrize("C", ref.CELL_COUNTS)
def test_cell_count_cases_fill_exactly_C_cells_with_one_pair_each(C):
    """the input does what it says: C occupied cells of the library's grid, two points less than the merge distance apart in each, the
    pairs at least three merge distances from one another -- and the restatement alone merges them into exactly C points"""
    dist, scans, P, col, sidx, mxr = ref.case("cells_%d" % C)
    assert len(P) == 2 * C
    cells = ref.grid_cells(dist, P)
    assert np.array_equal(cells[:C], cells[C:]) and len(np.unique(cells, axis=0)) == C
    within = np.sqrt(((P[:C].astype(np.float64) - P[C:]) ** 2).sum(1))
    assert (within > 0).all() and (within < 0.1 * dist).all()
    for i in range(2 * C):                                                      # every other pair: three merge distances away or more
        d = np.sqrt(((P.astype(np.float64) - P[i]) ** 2).sum(1))
        d[[i % C, C + i % C]] = np.inf
        assert d.min() >= 3.0 * dist
    R = ref.reference("cells_%d" % C)
    assert len(R["m"]) == C and (R["m"] == 2).all() and np.array_equal(R["centre"], np.arange(C))
    assert all(np.array_equal(nb, (i, C + i)) for i, nb in enumerate(R["nbrs"]))
    # the hash table's size by the library's rule, and that the counts sit where 2 C meets and crosses it
    tsize = 64
    while tsize < 2 * C:
        tsize <<= 1
    assert tsize == {1: 64, 32: 64, 33: 128, 64: 128, 65: 256, 1024: 2048, 1025: 4096}[C]


def test_chain_closed_form():
    R = ref.reference("chain_increasing")
    assert np.array_equal(R["centre"], np.arange(0, ref.CHAIN_N, 2))            # the even positions
    assert R["m"][0] == 2 and (R["m"][1:] == 3).all()
    for order in ("decreasing", "shuffled"):
        pos = ref.chain_positions(order)[ref.reference("chain_" + order)["centre"]]
        assert len(pos) >= ref.CHAIN_N // 3 and (np.diff(np.sort(pos)) >= 2).all() and (np.diff(np.sort(pos)) <= 3).all()
    assert np.array_equal(np.sort(ref.chain_positions("decreasing")[ref.reference("chain_decreasing")["centre"]]), np.arange(1, ref.CHAIN_N, 2))


def test_far_lattice_keeps_every_site_and_is_not_exact():
    P = ref.case("lattice_far")[2]
    base = ref.case("lattice")[2]
    shift = np.asarray(ref.LATTICE_SHIFTS["lattice_far"])
    assert np.array_equal(P.astype(np.float64) - shift, base.astype(np.float64))
    R, B = ref.reference("lattice_far"), ref.reference("lattice")
    assert np.array_equal(R["centre"], B["centre"]) and np.array_equal(R["scan"], B["scan"]) and np.array_equal(R["m"], B["m"])
    assert (R["xyz"].astype(np.float64) != R["mean64"].astype(np.float32).astype(np.float64)).any()       # sums beyond 2^24 steps round
