"""bin/StereoEvaluator on three pairs in tmp_path against the numpy restatement (tests/stereo_eval_ref.py): stdout, the JSON and the
error-map PNGs; the ways a pair's mask and estimate are found (PNG and binary PGM masks, a big-endian estimate, <pair>/disp0.pfm),
--pairs, and the refusals that name the pair."""
import json
import os
import subprocess

import numpy as np
import pytest

import stereo_eval_ref as ser
import stereo_ref as sr
from cli_util import BIN

pytestmark = pytest.mark.gpu
F = np.float32
TOOL = os.path.join(BIN, "StereoEvaluator")
W, H = 97, 61
THR, PCT = (0.5, 1, 2, 4), (50, 90, 95, 99)


def _png(path, img):
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(img, np.uint8)).save(path)


def _read_png(path):
    from PIL import Image
    return np.array(Image.open(path))


def _pair(seed):
    rng = np.random.default_rng(seed)
    gt = rng.uniform(1, 60, (H, W)).astype(F)
    gt[rng.random((H, W)) < 0.25] = np.inf
    mask = rng.choice(np.array([0, 128, 255], np.uint8), (H, W), p=[0.1, 0.3, 0.6])
    est = (np.where(np.isfinite(gt), gt, F(7)) + rng.normal(0, 1.5, (H, W))).astype(F)
    u = rng.random((H, W))
    est[u < 0.04] = np.inf                                                     # Middlebury's "no estimate"
    est[(u > 0.04) & (u < 0.06)] = np.nan
    est[(u > 0.06) & (u < 0.08)] = -3
    return gt, mask, est


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("stereo_eval"))
    gt_dir, est_dir = os.path.join(d, "gt"), os.path.join(d, "est")
    pairs = {"alley": _pair(1), "barn": _pair(2), "court": _pair(3)}
    for name, (gt, mask, est) in pairs.items():
        os.makedirs(os.path.join(gt_dir, name))
        sr.write_pfm(os.path.join(gt_dir, name, "disp0GT.pfm"), gt)
    os.makedirs(os.path.join(gt_dir, "notes"))                                 # a sub-folder without disp0GT.pfm is no pair
    os.makedirs(est_dir)
    # alley: a PNG mask, a little-endian estimate beside the folder
    _png(os.path.join(gt_dir, "alley", "mask0nocc.png"), pairs["alley"][1])
    sr.write_pfm(os.path.join(est_dir, "alley.pfm"), pairs["alley"][2])
    # barn: a binary PGM under the mask's name (read by content), a big-endian estimate whose header fields are separated by blanks and tabs
    with open(os.path.join(gt_dir, "barn", "mask0nocc.png"), "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (W, H) + pairs["barn"][1].tobytes())
    with open(os.path.join(est_dir, "barn.pfm"), "wb") as f:
        f.write(b"Pf %d\t%d  2.5\n" % (W, H) + np.ascontiguousarray(pairs["barn"][2][::-1]).astype(">f4").tobytes())
    # court: no mask, the estimate as <pair>/disp0.pfm
    os.makedirs(os.path.join(est_dir, "court"))
    sr.write_pfm(os.path.join(est_dir, "court", "disp0.pfm"), pairs["court"][2])
    pairs["court"] = (pairs["court"][0], None, pairs["court"][2])
    ref = {name: ser.evaluate(gt, mask, est, THR, PCT, error_maps=True) for name, (gt, mask, est) in pairs.items()}
    return d, gt_dir, est_dir, pairs, ref


def _run(args):
    return subprocess.run([TOOL] + args, capture_output=True, text=True, timeout=120)


def _parse(stdout):
    """-> {(name, region): {key: float}}"""
    out = {}
    for line in stdout.splitlines():
        f = line.split()
        out[(f[0], f[1])] = {kv.split("=")[0]: float(kv.split("=")[1]) for kv in f[2:]}
    return out


def _check_region(got, R, r):
    """got: one region's JSON record or stdout fields against the restatement's estimate 0, region r"""
    for key in ("coverage", "avgerr", "rms"):
        assert got[key] == pytest.approx(R[key][0, r], rel=1e-8), key
    for t, thr in enumerate(THR):
        for key in ("bad", "bad_or_missing"):
            v = got[key][t] if key in got else got["%s%g" % (key, thr)]
            assert v == pytest.approx(R[key][0, r, t], rel=1e-8), (key, thr)


def test_three_pairs(dataset):
    d, gt_dir, est_dir, pairs, ref = dataset
    out_json, maps = os.path.join(d, "scores.json"), os.path.join(d, "maps")
    r = _run(["--ground_truth_path", gt_dir, "--estimates_path", est_dir, "--output_path", out_json, "--error_maps_path", maps, "--timings"])
    assert r.returncode == 0, r.stderr
    for group in ("classify", "select", "sums"):
        assert "[timings] alley %s " % group in r.stderr
    lines = _parse(r.stdout)
    assert [k for k in lines] == [(n, reg) for n in ("alley", "barn", "court") for reg in ser.REGIONS] + [("mean", "all"), ("mean", "nocc")]
    J = json.load(open(out_json))
    assert J["thresholds"] == list(THR) and J["percentiles"] == list(PCT) and [p["name"] for p in J["pairs"]] == ["alley", "barn", "court"]
    for rec in J["pairs"]:
        R = ref[rec["name"]]
        assert (rec["width"], rec["height"]) == (W, H)
        for r_i, reg in enumerate(ser.REGIONS):
            g = rec["regions"][reg]
            assert [g["n_region"], g["n_valid"]] + g["n_bad"] == R["counts"][0, r_i].tolist()
            assert np.array_equal(np.array(g["quantiles"], F).view(np.uint32), R["quantiles"][0, r_i].view(np.uint32))
            for k, key in enumerate(("sum1", "sum2")):
                assert abs(g[key] - R["sums"][0, r_i, k]) <= (g["n_valid"] - 1) * 2.0 ** -53 * R["sums"][0, r_i, k]
            _check_region(g, R, r_i)
            _check_region(lines[(rec["name"], reg)], R, r_i)
            for k, p in enumerate(PCT):
                assert F(lines[(rec["name"], reg)]["A%d" % p]) == R["quantiles"][0, r_i, k]
        assert np.array_equal(_read_png(os.path.join(maps, rec["name"] + ".png")), R["error_maps"][0])
    assert sorted(os.listdir(maps)) == ["alley.png", "barn.png", "court.png"]
    # court has no mask: both regions are the known pixels
    assert J["pairs"][2]["regions"]["all"] == J["pairs"][2]["regions"]["nocc"]
    for r_i, reg in enumerate(ser.REGIONS):
        for key in ("coverage", "avgerr", "rms"):
            want = np.mean([ref[n][key][0, r_i] for n in ("alley", "barn", "court")])
            assert J["mean"][reg][key] == pytest.approx(want, rel=1e-12) and lines[("mean", reg)][key] == pytest.approx(want, rel=1e-8)
        for t, thr in enumerate(THR):
            for key in ("bad", "bad_or_missing"):
                want = np.mean([ref[n][key][0, r_i, t] for n in ("alley", "barn", "court")])
                assert J["mean"][reg][key][t] == pytest.approx(want, rel=1e-12) and lines[("mean", reg)]["%s%g" % (key, thr)] == pytest.approx(want, rel=1e-8)


def test_pairs_file_and_lists(dataset):
    d, gt_dir, est_dir, pairs, ref = dataset
    listing = os.path.join(d, "pairs.txt")
    with open(listing, "w") as f:
        f.write("# the order of the file, not of the folder\ncourt\n\n  alley   # trailing comment\n")
    r = _run(["--ground_truth_path", gt_dir, "--estimates_path", est_dir, "--pairs", listing, "--thresholds", "0,3", "--percentiles", "100"])
    assert r.returncode == 0, r.stderr
    lines = _parse(r.stdout)
    assert [k[0] for k in lines] == ["court", "court", "alley", "alley", "mean", "mean"]
    for name in ("court", "alley"):
        gt, mask, est = pairs[name]
        R = ser.evaluate(gt, mask, est, (0, 3), (100,))
        for r_i, reg in enumerate(ser.REGIONS):
            got = lines[(name, reg)]
            assert sorted(got) == sorted(["coverage", "avgerr", "rms", "bad0", "bad3", "bad_or_missing0", "bad_or_missing3", "A100"])
            assert got["bad3"] == pytest.approx(R["bad"][0, r_i, 1], rel=1e-8) and F(got["A100"]) == R["quantiles"][0, r_i, 0]


def test_refusals_name_the_pair(dataset, tmp_path):
    d, gt_dir, est_dir, pairs, ref = dataset
    listing = str(tmp_path / "pairs.txt")
    gt_dir = str(tmp_path / "gt")                                              # a ground truth of its own: alley and depot, no masks
    for name in ("alley", "depot"):
        os.makedirs(os.path.join(gt_dir, name))
        sr.write_pfm(os.path.join(gt_dir, name, "disp0GT.pfm"), pairs["alley"][0])
    # a pair without an estimate
    with open(listing, "w") as f:
        f.write("alley\ndepot\n")
    r = _run(["--ground_truth_path", gt_dir, "--estimates_path", est_dir, "--pairs", listing])
    assert r.returncode != 0 and "pair depot: no estimate" in r.stderr and r.stdout == ""
    # an estimate of another size
    other = str(tmp_path / "est")
    os.makedirs(other)
    sr.write_pfm(os.path.join(other, "alley.pfm"), pairs["alley"][2])
    sr.write_pfm(os.path.join(other, "depot.pfm"), pairs["alley"][2][:, :-1])
    r = _run(["--ground_truth_path", gt_dir, "--estimates_path", other, "--pairs", listing])
    assert r.returncode != 0 and "pair depot: the estimate is 96 x 61, the ground truth 97 x 61" in r.stderr and r.stdout == ""
    # a three-channel PFM
    with open(os.path.join(other, "depot.pfm"), "wb") as f:
        f.write(b"PF\n%d %d\n-1.0\n" % (W, H) + np.zeros((H, W, 3), "<f4").tobytes())
    r = _run(["--ground_truth_path", gt_dir, "--estimates_path", other, "--pairs", listing])
    assert r.returncode != 0 and "pair depot:" in r.stderr and "three-channel PFM (PF)" in r.stderr and r.stdout == ""
    # a pair the ground truth does not have
    with open(listing, "w") as f:
        f.write("nowhere\n")
    r = _run(["--ground_truth_path", gt_dir, "--estimates_path", est_dir, "--pairs", listing])
    assert r.returncode != 0 and "pair nowhere: cannot open" in r.stderr
