"""e3d_reg_mask_transfer_source / _target (DatasetInspector's "Label transfer" on the GPU) through capi.RegProblem, and bin/MaskTransfer
around them, against the CPU restatement in tests/mask_transfer_ref.py.  Projection and occlusion depth are bit-identical on both sides
for every camera model (test_gpu_reg.py), everything after them is integer work: every comparison is np.array_equal on uint8, no
tolerance, no pixel left out.  The scene, its masks and the restatement's results come from tests/test_mask_transfer_host.py, which
checks on the CPU that they are not trivial."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import mask_transfer_ref as ref
import test_mask_transfer_host as host
from cli_util import BIN, ROOT
from test_mask_transfer_host import HEIGHT, N_LEVELS, OCCLUSION_THRESHOLD, SOURCE, SPLAT_RADIUS, TARGETS, WIDTH

pytestmark = pytest.mark.gpu
sys.path.insert(0, ROOT)

MODELS = list(range(13))
F = np.float32


def _problem(e3d, S, shard=None, scan=True):
    M = S["M"]
    G = e3d.RegProblem(e3d.default_reg_params(image_scale_count=N_LEVELS))
    if shard is not None:            # the transfer calls no collective: the callbacks only have to exist
        G.set_shard(shard[0], shard[1], lambda buf: None, lambda ptr, count, dtype: None)
    G.set_intrinsics(0, WIDTH, HEIGHT, M["params"], 0, N_LEVELS, camera_type=S["model"])
    G.set_splat_points(S["scan"])
    for i, im in enumerate(M["images"]):
        G.set_image(i, 0, im["pyr"] if shard is None or i % shard[1] == shard[0] else None)
        G.set_image_pose(i, im["q_init"], im["t_init"])
    if scan:
        G.set_scan_points(S["scan"])
    return G


def _check(got, exp):
    out, stats = got
    assert out.dtype == np.uint8 and out.shape == exp["mask_out"].shape
    assert np.array_equal(out, exp["mask_out"]), "%d pixels differ" % int((out != exp["mask_out"]).sum())
    assert stats == exp["stats"], (stats, exp["stats"])


@pytest.mark.parametrize("model", MODELS)
def test_parity_over_models_and_flags(e3d, model):
    """Source image 0 -> targets 1 and 2, with and without transfer_eval_obs, with and without an existing mask: mask_out, the three
    stats and the number of labelled points equal the restatement's."""
    S = host.scene(model)
    G = _problem(e3d, S)
    smask, emask = host.source_mask(), host.existing_mask()
    for flag in (False, True):
        n = G.mask_transfer_source(SOURCE, smask, flag)
        assert n == host.expected(model, TARGETS[0], flag, False)["n_labelled"] and n > 2000
        for target in TARGETS:
            for with_existing in (False, True):
                exp = host.expected(model, target, flag, with_existing)
                _check(G.mask_transfer_target(target, emask if with_existing else None, return_stats=True), exp)
    # without return_stats: the mask alone
    assert np.array_equal(G.mask_transfer_target(1), host.expected(model, 1, True, False)["mask_out"])


def _mixed_scene():
    """Two cameras on one problem: THIN_PRISM_FISHEYE at 248 x 180 (image 0) and PINHOLE at 200 x 150 (image 1), the poses and the scan
    of the fisheye scene."""
    from oracle import binding as ob
    from oracle import reg_binding as rb
    from reg_util import camera_params
    S = host.scene(2)
    intr = {0: dict(w=WIDTH, h=HEIGHT, params=S["M"]["params"], model=2),
            1: dict(w=200, h=150, params=camera_params(0, 170.0, 168.5, 99.6, 75.3), model=0)}
    images = {}
    for i in (0, 1):
        im = S["M"]["images"][i]; I = intr[i]
        cam = rb.make_camera(I["w"], I["h"], I["params"], I["model"])
        R = ob.quat_to_R(np.asarray(im["q_init"], F))
        images[i] = dict(R=R, t=np.asarray(im["t_init"], F), cam=cam, occlusion=rb.splat_depth(S["scan"], R, im["t_init"], cam, SPLAT_RADIUS),
                         q=im["q_init"])
    return S, intr, images


def test_mixed_intrinsics(e3d):
    """Source and target with different camera models and image sizes, both ways, on one RegProblem built with the binding."""
    S, intr, images = _mixed_scene()
    G = e3d.RegProblem(e3d.default_reg_params(image_scale_count=1))
    for iid, I in intr.items():
        G.set_intrinsics(iid, I["w"], I["h"], I["params"], 0, 1, camera_type=I["model"])
    G.set_splat_points(S["scan"])
    for i, im in images.items():
        G.set_image(i, i, [np.zeros((intr[i]["h"], intr[i]["w"]), np.uint8)])
        G.set_image_pose(i, im["q"], im["t"])
    G.set_scan_points(S["scan"])
    masks = {0: host.source_mask(), 1: np.zeros((150, 200), np.uint8)}
    masks[1][0:50, 0:90] = 1; masks[1][40:110, 150:200] = 2; masks[1][60:100, 70:120] = 1; masks[1][100:104, 70:120] = 2
    existing = {0: host.existing_mask(), 1: np.zeros((150, 200), np.uint8)}
    existing[1][20:60, 30:80] = 2; existing[1][50:120, 120:190] = 1
    vis = {i: ref.visibility(S["scan"], images[i], OCCLUSION_THRESHOLD) for i in images}
    for source, target in ((0, 1), (1, 0)):
        for flag in (False, True):
            labels = ref.point_labels(vis[source], masks[source], flag)
            assert G.mask_transfer_source(source, masks[source], flag) == int((labels != 0).sum()) > 1000
            for ex in (None, existing[target]):
                exp = ref.transfer_from_labels(labels, vis[target], (intr[target]["h"], intr[target]["w"]), flag, ex)
                assert exp["stats"][0] >= 300 and exp["stats"][1] > exp["stats"][0]
                _check(G.mask_transfer_target(target, ex, return_stats=True), exp)
    # a mask of the other camera's size is refused by the binding (the library cannot see a buffer's size)
    with pytest.raises(e3d.E3DError):
        G.mask_transfer_source(0, masks[1])
    with pytest.raises(e3d.E3DError):
        G.mask_transfer_target(0, existing[1])


def test_batch_hygiene(e3d):
    """One source call, then targets 1, 2, 1 again and 0 (source = target): each equals what a fresh handle gives for that pair alone --
    the winners are cleared for every target and the labels are not used up.  A second source call replaces the labels."""
    model = 0
    S = host.scene(model)
    smask, emask = host.source_mask(), host.existing_mask()
    G = _problem(e3d, S)
    n = G.mask_transfer_source(SOURCE, smask, True)
    for target in (1, 2, 1, 0):
        got = G.mask_transfer_target(target, emask, return_stats=True)
        fresh = _problem(e3d, S)
        assert fresh.mask_transfer_source(SOURCE, smask, True) == n
        alone = fresh.mask_transfer_target(target, emask, return_stats=True)
        assert np.array_equal(got[0], alone[0]) and got[1] == alone[1]
        _check(got, host.expected(model, target, True, True))
    assert host.expected(model, 0, True, True)["stats"][0] >= 300                 # source = target is no empty case
    # another mask on the same handle: the old labels are gone
    other = np.ascontiguousarray(smask[::-1, ::-1])
    labels = ref.point_labels(host.scene_visibility(model, SOURCE), other, True)
    assert G.mask_transfer_source(SOURCE, other, True) == int((labels != 0).sum()) != n
    exp = ref.transfer_from_labels(labels, host.scene_visibility(model, 1), (HEIGHT, WIDTH), True, None)
    assert exp["stats"][0] >= 300 and not np.array_equal(exp["mask_out"], host.expected(model, 1, True, False)["mask_out"])
    _check(G.mask_transfer_target(1, return_stats=True), exp)
    # ... and the same flag change without a new mask object: transfer_eval_obs belongs to the source call
    G.mask_transfer_source(SOURCE, smask, False)
    _check(G.mask_transfer_target(2, return_stats=True), host.expected(model, 2, False, False))


def test_device_tensors_are_accepted(e3d):
    import torch
    model = 0
    G = _problem(e3d, host.scene(model))
    smask = torch.from_numpy(host.source_mask()).cuda()
    emask = torch.from_numpy(host.existing_mask()).cuda()
    assert G.mask_transfer_source(SOURCE, smask, True) == host.expected(model, 1, True, True)["n_labelled"]
    _check(G.mask_transfer_target(1, emask, return_stats=True), host.expected(model, 1, True, True))


def test_degenerate_inputs(e3d):
    model = 0
    S = host.scene(model)
    emask = host.existing_mask()
    G = _problem(e3d, S)
    zeros = np.zeros((HEIGHT, WIDTH), np.uint8)
    # an all-zero source mask: no labels, the existing mask (or zeros) comes back
    assert G.mask_transfer_source(SOURCE, zeros, True) == 0
    out, stats = G.mask_transfer_target(1, emask, return_stats=True)
    assert np.array_equal(out, emask) and stats == (0, 0, 0)
    out, stats = G.mask_transfer_target(2, return_stats=True)
    assert not out.any() and stats == (0, 0, 0)
    # all kObs: every pixel a point visible in both images reaches, plus the fill-in
    ones = np.ones((HEIGHT, WIDTH), np.uint8)
    sv, tv = host.scene_visibility(model, SOURCE), host.scene_visibility(model, 1)
    labels = ref.point_labels(sv, ones, False)
    assert G.mask_transfer_source(SOURCE, ones, False) == int(sv[0].sum()) == int((labels != 0).sum())
    exp = ref.transfer_from_labels(labels, tv, (HEIGHT, WIDTH), False, None)
    assert exp["stats"][0] > 5000 and exp["stats"][1] > exp["stats"][0]
    _check(G.mask_transfer_target(1, return_stats=True), exp)
    # a scan-point count that is no multiple of the block size (and one point more than a multiple): the first n points of the scan,
    # the occlusion geometry as it was
    smask = host.source_mask()
    for n in (12345, 256 * 40 + 1, 255, 1):
        G.set_scan_points(S["scan"][:n])
        cut = lambda v: tuple(a[:n] for a in v)
        labels = ref.point_labels(cut(sv), smask, True)
        assert G.mask_transfer_source(SOURCE, smask, True) == int((labels != 0).sum())
        _check(G.mask_transfer_target(1, emask, return_stats=True), ref.transfer_from_labels(labels, cut(tv), (HEIGHT, WIDTH), True, emask))
    # no scan points at all: not an error
    G.set_scan_points(np.zeros((0, 3), np.float32))
    assert G.mask_transfer_source(SOURCE, smask, True) == 0
    out, stats = G.mask_transfer_target(1, emask, return_stats=True)
    assert np.array_equal(out, emask) and stats == (0, 0, 0)
    assert not G.mask_transfer_target(2).any()


def test_errors_leave_the_handle_usable(e3d):
    model = 0
    S = host.scene(model)
    smask, emask = host.source_mask(), host.existing_mask()
    L = e3d.lib()
    import ctypes as C
    out = np.zeros((HEIGHT, WIDTH), np.uint8)

    def raw_target(G, image_id, existing, mask_out):
        return G._chk(L.e3d_reg_mask_transfer_target(G._h, image_id, C.c_void_p(existing.ctypes.data) if existing is not None else None,
                                                     C.c_void_p(mask_out.ctypes.data) if mask_out is not None else None, None), "e3d_reg_mask_transfer_target")
    # no scan points set
    G = _problem(e3d, S, scan=False)
    with pytest.raises(e3d.E3DError, match="no scan points"):
        G.mask_transfer_source(SOURCE, smask)
    with pytest.raises(e3d.E3DError, match="no scan points"):
        G.mask_transfer_target(1)
    G.set_scan_points(S["scan"])
    # target before source -- also after new scan points
    with pytest.raises(e3d.E3DError, match="mask_transfer_source first"):
        G.mask_transfer_target(1)
    G.mask_transfer_source(SOURCE, smask, True)
    G.set_scan_points(S["scan"])
    with pytest.raises(e3d.E3DError, match="mask_transfer_source first"):
        G.mask_transfer_target(1)
    G.mask_transfer_source(SOURCE, smask, True)
    # unknown image: the binding's own check and the library's
    with pytest.raises(e3d.E3DError):
        G.mask_transfer_source(99, smask)
    with pytest.raises(e3d.E3DError):
        G.mask_transfer_target(99)
    with pytest.raises(e3d.E3DError, match="image 99 not set"):
        G._chk(L.e3d_reg_mask_transfer_source(G._h, 99, C.c_void_p(smask.ctypes.data), 0), "e3d_reg_mask_transfer_source")
    with pytest.raises(e3d.E3DError, match="image 99 not set"):
        raw_target(G, 99, None, out)
    # mask_out == NULL, source_mask == NULL
    with pytest.raises(e3d.E3DError, match="null argument"):
        raw_target(G, 1, None, None)
    with pytest.raises(e3d.E3DError, match="null argument"):
        G._chk(L.e3d_reg_mask_transfer_source(G._h, SOURCE, None, 0), "e3d_reg_mask_transfer_source")
    # the failed calls changed nothing: the labels of the last good source call are still there
    _check(G.mask_transfer_target(1, emask, return_stats=True), host.expected(model, 1, True, True))
    # a mask value other than 0 / 1 / 2 in the existing mask: refused, the handle stays usable
    bad = emask.copy(); bad[HEIGHT - 1, WIDTH - 1] = 3
    with pytest.raises(e3d.E3DError, match="existing mask holds 1 values other than 0, 1, 2"):
        G.mask_transfer_target(1, bad)
    _check(G.mask_transfer_target(2, emask, return_stats=True), host.expected(model, 2, True, True))
    # ... in the source mask (at a pixel no point may see): refused, and no labels are left behind
    bad = smask.copy(); bad[179, 0] = 255; bad[100, 100] = 7
    with pytest.raises(e3d.E3DError, match="source mask holds 2 values other than 0, 1, 2"):
        G.mask_transfer_source(SOURCE, bad, True)
    with pytest.raises(e3d.E3DError, match="mask_transfer_source first"):
        G.mask_transfer_target(1)
    assert G.mask_transfer_source(SOURCE, smask, False) == host.expected(model, 1, False, False)["n_labelled"]
    _check(G.mask_transfer_target(1, return_stats=True), host.expected(model, 1, False, False))
    # an image owned by another rank (image id mod 2 != 0)
    R0 = _problem(e3d, S, shard=(0, 2))
    with pytest.raises(e3d.E3DError, match="image 1 belongs to rank 1"):
        R0.mask_transfer_source(1, smask)
    R0.mask_transfer_source(0, smask, True)
    with pytest.raises(e3d.E3DError, match="image 1 belongs to rank 1"):
        R0.mask_transfer_target(1)
    _check(R0.mask_transfer_target(2, return_stats=True), host.expected(model, 2, True, False))


def test_profile_groups(e3d):
    """One launch per call in each of the three kernel groups; units: scan points, scan points, target pixels."""
    S = host.scene(0)
    G = _problem(e3d, S)
    n = float(len(S["scan"]))
    G.profile(True)
    G.mask_transfer_source(SOURCE, host.source_mask(), True)
    G.profile(True)                                                 # (reads the record, leaves the profile on)
    assert G.kernel_groups["mask.label_points"][1:] == (1, n)
    assert "mask.scatter" not in G.kernel_groups and "mask.fill" not in G.kernel_groups
    G.mask_transfer_target(1)
    G.mask_transfer_target(2, host.existing_mask())
    G.profile(False)
    assert G.kernel_groups["mask.label_points"][1:] == (1, n)
    assert G.kernel_groups["mask.scatter"][1:] == (2, 2 * n) and G.kernel_groups["mask.fill"][1:] == (2, 2.0 * WIDTH * HEIGHT)
    assert all(G.kernel_groups[k][0] >= 0 for k in ("mask.label_points", "mask.scatter", "mask.fill"))


# ---- bin/MaskTransfer end to end -------------------------------------------------------------------------------------------------------
def _tree_digest(d, skip=()):
    out = {}
    for dirpath, _, files in os.walk(d):
        if any(os.path.abspath(dirpath).startswith(os.path.abspath(s)) for s in skip):
            continue
        for f in files:
            p = os.path.join(dirpath, f)
            out[os.path.relpath(p, d)] = hashlib.sha256(open(p, "rb").read()).hexdigest()
    return out


def _read_png(path):
    from PIL import Image
    im = Image.open(path)
    assert im.mode == "L", im.mode                              # 8 bit, one channel
    return np.array(im)


def test_cli_end_to_end(tmp_path, e3d):
    """A dataset on disk (three images, a mask on the source, existing masks on two targets): the PNGs the tool writes are the binding's
    mask_out, the dataset stays untouched with --output_folder_path, an unchanged target is not written, --in_place replaces the
    targets' files and GroundTruthCreator reads them."""
    from reg_util import make_multi_image_scene
    from test_gpu_cli_reg import _write_dataset, _write_png
    M = make_multi_image_scene(n_points=6000, n_images=3, seed=12, perturb=0.0)
    W, H = M["width"], M["height"]
    names = ["dslr/img_%d.png" % i for i in range(3)]
    d = _write_dataset(tmp_path, M, names)
    smask = np.zeros((H, W), np.uint8); smask[50:120, 70:150] = 1; smask[95:135, 120:175] = 2; smask[0:30, 0:40] = 1
    e1 = np.zeros((H, W), np.uint8); e1[60:90, 80:120] = 2; e1[100:130, 110:160] = 1
    e2 = np.full((H, W), 2, np.uint8)                             # kEvalObs everywhere: nothing can change
    mask_file = lambda root, i: os.path.join(root, "masks_for_images", "dslr", "img_%d.png" % i)
    own = os.path.join(d, "images")                               # Image::GetImageMaskPath: masks_for_images/ lies next to the camera directories
    _write_png(mask_file(own, 0), smask); _write_png(mask_file(own, 1), e1); _write_png(mask_file(own, 2), e2)
    # the same transfer through the binding, with the state as the tool reads it: parameters through their text, cx cy moved by -0.5f
    cam_line = [l for l in open(os.path.join(d, "state", "cameras.txt")) if not l.startswith("#")][0].split()
    params = np.array([float(v) for v in cam_line[4:]], np.float64).astype(np.float32)
    params[2] += np.float32(-0.5); params[3] += np.float32(-0.5)
    G = e3d.RegProblem(e3d.default_reg_params(image_scale_count=1))
    G.set_intrinsics(0, W, H, params, 0, 1)
    G.set_splat_points(M["pts"])
    for i, im in enumerate(M["images"]):
        G.set_image(i, 0, [im["pyr"][0]])
        G.set_image_pose(i, np.array(["%.9g" % v for v in im["q_init"]], np.float64).astype(np.float32),
                         np.array(["%.9g" % v for v in im["t_init"]], np.float64).astype(np.float32))
    G.set_scan_points(M["pts"])
    n_labelled = G.mask_transfer_source(0, smask, True)
    want = {1: G.mask_transfer_target(1, e1, return_stats=True), 2: G.mask_transfer_target(2, e2, return_stats=True),
            0: G.mask_transfer_target(0, smask, return_stats=True)}
    assert n_labelled > 500 and want[1][1][0] >= 300 and want[1][1][2] > 0 and want[0][1][2] > 0
    assert want[2][1][2] == 0 and want[2][1][0] >= 300 and np.array_equal(want[2][0], e2)
    assert (want[1][0] == 2).sum() > (e1 == 2).sum() and ((e1 == 2) & (want[1][0] != 2)).sum() == 0

    base = [os.path.join(BIN, "MaskTransfer"), "--scan_alignment_path", os.path.join(d, "scans.mlp"), "--image_base_path", os.path.join(d, "images"),
            "--state_path", os.path.join(d, "state"), "--source_image", names[0], "--target_images", "%s,2,%s,0" % (names[1], names[1]),
            "--transfer_eval_obs", "1"]
    before = _tree_digest(d)
    out_dir = os.path.join(d, "transferred")
    r = subprocess.run(base + ["--output_folder_path", out_dir], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert _tree_digest(d, skip=[out_dir]) == before                                 # the dataset's own files: untouched
    assert sorted(_tree_digest(out_dir)) == ["masks_for_images/dslr/img_0.png", "masks_for_images/dslr/img_1.png"]
    for i in (1, 0):
        assert np.array_equal(_read_png(mask_file(out_dir, i)), want[i][0]), i
    lines = [l for l in r.stdout.split("\n") if l.startswith("Target image ")]
    assert len(lines) == 3 and "%d of %d scan points carry a label" % (n_labelled, len(M["pts"])) in r.stdout
    for line, i in zip(lines, (1, 2, 0)):                                            # in the order given, img_1 once
        assert line.startswith("Target image %d " % i) and "point_pass %d filled %d changed %d" % want[i][1] in line, line
    assert "unchanged, not written" in lines[1] and "Wrote 2 of 3 masks." in r.stdout
    # default targets: every other image; transfer_eval_obs off by default
    G.mask_transfer_source(0, smask, False)
    plain = G.mask_transfer_target(1, e1, return_stats=True)
    out2 = os.path.join(d, "transferred2")
    r = subprocess.run(base[:9] + ["--output_folder_path", out2], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert sorted(_tree_digest(out2)) == ["masks_for_images/dslr/img_1.png"] and np.array_equal(_read_png(mask_file(out2, 1)), plain[0])
    assert not np.array_equal(plain[0], want[1][0])
    # --in_place 1: the targets' own files are replaced (img_2's is not: unchanged) ...
    r = subprocess.run(base + ["--in_place", "1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    after = _tree_digest(d, skip=[out_dir, out2])
    changed = sorted(k for k in after if after[k] != before.get(k))
    assert changed == ["images/masks_for_images/dslr/img_0.png", "images/masks_for_images/dslr/img_1.png"] and sorted(after) == sorted(before)
    for i in (1, 0):
        assert np.array_equal(_read_png(mask_file(own, i)), want[i][0]), i
    # ... and the next tool loads them without complaint
    r = subprocess.run([os.path.join(BIN, "GroundTruthCreator"), "--scan_alignment_path", os.path.join(d, "scans.mlp"), "--image_base_path",
                        os.path.join(d, "images"), "--state_path", os.path.join(d, "state"), "--output_folder_path", os.path.join(d, "gt"),
                        "--write_point_cloud", "0"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert os.path.isfile(os.path.join(d, "gt", "ground_truth_depth", "dslr", "img_1.png"))
