"""CPU restatement (numpy, f32 operation by operation) of DatasetInspector's label transfer, MainWindow::TransferLabels
(src/dataset_inspector/gui_main_window.cc:868-1054): the expected values of the e3d_reg_mask_transfer_* tests.  TEST INFRASTRUCTURE ONLY.

  1  an empty source mask: nothing happens (:895-898);
  2  point pass (:906-955): a serial loop over the scan points in cloud order on a blank target mask; a point visible in the source
     whose source pixel is masked (and, without transfer_eval_obs, not kEvalObs) and visible in the target writes the source value
     to its target pixel, later points over earlier ones;
  3  fill-in (:957-1032): integral images (cumulative sums) of the kObs and -- with transfer_eval_obs -- kEvalObs pixels of step 2,
     5 x 5 window clipped at the borders, threshold (int)(0.10f * 25 + 0.5f) = 3;
  4  merge (:1034-1047) into the target's existing mask.

Projection and occlusion depth come from the CPU checker's binding (reg_binding.cam_project, reg_binding.splat_depth), the pieces the
visibility tests show to be bit-identical to the device for every camera model.

An image is described as dict(R=(3, 3) f32 image_R_global, t=(3,) f32, cam=the level-0 camera of reg_binding, occlusion=(h, w) f32).
"""
import numpy as np

from debug_cloud_ref import F, transform

NO_MASK, OBS, EVAL_OBS = 0, 1, 2          # opt::MaskType (image.h:43-47)
RADIUS = 2                                # kRadius: the 5 x 5 window
FILL_IN_THRESHOLD = int(np.float32(0.10) * np.float32(25) + np.float32(0.5))       # static_cast<int>(kFillInThreshold * 25 + 0.5f)
assert FILL_IN_THRESHOLD == 3


def visibility(pts, image, occlusion_threshold=0.01, project=None):
    """The visibility test of :909-921 / :931-943 for every point -> (visible[n] bool, ix[n], iy[n], occluded[n] bool); occluded =
    inside the image but behind the occlusion depth.  One projection call per point in front of the camera; the comparisons around
    it are the same f32 operations on whole arrays."""
    if project is None:
        from oracle import reg_binding as rb
        project = rb.cam_project
    cam, occlusion = image["cam"], np.asarray(image["occlusion"], F)
    pp = transform(image["R"], image["t"], pts)
    n = len(pp)
    visible = np.zeros(n, bool); occluded = np.zeros(n, bool)
    ix = np.zeros(n, np.int64); iy = np.zeros(n, np.int64)
    front = np.nonzero(pp[:, 2] > F(0))[0]                       # source_point.z() > 0
    if len(front) == 0:
        return visible, ix, iy, occluded
    pxy = np.array([project(cam, pp[i]) for i in front], F).reshape(-1, 2)
    ax = pxy[:, 0] + F(0.5); ay = pxy[:, 1] + F(0.5)             # pxy + 0.5f, f32
    with np.errstate(invalid="ignore"):
        castable = np.isfinite(ax) & np.isfinite(ay) & (np.abs(ax) < 2147483648.0) & (np.abs(ay) < 2147483648.0)
        x = np.where(castable, np.trunc(ax), -1).astype(np.int64)    # int ix = pxy.x() + 0.5f: towards zero
        y = np.where(castable, np.trunc(ay), -1).astype(np.int64)
        inside = castable & (ax >= 0) & (ay >= 0) & (x >= 0) & (y >= 0) & (x < cam.width) & (y < cam.height)
    k = front[inside]; x = x[inside]; y = y[inside]
    ix[k] = x; iy[k] = y
    seen = occlusion[y, x] + F(occlusion_threshold) >= pp[k, 2]  # f32 + f32 >= f32
    visible[k[seen]] = True
    occluded[k[~seen]] = True
    return visible, ix, iy, occluded


def point_labels(source_vis, source_mask, transfer_eval_obs):
    """The value a point carries (:921-926): its source pixel's mask value if it is visible there, the value is not kNoMask and --
    without transfer_eval_obs -- not kEvalObs; else 0."""
    visible, ix, iy, _ = source_vis
    labels = np.zeros(len(visible), np.uint8)
    for i in np.nonzero(visible)[0]:
        v = source_mask[iy[i], ix[i]]
        if v == NO_MASK:
            continue
        if not transfer_eval_obs and v == EVAL_OBS:
            continue
        labels[i] = v
    return labels


def point_pass(labels, target_vis, shape):
    """:901-903, :931-951: blank mask, points in cloud order, a later point overwrites an earlier one."""
    visible, ix, iy, _ = target_vis
    mask = np.zeros(shape, np.uint8)
    for i in np.nonzero((labels != 0) & visible)[0]:           # ascending: cloud order
        mask[iy[i], ix[i]] = labels[i]
    return mask


def _integral(flags):
    """integral(y, x) = number of set flags in rows 0 .. y, columns 0 .. x (:968-995)."""
    return np.cumsum(np.cumsum(flags.astype(np.int64), axis=1), axis=0)


def _window_counts(integral):
    """:1004-1023 for every pixel: the sum over rows y - 2 .. min(rows - 1, y + 2) and columns x - 2 .. min(cols - 1, x + 2), from the
    four corners of the integral image; a corner with a negative index counts 0."""
    rows, cols = integral.shape
    padded = np.zeros((rows + 1, cols + 1), np.int64); padded[1:, 1:] = integral          # padded[y + 1, x + 1] = integral(y, x), index -1 -> 0
    y = np.arange(rows)[:, None]; x = np.arange(cols)[None, :]
    min_y_minus_one = np.maximum(y - RADIUS - 1, -1); max_y = np.minimum(rows - 1, y + RADIUS)
    min_x_minus_one = np.maximum(x - RADIUS - 1, -1); max_x = np.minimum(cols - 1, x + RADIUS)
    return (padded[min_y_minus_one + 1, min_x_minus_one + 1] + padded[max_y + 1, max_x + 1]
            - padded[min_y_minus_one + 1, max_x + 1] - padded[max_y + 1, min_x_minus_one + 1])


def fill_in(mask, transfer_eval_obs):
    """:957-1032.  The integral images are taken from the point pass's mask before any pixel is filled."""
    out = mask.copy()
    obs_count = _window_counts(_integral(mask == OBS))
    out[obs_count >= FILL_IN_THRESHOLD] = OBS
    if transfer_eval_obs:
        eval_obs_count = _window_counts(_integral(mask == EVAL_OBS))
        out[eval_obs_count >= FILL_IN_THRESHOLD] = EVAL_OBS             # after the kObs rule: it wins
    return out


def merge(new_mask, existing):
    """:1034-1047: without an existing mask the new one; else the new value wherever it is not 0 and the existing one is not kEvalObs."""
    if existing is None:
        return new_mask.copy()
    out = np.array(existing, np.uint8, copy=True)
    take = (new_mask != NO_MASK) & (out != EVAL_OBS)
    out[take] = new_mask[take]
    return out


def transfer_from_labels(labels, target_vis, shape, transfer_eval_obs, existing=None):
    """Steps 2 (target side) to 4 -> dict(mask_out, stats, point_mask, filled): stats = (pixels set by the point pass, non-zero pixels
    after the fill-in, pixels of mask_out that differ from `existing` -- from 0 without one)."""
    pm = point_pass(labels, target_vis, shape)
    filled = fill_in(pm, transfer_eval_obs)
    out = merge(filled, existing)
    before = existing if existing is not None else np.zeros(shape, np.uint8)
    stats = (int((pm != 0).sum()), int((filled != 0).sum()), int((out != before).sum()))
    return dict(mask_out=out, stats=stats, point_mask=pm, filled=filled)


def transfer_labels(pts, source, target, source_mask, transfer_eval_obs, existing=None, occlusion_threshold=0.01, project=None):
    """The whole of TransferLabels for one pair -> the dict of transfer_from_labels plus labels and n_labelled; None if the source has
    no mask (step 1: the target stays as it is)."""
    if source_mask is None:
        return None
    sv = visibility(pts, source, occlusion_threshold, project)
    tv = visibility(pts, target, occlusion_threshold, project)
    labels = point_labels(sv, np.asarray(source_mask, np.uint8), transfer_eval_obs)
    shape = (target["cam"].height, target["cam"].width)
    r = transfer_from_labels(labels, tv, shape, transfer_eval_obs, existing)
    r["labels"] = labels; r["n_labelled"] = int((labels != 0).sum())
    r["source_vis"] = sv; r["target_vis"] = tv
    return r
