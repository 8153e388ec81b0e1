"""NumPy restatement of particle-sfm_amd/csrc/psfm_ground_truth.h: the per-frame counts of motion_seg/eval_traj_iou.py
(per_img_traj_metrics) and the majority vote of scripts/prepare_flyingthings3d.py (find_traj_label).  tests/test_ground_truth_host.py
pins it to the reference's fixtures; the GPU tests use it where no fixture exists.

The sampler is the fp32 grid_sample of psfm_device.h, operation by operation.  NumPy has no fp32 fused multiply-add, so `fma32`
builds one: the product of two fp32 numbers is exact in f64, the f64 sum is rounded to ODD (its TwoSum error says whether it was
inexact), and 53 bits rounded to odd round to the correct 24."""
import numpy as np

F = np.float32
EVAL_CASES = ["gt_eval_48x64_t23", "gt_eval_24x32_t27", "gt_eval_synth_9x13_t6"]
VOTE_CASES = ["gt_vote_40x56_l10_01", "gt_vote_40x56_l10_0255", "gt_vote_hand_8x9_l4"]


def mask_table():
    """The reference's mask value per PNG byte: 1.0 - b / 255.0 in f64 (eval_traj_iou.py:49), cast to fp32 (:107)."""
    return np.float32(1.0 - np.arange(256) / 255.0)


def fma32(a, b, c):
    a, b, c = (np.asarray(v, F).astype(np.float64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b                                  # exact: 24 + 24 bits
        t = p + c
        bb = t - p
        err = (p - (t - bb)) + (c - bb)            # TwoSum: t + err = p + c exactly
        inexact = np.isfinite(t) & np.isfinite(err) & (err != 0)
        even = (t.view(np.int64) & 1) == 0
        t = np.where(inexact & even, np.nextafter(t, np.where(err > 0, np.inf, -np.inf)), t)
        return t.astype(F)


def sample_np(mask_u8, table, xy):
    """psfm_gt_sample for every row of xy (n,2) f64 on one (H,W) u8 mask: (n,) f32."""
    mask_u8 = np.asarray(mask_u8, np.uint8)
    H, W = mask_u8.shape
    table = np.asarray(table, F)
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    with np.errstate(all="ignore"):
        x, y = xy[:, 0].astype(F), xy[:, 1].astype(F)
        cw, ch = F((W - 1) / 2.0), F((H - 1) / 2.0)
        one = F(1.0)
        ix = ((x / cw - one) + one) * cw
        iy = ((y / ch - one) + one) * ch
        fx, fy = np.floor(ix), np.floor(iy)
        w = ix - fx; e = one - w
        n = iy - fy; s = one - n
        nw, ne, sw, se = s * e, s * w, n * e, n * w
        cx = np.where(np.isnan(fx), F(-2.0), np.minimum(np.maximum(fx, F(-2.0)), F(W + 1.0)))
        cy = np.where(np.isnan(fy), F(-2.0), np.minimum(np.maximum(fy, F(-2.0)), F(H + 1.0)))
        x0, y0 = cx.astype(np.int64), cy.astype(np.int64)

        def tap(xx, yy):
            inside = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
            v = table[mask_u8[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]]
            return np.where(inside, v, F(0.0)).astype(F), inside
        vnw, i0 = tap(x0, y0); vne, i1 = tap(x0 + 1, y0); vsw, i2 = tap(x0, y0 + 1); vse, i3 = tap(x0 + 1, y0 + 1)
        out = fma32(vse, se, fma32(vsw, sw, fma32(vne, ne, vnw * nw)))
    sample_np.last_outside = ~(i0 & i1 & i2 & i3)          # (for the fixtures' own assertions)
    return out


def frame_counts_np(masks_u8, frame_ids, xy, labels, table=None):
    """(n_frames, 4) int64 [tp, fp, fn, tn] per frame over the points whose frame id is that frame; other frame ids are ignored."""
    masks_u8 = np.asarray(masks_u8, np.uint8)
    T = masks_u8.shape[0]
    table = mask_table() if table is None else table
    frame_ids = np.asarray(frame_ids, np.int64).reshape(-1)
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    pred = np.asarray(labels).reshape(-1) != 0
    out = np.zeros((T, 4), np.int64)
    for f in range(T):
        sel = np.flatnonzero(frame_ids == f)
        if len(sel) == 0:
            continue
        gt = sample_np(masks_u8[f], table, xy[sel]) > F(0.5)
        p = pred[sel]
        out[f] = [(p & gt).sum(), (p & ~gt).sum(), (~p & gt).sum(), (~p & ~gt).sum()]
    return out


def vote_np(xy, mask_absent, gts_u8):
    """find_traj_label: xy (K,L,2) f64, mask_absent (K,L) or (K,L,1) (nonzero = padded), gts (L,H,W) u8 -> (labels (K,) u8, bad) where
    bad says that a present point was outside the map or not finite (never read; the labels are then unspecified)."""
    xy = np.asarray(xy, np.float64)
    K, L = xy.shape[:2]
    gts_u8 = np.asarray(gts_u8, np.uint8)
    H, W = gts_u8.shape[1:]
    present = ~(np.asarray(mask_absent, np.float64).reshape(K, L) != 0)
    with np.errstate(all="ignore"):
        rx, ry = np.rint(xy[:, :, 0]), np.rint(xy[:, :, 1])          # half to even, like round() on a numpy.float64
        ok = present & (rx >= 0) & (rx < W) & (ry >= 0) & (ry < H)
    bad = bool((present & ~ok).any())
    ix = np.where(ok, rx, 0).astype(np.int64)
    iy = np.where(ok, ry, 0).astype(np.int64)
    v = gts_u8[np.arange(L)[None, :], iy, ix].astype(np.int64)        # an integer sum that cannot wrap
    label_num = np.where(ok, v, 0).sum(1)
    total_num = ok.sum(1)
    return (label_num > total_num // 2).astype(np.uint8), bad


def seeded_eval_inputs(n, T, hw, seed, margin=2.0):
    """n points over T frames of (h,w) masks with blobs and in-between values; coordinates reach `margin` px outside the image."""
    rng = np.random.default_rng(seed)
    h, w = hw
    masks = rng.integers(0, 256, size=(T, h, w)).astype(np.uint8)
    masks[rng.uniform(size=(T, h, w)) < 0.3] = 0
    masks[rng.uniform(size=(T, h, w)) < 0.3] = 255
    frame_ids = rng.integers(0, T, size=n).astype(np.int32)
    xy = np.stack([rng.uniform(-margin, w - 1 + margin, size=n), rng.uniform(-margin, h - 1 + margin, size=n)], 1)
    labels = (rng.uniform(size=n) < 0.5).astype(np.uint8)
    return masks, frame_ids, xy, labels


def seeded_vote_inputs(K, L, hw, seed, maxval=1):
    rng = np.random.default_rng(seed)
    h, w = hw
    gts = (rng.integers(0, 2, size=(L, h, w)) * maxval).astype(np.uint8)
    xy = np.stack([rng.uniform(-0.49, w - 0.51, size=(K, L)), rng.uniform(-0.49, h - 0.51, size=(K, L))], -1)
    half = rng.uniform(size=(K, L)) < 0.2                               # some coordinates on exact halves, inside the map
    xy[half, 0] = np.clip(np.floor(xy[half, 0]) + 0.5, 0.5, w - 1.5)
    mask = (rng.uniform(size=(K, L)) < 0.3).astype(np.float64)
    xy[mask != 0] = 0.0
    return xy, mask, gts


def eval_fixture(name):
    """An evaluation fixture as a dict; the labelled set of the two real cases is the one stored in the labels_* fixture it names."""
    from _common import golden
    g = golden(name)
    out = {k: g[k] for k in g.files}
    if "source" in g.files:
        src = golden(str(g["source"]))
        for k in ("ids", "off", "frame_ids", "xy", "labels"):
            out[k] = src[k]
    return out
