"""Trajectories against ground-truth masks on the device (csrc/psfm_ground_truth.hip): how good the labels are, and which labels
to train on.

Scoring -- motion_seg/eval_traj_iou.py of the reference.  Its per_img_traj_metrics (:79-115) regroups every labelled point by frame
in a Python loop, bilinearly samples the frame's ground-truth mask at the frame's points (grid_sample, :53-65) and reports IoU,
precision, recall and F1 per frame (seg_metrics, :67-76).  All four are functions of the per-frame counts tp, fp, fn, tn, so the
device leaves those -- integers, one launch over the labelled set that psfm_labels_finish left in HBM, no track.npy -- and the
metrics are a few f64 operations per frame on the host.  The masks stay u8 (the PNG's channel); the reference's 1.0 - png / 255.0 is
a 256-entry fp32 table.

Supervision -- find_traj_label of scripts/prepare_flyingthings3d.py (:89-108): a trajectory's training label by majority vote of
the ground-truth mask at the rounded pixel of each of its points, from the window tensors sample_window_device returns.

There is no CPU fallback: without a HIP device the *_device functions raise RuntimeError.
"""
import numpy as np

CLASSES = 4      # tp, fp, fn, tn


def mask_table():
    """The reference's mask value per PNG byte: 1.0 - b / 255.0 in f64 (eval_traj_iou.py:49), cast to fp32 (:107).  (256,) float32.
    A caller whose masks hold 0 / 1 passes np.arange(256) != 0 instead."""
    return np.float32(1.0 - np.arange(256) / 255.0)


def _device_u8_stack(maps, dev, what):
    """A list of (H,W) u8 arrays / tensors or an (n,H,W) array / tensor -> (n,H,W) u8, contiguous, on `dev`."""
    import torch
    if isinstance(maps, (list, tuple)):
        maps = torch.stack([torch.as_tensor(np.ascontiguousarray(m) if not torch.is_tensor(m) else m) for m in maps], 0)
    elif not torch.is_tensor(maps):
        maps = torch.as_tensor(np.ascontiguousarray(maps))
    if maps.dim() != 3 or maps.dtype != torch.uint8:
        raise ValueError("%s: the maps must be (n,H,W) uint8, got %s %s" % (what, tuple(maps.shape), maps.dtype))
    return maps.to(dev).contiguous()


def frame_counts_device(masks_u8, frame_ids=None, xy=None, labels=None, table=None, ctx=None):
    """Per-frame tp, fp, fn, tn of labelled trajectory points against masks_u8 (n_frames,H,W) u8: an (n_frames, 4) int64 device
    tensor.  frame_ids (n,) / xy (n,2) / labels (n,) as LabelMerger.finish() returns them; all three None = the labelled set in the
    context.  A point is a positive when labels != 0, its ground truth is positive when the bilinear sample of table[mask] (zeros
    outside the image) is > 0.5 in fp32; a point whose frame id is outside [0, n_frames) is ignored.  table: (256,) fp32, default
    mask_table().  Asynchronous: a memset and one launch on the current stream."""
    import torch
    from point_trajectory import _hip
    ctx = ctx or _hip.context()                       # (no device: RuntimeError)
    dev = torch.device("cuda", ctx.device)
    masks = _device_u8_stack(masks_u8, dev, "frame_counts_device")
    T, H, W = (int(v) for v in masks.shape)
    table = np.ascontiguousarray(mask_table() if table is None else np.asarray(table, np.float32).reshape(256))
    given = [a is not None for a in (frame_ids, xy, labels)]
    if any(given) and not all(given):
        raise ValueError("frame_counts_device: frame_ids, xy and labels go together (or all None: the context's labelled set)")
    n = 0
    if all(given):
        frame_ids = torch.as_tensor(frame_ids).reshape(-1).to(dev).to(torch.int32).contiguous()
        n = int(frame_ids.numel())
        xy = torch.as_tensor(xy).to(dev).double().reshape(-1, 2).contiguous()
        labels = torch.as_tensor(labels).reshape(-1).to(dev)
        labels = (labels if labels.dtype == torch.uint8 else (labels != 0).to(torch.uint8)).contiguous()
        if xy.shape[0] != n or labels.numel() != n:
            raise ValueError("frame_counts_device: %d frame ids, %d points, %d labels" % (n, xy.shape[0], labels.numel()))
        if n == 0:          # (an empty tensor has no address; the ABI reads three NULLs as "the context's set")
            frame_ids, xy, labels = (torch.zeros((2,), dtype=t.dtype, device=dev) for t in (frame_ids, xy, labels))
    counts = torch.empty((T, CLASSES), dtype=torch.int64, device=dev)
    _hip.check(_hip.lib().psfm_traj_eval_counts(ctx.handle, _hip.ptr(frame_ids), _hip.ptr(xy), _hip.ptr(labels), n, _hip.ptr(masks),
                                                table.ctypes.data, T, H, W, _hip.ptr(counts), _hip.current_stream_ptr(ctx.device)))
    return counts


def frame_counts_file_device(track_npy, masks_u8, table=None, ctx=None):
    """frame_counts_device for a labelled track.npy (the dict stage 2 writes): merge_labels.set_labelled, then the counts.  ctx=None: the
    calling thread's context, whose labelled set is replaced."""
    from point_trajectory import _hip
    from .merge_labels import set_labelled
    ctx = ctx or _hip.context()
    set_labelled(ctx, np.load(track_npy, allow_pickle=True).item())
    return frame_counts_device(masks_u8, table=table, ctx=ctx)


def seg_metrics_from_counts(counts):
    """(n,4) counts [tp, fp, fn, tn] -> (n,4) f64 [iou, precision, recall, f1] as seg_metrics (eval_traj_iou.py:67-76) reports them:
    iou = tp / ((tp + fp + fn) + 1e-6) (:71-73); precision, recall and F1 the binary ones of
    sklearn.metrics.precision_recall_fscore_support with zero_division=0 (a zero denominator gives 0)."""
    c = np.asarray(counts, np.int64).reshape(-1, CLASSES)
    tp, fp, fn = c[:, 0].astype(np.float64), c[:, 1].astype(np.float64), c[:, 2].astype(np.float64)

    def ratio(num, den):
        return np.divide(num, den, out=np.zeros_like(num), where=den != 0)
    iou = tp / ((tp + fp + fn) + 1e-6)
    return np.stack([iou, ratio(tp, tp + fp), ratio(tp, tp + fn), ratio(2.0 * tp, 2.0 * tp + fp + fn)], 1)


def per_img_traj_metrics_device(gt_pngs, merger_or_arrays=None, ctx=None):
    """per_img_traj_metrics (eval_traj_iou.py:79-115).  gt_pngs: the list of u8 (H,W) arrays that cv2.imread(name)[:,:,0] yields for
    the ground-truth PNGs (load_masks, :45-51, without the 1.0 - x / 255.0).  merger_or_arrays: a finished LabelMerger, a tuple
    (frame_ids, xy, labels) or the five arrays LabelMerger.finish() returns, or None = the labelled set in the context.
    Frames 0 .. len-2 are scored (:97); a frame whose mask sums to less than 10 is skipped (:100, the reference's own expression on
    the host).  Returns the (n_kept, 4) f64 array [iou, precision, recall, f1] of the kept frames, or None when none is kept.
    Deviation: a kept frame without a single point is skipped too -- the reference raises KeyError there (:103)."""
    from point_trajectory import _hip
    arrays = merger_or_arrays
    if arrays is not None and hasattr(arrays, "finish"):
        ctx = ctx or arrays.ctx
        if arrays.n_points is None:
            arrays.finish()
        arrays = None                                  # the merger's set is the one in its context
    if arrays is not None:
        arrays = tuple(arrays)
        if len(arrays) == 5:
            arrays = arrays[2:]
        if len(arrays) != 3:
            raise ValueError("per_img_traj_metrics_device: expected (frame_ids, xy, labels) or the five arrays of LabelMerger.finish()")
    ctx = ctx or _hip.context()
    gt_pngs = [np.asarray(m) for m in gt_pngs]
    num = len(gt_pngs)
    candidates = [i for i in range(num - 1) if not np.sum(1.0 - gt_pngs[i] / 255.0) < 10]
    if not candidates:
        return None
    counts = frame_counts_device(gt_pngs, *(arrays or (None, None, None)), ctx=ctx).cpu().numpy()
    kept = [i for i in candidates if counts[i].sum() > 0]
    if not kept:
        return None
    return seg_metrics_from_counts(counts[kept])


def find_traj_label_device(raw_xy, mask_absent, gts_u8, ctx=None):
    """find_traj_label (prepare_flyingthings3d.py:89-108): raw_xy (K,L,2) and mask_absent (K,L,1) or (K,L) as sample_window_device
    returns them for a window that covers the sequence, gts_u8 (L,H,W) u8 (or a list of L maps) -> (K,) uint8 device tensor, 1 where
    the sum of the mask values at the rounded pixels (half to even) of the present points exceeds half their number (integer
    division).  Raises PsfmError when a present point lies outside the image or is not finite (the reference would wrap a negative
    index and raise on a large one).  Synchronises the current stream."""
    import torch
    from point_trajectory import _hip
    ctx = ctx or _hip.context()
    dev = torch.device("cuda", ctx.device)
    raw_xy, mask_absent = torch.as_tensor(raw_xy), torch.as_tensor(mask_absent)
    if raw_xy.dim() != 3 or raw_xy.shape[2] != 2:
        raise ValueError("find_traj_label_device: raw_xy must be (K,L,2), got %s" % (tuple(raw_xy.shape),))
    K, L = int(raw_xy.shape[0]), int(raw_xy.shape[1])
    if tuple(mask_absent.shape) not in ((K, L), (K, L, 1)):
        raise ValueError("find_traj_label_device: mask_absent must be (K,L) or (K,L,1), got %s" % (tuple(mask_absent.shape),))
    gts = _device_u8_stack(gts_u8, dev, "find_traj_label_device")
    if int(gts.shape[0]) != L:
        raise ValueError("find_traj_label_device: %d maps for %d columns" % (int(gts.shape[0]), L))
    xy = raw_xy.to(dev).double().contiguous()
    mask = mask_absent.to(dev).double().contiguous()
    out = torch.empty((K,), dtype=torch.uint8, device=dev)
    _hip.check(_hip.lib().psfm_traj_vote_labels(ctx.handle, _hip.ptr(xy), _hip.ptr(mask), _hip.ptr(gts), K, L, int(gts.shape[1]),
                                                int(gts.shape[2]), _hip.ptr(out), _hip.current_stream_ptr(ctx.device)))
    return out
