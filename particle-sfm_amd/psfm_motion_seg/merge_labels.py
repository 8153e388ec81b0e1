"""Per-window motion labels -> the labelled trajectory set: motion_seg/main_motion_segmentation.py:89-129 of the reference.

The reference merges the network's per-window predictions in a Python dict loop (:92-112) and saves the dict (:122-129) as the
track.npy that sfm/matches_from_flow.py reads.  What that loop produces:
  * a trajectory enters with the first window row that names it (:100-103); the dict lists the trajectories in that order of first
    appearance (window, then row) -- not by ascending id -- and traj_to_matches assigns keypoint indices in that order;
  * a point carries the prediction of the FIRST window that covered it; a later, overlapping window only adds the frames the
    trajectory does not hold yet (:105-112), so one trajectory can carry both labels;
  * only points inside windows where the trajectory was sampled enter: a trajectory left out of a middle window (traj_max_num) has
    a gap in its frames, one with fewer than 3 observations in every window never enters.
So the labelled set is NOT the saved set with a label array on top; it carries explicit per-point frames.

Three forms of the same model over the saved set (ascending ids, frames birth .. birth + length - 1):
  merge_labels_host    the NumPy statement: state per saved point (255 = not labelled), first-seen sequence number per trajectory
  LabelMerger          the device path (csrc/psfm_labels.hip): one asynchronous launch per window behind the network's output,
                       then one finish; everything stays in HBM and feeds psfm_sfm.matches_from_flow.*_labelled_device
  label_trajectories   the loop of main_motion_segmentation.py:69-112 without the video: window tensors -> predict -> merge
Rows whose trajectory has no point inside the window are ignored (the reference would file an empty entry, which changes no match;
the window sampler never emits one).  Ids must be unique within a window (the sampler guarantees it).
"""
import ctypes

import numpy as np

UNSET = 0xFFFFFFFF
NONE = 255


def merge_labels_host(ids, birth, length, off, xy, windows):
    """The saved set (ids (k,) ascending, birth (k,), length (k,), off (k+1,), xy (n,2)) and `windows`, a list of
    (frame0, n_frames, ids (K,), pred (K,)) in call order -> the labelled set as a CSR in order of first appearance:
    (ids (m,) i32, off (m+1,) i64, frame_ids (p,) i32, xy (p,2) f64, labels (p,) u8).  An id outside the saved set: ValueError."""
    ids = np.asarray(ids, np.int64)
    birth = np.asarray(birth, np.int64)
    length = np.asarray(length, np.int64)
    off = np.asarray(off, np.int64)
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    k = len(ids)
    state = np.full(int(off[-1]) if k else 0, NONE, np.uint8)
    first = np.full(k, UNSET, np.int64)
    rows_before = 0
    for frame0, n_frames, wids, pred in windows:
        wids = np.asarray(wids, np.int64).reshape(-1)
        pred = (np.asarray(pred).reshape(-1) != 0).astype(np.uint8)
        if len(wids) != len(pred):
            raise ValueError("merge_labels_host: %d ids, %d predictions" % (len(wids), len(pred)))
        r = np.searchsorted(ids, wids)
        if len(wids) and (k == 0 or np.any(ids[np.minimum(r, k - 1)] != wids)):
            raise ValueError("merge_labels_host: a window names a trajectory id that is not in the saved set")
        lo = np.maximum(birth[r], int(frame0))
        hi = np.minimum(birth[r] + length[r], int(frame0) + int(n_frames))
        cnt = np.maximum(hi - lo, 0)
        row = np.repeat(np.arange(len(wids)), cnt)
        j = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        p = (off[r] + lo - birth[r])[row] + j                    # the rows' points inside the window
        new = state[p] == NONE                                   # the first window that covers a point decides (:105-112)
        state[p[new]] = pred[row[new]]
        fresh = np.flatnonzero((cnt > 0) & (first[r] == UNSET))
        first[r[fresh]] = rows_before + fresh                    # (:100-103) the row that brought the trajectory in
        rows_before += len(wids)
    seen = np.flatnonzero(first != UNSET)
    order = seen[np.argsort(first[seen], kind="stable")]
    run = np.concatenate([[0], np.cumsum(state != NONE)])
    cnt_t = (run[off[1:]] - run[off[:-1]])[order] if k else np.zeros(0, np.int64)
    out_off = np.zeros(len(order) + 1, np.int64)
    np.cumsum(cnt_t, out=out_off[1:])
    n_all = length[order]
    owner = np.repeat(np.arange(len(order)), n_all)
    j = np.arange(int(n_all.sum())) - np.repeat(np.cumsum(n_all) - n_all, n_all)
    p = off[order][owner] + j                                    # every point of the labelled trajectories, in time order
    have = state[p] != NONE
    p, owner, j = p[have], owner[have], j[have]
    frame_ids = (birth[order][owner] + j).astype(np.int32)
    return ids[order].astype(np.int32), out_off, frame_ids, xy[p], state[p]


def labelled_as_dict(ids, off, frame_ids, xy, labels):
    """The plain dict main_motion_segmentation.py:122-129 saves as track.npy: keys in the set's order, per trajectory `locations`
    (n,2) f64, `labels` (n,) bool, `frame_ids` (n,) i64."""
    ids, off = np.asarray(ids), np.asarray(off, np.int64)
    frame_ids, labels = np.asarray(frame_ids, np.int64), np.asarray(labels).astype(bool)
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    return {int(ids[i]): {"locations": xy[off[i]:off[i + 1]], "labels": labels[off[i]:off[i + 1]], "frame_ids": frame_ids[off[i]:off[i + 1]]}
            for i in range(len(ids))}


class LabelMerger:
    """The device path.  Construction runs psfm_labels_begin on the saved set that psfm_result_filter left in `ctx` (a later
    psfm_result_filter / psfm_track / psfm_connect on the context voids the merger: add_window and finish then raise PsfmError)."""

    def __init__(self, ctx=None):
        from point_trajectory import _hip
        self._hip = _hip
        self.ctx = ctx or _hip.context()
        self.n_windows = 0
        self.n_traj = self.n_points = None
        _hip.check(_hip.lib().psfm_labels_begin(self.ctx.handle, _hip.current_stream_ptr(self.ctx.device)))

    def add_window(self, frame0, n_frames, ids, pred):
        """ids (K,) int32 device tensor (unique; what sample_window_device returned), pred (K,) bool / uint8 device tensor, nonzero =
        dynamic.  Asynchronous: one launch on the current stream, behind whatever produced `pred`."""
        import torch
        _hip = self._hip
        ids = ids.reshape(-1)
        if ids.dtype != torch.int32 or not ids.is_contiguous():
            ids = ids.to(torch.int32).contiguous()
        pred = pred.reshape(-1)
        if pred.dtype != torch.uint8 or not pred.is_contiguous():
            pred = (pred != 0).to(torch.uint8).contiguous()
        if not (ids.is_cuda and pred.is_cuda) or ids.numel() != pred.numel():
            raise ValueError("LabelMerger.add_window: ids and pred must be device tensors of one length")
        _hip.check(_hip.lib().psfm_labels_merge_window(self.ctx.handle, int(frame0), int(n_frames), _hip.ptr(ids), _hip.ptr(pred),
                                                       int(ids.numel()), _hip.current_stream_ptr(self.ctx.device)))
        self.n_windows += 1
        self.n_traj = self.n_points = None

    def finish(self):
        """psfm_labels_finish: the labelled set stays in the context (match_tables_labelled_device reads it there); returned as
        device tensors (ids (m,) i32, off (m+1,) i64, frame_ids (p,) i32, xy (p,2) f64, labels (p,) u8)."""
        import torch
        _hip = self._hip
        L, sp = _hip.lib(), _hip.current_stream_ptr(self.ctx.device)
        m, p = ctypes.c_int64(0), ctypes.c_int64(0)
        _hip.check(L.psfm_labels_finish(self.ctx.handle, ctypes.byref(m), ctypes.byref(p), sp))
        self.n_traj, self.n_points = int(m.value), int(p.value)
        dev = torch.device("cuda", self.ctx.device)
        ids = torch.empty((self.n_traj,), dtype=torch.int32, device=dev)
        off = torch.zeros((self.n_traj + 1,), dtype=torch.int64, device=dev)
        frame_ids = torch.empty((self.n_points,), dtype=torch.int32, device=dev)
        xy = torch.empty((self.n_points, 2), dtype=torch.float64, device=dev)
        labels = torch.empty((self.n_points,), dtype=torch.uint8, device=dev)
        _hip.check(L.psfm_labels_copy(self.ctx.handle, _hip.ptr(ids), _hip.ptr(off), _hip.ptr(frame_ids), _hip.ptr(xy), _hip.ptr(labels), sp))
        return ids, off, frame_ids, xy, labels

    def as_dict(self):
        """finish() -> the dict the reference saves (np.save(path, merger.as_dict()) is a labelled track.npy)."""
        return labelled_as_dict(*[t.cpu().numpy() for t in self.finish()])


def label_trajectories(length, window, raw_hw, input_size, traj_max_num, predict, seed=0, traj_min_len=3, ctx=None):
    """main_motion_segmentation.py:69-112 for the trajectories of the result the last psfm_track / psfm_connect left in `ctx`: the
    saved set (psfm_result_filter(traj_min_len)), then per window of load_cut_seq.window_ranges the window tensors
    (sample_window_device) -> predict(raw (K,L,2), normalised (K,L,2), mask_absent (K,L,1), time_idx (L,)) -> a (K,) bool device
    tensor, True = dynamic -> LabelMerger.add_window.  Returns the merger, finished (its set is in the context); `merger.window_ids`
    lists the sampled ids per window."""
    from point_trajectory import _hip
    from .load_cut_seq import sample_window_device, window_ranges
    ctx = ctx or _hip.context()
    k, n = ctypes.c_int64(0), ctypes.c_int64(0)
    _hip.check(_hip.lib().psfm_result_filter(ctx.handle, int(traj_min_len), ctypes.byref(k), ctypes.byref(n), _hip.current_stream_ptr(ctx.device)))
    merger = LabelMerger(ctx)
    merger.window_ids = []
    for w, (f0, nf) in enumerate(window_ranges(length, window)):
        ids, raw, nor, mask = sample_window_device(ctx, f0, nf, raw_hw, input_size, traj_max_num, 3, traj_min_len, seed + w)
        pred = predict(raw, nor, mask, np.arange(f0, f0 + nf))
        merger.add_window(f0, nf, ids, pred)
        merger.window_ids.append(ids)
    merger.finish()
    return merger
