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


def set_labelled(ctx, trajectories_dict):
    """A labelled set from elsewhere -- the dict a labelled track.npy holds, {id: {"frame_ids", "locations", "labels"}} -- becomes the
    context's labelled set (psfm_labels_set), flattened in the dict's order: the order sfm/matches_from_flow.py:67 iterates in.  A
    trajectory's frames may have gaps.  match_tables_labelled_device, database_tables_device and ground_truth.frame_counts_device then
    run on it as on LabelMerger.finish()'s.  Returns (n_traj, n_points)."""
    from point_trajectory import _hip
    keys = list(trajectories_dict)
    cnt = [len(trajectories_dict[k]["frame_ids"]) for k in keys]
    off = np.zeros(len(keys) + 1, np.int64)
    np.cumsum(cnt, out=off[1:])
    cat = lambda name, dt, shape: (np.concatenate([np.asarray(trajectories_dict[k][name]).reshape(shape).astype(dt) for k in keys])
                                   if keys else np.zeros((0,) + shape[1:], dt))
    ids = np.ascontiguousarray(np.asarray(keys, np.int64).astype(np.int32))
    frames = np.ascontiguousarray(cat("frame_ids", np.int32, (-1,)))
    xy = np.ascontiguousarray(cat("locations", np.float64, (-1, 2)))
    labels = np.ascontiguousarray(cat("labels", bool, (-1,)).astype(np.uint8))
    if len(xy) != int(off[-1]) or len(labels) != int(off[-1]):
        raise ValueError("set_labelled: frame_ids, locations and labels of a trajectory must have one entry per point")
    vp = lambda a: ctypes.c_void_p(a.ctypes.data if a.size else 0)
    _hip.check(_hip.lib().psfm_labels_set(ctx.handle, len(keys), int(off[-1]), vp(ids), vp(off), vp(frames), vp(xy), vp(labels),
                                          _hip.current_stream_ptr(ctx.device)))
    return len(keys), int(off[-1])


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


# Rows (trajectories over all windows) that one decode group may hold: psfm_traj_decode_batch needs its windows' workspaces at the
# same time, 2.6 KB per row, so 2^18 rows bound the workspace at about 0.7 GB -- two and a half windows at the shipped cap of 100 000
# trajectories, tens of windows of a DAVIS-sized sequence.  A window above the cap forms a group of its own.
DEFAULT_MAX_ROWS = 1 << 18


def _sample_and_encode(ctx, length, window, raw_hw, input_size, traj_max_num, enc_weights, depth_of, seed, traj_min_len, kinv):
    """Phase 1 for one context: the saved set, the merger, and per window (frame0, n_frames, ids, encoding (1,16,K), mask_absent)."""
    from point_trajectory import _hip
    from .augment import augment_traj_device
    from .encoder import encode_traj_device
    from .load_cut_seq import sample_window_device, window_ranges
    k, n = ctypes.c_int64(0), ctypes.c_int64(0)
    _hip.check(_hip.lib().psfm_result_filter(ctx.handle, int(traj_min_len), ctypes.byref(k), ctypes.byref(n), _hip.current_stream_ptr(ctx.device)))
    merger = LabelMerger(ctx)
    windows = []
    for w, (f0, nf) in enumerate(window_ranges(length, window)):
        ids, raw, nor, mask = sample_window_device(ctx, f0, nf, raw_hw, input_size, traj_max_num, 3, traj_min_len, seed + w)
        feat = augment_traj_device(nor, mask, depth_of(np.arange(f0, f0 + nf)), input_size, kinv=kinv, ctx=ctx)
        windows.append((f0, nf, ids, encode_traj_device(feat, mask, enc_weights, ctx=ctx), mask))
    return merger, windows


def _sample_and_encode_batch(ctxs, lengths, window, raw_hw, input_size, traj_max_num, enc_weights, depth_ofs, seed, traj_min_len, kinv):
    """Phase 1 of front="batch" for several contexts on one device: what _sample_and_encode returns per context, with ONE sampler
    pass per context (load_cut_seq.sample_windows_device: one host synchronisation per 64 windows) and ONE augment and ONE encoder
    launch per 64 windows of ALL contexts (augment.augment_windows_device, encoder.encode_windows_device).  Same saved sets, same
    windows, same seeds, the depth maps asked for in the same order, the same bits."""
    from point_trajectory import _hip
    from .augment import augment_windows_device
    from .encoder import encode_windows_device
    from .load_cut_seq import sample_windows_device, window_ranges
    mergers, per_ctx, flat = [], [], []
    for ctx, length, depth_of in zip(ctxs, lengths, depth_ofs):
        k, n = ctypes.c_int64(0), ctypes.c_int64(0)
        _hip.check(_hip.lib().psfm_result_filter(ctx.handle, int(traj_min_len), ctypes.byref(k), ctypes.byref(n), _hip.current_stream_ptr(ctx.device)))
        mergers.append(LabelMerger(ctx))
        ranges = window_ranges(length, window)
        sampled = sample_windows_device(ctx, ranges, raw_hw, input_size, traj_max_num, 3, traj_min_len, [seed + w for w in range(len(ranges))])
        windows = [[f0, nf, ids, None, mask] for (f0, nf), (ids, raw, nor, mask) in zip(ranges, sampled)]
        flat += [(win, nor, depth_of(np.arange(f0, f0 + nf))) for win, (f0, nf), (_, _, nor, _) in zip(windows, ranges, sampled)]
        per_ctx.append(windows)
    lo = 0
    while lo < len(flat):           # (a sequence shorter than the window has windows of its own length: runs of one n_frames)
        hi = lo
        while hi < len(flat) and flat[hi][0][1] == flat[lo][0][1]:
            hi += 1
        run = flat[lo:hi]
        feats = augment_windows_device([r[1] for r in run], [r[0][4] for r in run], [r[2] for r in run], input_size, kinv=kinv, ctx=ctxs[0])
        for r, enc in zip(run, encode_windows_device(feats, [r[0][4] for r in run], enc_weights, ctx=ctxs[0])):
            r[0][3] = enc
        lo = hi
    return mergers, [[tuple(win) for win in windows] for windows in per_ctx]


def _check_front(front):
    if front not in ("window", "batch"):
        raise ValueError("front must be \"window\" or \"batch\", got %r" % (front,))


def decode_groups(rows, max_rows=None):
    """Consecutive windows with `rows` trajectories each -> [(first, last + 1), ...]: a group closes before the window that would take
    it above max_rows (default DEFAULT_MAX_ROWS); a window larger than that stands alone."""
    cap = DEFAULT_MAX_ROWS if max_rows is None else int(max_rows)
    groups, lo, total = [], 0, 0
    for i, r in enumerate(rows):
        if i > lo and total + int(r) > cap:
            groups.append((lo, i))
            lo, total = i, 0
        total += int(r)
    if len(rows) > lo:
        groups.append((lo, len(rows)))
    return groups


def _decode_and_merge(mergers, windows_per_ctx, dec_weights, ctx, max_rows):
    """Phases 2 and 3: every window of every context through decode_windows_device in groups of consecutive windows, then add_window
    per context in window order and finish."""
    from .decoder import decode_windows_device
    flat = [w for windows in windows_per_ctx for w in windows]
    preds = []
    for lo, hi in decode_groups([int(w[2].numel()) for w in flat], max_rows):
        preds += [p[2] for p in decode_windows_device([w[3] for w in flat[lo:hi]], dec_weights, ctx=ctx)]
    at = 0
    for merger, windows in zip(mergers, windows_per_ctx):
        merger.window_ids = []
        for (f0, nf, ids, _, _), pred in zip(windows, preds[at:at + len(windows)]):
            merger.add_window(f0, nf, ids, pred)
            merger.window_ids.append(ids)
        at += len(windows)
        merger.finish()


def label_trajectories_batched(length, window, raw_hw, input_size, traj_max_num, enc_weights, dec_weights, depth_for_window, seed=0,
                               traj_min_len=3, kinv=None, ctx=None, max_rows=None, front="window"):
    """label_trajectories(..., predict=decoder.device_predictor(enc_weights, dec_weights, depth_for_window, input_size, kinv, ctx))
    with the decoder run once per GROUP of windows instead of once per window: the same saved set, the same windows
    (load_cut_seq.window_ranges), the same seeds (seed + w), the same merger, the same bytes out of finish().
      1. per window: sample_window_device, augment_traj_device (depth_for_window(time_idx) as device_predictor calls it),
         encode_traj_device; the ids, the encoding and the mask are kept;
      2. decoder.decode_windows_device over groups of consecutive windows (decode_groups: at most max_rows trajectories per group,
         default DEFAULT_MAX_ROWS, so that the group's workspace, 2.6 KB per row, stays bounded).  A window's result is that of
         psfm_traj_decode on the window alone, so the grouping changes no bit;
      3. LabelMerger.add_window in window order, then finish().
    front="batch" runs step 1 for all windows at once -- load_cut_seq.sample_windows_device, augment.augment_windows_device,
    encoder.encode_windows_device: one sampler pass with one host synchronisation, one augment and one encoder launch per 64
    windows -- with the same bytes out of finish(); the default "window" is the per-window loop.
    Returns the merger, finished, with `window_ids`."""
    from point_trajectory import _hip
    _check_front(front)
    ctx = ctx or _hip.context()
    if front == "batch":
        (merger,), (windows,) = _sample_and_encode_batch([ctx], [length], window, raw_hw, input_size, traj_max_num, enc_weights,
                                                         [depth_for_window], seed, traj_min_len, kinv)
    else:
        merger, windows = _sample_and_encode(ctx, length, window, raw_hw, input_size, traj_max_num, enc_weights, depth_for_window, seed,
                                             traj_min_len, kinv)
    _decode_and_merge([merger], [windows], dec_weights, ctx, max_rows)
    return merger


def label_sequences_batched(ctxs, lengths, window, raw_hw, input_size, traj_max_num, enc_weights, dec_weights, depth_for_window, seed=0,
                            traj_min_len=3, kinv=None, max_rows=None, front="window"):
    """label_trajectories_batched for several contexts on one device -- what trajectory.run_connect_batch returns -- with the windows
    of ALL sequences going through the same decode groups: sequence after sequence, window after window.  lengths[i]: frames of
    sequence i; depth_for_window(seq_index, time_idx).  Sampling, augment and encode (phase 1) and the merge (phase 3) stay per context;
    every context's labelled set equals what label_trajectories_batched gives for it alone.  front="batch": the sampler runs one
    pass per context (every context has its own result), augment and encoder run over the windows of ALL contexts in one launch each
    per 64 windows; the same bytes.  Returns the finished mergers."""
    _check_front(front)
    ctxs = list(ctxs)
    if len(ctxs) != len(lengths):
        raise ValueError("label_sequences_batched: %d contexts, %d lengths" % (len(ctxs), len(lengths)))
    if any(c.device != ctxs[0].device for c in ctxs):
        raise ValueError("label_sequences_batched: the contexts must be on one device")
    mergers, per_ctx = [], []
    if front == "batch" and ctxs:
        mergers, per_ctx = _sample_and_encode_batch(ctxs, [int(n) for n in lengths], window, raw_hw, input_size, traj_max_num, enc_weights,
                                                    [lambda t, i=i: depth_for_window(i, t) for i in range(len(ctxs))], seed, traj_min_len, kinv)
    for i, (ctx, length) in enumerate(zip(ctxs, lengths) if front == "window" else []):
        merger, windows = _sample_and_encode(ctx, int(length), window, raw_hw, input_size, traj_max_num, enc_weights,
                                             lambda t, i=i: depth_for_window(i, t), seed, traj_min_len, kinv)
        mergers.append(merger)
        per_ctx.append(windows)
    if ctxs:
        _decode_and_merge(mergers, per_ctx, dec_weights, ctxs[0], max_rows)
    return mergers


def label_track_npy(traj_dir, output_traj_dir, length, raw_hw, input_size, enc_weights, dec_weights, depth_for_window, window=10,
                    traj_max_num=100000, seed=0, front="window"):
    """Stage 2 from file to file (motion_seg/main_motion_segmentation.py with the trajectories of traj_dir/track.npy): the file goes
    into a context (point_trajectory.trajectory.load_track_npy_device), label_trajectories_batched runs on that context with
    traj_min_len = 1 -- the file IS the saved set -- and the labelled dict is saved as output_traj_dir/track.npy, the file
    sfm/matches_from_flow.py reads.  Depth maps stay the caller's (depth_for_window(time_idx), as everywhere else).  Returns the
    finished merger (its labelled set stays in its context).  The file is loaded into the calling thread's context
    (load_track_npy_device with ctx=None): whatever result a tracker left there is replaced."""
    import os
    from point_trajectory.trajectory import load_track_npy_device
    ctx, kind, _ = load_track_npy_device(os.path.join(traj_dir, "track.npy"))
    if kind != "set":
        raise ValueError("label_track_npy: %s holds a labelled dict, not a TrajectorySet" % os.path.join(traj_dir, "track.npy"))
    merger = label_trajectories_batched(length, window, raw_hw, input_size, traj_max_num, enc_weights, dec_weights, depth_for_window,
                                        seed=seed, traj_min_len=1, ctx=ctx, front=front)
    os.makedirs(output_traj_dir, exist_ok=True)
    np.save(os.path.join(output_traj_dir, "track.npy"), merger.as_dict())
    return merger
