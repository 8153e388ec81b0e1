"""Trajectories -> per-image keypoints and sampled pair matches for the COLMAP database: the consumer
sfm/matches_from_flow.py:51-118 of the reference, as array work instead of its per-trajectory /
per-point Python loops (O(sum(len) * K) interpreter steps).

Two producers feed ONE assembler:
  * `traj_to_matches(img_dir, traj_dir, match_list_file, remove_dynamic=True)` -- the reference's signature; reads
    track.npy and does the index arithmetic in NumPy on the host;
  * `traj_to_matches_device(ctx, image_names, match_list_file)` -- the same tables computed by
    psfm_traj_to_matches (csrc/psfm_matches.hip) straight from the saved set that psfm_result_filter left in HBM; only
    the finished tables cross PCIe.
Both return what the reference returns: {image name: object with .keypoints and .match_pairs} in image order, and write
the pair list file.  Element for element equal to the reference's own function (tests/test_reference_consumers.py,
tests/golden/matches_*.npz).

What the reference computes, as tables:
  keypoints   image i lists the points observed in frame i in trajectory (id) order (:67-81); a point's keypoint index
              is its rank in that list
  matches     point j of a trajectory with n kept points pairs with every other point when n <= K = 20, otherwise with
              the K points at k * (n // K), itself skipped (:83-101); a match is filed under the ordered image pair
              (frame of j, frame of the target) as the row [keypoint index of j, keypoint index of the target], rows in
              the order the loops produce them (trajectory, j, k); the pairs of an image appear in order of first use.
"""
import os

import numpy as np

SAMPLE_K = 20     # sfm/matches_from_flow.py:52


class ImageMatches:
    """What sfm/import_feature_matches.py:76-104 reads per image: `.keypoints` ((n,2) coordinates) and `.match_pairs`
    ({"<image name>-<image name>": rows of [own keypoint index, other keypoint index]})."""
    __slots__ = ("image_id", "keypoints", "match_pairs")

    def __init__(self, image_id, keypoints=None):
        self.image_id = int(image_id)
        self.keypoints = [] if keypoints is None else keypoints
        self.match_pairs = {}


imageMatchData = ImageMatches   # the reference's name for this container (sfm/matches_from_flow.py:21)


def _flatten(trajectories):
    """TrajectorySet (CSR or map backed) or plain dict -> (off, frames, xy, labels) in iteration (id) order."""
    if hasattr(trajectories, "_to_csr"):
        ids, off, frames, xy, labels = trajectories._to_csr()
        if labels is None:
            labels = np.zeros(len(frames), bool)
        return off, frames, xy, labels
    cnt, fr, loc, lab = [], [], [], []
    for key in trajectories:                      # dict written by motion_seg (main_motion_segmentation.py:122-129)
        t = trajectories[key]
        f = np.asarray(t["frame_ids"], np.int64)
        cnt.append(len(f))
        fr.append(f)
        loc.append(np.asarray(t["locations"], np.float64).reshape(-1, 2))
        lab.append(np.asarray(t["labels"]).astype(bool))
    off = np.zeros(len(cnt) + 1, np.int64)
    np.cumsum(cnt, out=off[1:])
    cat = lambda a, shape, dt: np.concatenate(a) if a else np.zeros(shape, dt)
    return off, cat(fr, (0,), np.int64), cat(loc, (0, 2), np.float64), cat(lab, (0,), bool)


def match_tables_host(off, frames, xy, labels, n_img, remove_dynamic=True, sample_k=SAMPLE_K):
    """The tables of the module docstring from flat trajectory arrays (NumPy):
    kp_off (n_img+1), kp_xy (n_kept,2), pair_key (n_pairs) = src_image * n_img + tgt_image in ascending key order,
    pair_off (n_pairs+1), pair_first (n_pairs) = position of the pair's first match in the loop order, rows (n_matches,2)."""
    n_traj = len(off) - 1
    if len(frames) and (int(np.min(frames)) < 0 or int(np.max(frames)) >= n_img):
        # the reference indexes image_names[frame] (matches_from_flow.py:79) and raises; the device path returns PSFM_ERR_ARG
        raise IndexError("traj_to_matches: frame ids span [%d, %d], %d images" % (int(np.min(frames)), int(np.max(frames)), n_img))
    owner = np.repeat(np.arange(n_traj), np.diff(off))
    keep = ~labels if remove_dynamic else np.ones(len(frames), bool)     # :71-74
    frames, xy, owner = frames[keep], xy[keep], owner[keep]
    n_pts = len(frames)
    cnt = np.bincount(owner, minlength=n_traj).astype(np.int64)          # kept points per trajectory
    toff = np.zeros(n_traj + 1, np.int64)
    np.cumsum(cnt, out=toff[1:])

    # keypoint index = running count per image in trajectory order (:78-81): one stable sort by frame
    order = np.argsort(frames, kind="stable")
    fsorted = frames[order]
    kp_off = np.searchsorted(fsorted, np.arange(n_img + 1)).astype(np.int64)
    kp_ind = np.empty(n_pts, np.int64)
    kp_ind[order] = np.arange(n_pts) - kp_off[fsorted]
    kp_xy = xy[order]

    # matches (:83-101)
    n_of = cnt[owner]
    j_loc = np.arange(n_pts) - toff[owner]
    reps = np.where(n_of <= sample_k, n_of, sample_k)
    src = np.repeat(np.arange(n_pts), reps)
    r = np.arange(len(src)) - np.repeat(np.cumsum(reps) - reps, reps)     # 0..reps-1 inside each source point
    n_src = n_of[src]
    stride = np.where(n_src <= sample_k, 1, n_src // sample_k)
    tgt_loc = r * stride
    ok = tgt_loc != j_loc[src]
    src, tgt = src[ok], (toff[owner[src]] + tgt_loc)[ok]
    key = frames[src] * n_img + frames[tgt]
    po = np.argsort(key, kind="stable")             # inside a pair the loop order (trajectory, j, k) survives
    pk = key[po]
    rows = np.stack([kp_ind[src[po]], kp_ind[tgt[po]]], 1).astype(np.int32)
    bounds = np.flatnonzero(np.r_[True, pk[1:] != pk[:-1], True]) if len(pk) else np.zeros(1, np.int64)
    pair_key = pk[bounds[:-1]] if len(pk) else np.zeros(0, np.int64)
    pair_first = po[bounds[:-1]] if len(pk) else np.zeros(0, np.int64)
    return kp_off, kp_xy, pair_key.astype(np.int64), bounds.astype(np.int64), pair_first.astype(np.int64), rows


def assemble(image_names, tables, match_list_file, as_arrays=False):
    """Tables -> {image name: ImageMatches} (:103-108) + the pair list file (:110-117)."""
    kp_off, kp_xy, pair_key, pair_off, pair_first, rows = tables
    n_img = len(image_names)
    datas = [ImageMatches(i, kp_xy[kp_off[i]:kp_off[i + 1]] if as_arrays else kp_xy[kp_off[i]:kp_off[i + 1]].tolist())
             for i in range(n_img)]
    for g in np.argsort(pair_first, kind="stable"):       # dict order of the reference = order of first use
        si, ti = divmod(int(pair_key[g]), n_img)
        block = rows[pair_off[g]:pair_off[g + 1]]
        datas[si].match_pairs[image_names[si] + "-" + image_names[ti]] = block if as_arrays else block.tolist()
    out = {name: datas[i] for i, name in enumerate(image_names)}
    with open(match_list_file, "w") as fp:
        for data in out.values():
            for pair in data.match_pairs:
                a, b = pair.split("-")
                fp.write(a + " " + b + "\n")
    return out


def match_tables_file_device(track_npy, n_img, remove_dynamic=True, sample_k=SAMPLE_K, ctx=None):
    """The match tables of a track.npy on the device: the file into a context (load_track_npy_device), then -- a TrajectorySet file --
    psfm_result_filter(ctx, 1) and psfm_traj_to_matches (the reference iterates EVERY trajectory of the file and applies no length
    filter there), or -- a labelled dict -- psfm_labels_to_matches.  A TrajectorySet file that carries True labels (a result holds
    none) takes the host tables, so that remove_dynamic means what it means on the host route.  Returns (ctx, kind, tables).
    ctx=None: the calling thread's context, whose result or labelled set is replaced (load_track_npy_device)."""
    from point_trajectory.trajectory import load_track_npy, load_track_npy_device
    ctx, kind, sizes = load_track_npy_device(track_npy, ctx)
    if kind == "set" and sizes.get("true_labels"):
        off, frames, xy, labels = _flatten(load_track_npy(track_npy))
        return ctx, kind, match_tables_host(off, frames, xy, labels, n_img, remove_dynamic, sample_k)
    if kind == "set":
        return ctx, kind, match_tables_device(ctx, n_img, 1, sample_k)
    return ctx, kind, match_tables_labelled_device(ctx, n_img, remove_dynamic, sample_k)


def traj_to_matches(img_dir, traj_dir, match_list_file, remove_dynamic=True, sample_k=SAMPLE_K, as_arrays=False, device=False):
    """sfm/matches_from_flow.py:51-118, same arguments.  as_arrays=True keeps `.keypoints` / `.match_pairs[...]` as
    (n,2) ndarrays instead of nested lists -- the only consumer (sfm/import_feature_matches.py:82,96) wraps them in
    np.array() anyway, and building ~1e7 two-element lists is what dominates the list form.
    device=True: the file goes into a context and the tables come from the device kernels (match_tables_file_device); what is
    returned and written is the same (a TrajectorySet file that carries True labels takes the host tables: a result has none).  The
    file is loaded into the calling thread's context, whose result a tracker may have left there: it is replaced."""
    from point_trajectory.trajectory import load_track_npy
    if device:
        image_names = sorted(os.listdir(img_dir))
        _, _, tables = match_tables_file_device(os.path.join(traj_dir, "track.npy"), len(image_names), remove_dynamic, sample_k)
        return assemble(image_names, tables, match_list_file, as_arrays)
    trajectories = load_track_npy(os.path.join(traj_dir, "track.npy"))      # (either layout; this package's files at array speed)
    image_names = sorted(os.listdir(img_dir))
    off, frames, xy, labels = _flatten(trajectories)
    tables = match_tables_host(off, frames, xy, labels, len(image_names), remove_dynamic, sample_k)
    return assemble(image_names, tables, match_list_file, as_arrays)


def _copy_tables(ctx, n_img, n_kp, n_m, n_p):
    """psfm_matches_copy: the finished tables of the context, one copy."""
    import ctypes
    from point_trajectory import _hip
    L = _hip.lib()
    sp = _hip.current_stream_ptr(ctx.device)
    kp_off = np.zeros(n_img + 1, np.int64)
    kp_xy = np.empty((n_kp, 2), np.float64)
    pair_key = np.empty(n_p, np.int64)
    pair_off = np.zeros(n_p + 1, np.int64)
    pair_first = np.empty(n_p, np.int64)
    rows = np.empty((n_m, 2), np.int32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    _hip.check(L.psfm_matches_copy(ctx.handle, vp(kp_off), vp(kp_xy), vp(pair_key), vp(pair_off), vp(pair_first), vp(rows), sp))
    return kp_off, kp_xy, pair_key, pair_off, pair_first, rows


def match_tables_device(ctx, n_img, traj_min_len=3, sample_k=SAMPLE_K, labels=None):
    """The same tables from the result the last psfm_track / psfm_connect of `ctx` left in HBM: the saved set
    (length >= traj_min_len, psfm_result_filter) -> psfm_traj_to_matches -> one copy of the finished tables.
    labels: optional (n_points,) uint8 device tensor over the saved set's points (1 = dynamic, dropped).  This equals the
    reference only when EVERY saved point is labelled (--assume_static, or labels from elsewhere); the set motion segmentation
    produces drops and reorders trajectories -- use match_tables_labelled_device for it."""
    import ctypes
    from point_trajectory import _hip
    L = _hip.lib()
    sp = _hip.current_stream_ptr(ctx.device)
    k, npt = ctypes.c_int64(0), ctypes.c_int64(0)
    _hip.check(L.psfm_result_filter(ctx.handle, int(traj_min_len), ctypes.byref(k), ctypes.byref(npt), sp))
    n_kp, n_m, n_p = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    _hip.check(L.psfm_traj_to_matches(ctx.handle, int(n_img), int(sample_k), _hip.ptr(labels), ctypes.byref(n_kp),
                                      ctypes.byref(n_m), ctypes.byref(n_p), sp))
    return _copy_tables(ctx, n_img, int(n_kp.value), int(n_m.value), int(n_p.value))


def match_tables_labelled_device(ctx, n_img, remove_dynamic=True, sample_k=SAMPLE_K):
    """The tables over the labelled set that psfm_labels_finish (psfm_motion_seg.merge_labels.LabelMerger.finish) left in `ctx`:
    trajectories in the set's order of first appearance -- the dict order the reference iterates in (:67) --, frames from the set's
    frame_ids (gaps allowed), kept points = labels == 0 when remove_dynamic (:71-74), all points otherwise."""
    import ctypes
    from point_trajectory import _hip
    L = _hip.lib()
    n_kp, n_m, n_p = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    _hip.check(L.psfm_labels_to_matches(ctx.handle, int(n_img), int(sample_k), 1 if remove_dynamic else 0, ctypes.byref(n_kp),
                                        ctypes.byref(n_m), ctypes.byref(n_p), _hip.current_stream_ptr(ctx.device)))
    return _copy_tables(ctx, n_img, int(n_kp.value), int(n_m.value), int(n_p.value))


def traj_to_matches_device(ctx, image_names, match_list_file, traj_min_len=3, sample_k=SAMPLE_K, labels=None, as_arrays=True):
    """traj_to_matches without the track.npy round trip (e.g. --assume_static, where the trajectory stage feeds SfM
    directly, run_particlesfm.py:114): tables from HBM, assembled like the host path."""
    tables = match_tables_device(ctx, len(image_names), traj_min_len, sample_k, labels)
    return assemble(list(image_names), tables, match_list_file, as_arrays)


def traj_to_matches_labelled_device(ctx, image_names, match_list_file, remove_dynamic=True, sample_k=SAMPLE_K, as_arrays=True):
    """traj_to_matches over the labelled set in HBM (connect -> window tensors -> network -> LabelMerger -> here: no labelled
    track.npy round trip), assembled like the host path."""
    tables = match_tables_labelled_device(ctx, len(image_names), remove_dynamic, sample_k)
    return assemble(list(image_names), tables, match_list_file, as_arrays)


# ---- all sequences of a batch in one pass (csrc/psfm_matches_batch.hip) -------------------------------------------------------------
BATCH_MAX = 64          # sequences per call: PSFM_BATCH_MAX
# Points per batched call.  In the worst case every point emits sample_k = 20 matches of 40 bytes of scratch each: 2^25 points are
# 27 GB, under the 48 GiB BATCH_BYTES of point_trajectory/batch.py.  (The scratch itself is sized from the counted matches.)
MAX_POINTS = 1 << 25


def group_sequences(n_points, max_points=MAX_POINTS, max_seq=BATCH_MAX):
    """The grouping rule of the batched calls (psfm_mtb_group_end of csrc/psfm_matches_batch.h): the list is cut into consecutive
    groups of at most `max_seq` sequences and at most `max_points` points; a sequence above the cap is a group of its own and goes
    through the single entry points.  Returns [(start, end, alone)]."""
    out, i, n = [], 0, len(n_points)
    while i < n:
        if n_points[i] > max_points:
            out.append((i, i + 1, True))
            i += 1
            continue
        e, total = i, 0
        while e < n and e - i < max_seq and n_points[e] <= max_points and total + n_points[e] <= max_points:
            total += n_points[e]
            e += 1
        out.append((i, e, False))
        i = e
    return out


def _handles(ctxs):
    import ctypes
    if len({c.device for c in ctxs}) > 1:
        raise ValueError("the contexts of a batch must be on one device")
    return (ctypes.c_void_p * len(ctxs))(*[c.handle.value for c in ctxs])


def result_filter_batch_device(ctxs, traj_min_len=3):
    """psfm_result_filter for every context, at most 64 per call: [(n_traj, n_points)] in the order given."""
    import ctypes
    from point_trajectory import _hip
    L = _hip.lib()
    out = []
    for lo in range(0, len(ctxs), BATCH_MAX):
        part = ctxs[lo:lo + BATCH_MAX]
        k, npt = (ctypes.c_int64 * len(part))(), (ctypes.c_int64 * len(part))()
        _hip.check(L.psfm_result_filter_batch(_handles(part), len(part), int(traj_min_len), k, npt, _hip.current_stream_ptr(part[0].device)))
        out += [(int(k[i]), int(npt[i])) for i in range(len(part))]
    return out


def _tables_batch(ctxs, n_imgs, n_points, max_points, single, batch):
    """Groups by the grouping rule; `single(i)` / `batch(lo, hi, handles, n_img, kp, m, p, stream)` run the entry points; then one
    psfm_matches_copy per context."""
    import ctypes
    from point_trajectory import _hip
    tables = []
    for lo, hi, alone in group_sequences(n_points, max_points):
        if alone:
            sizes = [single(lo)]
        else:
            part = ctxs[lo:hi]
            n = hi - lo
            kp, m, p = (ctypes.c_int64 * n)(), (ctypes.c_int64 * n)(), (ctypes.c_int64 * n)()
            n_img = (ctypes.c_int32 * n)(*[int(v) for v in n_imgs[lo:hi]])
            _hip.check(batch(lo, hi, _handles(part), n_img, kp, m, p, _hip.current_stream_ptr(part[0].device)))
            sizes = [(int(kp[i]), int(m[i]), int(p[i])) for i in range(n)]
        tables += [_copy_tables(ctxs[lo + i], int(n_imgs[lo + i]), *sizes[i]) for i in range(hi - lo)]
    return tables


def match_tables_batch_device(ctxs, n_imgs, traj_min_len=3, sample_k=SAMPLE_K, labels=None, max_points=MAX_POINTS):
    """match_tables_device for every context of a batch (psfm_connect_batch leaves one per sequence): the saved sets through
    psfm_result_filter_batch, the tables through psfm_traj_to_matches_batch -- host synchronisations and launches per call that do
    not depend on the number of sequences -- then one copy of the finished tables per context.  labels: None, or one entry per
    sequence (a uint8 device tensor over the saved set's points, or None).  Returns the table tuples in the order given, equal
    to the per-sequence function's."""
    import ctypes
    from point_trajectory import _hip
    L = _hip.lib()
    ctxs, labels = list(ctxs), (None if labels is None else list(labels))
    if len(n_imgs) != len(ctxs) or (labels is not None and len(labels) != len(ctxs)):
        raise ValueError("one n_img (and one labels entry) per context")
    n_points = [n for _, n in result_filter_batch_device(ctxs, traj_min_len)]

    def single(i):
        a, b, c = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        _hip.check(L.psfm_traj_to_matches(ctxs[i].handle, int(n_imgs[i]), int(sample_k), _hip.ptr(None if labels is None else labels[i]),
                                          ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), _hip.current_stream_ptr(ctxs[i].device)))
        return int(a.value), int(b.value), int(c.value)

    def batch(lo, hi, handles, n_img, kp, m, p, sp):
        lab = None
        if labels is not None:
            lab = (ctypes.c_void_p * (hi - lo))(*[_hip.ptr(t).value for t in labels[lo:hi]])
        return L.psfm_traj_to_matches_batch(handles, hi - lo, n_img, int(sample_k), lab, kp, m, p, sp)

    return _tables_batch(ctxs, n_imgs, n_points, max_points, single, batch)


def match_tables_labelled_batch_device(ctxs, n_imgs, remove_dynamic=True, sample_k=SAMPLE_K, max_points=MAX_POINTS):
    """match_tables_labelled_device for every context of a batch (label_sequences_batched leaves a labelled set in each): the tables
    through psfm_labels_to_matches_batch, then one copy per context.  Returns the table tuples in the order given."""
    import ctypes
    from point_trajectory import _hip
    L = _hip.lib()
    ctxs = list(ctxs)
    if len(n_imgs) != len(ctxs):
        raise ValueError("one n_img per context")
    n_points = []
    for c in ctxs:
        n = ctypes.c_int64(0)
        _hip.check(L.psfm_labels_sizes(c.handle, None, ctypes.byref(n)))
        n_points.append(int(n.value))
    rd = 1 if remove_dynamic else 0

    def single(i):
        a, b, c = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        _hip.check(L.psfm_labels_to_matches(ctxs[i].handle, int(n_imgs[i]), int(sample_k), rd, ctypes.byref(a), ctypes.byref(b),
                                            ctypes.byref(c), _hip.current_stream_ptr(ctxs[i].device)))
        return int(a.value), int(b.value), int(c.value)

    def batch(lo, hi, handles, n_img, kp, m, p, sp):
        return L.psfm_labels_to_matches_batch(handles, hi - lo, n_img, int(sample_k), rd, kp, m, p, sp)

    return _tables_batch(ctxs, n_imgs, n_points, max_points, single, batch)


def traj_to_matches_batch_device(ctxs, image_names, match_list_files, traj_min_len=3, sample_k=SAMPLE_K, labels=None, as_arrays=True,
                                 max_points=MAX_POINTS):
    """traj_to_matches_device for every sequence of a batch: image_names and match_list_files hold one entry per sequence.  Returns
    the `assemble` results in the order given."""
    tables = match_tables_batch_device(ctxs, [len(n) for n in image_names], traj_min_len, sample_k, labels, max_points)
    return [assemble(list(n), t, f, as_arrays) for n, t, f in zip(image_names, tables, match_list_files)]


def traj_to_matches_labelled_batch_device(ctxs, image_names, match_list_files, remove_dynamic=True, sample_k=SAMPLE_K, as_arrays=True,
                                          max_points=MAX_POINTS):
    """traj_to_matches_labelled_device for every sequence of a batch.  Returns the `assemble` results in the order given."""
    tables = match_tables_labelled_batch_device(ctxs, [len(n) for n in image_names], remove_dynamic, sample_k, max_points)
    return [assemble(list(n), t, f, as_arrays) for n, t, f in zip(image_names, tables, match_list_files)]
