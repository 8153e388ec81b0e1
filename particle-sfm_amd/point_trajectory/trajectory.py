"""Mirror of the reference's point_trajectory/trajectory.py on top of libpsfm_hip.so.

What the reference does per frame with Python lists of pybind objects (IncrementalTrajectorySet,
trajectory.py:98-194) lives on the device here: lanes + a frame-major position log (csrc/psfm_track.hip).
This module keeps the reference's *callable surface*: `grid_sample` (:25-37) and the result container that
`track()` / `track_optimize()` return -- a list-like of Trajectory in full_trajs order.
"""
import ctypes
import os
import sys

import numpy as np

from . import _hip
from .optimize.build import particlesfm
from . import reference_pickle


def grid_sample(data, xy):
    """trajectory.py:25-37.  data: [C,H,W] torch tensor (C in {1,2}); xy: [N,2] array -> [N,C] float32 ndarray.
    Bit-exact with the reference's torch-CPU F.grid_sample(bilinear, zeros, align_corners=True)."""
    import torch
    ctx = _hip.context()
    dev = torch.device("cuda", ctx.device)
    C, H, W = int(data.shape[0]), int(data.shape[1]), int(data.shape[2])
    m = data.detach().to(dev, torch.float32).permute(1, 2, 0).contiguous()   # HWC, the kernels' native layout
    pts = torch.from_numpy(np.ascontiguousarray(np.asarray(xy, dtype=np.float64).reshape(-1, 2))).to(dev)
    out = torch.empty((pts.shape[0], C), dtype=torch.float32, device=dev)
    _hip.check(_hip.lib().psfm_grid_sample(ctx.handle, _hip.ptr(m), C, H, W, _hip.ptr(pts), pts.shape[0],
                                           _hip.ptr(out), _hip.current_stream_ptr(ctx.device)))
    return out.cpu().numpy()


def motion_boundary(flow, thres=0.02):
    """trajectory.py:39-43: the bool map of pixels whose flow gradient exceeds thres x the flow's norm.  flow: (H,W,2) float32.
    A device tensor is answered by the device (psfm_motion_boundary, a bool tensor on the same device); anything else by NumPy,
    operation by operation as the reference evaluates it (every intermediate an f32 array)."""
    try:
        import torch
        on_device = isinstance(flow, torch.Tensor) and flow.is_cuda
    except ImportError:
        on_device = False
    if on_device:
        ctx = _hip.context(flow.device.index)
        f = flow.detach().to(torch.float32).contiguous()
        H, W = int(f.shape[0]), int(f.shape[1])
        out = torch.empty((H, W), dtype=torch.uint8, device=f.device)
        _hip.check(_hip.lib().psfm_motion_boundary(ctx.handle, _hip.ptr(f), 1, H, W, float(thres), _hip.ptr(out),
                                                   _hip.current_stream_ptr(ctx.device)))
        return out.to(torch.bool)
    f = np.asarray(flow.detach().cpu().numpy() if hasattr(flow, "detach") else flow)
    with np.errstate(all="ignore"):
        dx, dy = np.zeros_like(f), np.zeros_like(f)
        dx[:, :-1, :] = np.abs(f[:, :-1, :] - f[:, 1:, :])
        dy[:-1, :, :] = np.abs(f[:-1, :, :] - f[1:, :, :])
        f_dx, f_dy = np.mean(dx, -1), np.mean(dy, -1)
        motion = np.sqrt(f_dx ** 2 + f_dy ** 2)
        return motion > thres * np.linalg.norm(f, ord=2, axis=-1)


def kill_map_batch(flows, occ, thres=0.02, pair0=0, n_pairs=None, out=None, ctx=None):
    """psfm_kill_map_batch: the kill maps (bit 0 occlusion, bit 1 motion boundary) of up to 64 same-shape stacks in ONE launch,
    frames [pair0, pair0 + n_pairs) of every stack (default: to the end of the longest).
    flows: list of (n_i,H,W,2) float32 device tensors; occ: list of (n_i,H,W) uint8 device tensors; thres: one value or one per
    stack; out: list of (n_i,H,W) uint8 device tensors to write into (default: new ones, zero outside the range).  Returns `out`.
    Only the occlusion bytes of the frames of the range are read and only their kill bytes written."""
    import torch
    n_seq = len(flows)
    if ctx is None:
        ctx = _hip.context()
    th = [float(thres)] * n_seq if np.isscalar(thres) else [float(t) for t in thres]
    if len(occ) != n_seq or len(th) != n_seq or (out is not None and len(out) != n_seq):
        raise ValueError("kill_map_batch: %d stacks need as many occlusion stacks, thresholds and outputs" % n_seq)
    H, W = (int(flows[0].shape[1]), int(flows[0].shape[2])) if n_seq else (0, 0)
    for i in range(n_seq):
        if (not flows[i].is_cuda or flows[i].dtype != torch.float32 or not flows[i].is_contiguous() or tuple(flows[i].shape[1:]) != (H, W, 2)
                or occ[i].dtype != torch.uint8 or not occ[i].is_contiguous() or tuple(occ[i].shape) != tuple(flows[i].shape[:3])):
            raise ValueError("kill_map_batch: stack %d is not a contiguous (n,%d,%d,2) float32 / (n,%d,%d) uint8 pair on the device" % (i, H, W, H, W))
    if out is None:
        out = [torch.zeros_like(o) for o in occ]
    n = [int(f.shape[0]) for f in flows]
    if n_pairs is None:
        n_pairs = max(max(n, default=0) - int(pair0), 0)
    vp = ctypes.c_void_p
    _hip.check(_hip.lib().psfm_kill_map_batch(
        ctx.handle, (vp * n_seq)(*[f.data_ptr() for f in flows]), (vp * n_seq)(*[o.data_ptr() for o in occ]), (ctypes.c_int * n_seq)(*n), n_seq,
        H, W, (ctypes.c_float * n_seq)(*th), int(pair0), int(n_pairs), (vp * n_seq)(*[o.data_ptr() for o in out]),
        _hip.current_stream_ptr(ctx.device)))
    return out


class _MotionBoundary:
    """Sets psfm_ctx_set_motion_boundary on a context for the duration of one call (the option is per context, off by default)."""

    def __init__(self, ctx, enable, thres):
        self.ctx, self.enable, self.thres = ctx, bool(enable), float(thres)

    def __enter__(self):
        if self.enable:
            self.ctx.set_motion_boundary(True, self.thres)

    def __exit__(self, *exc):
        if self.enable:
            self.ctx.set_motion_boundary(False)
        return False


class TrajectoryList:
    """What track()/track_optimize() return: trajectories in full_trajs order (index == saved id,
    main_connect_point_trajectories.py:56-60), stored as CSR arrays copied once from HBM.

    Behaves like the reference's list of Trajectory objects (len, indexing, iteration; elements expose
    .length(), .times, .xys, .labels, .as_dict()) without materialising ~5e7 Python objects up front."""

    def __init__(self, birth, length, off, xy, info=None, solve_stats=None):
        self.birth = birth          # (n,) int32
        self.length = length        # (n,) int32
        self.off = off              # (n+1,) int64
        self.xy = xy                # (n_points, 2) float64
        self.info = info or {}
        self.solve_stats = solve_stats or []

    def __len__(self):
        return int(self.birth.shape[0])

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(len(self)))]
        if i < 0:
            i += len(self)
        if not 0 <= i < len(self):
            raise IndexError(i)
        return particlesfm.Trajectory._from_arrays(self.birth[i], self.xy[self.off[i]:self.off[i + 1]])

    def __iter__(self):
        for i in range(len(self)):
            yield self[i]

    @property
    def n_points(self):
        return int(self.xy.shape[0])

    def to_trajectory_set(self, traj_min_len=3):
        """main_connect_point_trajectories.py:56-61: ids are list indices, short tracks dropped."""
        keep_mask = self.length >= int(traj_min_len)
        keep = np.nonzero(keep_mask)[0]
        length = self.length[keep]
        off = np.zeros(len(keep) + 1, np.int64)
        np.cumsum(length, out=off[1:])
        xy = self.xy[np.repeat(keep_mask, self.length)]     # array-speed: no per-trajectory Python objects
        return particlesfm.TrajectorySet._from_csr(keep, self.birth[keep], length, off, xy)


def _host_arrays(sizes_bytes, pinned_limit=2 << 30):
    """One host allocation cut into 64-byte aligned uint8 views.  Page-locked (torch's caching host allocator: no
    hipHostMalloc per call once warm, D2H at the full PCIe rate) up to `pinned_limit` bytes, pageable beyond."""
    offs = np.concatenate([[0], np.cumsum([(int(x) + 63) // 64 * 64 for x in sizes_bytes])])
    total = int(offs[-1])
    raw = None
    if 0 < total <= pinned_limit:
        try:
            import torch
            raw = torch.empty(total, dtype=torch.uint8, pin_memory=True).numpy()   # the views keep the tensor alive
        except Exception:
            raw = None
    if raw is None:
        raw = np.empty(total, np.uint8)
    return [raw[offs[i]:offs[i] + int(sizes_bytes[i])] for i in range(len(sizes_bytes))]


def _result_to_host(ctx, info):
    n, npnt = int(info.n_traj), int(info.n_points)
    b_birth, b_len, b_off, b_xy = _host_arrays([4 * n, 4 * n, 8 * (n + 1), 16 * npnt])
    birth = b_birth.view(np.int32)
    length = b_len.view(np.int32)
    off = b_off.view(np.int64)
    off[:] = 0
    xy = b_xy.view(np.float64).reshape(-1, 2)
    _hip.check(_hip.lib().psfm_result_copy(ctx.handle, birth.ctypes.data_as(ctypes.c_void_p),
                                           length.ctypes.data_as(ctypes.c_void_p), off.ctypes.data_as(ctypes.c_void_p),
                                           xy.ctypes.data_as(ctypes.c_void_p), _hip.current_stream_ptr(ctx.device)))
    stats = []
    if info.n_solves:
        arr = (_hip.SolveStats * int(info.n_solves))()
        nout = ctypes.c_int32()
        _hip.check(_hip.lib().psfm_result_solve_stats(ctx.handle, arr, int(info.n_solves), ctypes.byref(nout)))
        stats = [arr[i].as_dict() for i in range(nout.value)]
    return TrajectoryList(birth, length, off, xy, info.as_dict(), stats)


def result_to_trajectory_set(ctx, info, traj_min_len=3, reuse_pinned=False):
    """The saved set of main_connect_point_trajectories.py:56-61 from the device-resident result: the min-length filter
    runs on the GPU (psfm_result_filter) and only the kept trajectories cross PCIe.  reuse_pinned=True stages them in
    a pinned buffer owned by the context -- twice the copy rate, but the arrays of the returned TrajectorySet are views
    of that buffer and are overwritten by the next call (for callers that save the set straight away)."""
    import torch
    L = _hip.lib()
    k, npt = ctypes.c_int64(0), ctypes.c_int64(0)
    _hip.check(L.psfm_result_filter(ctx.handle, int(traj_min_len), ctypes.byref(k), ctypes.byref(npt), _hip.current_stream_ptr(ctx.device)))
    k, npt = int(k.value), int(npt.value)
    sizes = [4 * k, 4 * k, 4 * k, 8 * (k + 1), 16 * npt]
    offs = np.concatenate([[0], np.cumsum([(x + 63) // 64 * 64 for x in sizes])])
    if reuse_pinned:
        buf = getattr(ctx, "_pinned_result", None)
        if buf is None or buf.numel() < int(offs[-1]):
            buf = torch.empty(int(offs[-1]) + (64 << 20), dtype=torch.uint8, pin_memory=True)
            ctx._pinned_result = buf
        raw = buf.numpy()
    else:
        raw = np.empty(int(offs[-1]), np.uint8)
    ids = raw[offs[0]:offs[0] + sizes[0]].view(np.int32)
    birth = raw[offs[1]:offs[1] + sizes[1]].view(np.int32)
    length = raw[offs[2]:offs[2] + sizes[2]].view(np.int32)
    off = raw[offs[3]:offs[3] + sizes[3]].view(np.int64)
    xy = raw[offs[4]:offs[4] + sizes[4]].view(np.float64).reshape(-1, 2)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    _hip.check(L.psfm_result_filtered_copy(ctx.handle, vp(ids), vp(birth), vp(length), vp(off), vp(xy), _hip.current_stream_ptr(ctx.device)))
    return particlesfm.TrajectorySet._from_csr(ids.astype(np.int64), birth, length, off, xy)


def save_track_npy(path, trajectories, layout="reference"):
    """np.save(path, trajectories) for consumers that np.load(path, allow_pickle=True).item(): the same .npy container
    (object array header + pickle), written with pickle protocol 5 so that the point array streams to the file without an
    intermediate bytes copy.
    layout "reference" (default): the pickle state of the reference's pybind class (bindings.cc:64-71) -- the file loads
    with the original module as well; "csr": this package's compact array state (array-speed save / load at 1e6+
    trajectories, readable only where this package provides `point_trajectory.optimize.build.particlesfm`)."""
    import pickle
    if layout not in ("reference", "csr"):
        raise ValueError("save_track_npy: layout must be 'reference' or 'csr'")
    if isinstance(trajectories, particlesfm.TrajectorySet):
        trajectories.pickle_layout = layout
    arr = np.empty((), dtype=object)
    arr[()] = trajectories
    # written beside the target and moved over it: a TrajectorySet loaded from the SAME path maps its points from the old file
    # (reference_pickle.load), and truncating that file in place would take the pages away under it (SIGBUS)
    target = path if str(path).endswith(".npy") else str(path) + ".npy"
    tmp = "%s.tmp-%d" % (target, os.getpid())
    try:
        with open(tmp, "w+b") as fp:
            np.lib.format.write_array_header_1_0(fp, np.lib.format.header_data_from_array_1_0(arr))
            if layout == "reference" and reference_pickle.can_stream(trajectories):
                reference_pickle.dump(fp, trajectories)      # the reference's object graph as opcodes, straight from the CSR
            else:
                pickle.dump(arr, fp, protocol=5)
        _replace_deferring_reclaim(tmp, target)
    except BaseException:
        if os.path.exists(tmp):
            os.unlink(tmp)
        raise


_reclaims = []      # helper threads that drop replaced files (joined by wait_for_reclaims / at interpreter exit: they are not daemons)


def _replace_deferring_reclaim(tmp, target):
    """os.replace(tmp, target), without waiting for the kernel to give back the pages of the file it replaces: rename() frees the old
    inode's page cache before it returns (0.94 GB of track.npy on tmpfs: 50-70 ms of the stage's 0.29 s when it runs over an
    existing output, scripts/micro/e2e_overwrite.py).  A second link keeps the old inode alive across the rename; a helper thread
    drops it.  File systems without hard links take the plain rename."""
    import threading
    doomed = None
    if os.path.exists(target):
        doomed = "%s.old-%d-%d" % (target, os.getpid(), len(_reclaims))
        try:
            os.link(target, doomed)
        except OSError:
            doomed = None
    os.replace(tmp, target)
    if doomed is not None:
        def drop():
            try:
                os.unlink(doomed)
            except OSError:
                pass
        th = threading.Thread(target=drop, name="psfm-reclaim")
        th.start()
        _reclaims[:] = [t for t in _reclaims if t.is_alive()] + [th]


def wait_for_reclaims():
    """Blocks until the files replaced by save_track_npy are gone (tests; callers that are about to remove the directory)."""
    for t in list(_reclaims):
        t.join()
    del _reclaims[:]


def load_track_npy(path):
    """track.npy -> TrajectorySet, for this package's own consumers.  A file written by save_track_npy in the reference layout is
    read back through the footer the writer leaves behind the pickle (CSR arrays straight from the file: ~1 s instead of the
    ~25 s the reference layout takes to unpickle at 1.9 M trajectories); any other file through
    np.load(path, allow_pickle=True).item()."""
    return reference_pickle.load(path)


def _trajectory_set_to_device(self, ctx=None):
    """TrajectorySet.to_device(ctx=None): this set as the RESULT of a context (psfm_result_set), so that the device consumers of a
    tracker's result -- the window sampler, the label merge, the match tables, the database rows -- run on it.  Trajectories go in
    ascending id order, as the reference's std::map iterates; labels are not carried (a result has none).  A trajectory whose
    frame_ids are not consecutive raises ValueError naming its id: a result holds frames birth .. birth + len - 1, sets with gaps
    enter as a labelled set (psfm_motion_seg.merge_labels.set_labelled).  Returns the context (default: the calling thread's)."""
    if self._csr is not None and self._map is None:
        ids, birth, length, off, xy, _ = self._csr
        ids, birth, length = np.asarray(ids, np.int64), np.asarray(birth, np.int32), np.asarray(length, np.int32)
        if len(ids) > 1 and np.any(ids[1:] <= ids[:-1]):
            order = np.argsort(ids, kind="stable")
            n_of = length[order].astype(np.int64)
            pts = np.repeat(np.asarray(off[:-1], np.int64)[order], n_of) + (np.arange(int(n_of.sum())) - np.repeat(np.cumsum(n_of) - n_of, n_of))
            ids, birth, length, xy = ids[order], birth[order], length[order], np.asarray(xy)[pts]
    else:
        keys = sorted(self._map)
        ids = np.asarray(keys, np.int64)
        birth, length, locs = np.zeros(len(keys), np.int32), np.zeros(len(keys), np.int32), []
        for j, k in enumerate(keys):
            t = self._map[k]
            times = np.fromiter(t._times, np.int64, count=len(t._times))[:len(t._xys)]
            if len(times) == 0 or np.any(times != times[0] + np.arange(len(times))):
                raise ValueError("TrajectorySet.to_device: trajectory %d has no points or frame_ids that are not consecutive "
                                 "(a result holds frames birth .. birth + len - 1; psfm_labels_set takes sets with gaps)" % int(k))
            birth[j], length[j] = times[0], len(times)
            locs.append(np.asarray(t._xys, dtype=np.float64).reshape(-1, 2))
        xy = np.concatenate(locs) if locs else np.zeros((0, 2))
    if len(ids) and (int(ids[0]) < 0 or int(ids[-1]) >= 1 << 28):
        raise ValueError("TrajectorySet.to_device: ids must lie in [0, 2^28)")
    ctx = ctx or _hip.context()
    ctx.set_result(ids.astype(np.int32), birth, length, xy)
    return ctx


# The container class mirrors the reference's pybind module and knows nothing of contexts; its device entry is attached here, where
# the package's other context routes live (importing point_trajectory, or anything inside it, imports this module).
particlesfm.TrajectorySet.to_device = _trajectory_set_to_device


def load_track_npy_device(path, ctx=None, threads=4):
    """track.npy -> a context, for the device consumers of a stage that starts from a file.  Returns (ctx, kind, sizes):
      kind "set"       the file held a TrajectorySet: it is the context's RESULT now (psfm_result_set: index == id, ids the file does
                       not hold are entries of length 0; psfm_result_filter(ctx, 1) gives the file's set back).  A file this package
                       wrote in the reference layout goes from the file into HBM (psfm_load_track_npy, `threads` reader threads); when
                       that call refuses it (PSFM_ERR_ARG: no footer -- the csr layout, a file the reference's own module pickled --
                       or a footer that fails a check) the file goes through load_track_npy and TrajectorySet.to_device.
                       sizes = {"n_traj", "n_points", "n_result", "route": "file" | "host"}
      kind "labelled"  the file held the plain dict stage 2 writes: flattened in the dict's order, it is the context's LABELLED set
                       (psfm_labels_set).  sizes = {"n_traj", "n_points", "route": "host"}
    sizes["true_labels"] (kind "set", host route): the file's set carries True labels, which a result cannot hold (they are dropped).
    ctx=None takes the calling thread's context, the one run_connect uses by default: the result (or labelled set) a tracker left
    there is REPLACED without notice -- pass a context of your own (_hip.Context(device)) to keep it."""
    ctx = ctx or _hip.context()
    try:
        n, p, r = ctx.load_track_npy(path, threads)
        return ctx, "set", {"n_traj": n, "n_points": p, "n_result": r, "route": "file"}
    except _hip.PsfmError as e:
        if e.status != _hip.PSFM_ERR_ARG:
            raise
    obj = load_track_npy(path)
    if isinstance(obj, particlesfm.TrajectorySet):
        obj.to_device(ctx)
        n_points = int(obj._csr[3][-1]) if obj._map is None else sum(len(t._xys) for t in obj._map.values())
        ids = obj._csr[0] if obj._map is None else list(obj._map)
        if obj._map is None:
            true_labels = obj._csr[5] is not None and bool(np.any(obj._csr[5]))
        else:
            true_labels = any(t._labels is not None and any(t._labels) for t in obj._map.values())
        return ctx, "set", {"n_traj": len(obj), "n_points": n_points, "n_result": (int(max(ids)) + 1) if len(obj) else 0, "route": "host",
                            "true_labels": true_labels}
    if isinstance(obj, dict):
        from psfm_motion_seg.merge_labels import set_labelled
        n, p = set_labelled(ctx, obj)
        return ctx, "labelled", {"n_traj": n, "n_points": p, "route": "host"}
    raise TypeError("load_track_npy_device: %s holds a %s, neither a TrajectorySet nor a labelled dict" % (path, type(obj).__name__))


def _as_device_stack(maps, dtype, trailing):
    """list of (H,W[,2]) arrays | (n,H,W[,2]) array/tensor -> contiguous device tensor."""
    import torch
    ctx = _hip.context()
    dev = torch.device("cuda", ctx.device)
    if isinstance(maps, torch.Tensor):
        t = maps
    else:
        if isinstance(maps, (list, tuple)):
            if len(maps) and isinstance(maps[0], torch.Tensor):
                t = torch.stack(list(maps))
            else:
                t = torch.from_numpy(np.stack([np.asarray(m) for m in maps])) if len(maps) else torch.zeros((0,) + trailing)
        else:
            t = torch.from_numpy(np.asarray(maps))
    if t.dtype == torch.bool and dtype == torch.uint8:
        t = t.to(torch.uint8)
    return t.to(device=dev, dtype=dtype).contiguous()


def _capacity_of(ctx, key):
    """Table factors that worked for this shape on this context (default 2 x lanes, 8 x trajectory records)."""
    if not isinstance(getattr(ctx, "_capacity", None), dict):
        ctx._capacity = {}
    return ctx._capacity.get(key, (2.0, 8.0))


def run_connect(flows_f, flows_b, flows_f2, flows_b2, thres, sample_ratio, return_device=False, motion_boundary=False, mb_thres=0.02,
                ctx=None):
    """flow_check + track / track_optimize in ONE psfm_connect call (the compute part of
    main_connect_point_trajectories.py:36-53): the occlusion maps are produced on a side stream while the frame
    loop consumes them.  Inputs: (n,H,W,2) float32 device tensors (stride-2 stacks None to skip path consistency).
    motion_boundary: tracks also die on motion boundaries of threshold mb_thres (the reference's commented kill rule,
    trajectory.py:60); ctx: the context that runs the call and keeps the result (default: the calling thread's)."""
    import torch
    if ctx is None:
        ctx = _hip.context()
    n, H, W = int(flows_f.shape[0]), int(flows_f.shape[1]), int(flows_f.shape[2])
    if n < 1:
        raise ValueError("connect: need at least one flow field")
    n = min(n, int(flows_b.shape[0]))
    f2 = b2 = None
    if flows_f2 is not None:
        f2, b2 = flows_f2, flows_b2
        if n > 1 and (f2.shape[0] < n - 1 or b2.shape[0] < n - 1):
            raise ValueError("connect: need %d stride-2 flows" % (n - 1))
        if f2.numel() == 0:
            f2 = torch.zeros((1, H, W, 2), dtype=torch.float32, device=flows_f.device)
            b2 = f2
    info = _hip.TrackInfo()
    cap_key = ("connect", n, H, W, int(sample_ratio), f2 is not None)
    lane_f, traj_f = _capacity_of(ctx, cap_key)
    with _MotionBoundary(ctx, motion_boundary, mb_thres):
        for attempt in range(6):
            ctx.set_capacity(lane_f, traj_f)
            ctx._capacity[cap_key] = (lane_f, traj_f)      # remembered per shape: a sequence that needed larger tables keeps them
            st = _hip.lib().psfm_connect(ctx.handle, _hip.ptr(flows_f), _hip.ptr(flows_b), _hip.ptr(f2), _hip.ptr(b2), n, H, W,
                                         float(thres), int(sample_ratio), None, None, ctypes.byref(info),
                                         _hip.current_stream_ptr(ctx.device))
            if st != _hip.PSFM_ERR_CAPACITY:
                break
            lane_f, traj_f = lane_f * 2.0, traj_f * 4.0
    _hip.check(st)
    if return_device:
        return info
    return _result_to_host(ctx, info)


# How run_connect_batch(..., motion_boundary=True) runs when the caller does not say: "batch" (psfm_connect_batch with the option on in
# every context) or "loop" (one psfm_connect per sequence).  Measured (scripts/micro/motion_boundary_batch.py, profiles/EXPERIMENTS.md
# section 28): 5.1-5.4x on DAVIS-sized batches in track mode, 3.0x on Sintel-sized ones with path consistency, same results.
MB_ENGINE_DEFAULT = "batch"


def run_connect_batch(seqs, thres, sample_ratio, motion_boundary=False, mb_thres=0.02, mb_engine=None, redo=None):
    """psfm_connect_batch: flow_check + track / track_optimize for a BATCH of sequences (the directory of sequences the
    reference's driver walks, run_particlesfm.py:168-176) with every frame launch covering the whole batch.
    seqs: list of (flows_f, flows_b, flows_f2 | None, flows_b2 | None) device tensors (n_i,H_i,W_i,2) -- all with stride-2 stacks or
    none.  Sequences of one frame size make the call with that size; with several sizes every batch context is given its sequence's
    (Context.set_frame_size, cleared again behind the call) and the call is made with h = w = 0: same results.  Returns (contexts, infos): context i holds sequence i's result (`_result_to_host(ctx, info)`,
    `result_to_trajectory_set(ctx, info)`) until the calling thread's next batch.
    motion_boundary: tracks also die on motion boundaries of threshold mb_thres (one value, or one per sequence).  mb_engine "batch":
    the option is set on every batch context for the duration of the call and the batched launches form the verdict; "loop": the
    sequences go through run_connect one after the other, each on its own context; None: MB_ENGINE_DEFAULT.  Same results.
    redo: how the sequences that leave the fused batch (path consistency on flows whose solves reject steps) are run again -- "alone":
    each through psfm_connect; "together": all of them through one set of launches (Context.set_batch_redo; info.chain_mode 8, census
    in ctxs[0].connect_batch_census()); None: as the batch's first context is set (default "alone"; PSFM_BATCH_REDO=together|alone
    overrides all of it, for measurements).  A string sets the option for the duration of the call."""
    import torch
    n_seq = len(seqs)
    if n_seq < 1:
        return [], []
    if redo not in (None, "alone", "together"):
        raise ValueError("connect_batch: redo must be 'alone', 'together' or None")
    mb_list = None
    if motion_boundary:
        mb_list = [float(mb_thres)] * n_seq if np.isscalar(mb_thres) else [float(t) for t in mb_thres]
        if len(mb_list) != n_seq:
            raise ValueError("connect_batch: %d thresholds for %d sequences" % (len(mb_list), n_seq))
        engine = MB_ENGINE_DEFAULT if mb_engine is None else mb_engine
        if engine not in ("batch", "loop"):
            raise ValueError("connect_batch: mb_engine must be 'batch', 'loop' or None")
        if engine == "loop":
            ctxs = _hip.batch_contexts(n_seq)
            infos = [run_connect(a, b, a2, b2_, thres, sample_ratio, return_device=True, motion_boundary=True, mb_thres=t, ctx=c)
                     for c, t, (a, b, a2, b2_) in zip(ctxs, mb_list, seqs)]
            return ctxs, infos
    shapes = [(int(a.shape[1]), int(a.shape[2])) for a, _, _, _ in seqs]
    H, W = shapes[0]
    mixed = any(sh != shapes[0] for sh in shapes)      # several frame sizes: every batch context carries its sequence's, the call has h = w = 0
    opt = seqs[0][2] is not None
    keep = []           # (tensors created here must outlive the call)
    nf = (ctypes.c_int * n_seq)()
    vp = ctypes.c_void_p
    ff, fb, f2, b2 = (vp * n_seq)(), (vp * n_seq)(), (vp * n_seq)(), (vp * n_seq)()
    for i, (a, b, a2, b2_) in enumerate(seqs):
        if (a2 is not None) != opt:
            raise ValueError("connect_batch: sequence %d differs in stride-2 stacks from sequence 0 (all sequences with them, or none)" % i)
        if tuple(b.shape[1:3]) != shapes[i] or (a2 is not None and a2.numel() > 0 and (tuple(a2.shape[1:3]) != shapes[i] or tuple(b2_.shape[1:3]) != shapes[i])):
            raise ValueError("connect_batch: the stacks of sequence %d differ in frame size" % i)
        n = min(int(a.shape[0]), int(b.shape[0]))
        if n < 1:
            raise ValueError("connect_batch: sequence %d has no flow field" % i)
        if opt and n > 1 and (a2.shape[0] < n - 1 or b2_.shape[0] < n - 1):
            raise ValueError("connect_batch: sequence %d needs %d stride-2 flows" % (i, n - 1))
        nf[i] = n
        ff[i], fb[i] = a.data_ptr(), b.data_ptr()
        if opt:
            if a2.numel() == 0:
                a2 = b2_ = torch.zeros((1,) + shapes[i] + (2,), dtype=torch.float32, device=a.device)
                keep.append(a2)
            f2[i], b2[i] = a2.data_ptr(), b2_.data_ptr()
    ctxs = _hip.batch_contexts(n_seq)
    handles = (vp * n_seq)(*[c.handle for c in ctxs])
    infos = (_hip.TrackInfo * n_seq)()
    cap_key = ("batch", tuple(sorted(set(shapes))), int(sample_ratio), opt) if mixed else ("batch", H, W, int(sample_ratio), opt)
    lane_f, traj_f = _capacity_of(ctxs[0], cap_key)
    redo_before = ctxs[0].batch_redo
    try:
        if mixed:
            for c, (hi, wi) in zip(ctxs, shapes):
                c.set_frame_size(hi, wi)
            H = W = 0
        if redo is not None:
            ctxs[0].set_batch_redo(redo)
        if mb_list is not None:
            for c, t in zip(ctxs, mb_list):
                c.set_motion_boundary(True, t)
        for attempt in range(6):
            for c in ctxs:
                c.set_capacity(lane_f, traj_f)
            ctxs[0]._capacity[cap_key] = (lane_f, traj_f)
            st = _hip.lib().psfm_connect_batch(handles, n_seq, ff, fb, f2 if opt else None, b2 if opt else None, nf, H, W, float(thres),
                                               int(sample_ratio), infos, _hip.current_stream_ptr(ctxs[0].device))
            if st != _hip.PSFM_ERR_CAPACITY:
                break
            lane_f, traj_f = lane_f * 2.0, traj_f * 4.0      # tables too small for one of the sequences: grow all and rerun
    finally:
        if mb_list is not None:      # (the option is per context and the thread's batch contexts are reused: off again, whatever happened)
            for c in ctxs:
                c.set_motion_boundary(False)
        if redo is not None:
            ctxs[0].set_batch_redo(redo_before)
        if mixed:                    # (as the option: per context, and the thread's batch contexts are reused)
            for c in ctxs:
                c.set_frame_size(0, 0)
    _hip.check(st)
    return ctxs, [infos[i] for i in range(n_seq)]


def run_track(flows, occ_maps, flows_f2, occ_maps_s2, sample_ratio, return_device=False, motion_boundary=False, mb_thres=0.02):
    """Shared driver of track() / track_optimize(): one psfm_track call (whole frame loop on the device).
    motion_boundary / mb_thres: as in run_connect."""
    import torch
    ctx = _hip.context()
    fl = _as_device_stack(flows, torch.float32, (1, 1, 2))
    oc = _as_device_stack(occ_maps, torch.uint8, (1, 1))
    n, H, W = int(fl.shape[0]), int(fl.shape[1]), int(fl.shape[2])
    if n < 1:
        raise ValueError("track: need at least one flow field")
    if oc.shape[0] < n:
        raise ValueError("track: %d occlusion maps for %d flows" % (oc.shape[0], n))
    f2 = o2 = None
    if flows_f2 is not None:
        f2 = _as_device_stack(flows_f2, torch.float32, (1, 1, 2))
        o2 = _as_device_stack(occ_maps_s2, torch.uint8, (1, 1))
        if n > 1 and (f2.shape[0] < n - 1 or o2.shape[0] < n - 1):
            raise ValueError("track_optimize: need %d stride-2 flows / occlusion maps" % (n - 1))
        if f2.numel() == 0:   # single-pair sequence: the stride-2 stack is empty but must be non-NULL
            f2 = torch.zeros((1, H, W, 2), dtype=torch.float32, device=fl.device)
            o2 = torch.zeros((1, H, W), dtype=torch.uint8, device=fl.device)
    info = _hip.TrackInfo()
    cap_key = ("track", n, H, W, int(sample_ratio), f2 is not None)
    lane_f, traj_f = _capacity_of(ctx, cap_key)
    with _MotionBoundary(ctx, motion_boundary, mb_thres):
        for attempt in range(6):
            ctx.set_capacity(lane_f, traj_f)
            ctx._capacity[cap_key] = (lane_f, traj_f)
            st = _hip.lib().psfm_track(ctx.handle, _hip.ptr(fl), _hip.ptr(oc), _hip.ptr(f2), _hip.ptr(o2), n, H, W,
                                       int(sample_ratio), ctypes.byref(info), _hip.current_stream_ptr(ctx.device))
            if st != _hip.PSFM_ERR_CAPACITY:
                break
            if os.environ.get("PSFM_VERBOSE"):
                print("psfm_track: %s -> retry with larger tables" % _hip.lib().psfm_last_error().decode(), file=sys.stderr)
            lane_f, traj_f = lane_f * 2.0, traj_f * 4.0   # tables too small for this sequence: grow and rerun
    _hip.check(st)
    if return_device:
        return info
    return _result_to_host(ctx, info)


def run_track_queries(xy, t, flows=None, occ=None, flows_b=None, occ_b=None, motion_boundary=False, mb_thres=0.02, return_device=False,
                      flows_f2=None, occ_f2=None, flows_b2=None, occ_b2=None):
    """Caller-given query points tracked through a flow stack in ONE psfm_track_queries call: query i is the position xy[i] ((Q,2)
    float64) at frame t[i] ((Q,) int, 0 <= t <= n_flows); per query the body of track.py:37-47 (grid_sample + step_forward) until the
    first step that is not alive or the end of the stack.
    flows / occ: the forward stack (n,H,W,2) and its occlusion maps (n,H,W); flows_b / occ_b: the BACKWARD stack (flows_b[f]: frame
    f+1 -> f) and ITS occlusion maps, flow_check(flows_b, flows).  One stack: tracked that way; both: both ways, one trajectory.
    Returns a TrajectoryList whose trajectory i is query i (length >= 1); the result also replaces the context's result set, so the
    consumers of a tracking result (result_to_trajectory_set, sample_window_device, match_tables_device ...) work on it.
    A non-finite coordinate or a frame outside [0, n_flows] raises PsfmError (status PSFM_ERR_ARG) naming the first such query.
    flows_f2 / occ_f2 (forward) and flows_b2 / occ_b2 (backward; flows_b2[f]: frame f+2 -> f, occ_b2 = flow_check(flows_b2, flows_f2)):
    the stride-2 stacks (n-1,H,W,2) and THEIR occlusion maps (n-1,H,W).  With any of them given ONE psfm_track_queries_optimize call
    runs instead: after every step the queries that hold three positions are corrected by the stride-2 path-consistency solve of
    track_optimize.py:49-50, jointly over the call's queries (a query's positions then depend on its companions, as a grid track's
    do); a frame with no such query runs no solve.  R.info["chain_mode"] is 5 and R.info["n_solves"] counts the solves.  Without them
    the call is exactly psfm_track_queries."""
    import torch
    ctx = _hip.context()
    dev = torch.device("cuda", ctx.device)
    fl = oc = fb = ob = None
    stride2 = {"flows_f2": flows_f2, "occ_f2": occ_f2, "flows_b2": flows_b2, "occ_b2": occ_b2}
    optimize = any(v is not None for v in stride2.values())
    if flows is not None:
        fl = _as_device_stack(flows, torch.float32, (1, 1, 2))
    if occ is not None:
        oc = _as_device_stack(occ, torch.uint8, (1, 1))
    if flows_b is not None:
        fb = _as_device_stack(flows_b, torch.float32, (1, 1, 2))
    if occ_b is not None:
        ob = _as_device_stack(occ_b, torch.uint8, (1, 1))
    ref = fl if fl is not None else fb
    if ref is None:
        n, H, W = 0, 0, 0                 # (refused by the library: no stack given)
    else:
        n, H, W = int(ref.shape[0]), int(ref.shape[1]), int(ref.shape[2])
        for name, m, tail in (("flows", fl, (H, W, 2)), ("occ", oc, (H, W)), ("flows_b", fb, (H, W, 2)), ("occ_b", ob, (H, W))):
            if m is not None and (int(m.shape[0]) != n or tuple(m.shape[1:]) != tail):
                raise ValueError("track_queries: %s has shape %s, expected %s" % (name, tuple(m.shape), (n,) + tail))
    s2 = {}
    for name, m in stride2.items():
        if m is None:
            s2[name] = None
            continue
        flow = name.startswith("flows")
        m = _as_device_stack(m, torch.float32 if flow else torch.uint8, (1, 1, 2) if flow else (1, 1))
        tail = (H, W, 2) if flow else (H, W)
        if ref is not None and (int(m.shape[0]) != n - 1 or (m.numel() > 0 and tuple(m.shape[1:]) != tail)):
            raise ValueError("track_queries: %s has shape %s, expected %s" % (name, tuple(m.shape), (n - 1,) + tail))
        s2[name] = m if m.numel() > 0 else None       # (one flow: no solve can happen, the library takes NULL)

    def as_t(a, dt):
        a = a.detach() if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
        return a.to(device=dev, dtype=dt)
    q_xy = as_t(xy, torch.float64).reshape(-1, 2).contiguous()
    q_t = as_t(t, torch.int32).reshape(-1).contiguous()
    if q_t.shape[0] != q_xy.shape[0]:
        raise ValueError("track_queries: %d positions for %d frames" % (q_xy.shape[0], q_t.shape[0]))
    info = _hip.TrackInfo()
    with _MotionBoundary(ctx, motion_boundary, mb_thres):
        if optimize:
            st = _hip.lib().psfm_track_queries_optimize(ctx.handle, _hip.ptr(fl), _hip.ptr(oc), _hip.ptr(s2["flows_f2"]), _hip.ptr(s2["occ_f2"]),
                                                        _hip.ptr(fb), _hip.ptr(ob), _hip.ptr(s2["flows_b2"]), _hip.ptr(s2["occ_b2"]), n, H, W,
                                                        _hip.ptr(q_xy), _hip.ptr(q_t), int(q_xy.shape[0]), ctypes.byref(info),
                                                        _hip.current_stream_ptr(ctx.device))
        else:
            st = _hip.lib().psfm_track_queries(ctx.handle, _hip.ptr(fl), _hip.ptr(oc), _hip.ptr(fb), _hip.ptr(ob), n, H, W, _hip.ptr(q_xy),
                                               _hip.ptr(q_t), int(q_xy.shape[0]), ctypes.byref(info), _hip.current_stream_ptr(ctx.device))
    _hip.check(st)
    if return_device:
        return info
    return _result_to_host(ctx, info)


def run_connect_queries(xy, t, flows_f, flows_b, thres=1.0, direction="forward", motion_boundary=False, mb_thres=0.02, return_device=False,
                        flows_f2=None, flows_b2=None):
    """flow_check + run_track_queries: the occlusion maps each direction needs come from flow_check_device in that direction's own
    orientation -- forward: flow_check(flows_f, flows_b); backward: flow_check(flows_b, flows_f).  direction: "forward", "backward"
    or "both".  flows_f, flows_b: (n,H,W,2) stacks, flows_b[f] being the flow from frame f+1 to frame f.
    flows_f2, flows_b2 (both, (n-1,H,W,2), flows_b2[f]: frame f+2 -> f): the query tracks get the stride-2 path-consistency solve
    (run_track_queries); each direction's stride-2 maps are flow_check_device in that direction's orientation -- forward:
    flow_check(flows_f2, flows_b2); backward: flow_check(flows_b2, flows_f2)."""
    import torch
    from .utils import flow_check_device
    if direction not in ("forward", "backward", "both"):
        raise ValueError("connect_queries: direction must be 'forward', 'backward' or 'both'")
    ff = _as_device_stack(flows_f, torch.float32, (1, 1, 2))
    fb = _as_device_stack(flows_b, torch.float32, (1, 1, 2))
    n = min(int(ff.shape[0]), int(fb.shape[0]))
    ff, fb = ff[:n], fb[:n]
    kw = {}
    if (flows_f2 is None) != (flows_b2 is None):
        raise ValueError("connect_queries: the stride-2 maps of either direction need both stride-2 stacks")
    f2 = b2 = None
    if flows_f2 is not None:
        f2 = _as_device_stack(flows_f2, torch.float32, (1, 1, 2))[:max(n - 1, 0)]
        b2 = _as_device_stack(flows_b2, torch.float32, (1, 1, 2))[:max(n - 1, 0)]
        if int(f2.shape[0]) != n - 1 or int(b2.shape[0]) != n - 1:
            raise ValueError("connect_queries: need %d stride-2 flows per direction" % (n - 1))
    if direction in ("forward", "both"):
        kw.update(flows=ff, occ=flow_check_device(ff, fb, thres)[1])
        if f2 is not None:
            kw.update(flows_f2=f2, occ_f2=flow_check_device(f2, b2, thres)[1] if n > 1 else f2.new_zeros((0,) + tuple(ff.shape[1:3]), dtype=torch.uint8))
    if direction in ("backward", "both"):
        kw.update(flows_b=fb, occ_b=flow_check_device(fb, ff, thres)[1])
        if f2 is not None:
            kw.update(flows_b2=b2, occ_b2=flow_check_device(b2, f2, thres)[1] if n > 1 else f2.new_zeros((0,) + tuple(ff.shape[1:3]), dtype=torch.uint8))
    return run_track_queries(xy, t, motion_boundary=motion_boundary, mb_thres=mb_thres, return_device=return_device, **kw)


QUERY_BATCH_MAX_SEQ = 64             # PSFM_BATCH_MAX
QUERY_BATCH_MAX_QUERIES = 1 << 28    # queries of one psfm_track_queries_batch call: fewer than this


def _query_batch_groups(n_q):
    """Consecutive groups of at most 64 sequences and fewer than 2^28 queries: [(start, end)].  (A single sequence at or above the
    bound forms a group of its own, which the library refuses as it refuses it in psfm_track_queries.)"""
    groups, start, total = [], 0, 0
    for i, n in enumerate(n_q):
        if i > start and (i - start >= QUERY_BATCH_MAX_SEQ or total + n >= QUERY_BATCH_MAX_QUERIES):
            groups.append((start, i))
            start, total = i, 0
        total += n
    if len(n_q) > start:
        groups.append((start, len(n_q)))
    return groups


def run_track_queries_batch(seqs, motion_boundary=False, mb_thres=0.02, return_device=False):
    """run_track_queries for a LIST of sequences in one psfm_track_queries_batch call per group of at most 64 sequences (and fewer
    than 2^28 queries): every launch covers the queries of the whole group, so a directory of small videos pays the fixed cost of a
    call once.  seqs: dicts with `xy` ((Q,2) float64), `t` ((Q,) int) and the stacks of run_track_queries -- `flows`, `occ` (forward)
    and / or `flows_b`, `occ_b` (backward) -- each sequence with its own frame size, length and query count (zero queries: the empty
    result).  Every sequence must give the same direction(s): a ValueError otherwise.  Sequence i's result is byte for byte that of
    run_track_queries on it alone; R.info["chain_mode"] is 6.
    motion_boundary / mb_thres: as in run_connect_batch -- one threshold, or one per sequence; the option is set on the batch contexts
    (_hip.batch_contexts) for the duration of the call.
    Returns one TrajectoryList per sequence; with return_device=True (contexts, infos) -- context i holds sequence i's result until
    the calling thread's next batch -- which needs the list to fit one group.
    The stride-2 path-consistency form is out of scope (psfm_track_queries_optimize solves jointly per sequence with a host decision
    per frame): a sequence that comes with flows_f2 / occ_f2 / flows_b2 / occ_b2 is a ValueError; use run_track_queries_pc_batch
    (or run_track_queries) for it."""
    return _track_queries_batch(seqs, motion_boundary, mb_thres, return_device, False)


_STRIDE2 = (("flows_f2", "occ_f2"), ("flows_b2", "occ_b2"))


def _track_queries_batch(seqs, motion_boundary, mb_thres, return_device, optimize):
    """run_track_queries_batch (optimize False: stride-2 stacks are refused) and run_track_queries_pc_batch (optimize True: ONE
    psfm_track_queries_optimize_batch call per group)."""
    import torch
    who = "track_queries_pc_batch" if optimize else "track_queries_batch"
    n_seq = len(seqs)
    if n_seq < 1:
        return ([], []) if return_device else []
    mb_list = None
    if motion_boundary:
        mb_list = [float(mb_thres)] * n_seq if np.isscalar(mb_thres) else [float(v) for v in mb_thres]
        if len(mb_list) != n_seq:
            raise ValueError("%s: %d thresholds for %d sequences" % (who, len(mb_list), n_seq))
    first = _hip.context()
    dev = torch.device("cuda", first.device)

    def as_t(a, dt):
        a = a.detach() if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
        return a.to(device=dev, dtype=dt)
    prepared, dirs0 = [], None
    for i, sq in enumerate(seqs):
        if not optimize and any(sq.get(k) is not None for k in ("flows_f2", "occ_f2", "flows_b2", "occ_b2")):
            raise ValueError("track_queries_batch: sequence %d comes with stride-2 stacks; path consistency for a batch of sequences "
                             "is out of scope, use run_track_queries for it" % i)
        m = {}
        for name, dt, tail in (("flows", torch.float32, (1, 1, 2)), ("occ", torch.uint8, (1, 1)), ("flows_b", torch.float32, (1, 1, 2)),
                               ("occ_b", torch.uint8, (1, 1))):
            m[name] = _as_device_stack(sq[name], dt, tail) if sq.get(name) is not None else None
        if (m["flows"] is None) != (m["occ"] is None) or (m["flows_b"] is None) != (m["occ_b"] is None) or (m["flows"] is None and m["flows_b"] is None):
            raise ValueError("%s: sequence %d: give at least one stack, and every stack with its occlusion maps" % (who, i))
        dirs = (m["flows"] is not None, m["flows_b"] is not None)
        if dirs0 is None:
            dirs0 = dirs
        elif dirs != dirs0:
            raise ValueError("%s: sequence %d gives other directions than sequence 0 (a direction is given for the whole batch)" % (who, i))
        ref = m["flows"] if m["flows"] is not None else m["flows_b"]
        n, H, W = int(ref.shape[0]), int(ref.shape[1]), int(ref.shape[2])
        for name, tail in (("flows", (H, W, 2)), ("occ", (H, W)), ("flows_b", (H, W, 2)), ("occ_b", (H, W))):
            if m[name] is not None and (int(m[name].shape[0]) != n or tuple(m[name].shape[1:]) != tail):
                raise ValueError("%s: sequence %d: %s has shape %s, expected %s" % (who, i, name, tuple(m[name].shape), (n,) + tail))
        q_xy = as_t(sq["xy"], torch.float64).reshape(-1, 2).contiguous()
        q_t = as_t(sq["t"], torch.int32).reshape(-1).contiguous()
        if q_t.shape[0] != q_xy.shape[0]:
            raise ValueError("%s: sequence %d: %d positions for %d frames" % (who, i, q_xy.shape[0], q_t.shape[0]))
        s2 = {}
        if optimize:   # the stride-2 stacks: (n-1,H,W,2) and (n-1,H,W); empty (one flow) goes as NULL; the library refuses what does not fit
            for f2, o2 in _STRIDE2:
                for name, dt, tail in ((f2, torch.float32, (H, W, 2)), (o2, torch.uint8, (H, W))):
                    a = sq.get(name)
                    if a is None:
                        s2[name] = None
                        continue
                    a = _as_device_stack(a, dt, (1, 1, 2) if len(tail) == 3 else (1, 1))
                    if int(a.shape[0]) != n - 1 or (a.numel() > 0 and tuple(a.shape[1:]) != tail):
                        raise ValueError("%s: sequence %d: %s has shape %s, expected %s" % (who, i, name, tuple(a.shape), (n - 1,) + tail))
                    s2[name] = a if a.numel() > 0 else None
        prepared.append((m, n, H, W, q_xy, q_t, s2))
    groups = _query_batch_groups([int(p[4].shape[0]) for p in prepared])
    if return_device and len(groups) > 1:
        raise ValueError("%s: return_device needs at most %d sequences and fewer than 2^28 queries (one call)" % (who, QUERY_BATCH_MAX_SEQ))
    vp = ctypes.c_void_p
    results = []
    for g0, g1 in groups:
        B = g1 - g0
        ctxs = _hip.batch_contexts(B)
        handles = (vp * B)(*[c.handle for c in ctxs])
        ff, of, fb, ob, qx, qt = ((vp * B)() for _ in range(6))
        nf, hh, ww, nq = (ctypes.c_int * B)(), (ctypes.c_int * B)(), (ctypes.c_int * B)(), (ctypes.c_int64 * B)()
        f2, o2, b2, p2 = ((vp * B)() for _ in range(4))
        for k, (m, n, H, W, q_xy, q_t, s2) in enumerate(prepared[g0:g1]):
            for arr, name in ((f2, "flows_f2"), (o2, "occ_f2"), (b2, "flows_b2"), (p2, "occ_b2")):
                if s2.get(name) is not None:
                    arr[k] = s2[name].data_ptr()
            if dirs0[0]:
                ff[k], of[k] = m["flows"].data_ptr(), m["occ"].data_ptr()
            if dirs0[1]:
                fb[k], ob[k] = m["flows_b"].data_ptr(), m["occ_b"].data_ptr()
            nf[k], hh[k], ww[k], nq[k] = n, H, W, int(q_xy.shape[0])
            if nq[k] > 0:
                qx[k], qt[k] = q_xy.data_ptr(), q_t.data_ptr()
        infos = (_hip.TrackInfo * B)()

        def given(d, name):     # a stride-2 array goes with its direction, or when some sequence brings an entry for it
            return dirs0[d] or any(p[6].get(name) is not None for p in prepared[g0:g1])
        try:
            if mb_list is not None:
                for c, v in zip(ctxs, mb_list[g0:g1]):
                    c.set_motion_boundary(True, v)
            if optimize:
                st = _hip.lib().psfm_track_queries_optimize_batch(
                    handles, B, ff if dirs0[0] else None, of if dirs0[0] else None, f2 if given(0, "flows_f2") else None,
                    o2 if given(0, "occ_f2") else None, fb if dirs0[1] else None, ob if dirs0[1] else None,
                    b2 if given(1, "flows_b2") else None, p2 if given(1, "occ_b2") else None,
                    nf, hh, ww, qx, qt, nq, infos, _hip.current_stream_ptr(ctxs[0].device))
            else:
                st = _hip.lib().psfm_track_queries_batch(handles, B, ff if dirs0[0] else None, of if dirs0[0] else None, fb if dirs0[1] else None,
                                                         ob if dirs0[1] else None, nf, hh, ww, qx, qt, nq, infos,
                                                         _hip.current_stream_ptr(ctxs[0].device))
        finally:
            if mb_list is not None:      # (the option is per context and the thread's batch contexts are reused: off again, whatever happened)
                for c in ctxs:
                    c.set_motion_boundary(False)
        _hip.check(st)
        if return_device:
            return ctxs, [infos[k] for k in range(B)]
        results.extend(_result_to_host(c, infos[k]) for k, c in enumerate(ctxs))
    return results


def run_connect_queries_batch(seqs, thres=1.0, direction="forward", motion_boundary=False, mb_thres=0.02, return_device=False):
    """flow_check + run_track_queries_batch: seqs are dicts with `xy`, `t`, `flows_f` and `flows_b` ((n,H,W,2), flows_b[f]: frame f+1
    -> f); the occlusion maps each direction needs come from flow_check_device in that direction's own orientation, as in
    run_connect_queries -- forward: flow_check(flows_f, flows_b); backward: flow_check(flows_b, flows_f).  direction: "forward",
    "backward" or "both", for the whole batch.  Path consistency for a batch of sequences is out of scope: a sequence that comes with
    flows_f2 / flows_b2 is a ValueError; use run_connect_queries for it."""
    import torch
    from .utils import flow_check_device
    if direction not in ("forward", "backward", "both"):
        raise ValueError("connect_queries_batch: direction must be 'forward', 'backward' or 'both'")
    out = []
    for i, sq in enumerate(seqs):
        if sq.get("flows_f2") is not None or sq.get("flows_b2") is not None:
            raise ValueError("connect_queries_batch: sequence %d comes with stride-2 stacks; path consistency for a batch of sequences "
                             "is out of scope, use run_connect_queries (run_track_queries) for it" % i)
        ff = _as_device_stack(sq["flows_f"], torch.float32, (1, 1, 2))
        fb = _as_device_stack(sq["flows_b"], torch.float32, (1, 1, 2))
        n = min(int(ff.shape[0]), int(fb.shape[0]))
        ff, fb = ff[:n], fb[:n]
        kw = dict(xy=sq["xy"], t=sq["t"])
        if direction in ("forward", "both"):
            kw.update(flows=ff, occ=flow_check_device(ff, fb, thres)[1])
        if direction in ("backward", "both"):
            kw.update(flows_b=fb, occ_b=flow_check_device(fb, ff, thres)[1])
        out.append(kw)
    return run_track_queries_batch(out, motion_boundary=motion_boundary, mb_thres=mb_thres, return_device=return_device)


def run_track_queries_pc_batch(seqs, motion_boundary=False, mb_thres=0.02, return_device=False):
    """run_track_queries WITH the stride-2 path-consistency solve for a LIST of sequences, in one psfm_track_queries_optimize_batch call
    per group of at most 64 sequences (and fewer than 2^28 queries): per step ONE set of launches covers every sequence -- the step,
    the row scan, the rows, the multi-problem solve (one grid over all sequences' solves), one poll with one synchronisation, the
    write-back -- so a directory of small videos pays the fixed cost of a frame once.  seqs: the dicts of run_track_queries_batch plus
    the stride-2 keys of run_track_queries: `flows_f2`, `occ_f2` (with `flows`, `occ`) and / or `flows_b2`, `occ_b2` (with `flows_b`,
    `occ_b`), (n-1,H,W,2) and (n-1,H,W); a sequence of one flow may leave them out or give empty stacks.  Each sequence keeps its own
    frame size, length and query count.  Sequence i's result -- births, lengths, offsets, positions, solve statistics -- is that of
    run_track_queries(... stride-2 ...) on it alone; R.info["chain_mode"] is 7, R.info["n_solves"] and ["solver_iterations"] are the
    sequence's own.  motion_boundary / mb_thres, return_device and the refusals: as run_track_queries_batch, and a direction whose
    stride-1 stack lacks its stride-2 stack in a sequence of two or more flows is refused by the library (PsfmError, naming the
    sequence)."""
    return _track_queries_batch(seqs, motion_boundary, mb_thres, return_device, True)


def run_connect_queries_pc_batch(seqs, thres=1.0, direction="forward", motion_boundary=False, mb_thres=0.02, return_device=False):
    """flow_check + run_track_queries_pc_batch: seqs are dicts with `xy`, `t`, `flows_f`, `flows_b` ((n,H,W,2), flows_b[f]: frame f+1 ->
    f) and `flows_f2`, `flows_b2` ((n-1,H,W,2), flows_b2[f]: frame f+2 -> f).  Each direction's stride-1 and stride-2 occlusion maps
    come from flow_check_device in that direction's orientation, as in run_connect_queries -- forward: flow_check(flows_f, flows_b)
    and flow_check(flows_f2, flows_b2); backward: flow_check(flows_b, flows_f) and flow_check(flows_b2, flows_f2).  direction:
    "forward", "backward" or "both", for the whole batch."""
    import torch
    from .utils import flow_check_device
    if direction not in ("forward", "backward", "both"):
        raise ValueError("connect_queries_pc_batch: direction must be 'forward', 'backward' or 'both'")
    out = []
    for i, sq in enumerate(seqs):
        ff = _as_device_stack(sq["flows_f"], torch.float32, (1, 1, 2))
        fb = _as_device_stack(sq["flows_b"], torch.float32, (1, 1, 2))
        n = min(int(ff.shape[0]), int(fb.shape[0]))
        ff, fb = ff[:n], fb[:n]
        f2 = b2 = None
        if n > 1:
            if sq.get("flows_f2") is None or sq.get("flows_b2") is None:
                raise ValueError("connect_queries_pc_batch: sequence %d: the stride-2 maps of either direction need both stride-2 stacks" % i)
            f2 = _as_device_stack(sq["flows_f2"], torch.float32, (1, 1, 2))[:n - 1]
            b2 = _as_device_stack(sq["flows_b2"], torch.float32, (1, 1, 2))[:n - 1]
            if int(f2.shape[0]) != n - 1 or int(b2.shape[0]) != n - 1:
                raise ValueError("connect_queries_pc_batch: sequence %d: need %d stride-2 flows per direction" % (i, n - 1))
        kw = dict(xy=sq["xy"], t=sq["t"])
        if direction in ("forward", "both"):
            kw.update(flows=ff, occ=flow_check_device(ff, fb, thres)[1])
            if f2 is not None:
                kw.update(flows_f2=f2, occ_f2=flow_check_device(f2, b2, thres)[1])
        if direction in ("backward", "both"):
            kw.update(flows_b=fb, occ_b=flow_check_device(fb, ff, thres)[1])
            if f2 is not None:
                kw.update(flows_b2=b2, occ_b2=flow_check_device(b2, f2, thres)[1])
        out.append(kw)
    return run_track_queries_pc_batch(out, motion_boundary=motion_boundary, mb_thres=mb_thres, return_device=return_device)
