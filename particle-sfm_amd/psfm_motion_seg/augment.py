"""The motion classifier's 10-channel input on the device: traj_oa_depth.augment_traj of the reference
(motion_seg/core/network/traj_oa_depth.py:72-114 -- image_grid, depth_project, gather_point, augment_traj) behind the host glue of
motion_seg/main_motion_segmentation.py:71-78 (ToTensor, .float(), permutes), as ONE launch of csrc/psfm_augment.hip.

It consumes the f64 window tensors exactly as `sample_window_device` returns them plus the depth maps at the network input size,
and returns the reference's [1,10,K,L] fp32 tensor bit for bit: channels 0-1 the normalised coordinates, 2-3 their frame-to-frame
motion, 4-6 the back-projected 3-D point under the trajectory, 7-9 its motion.  The reference's [B,3,H,W,L] point cloud is never
built.  There is no CPU fallback: without a HIP device every entry point raises RuntimeError.
"""
import numpy as np

PLANES = 10


def reference_kinv(input_hw):
    """K^-1 as image_grid builds it (traj_oa_depth.py:78-82): fx = fy = (h+w)/2, cx = w/2, cy = h/2, np.linalg.inv in f64, cast to
    f32.  (3,3) float32."""
    h, w = input_hw[0], input_hw[1]
    fx, fy = (h + w) / 2.0, (h + w) / 2.0
    cx, cy = w / 2.0, h / 2.0
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]])
    return np.linalg.inv(K).astype(np.float32)


def _depth_stack(depth, n_frames, h, w, dev):
    """A list of L (h,w) maps, an (L,h,w) tensor or the reference's (1,1,h,w,L) tensor -> (L,h,w) f32, contiguous, on `dev`
    (f64 is rounded with .float(), as main_motion_segmentation.py:73 does)."""
    import torch
    if isinstance(depth, (list, tuple)):
        depth = torch.stack([torch.as_tensor(np.asarray(d) if not torch.is_tensor(d) else d) for d in depth], 0)
    elif not torch.is_tensor(depth):
        depth = torch.as_tensor(np.asarray(depth))
    if depth.dim() == 5:
        if tuple(depth.shape[:2]) != (1, 1):
            raise ValueError("augment_traj_device: a 5-d depth tensor must be (1,1,h,w,L), got %s" % (tuple(depth.shape),))
        depth = depth[0, 0].permute(2, 0, 1)
    if tuple(depth.shape) != (n_frames, h, w):
        raise ValueError("augment_traj_device: depth is %s, the window needs (%d,%d,%d)" % (tuple(depth.shape), n_frames, h, w))
    if not depth.is_floating_point():
        raise ValueError("augment_traj_device: depth must be a floating-point tensor")
    return depth.to(dev).float().contiguous()


def augment_traj_device(xy_norm, mask_absent, depth, input_hw, kinv=None, ctx=None):
    """xy_norm (K,L,2) and mask_absent (K,L,1) or (K,L) as sample_window_device returns them (f32 inputs are widened exactly),
    depth as `_depth_stack` takes it, input_hw = the network input size (h,w), kinv (3,3) (default reference_kinv(input_hw)).
    Returns the (1,10,K,L) f32 device tensor of traj_oa_depth.augment_traj.  Asynchronous: one launch on the current stream."""
    import torch
    from point_trajectory import _hip
    ctx = ctx or _hip.context()                       # (no device: RuntimeError)
    dev = torch.device("cuda", ctx.device)
    h, w = int(input_hw[0]), int(input_hw[1])
    xy_norm, mask_absent = torch.as_tensor(xy_norm), torch.as_tensor(mask_absent)
    if xy_norm.dim() != 3 or xy_norm.shape[2] != 2:
        raise ValueError("augment_traj_device: xy_norm must be (K,L,2), got %s" % (tuple(xy_norm.shape),))
    K, L = int(xy_norm.shape[0]), int(xy_norm.shape[1])
    if tuple(mask_absent.shape) not in ((K, L), (K, L, 1)):
        raise ValueError("augment_traj_device: mask_absent must be (K,L) or (K,L,1), got %s" % (tuple(mask_absent.shape),))
    xy = xy_norm.to(dev).double().contiguous()
    mask = mask_absent.to(dev).double().contiguous()
    dep = _depth_stack(depth, L, h, w, dev)
    kinv = np.ascontiguousarray(reference_kinv((h, w)) if kinv is None else np.asarray(kinv, np.float32).reshape(3, 3))
    out = torch.empty((1, PLANES, K, L), dtype=torch.float32, device=dev)
    _hip.check(_hip.lib().psfm_traj_augment(ctx.handle, _hip.ptr(xy), _hip.ptr(mask), _hip.ptr(dep), K, L, h, w,
                                            kinv.ctypes.data, _hip.ptr(out), _hip.current_stream_ptr(ctx.device)))
    return out


def augment_windows_device(nors, masks, depths, input_hw, kinv=None, ctx=None):
    """augment_traj_device for a list of windows of ONE n_frames through psfm_traj_augment_batch: one launch per call of at most 64
    windows (longer lists are split).  nors[b] (K_b,L,2), masks[b] (K_b,L,1) or (K_b,L) as sample_windows_device returns them,
    depths[b] as `_depth_stack` takes it.  Returns a list of (1,10,K_b,L) f32 views of one buffer, each bit-identical to
    augment_traj_device on that window alone.  Asynchronous on the current stream."""
    import ctypes
    import torch
    from point_trajectory import _hip
    from .load_cut_seq import BATCH_MAX
    ctx = ctx or _hip.context()                       # (no device: RuntimeError)
    dev = torch.device("cuda", ctx.device)
    h, w = int(input_hw[0]), int(input_hw[1])
    if not (len(nors) == len(masks) == len(depths)):
        raise ValueError("augment_windows_device: %d, %d and %d windows" % (len(nors), len(masks), len(depths)))
    xys, mks, deps = [], [], []
    for b, (xy_norm, mask_absent, depth) in enumerate(zip(nors, masks, depths)):
        xy_norm, mask_absent = torch.as_tensor(xy_norm), torch.as_tensor(mask_absent)
        if xy_norm.dim() != 3 or xy_norm.shape[2] != 2:
            raise ValueError("augment_windows_device: window %d: xy_norm must be (K,L,2), got %s" % (b, tuple(xy_norm.shape)))
        K, L = int(xy_norm.shape[0]), int(xy_norm.shape[1])
        if tuple(mask_absent.shape) not in ((K, L), (K, L, 1)):
            raise ValueError("augment_windows_device: window %d: mask_absent must be (K,L) or (K,L,1), got %s" % (b, tuple(mask_absent.shape)))
        if xys and L != int(xys[0].shape[1]):
            raise ValueError("augment_windows_device: the windows of one call must have one L, got %d and %d" % (int(xys[0].shape[1]), L))
        xys.append(xy_norm.to(dev).double().contiguous())
        mks.append(mask_absent.to(dev).double().contiguous())
        deps.append(_depth_stack(depth, L, h, w, dev))
    kinv = np.ascontiguousarray(reference_kinv((h, w)) if kinv is None else np.asarray(kinv, np.float32).reshape(3, 3))
    lib, vp, out = _hip.lib(), ctypes.c_void_p, []
    for lo in range(0, len(xys), BATCH_MAX):
        part = xys[lo:lo + BATCH_MAX]
        n, L = len(part), int(part[0].shape[1])
        ks = [int(x.shape[0]) for x in part]
        buf = torch.empty((PLANES * sum(ks) * L,), dtype=torch.float32, device=dev)        # one allocation; the windows are views of it
        views, at = [], 0
        for kb in ks:
            views.append(buf[at:at + PLANES * kb * L].view(1, PLANES, kb, L))
            at += PLANES * kb * L
        col = lambda ts: (vp * n)(*[t.data_ptr() if t.numel() else None for t in ts])
        _hip.check(lib.psfm_traj_augment_batch(ctx.handle, n, col(part), col(mks[lo:lo + n]), col(deps[lo:lo + n]), (ctypes.c_int64 * n)(*ks),
                                               L, h, w, kinv.ctypes.data, col(views), _hip.current_stream_ptr(ctx.device)))
        out += views
    return out


def window_features(ctx, frame0, n_frames, raw_hw, input_size, depth, traj_max_num=100000, min_length=3, traj_min_len=3, seed=0,
                    kinv=None):
    """One window from the result the last psfm_track / psfm_connect left in `ctx` to the classifier's input, on the current
    stream: sample_window_device, then augment_traj_device on its tensors.  depth: the window's maps at `input_size`.
    Returns (ids (K,) i32, raw (K,L,2) f64, mask_absent (K,L,1) f64, features (1,10,K,L) f32)."""
    from .load_cut_seq import sample_window_device
    ids, raw, nor, mask = sample_window_device(ctx, frame0, n_frames, raw_hw, input_size, traj_max_num, min_length, traj_min_len, seed)
    return ids, raw, mask, augment_traj_device(nor, mask, depth, input_size, kinv=kinv, ctx=ctx)
