"""The motion classifier's OANet decoder on the device: traj_oa_depth.decoder of the reference (OANBlock(128, 16, depth 8, 100
clusters), motion_seg/core/network/oanet.py:13-206, eval mode), torch.sigmoid and the `> 0.5` of
motion_seg/main_motion_segmentation.py:80 as a fixed sequence of launches of csrc/psfm_decoder.hip behind psfm_traj_encode.

It consumes the (1,16,K) fp32 tensor exactly as `encode_traj_device` returns it and returns the logits, the probabilities and the
(K,) bool prediction that merge_labels.LabelMerger.add_window takes: with `device_predictor` the whole labelled set of
main_motion_segmentation.py:69-112 comes from device code, no torch module in the loop.  fp32 throughout (the products run on the
exact fp32 MFMA).  K = 1 is refused as the reference refuses it (InstanceNorm2d needs more than one point).  There is no CPU
fallback: without a HIP device every entry point that computes raises RuntimeError.
"""
import numpy as np

CHANNELS, D_IN, CLUSTERS = 128, 16, 100


def _bn(p, n):
    return [(p + "weight", (n,)), (p + "bias", (n,)), (p + "running_mean", (n,)), (p + "running_var", (n,))]


def _conv(p, out, cin):
    return [(p + "weight", (out, cin, 1, 1)), (p + "bias", (out,))]


def _point_cn(p, cin=CHANNELS, out=CHANNELS):
    keys = _conv(p + "shot_cut.", out, cin) if cin != out else []
    return keys + _bn(p + "conv.1.", cin) + _conv(p + "conv.3.", out, cin) + _bn(p + "conv.5.", out) + _conv(p + "conv.7.", out, out)


def _oa_filter(p):
    return (_bn(p + "conv1.1.", CHANNELS) + _conv(p + "conv1.3.", CHANNELS, CHANNELS) + _bn(p + "conv2.0.", CLUSTERS)
            + _conv(p + "conv2.2.", CLUSTERS, CLUSTERS) + _bn(p + "conv3.2.", CHANNELS) + _conv(p + "conv3.4.", CHANNELS, CHANNELS))


def _pool(p):
    return _bn(p + "conv.1.", CHANNELS) + _conv(p + "conv.3.", CLUSTERS, CHANNELS)


def _keys():
    keys = _conv("conv1.", CHANNELS, D_IN) + _pool("down1.") + _pool("up1.")
    for i in range(4):
        keys += _point_cn("l1_1.%d." % i)
    keys += _point_cn("l1_2.0.", 2 * CHANNELS, CHANNELS)
    for i in range(1, 4):
        keys += _point_cn("l1_2.%d." % i)
    for i in range(4):
        keys += _oa_filter("l2.%d." % i)
    return keys + _conv("output.", 1, CHANNELS)


# The packed order of include/psfm.h (psfm_traj_decode): the module's own state_dict order (OANBlock registers conv1, down1, up1, then
# the three Sequentials l1_1, l1_2, l2, then output) without the 30 num_batches_tracked, every tensor row-major as stored.
DECODER_KEYS = _keys()
WEIGHT_COUNT = sum(int(np.prod(s)) for _, s in DECODER_KEYS)        # 529497


def pack_decoder_weights_host(state_dict, prefix="decoder."):
    """The 186 float tensors of OANBlock in the reference's checkpoint layout -- keys with or without `prefix`, torch tensors or
    NumPy arrays -- checked for presence and shape and packed in DECODER_KEYS order.  (WEIGHT_COUNT,) float32 NumPy array."""
    parts = []
    for key, shape in DECODER_KEYS:
        if prefix + key in state_dict:
            v = state_dict[prefix + key]
        elif key in state_dict:
            v = state_dict[key]
        else:
            raise ValueError("pack_decoder_weights: missing key %r (looked for it with and without the prefix %r)" % (key, prefix))
        if hasattr(v, "detach"):
            v = v.detach().cpu().numpy()
        v = np.asarray(v)
        if tuple(v.shape) != shape:
            raise ValueError("pack_decoder_weights: %r has shape %s, expected %s" % (key, tuple(v.shape), shape))
        parts.append(v.astype(np.float32).reshape(-1))
    out = np.concatenate(parts)
    assert out.size == WEIGHT_COUNT
    return out


def pack_decoder_weights(state_dict, prefix="decoder.", device=None):
    """pack_decoder_weights_host on the device: one (529497,) fp32 tensor, what psfm_traj_decode takes (the kernels fold the
    BatchNorms themselves).  ValueError names a missing or mis-shaped key."""
    import torch
    host = pack_decoder_weights_host(state_dict, prefix)
    from point_trajectory import _hip
    ctx = _hip.context(device)                        # (no device: RuntimeError)
    assert _hip.lib().psfm_traj_decode_weight_count() == WEIGHT_COUNT
    return torch.from_numpy(host).to(torch.device("cuda", ctx.device))


_workspaces = {}


def _workspace(dev, need):
    import torch
    ws = _workspaces.get(dev)
    if ws is None or ws.numel() < need:
        ws = _workspaces[dev] = torch.empty((need,), dtype=torch.uint8, device=dev)
    return ws


def decode_traj_device(encoding, weights, ctx=None, workspace=None):
    """encoding (1,16,K) or (16,K) fp32 as encode_traj_device returns it, weights from pack_decoder_weights, workspace: a device
    tensor of at least psfm_traj_decode_workspace_bytes(K) bytes (default: one cached per device, grown on demand).
    Returns (logits (1,1,K) f32, prob (1,1,K) f32 = sigmoid(logits), pred (K,) bool = prob > 0.5) on the device.  Asynchronous: a
    fixed sequence of launches on the current stream."""
    import torch
    from point_trajectory import _hip
    ctx = ctx or _hip.context()                       # (no device: RuntimeError)
    dev = torch.device("cuda", ctx.device)
    encoding, weights = torch.as_tensor(encoding), torch.as_tensor(weights)
    if encoding.dim() == 3 and encoding.shape[0] == 1:
        encoding = encoding[0]
    if encoding.dim() != 2 or encoding.shape[0] != D_IN:
        raise ValueError("decode_traj_device: encoding must be (1,16,K) or (16,K), got %s" % (tuple(encoding.shape),))
    K = int(encoding.shape[1])
    if K == 1:
        raise ValueError("decode_traj_device: K = 1: the decoder's InstanceNorm2d needs more than one trajectory (the reference raises)")
    if weights.numel() != WEIGHT_COUNT:
        raise ValueError("decode_traj_device: weights has %d elements, pack_decoder_weights gives %d" % (weights.numel(), WEIGHT_COUNT))
    enc = encoding.to(dev).float().contiguous()
    wts = weights.to(dev).float().contiguous()
    L = _hip.lib()
    need = int(L.psfm_traj_decode_workspace_bytes(K))
    if workspace is None:
        workspace = _workspace(dev, need)
    elif not workspace.is_cuda or not workspace.is_contiguous() or workspace.numel() * workspace.element_size() < need:
        raise ValueError("decode_traj_device: workspace must be a contiguous device tensor of at least %d bytes" % need)
    logits = torch.empty((1, 1, K), dtype=torch.float32, device=dev)
    prob = torch.empty((1, 1, K), dtype=torch.float32, device=dev)
    pred = torch.empty((K,), dtype=torch.uint8, device=dev)
    _hip.check(L.psfm_traj_decode(ctx.handle, _hip.ptr(enc), _hip.ptr(wts), K, _hip.ptr(workspace),
                                  workspace.numel() * workspace.element_size(), _hip.ptr(logits), _hip.ptr(prob), _hip.ptr(pred),
                                  _hip.current_stream_ptr(ctx.device)))
    return logits, prob, pred.view(torch.bool)


def window_prediction(ctx, frame0, n_frames, raw_hw, input_size, depth, enc_weights, dec_weights, traj_max_num=100000, min_length=3,
                      traj_min_len=3, seed=0, kinv=None, workspace=None):
    """One window from the result the last psfm_track / psfm_connect left in `ctx` to the classifier's verdict, on the current stream:
    encoder.window_encoding, then decode_traj_device on its encoding.
    Returns (ids (K,) i32, raw (K,L,2) f64, mask_absent (K,L,1) f64, encoding (1,16,K) f32, logits (1,1,K), prob (1,1,K), pred (K,))."""
    from .encoder import window_encoding
    ids, raw, mask, _, enc = window_encoding(ctx, frame0, n_frames, raw_hw, input_size, depth, enc_weights, traj_max_num, min_length,
                                             traj_min_len, seed, kinv=kinv)
    logits, prob, pred = decode_traj_device(enc, dec_weights, ctx=ctx, workspace=workspace)
    return ids, raw, mask, enc, logits, prob, pred


def device_predictor(enc_weights, dec_weights, depth_for_window, input_size, kinv=None, ctx=None):
    """The `predict` callable of merge_labels.label_trajectories: (raw, normalised, mask_absent, time_idx) -> (K,) bool device
    tensor, True = dynamic, through augment_traj_device, encode_traj_device and decode_traj_device.  depth_for_window(time_idx)
    returns the window's depth maps at `input_size` (reading and resizing them stays with the caller)."""
    from .augment import augment_traj_device
    from .encoder import encode_traj_device

    def predict(raw, nor, mask, time_idx):
        feat = augment_traj_device(nor, mask, depth_for_window(time_idx), input_size, kinv=kinv, ctx=ctx)
        enc = encode_traj_device(feat, mask, enc_weights, ctx=ctx)
        return decode_traj_device(enc, dec_weights, ctx=ctx)[2]
    return predict


BATCH_MAX = 64                 # PSFM_DEC_BATCH_MAX of csrc/psfm_decoder_batch.h: windows per psfm_traj_decode_batch call


def decode_windows_device(encodings, weights, ctx=None, workspace=None):
    """decode_traj_device for a list of windows through psfm_traj_decode_batch: ONE sequence of launches per call of at most BATCH_MAX
    windows (longer lists are split) instead of one per window.  encodings: a list of (1,16,K_b) or (16,K_b) fp32 tensors, the K_b
    may differ and may be 0; workspace: a device tensor of at least psfm_traj_decode_batch_workspace_bytes bytes for every call
    (default: the one cached per device, grown on demand).  Returns a list of (logits (1,1,K_b), prob (1,1,K_b), pred (K_b,) bool),
    each bit-identical to decode_traj_device on that window alone.  Asynchronous on the current stream."""
    import ctypes
    import torch
    from point_trajectory import _hip
    ctx = ctx or _hip.context()                       # (no device: RuntimeError)
    dev = torch.device("cuda", ctx.device)
    weights = torch.as_tensor(weights)
    if weights.numel() != WEIGHT_COUNT:
        raise ValueError("decode_windows_device: weights has %d elements, pack_decoder_weights gives %d" % (weights.numel(), WEIGHT_COUNT))
    encs = []
    for b, e in enumerate(encodings):
        e = torch.as_tensor(e)
        if e.dim() == 3 and e.shape[0] == 1:
            e = e[0]
        if e.dim() != 2 or e.shape[0] != D_IN:
            raise ValueError("decode_windows_device: window %d: encoding must be (1,16,K) or (16,K), got %s" % (b, tuple(e.shape)))
        if int(e.shape[1]) == 1:
            raise ValueError("decode_windows_device: window %d: K = 1: the decoder's InstanceNorm2d needs more than one trajectory "
                             "(the reference raises)" % b)
        encs.append(e.to(dev).float().contiguous())
    wts = weights.to(dev).float().contiguous()
    L, vp = _hip.lib(), ctypes.c_void_p
    out = []
    for lo in range(0, len(encs), BATCH_MAX):
        part = encs[lo:lo + BATCH_MAX]
        n = len(part)
        ks = [int(e.shape[1]) for e in part]
        k = (ctypes.c_int64 * n)(*ks)
        need = int(L.psfm_traj_decode_batch_workspace_bytes(k, n))
        ws = workspace
        if ws is None:
            ws = _workspace(dev, need)
        elif not ws.is_cuda or not ws.is_contiguous() or ws.numel() * ws.element_size() < need:
            raise ValueError("decode_windows_device: workspace must be a contiguous device tensor of at least %d bytes" % need)
        # one allocation per output kind; the windows' tensors are views of it
        total = sum(ks)
        logits = torch.empty((total,), dtype=torch.float32, device=dev)
        prob = torch.empty((total,), dtype=torch.float32, device=dev)
        pred = torch.empty((total,), dtype=torch.uint8, device=dev)
        views, at = [], 0
        for kb in ks:
            views.append((logits[at:at + kb], prob[at:at + kb], pred[at:at + kb]))
            at += kb
        col = lambda ts: (vp * n)(*[t.data_ptr() if t.numel() else None for t in ts])
        _hip.check(L.psfm_traj_decode_batch(ctx.handle, n, col(part), k, _hip.ptr(wts), _hip.ptr(ws), ws.numel() * ws.element_size(),
                                            col([v[0] for v in views]), col([v[1] for v in views]), col([v[2] for v in views]),
                                            _hip.current_stream_ptr(ctx.device)))
        out += [(lo_.view(1, 1, -1), pr.view(1, 1, -1), pd.view(torch.bool)) for lo_, pr, pd in views]
    return out
