"""The motion classifier's trajectory transformer on the device: traj_oa_depth.joint_encoder of the reference
(pt_transformer.forward, motion_seg/core/network/traj_oa_depth.py:25-60, eval mode) as ONE launch of csrc/psfm_encoder.hip behind
psfm_traj_augment: two 1x1 convolutions (10 -> 16 -> 16, ReLU), nn.Transformer(d_model 16, 4 heads, 2 encoder + 2 decoder layers,
feed-forward 64) over each trajectory's L tokens, and the max over the tokens.

It consumes the [1,10,K,L] fp32 tensor exactly as `augment_traj_device` returns it and the f64 mask_absent exactly as
`sample_window_device` returns it, and returns the (1,16,K) fp32 tensor the reference hands to its OANet decoder as
`feat.unsqueeze(-1)`.  fp32 throughout, 1 <= L <= 64.  The OANet decoder and the sigmoid stay with the caller.  There is no CPU
fallback: without a HIP device every entry point that computes raises RuntimeError.
"""
import numpy as np

D_MODEL, N_IN, N_FF, MAX_FRAMES = 16, 10, 64, 64


def _attention(p):
    return [(p + "in_proj_weight", (48, 16)), (p + "in_proj_bias", (48,)), (p + "out_proj.weight", (16, 16)), (p + "out_proj.bias", (16,))]


def _feed_forward(p):
    return [(p + "linear1.weight", (64, 16)), (p + "linear1.bias", (64,)), (p + "linear2.weight", (16, 64)), (p + "linear2.bias", (16,))]


def _norm(p):
    return [(p + "weight", (16,)), (p + "bias", (16,))]


def _keys():
    t = "transformer_model."
    keys = [("input_fc1.weight", (16, 10, 1, 1)), ("input_fc1.bias", (16,)), ("fc2.weight", (16, 16, 1, 1)), ("fc2.bias", (16,))]
    for i in range(2):
        p = "%sencoder.layers.%d." % (t, i)
        keys += _attention(p + "self_attn.") + _feed_forward(p) + _norm(p + "norm1.") + _norm(p + "norm2.")
    keys += _norm(t + "encoder.norm.")
    for i in range(2):
        p = "%sdecoder.layers.%d." % (t, i)
        keys += (_attention(p + "self_attn.") + _attention(p + "multihead_attn.") + _feed_forward(p) + _norm(p + "norm1.")
                 + _norm(p + "norm2.") + _norm(p + "norm3."))
    return keys + _norm(t + "decoder.norm.")


# The packed order of include/psfm.h (psfm_traj_encode): the module's own state_dict order, every tensor row-major as stored.
ENCODER_KEYS = _keys()
WEIGHT_COUNT = sum(int(np.prod(s)) for _, s in ENCODER_KEYS)        # 15872


def pack_encoder_weights_host(state_dict, prefix="joint_encoder."):
    """The 68 tensors of pt_transformer in the reference's checkpoint layout -- keys with or without `prefix`, torch tensors or NumPy
    arrays -- checked for presence and shape and packed in ENCODER_KEYS order.  (WEIGHT_COUNT,) float32 NumPy array."""
    parts = []
    for key, shape in ENCODER_KEYS:
        if prefix + key in state_dict:
            v = state_dict[prefix + key]
        elif key in state_dict:
            v = state_dict[key]
        else:
            raise ValueError("pack_encoder_weights: missing key %r (looked for it with and without the prefix %r)" % (key, prefix))
        if hasattr(v, "detach"):
            v = v.detach().cpu().numpy()
        v = np.asarray(v)
        if tuple(v.shape) != shape:
            raise ValueError("pack_encoder_weights: %r has shape %s, expected %s" % (key, tuple(v.shape), shape))
        parts.append(v.astype(np.float32).reshape(-1))
    out = np.concatenate(parts)
    assert out.size == WEIGHT_COUNT
    return out


def pack_encoder_weights(state_dict, prefix="joint_encoder.", device=None):
    """pack_encoder_weights_host on the device: one (15872,) fp32 tensor, what psfm_traj_encode takes.  ValueError names a missing or
    mis-shaped key."""
    import torch
    host = pack_encoder_weights_host(state_dict, prefix)
    from point_trajectory import _hip
    ctx = _hip.context(device)                        # (no device: RuntimeError)
    assert _hip.lib().psfm_traj_encode_weight_count() == WEIGHT_COUNT
    return torch.from_numpy(host).to(torch.device("cuda", ctx.device))


def encode_traj_device(features, mask_absent, weights, ctx=None):
    """features (1,10,K,L) or (10,K,L) fp32 as augment_traj_device returns it, mask_absent (K,L,1) or (K,L) as sample_window_device
    returns it (f32 is widened exactly), weights from pack_encoder_weights.  Returns the (1,16,K) fp32 device tensor of
    traj_oa_depth.joint_encoder, ready for .unsqueeze(-1).  Asynchronous: one launch on the current stream."""
    import torch
    from point_trajectory import _hip
    ctx = ctx or _hip.context()                       # (no device: RuntimeError)
    dev = torch.device("cuda", ctx.device)
    features, mask_absent, weights = torch.as_tensor(features), torch.as_tensor(mask_absent), torch.as_tensor(weights)
    if features.dim() == 4 and features.shape[0] == 1:
        features = features[0]
    if features.dim() != 3 or features.shape[0] != N_IN:
        raise ValueError("encode_traj_device: features must be (1,10,K,L) or (10,K,L), got %s" % (tuple(features.shape),))
    K, L = int(features.shape[1]), int(features.shape[2])
    if tuple(mask_absent.shape) not in ((K, L), (K, L, 1)):
        raise ValueError("encode_traj_device: mask_absent must be (K,L) or (K,L,1), got %s" % (tuple(mask_absent.shape),))
    if not 1 <= L <= MAX_FRAMES:
        raise ValueError("encode_traj_device: L = %d, supported is 1 <= L <= %d (one trajectory inside one wave)" % (L, MAX_FRAMES))
    if weights.numel() != WEIGHT_COUNT:
        raise ValueError("encode_traj_device: weights has %d elements, pack_encoder_weights gives %d" % (weights.numel(), WEIGHT_COUNT))
    feat = features.to(dev).float().contiguous()
    mask = mask_absent.to(dev).double().contiguous()
    wts = weights.to(dev).float().contiguous()
    out = torch.empty((1, D_MODEL, K), dtype=torch.float32, device=dev)
    _hip.check(_hip.lib().psfm_traj_encode(ctx.handle, _hip.ptr(feat), _hip.ptr(mask), _hip.ptr(wts), K, L, _hip.ptr(out),
                                           _hip.current_stream_ptr(ctx.device)))
    return out


def encode_windows_device(feats, masks, weights, ctx=None):
    """encode_traj_device for a list of windows of ONE L through psfm_traj_encode_batch: one launch per call of at most 64 windows
    (longer lists are split).  feats[b] (1,10,K_b,L) or (10,K_b,L) fp32 as augment_windows_device returns them, masks[b] (K_b,L,1) or
    (K_b,L).  Returns a list of (1,16,K_b) fp32 contiguous views of one buffer -- what decode_windows_device takes -- each
    bit-identical to encode_traj_device on that window alone.  Asynchronous on the current stream."""
    import ctypes
    import torch
    from point_trajectory import _hip
    from .load_cut_seq import BATCH_MAX
    ctx = ctx or _hip.context()                       # (no device: RuntimeError)
    dev = torch.device("cuda", ctx.device)
    weights = torch.as_tensor(weights)
    if weights.numel() != WEIGHT_COUNT:
        raise ValueError("encode_windows_device: weights has %d elements, pack_encoder_weights gives %d" % (weights.numel(), WEIGHT_COUNT))
    if len(feats) != len(masks):
        raise ValueError("encode_windows_device: %d feature tensors, %d masks" % (len(feats), len(masks)))
    fts, mks = [], []
    for b, (features, mask_absent) in enumerate(zip(feats, masks)):
        features, mask_absent = torch.as_tensor(features), torch.as_tensor(mask_absent)
        if features.dim() == 4 and features.shape[0] == 1:
            features = features[0]
        if features.dim() != 3 or features.shape[0] != N_IN:
            raise ValueError("encode_windows_device: window %d: features must be (1,10,K,L) or (10,K,L), got %s" % (b, tuple(features.shape)))
        K, L = int(features.shape[1]), int(features.shape[2])
        if tuple(mask_absent.shape) not in ((K, L), (K, L, 1)):
            raise ValueError("encode_windows_device: window %d: mask_absent must be (K,L) or (K,L,1), got %s" % (b, tuple(mask_absent.shape)))
        if not 1 <= L <= MAX_FRAMES:
            raise ValueError("encode_windows_device: L = %d, supported is 1 <= L <= %d (one trajectory inside one wave)" % (L, MAX_FRAMES))
        if fts and L != int(fts[0].shape[2]):
            raise ValueError("encode_windows_device: the windows of one call must have one L, got %d and %d" % (int(fts[0].shape[2]), L))
        fts.append(features.to(dev).float().contiguous())
        mks.append(mask_absent.to(dev).double().contiguous())
    wts = weights.to(dev).float().contiguous()
    lib, vp, out = _hip.lib(), ctypes.c_void_p, []
    for lo in range(0, len(fts), BATCH_MAX):
        part = fts[lo:lo + BATCH_MAX]
        n, L = len(part), int(part[0].shape[2])
        ks = [int(f.shape[1]) for f in part]
        buf = torch.empty((D_MODEL * sum(ks),), dtype=torch.float32, device=dev)            # one allocation; the windows are views of it
        views, at = [], 0
        for kb in ks:
            views.append(buf[at:at + D_MODEL * kb].view(1, D_MODEL, kb))
            at += D_MODEL * kb
        col = lambda ts: (vp * n)(*[t.data_ptr() if t.numel() else None for t in ts])
        _hip.check(lib.psfm_traj_encode_batch(ctx.handle, n, col(part), col(mks[lo:lo + n]), _hip.ptr(wts), (ctypes.c_int64 * n)(*ks), L,
                                              col(views), _hip.current_stream_ptr(ctx.device)))
        out += views
    return out


def window_encoding(ctx, frame0, n_frames, raw_hw, input_size, depth, weights, traj_max_num=100000, min_length=3, traj_min_len=3,
                    seed=0, kinv=None):
    """One window from the result the last psfm_track / psfm_connect left in `ctx` to the encoder's output, on the current stream:
    window_features, then encode_traj_device on its tensors.
    Returns (ids (K,) i32, raw (K,L,2) f64, mask_absent (K,L,1) f64, features (1,10,K,L) f32, encoding (1,16,K) f32)."""
    from .augment import window_features
    ids, raw, mask, feat = window_features(ctx, frame0, n_frames, raw_hw, input_size, depth, traj_max_num, min_length, traj_min_len,
                                           seed, kinv=kinv)
    return ids, raw, mask, feat, encode_traj_device(feat, mask, weights, ctx=ctx)
