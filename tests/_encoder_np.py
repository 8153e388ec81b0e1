"""f64 NumPy restatement of the classifier's trajectory transformer, traj_oa_depth.joint_encoder = pt_transformer.forward
(motion_seg/core/network/traj_oa_depth.py:25-60) in eval mode: what psfm_traj_encode implements in fp32.  tests/golden/
make_encoder_golden.py asserts that it equals the reference module's own .double() output to 1e-12, and tests/test_encoder_host.py
pins it to the stored vectors again.  Three switches state the plausible misreadings of the reference; the generator asserts that
each of them misses the tolerance by at least 100x on every fixture, so the fixtures pin these points:
  mask_memory     cross-attention masks the padded memory positions     (the reference passes no memory_key_padding_mask)
  max_valid_only  the final max runs over the valid tokens only         (the reference takes it over all L)
  zero_padded     padded positions of the memory and of the decoder output are zeroed (torch's nested-tensor fast path, which
                  batch_first=False never takes)"""
import os

import numpy as np

from psfm_motion_seg.encoder import ENCODER_KEYS, WEIGHT_COUNT

ENCODER_CASES = ["augment_48x64_t23_w0", "augment_48x64_t23_w2", "augment_24x32_t27_full", "augment_synth_37x53"]   # the inputs
WEIGHTS_FIXTURE = "encoder_weights"                      # the 68 arrays by packed key, `e` and `tol`
CHUNK = 4096
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def encoder_fixture(name):
    return np.load(os.path.join(GOLDEN, "encoder_" + name + ".npz"))


def fixture_weights():
    """(dict key -> array in the checkpoint's shapes, tol)."""
    g = np.load(os.path.join(GOLDEN, WEIGHTS_FIXTURE + ".npz"))
    return {k: g[k] for k, _ in ENCODER_KEYS}, float(g["tol"])


def unpack(packed):
    packed = np.asarray(packed).reshape(-1)
    assert packed.size == WEIGHT_COUNT
    out, o = {}, 0
    for k, s in ENCODER_KEYS:
        n = int(np.prod(s))
        out[k] = packed[o:o + n].reshape(s)
        o += n
    return out


def pad_bits(mask_absent, K, L):
    """extract_feature (:47): (pad_mask.reshape(-1, L) > 0.5) on the .float() mask."""
    return np.asarray(mask_absent).astype(np.float32).reshape(K, L) > np.float32(0.5)


def _ln(v, W, p):
    mu = v.mean(-1, keepdims=True)
    var = ((v - mu) ** 2).mean(-1, keepdims=True)                  # biased
    return (v - mu) / np.sqrt(var + 1e-5) * W[p + "weight"] + W[p + "bias"]


def _lin(a, Wm, b):
    """a (K,L,n) -> (K,L,m) through one 2-D product."""
    return (a.reshape(-1, a.shape[-1]) @ Wm.T + b).reshape(a.shape[:-1] + (Wm.shape[0],))


def _mha(q_src, kv_src, W, p, key_pad):
    """nn.MultiheadAttention, 4 heads of width 4; key_pad (K,L) bool or None.  (K,L,16) -> (K,L,16)."""
    Wi, bi = W[p + "in_proj_weight"], W[p + "in_proj_bias"]
    K, L, _ = q_src.shape
    q = _lin(q_src, Wi[:16], bi[:16]) * 0.5                        # 1 / sqrt(head width 4)
    kv = _lin(kv_src, Wi[16:], bi[16:])
    q, k, v = (a.reshape(K, L, 4, 4).transpose(0, 2, 1, 3) for a in (q, kv[..., :16], kv[..., 16:]))       # (K,head,L,4)
    s = q @ k.transpose(0, 1, 3, 2)                                # (K,head,i,j)
    if key_pad is not None:
        s = np.where(key_pad[:, None, None, :], -np.inf, s)
    with np.errstate(all="ignore"):                                # (a row with every key padded: NaN, unspecified)
        s = np.exp(s - s.max(-1, keepdims=True))
        s = s / s.sum(-1, keepdims=True)
    o = (s @ v).transpose(0, 2, 1, 3).reshape(K, L, 16)
    return _lin(o, W[p + "out_proj.weight"], W[p + "out_proj.bias"])


def _ffn(h, W, p):
    return _lin(np.maximum(_lin(h, W[p + "linear1.weight"], W[p + "linear1.bias"]), 0.0), W[p + "linear2.weight"], W[p + "linear2.bias"])


def encoder_np(features, mask_absent, weights, mask_memory=False, max_valid_only=False, zero_padded=False):
    """features (10,K,L) or (1,10,K,L), mask_absent (K,L) or (K,L,1), weights: dict by key or the packed array -> (16,K) f64."""
    W = weights if isinstance(weights, dict) else unpack(weights)
    W = {k: np.asarray(v, np.float64) for k, v in W.items()}
    f = np.asarray(features, np.float64)
    f = f[0] if f.ndim == 4 else f
    _, K, L = f.shape
    if K > CHUNK:                                                  # trajectories are independent: bounded temporaries, a few threads
        from concurrent.futures import ThreadPoolExecutor
        m = np.asarray(mask_absent).reshape(K, L)
        with ThreadPoolExecutor(max_workers=8) as ex:
            parts = ex.map(lambda a: encoder_np(f[:, a:a + CHUNK], m[a:a + CHUNK], W, mask_memory, max_valid_only, zero_padded),
                           range(0, K, CHUNK))
            return np.concatenate(list(parts), 1)
    pad = pad_bits(mask_absent, K, L)
    t = "transformer_model."
    x = np.maximum(_lin(np.ascontiguousarray(np.moveaxis(f, 0, 2)), W["input_fc1.weight"].reshape(16, 10), W["input_fc1.bias"]), 0.0)     # project (:37-40)
    x = np.maximum(_lin(x, W["fc2.weight"].reshape(16, 16), W["fc2.bias"]), 0.0)
    h = x
    for i in range(2):                                             # post-norm encoder layers
        p = "%sencoder.layers.%d." % (t, i)
        h = _ln(h + _mha(h, h, W, p + "self_attn.", pad), W, p + "norm1.")
        h = _ln(h + _ffn(h, W, p), W, p + "norm2.")
    mem = _ln(h, W, t + "encoder.norm.")
    if zero_padded:
        mem = np.where(pad[:, :, None], 0.0, mem)
    d = x                                                          # the reference passes the same tensor as src and tgt (:48)
    for i in range(2):
        p = "%sdecoder.layers.%d." % (t, i)
        d = _ln(d + _mha(d, d, W, p + "self_attn.", pad), W, p + "norm1.")
        d = _ln(d + _mha(d, mem, W, p + "multihead_attn.", pad if mask_memory else None), W, p + "norm2.")
        d = _ln(d + _ffn(d, W, p), W, p + "norm3.")
    d = _ln(d, W, t + "decoder.norm.")
    if zero_padded:
        d = np.where(pad[:, :, None], 0.0, d)
    if max_valid_only:
        d = np.where(pad[:, :, None], -np.inf, d)
    return d.max(1).T.copy()                                       # max over all L tokens (:51), [16,K] (:60)


def seeded_encoder_inputs(K, L, seed, min_valid=1):
    """Features N(0,1) per channel scaled like the augment planes (coordinates in [0,1], small motions), 30 % padded slots, every
    row with at least `min_valid` valid tokens.  features (10,K,L) f32, mask_absent (K,L,1) f64."""
    rng = np.random.default_rng(seed)
    mask = rng.uniform(size=(K, L)) < 0.3
    for k in np.flatnonzero((~mask).sum(1) < min_valid):
        mask[k, rng.choice(L, size=min_valid, replace=False)] = False
    f = rng.normal(size=(10, K, L)) * np.array([0.3, 0.3, 0.05, 0.05, 0.3, 0.3, 0.5, 0.05, 0.05, 0.05])[:, None, None]
    f[:2] = np.clip(f[:2] + 0.5, 0.0, 1.0) * ~mask
    return f.astype(np.float32), mask.astype(np.float64)[:, :, None]
