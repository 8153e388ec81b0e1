"""NumPy restatement of the classifier's input step (motion_seg/core/network/traj_oa_depth.py:72-114 behind the casts of
motion_seg/main_motion_segmentation.py:71-78): the unfused fp32 formula that psfm_traj_augment implements.  NumPy's float32 array
arithmetic rounds every operation on its own, which is what the reference's torch CPU ops do; tests/test_augment_host.py pins this
restatement to the fixtures the reference's own augment_traj produced, bit for bit."""
import numpy as np

AUGMENT_CASES = ["augment_48x64_t23_w0",       # (a) real windows of 10 over 23 frames: the first ...
                 "augment_48x64_t23_w2",       # ... and the last, which overlaps the one before it
                 "augment_24x32_t27_full",     # (b) window >= length: L = 27
                 "augment_synth_37x53"]        # (c) clipped ends, the clamp, 30 % padding


def pixel_index(traj32, h, w):
    """gather_point (:97-98): ((y*h).int() * w + (x*w).int()).clamp(0, h*w-1), and the unclamped value."""
    f32 = np.float32
    iy = (traj32[..., 1] * f32(h)).astype(np.int32)
    ix = (traj32[..., 0] * f32(w)).astype(np.int32)
    raw = iy.astype(np.int64) * w + ix
    return np.clip(raw, 0, h * w - 1), raw, ix


def augment_np(xy_norm, mask_absent, depth, input_hw, kinv):
    """xy_norm (K,L,2), mask_absent (K,L) or (K,L,1), depth (L,h,w), kinv (3,3) f32 -> (10,K,L) f32."""
    f32 = np.float32
    h, w = int(input_hw[0]), int(input_hw[1])
    t = np.asarray(xy_norm).astype(f32)
    m = np.asarray(mask_absent).astype(f32).reshape(t.shape[:2])
    d = np.asarray(depth).astype(f32)
    kinv = np.asarray(kinv, f32).reshape(3, 3)
    K, L = t.shape[:2]
    idx, _, _ = pixel_index(t, h, w)
    py, px = idx // w, idx % w
    dd = d.reshape(L, h * w)[np.arange(L)[None, :], idx]
    fx, fy = px.astype(f32), py.astype(f32)
    P = np.stack([dd * ((kinv[r, 0] * fx + kinv[r, 1] * fy) + kinv[r, 2]) for r in range(3)], 0)      # (3,K,L)
    v = np.concatenate([np.moveaxis(t, 2, 0), P], 0)                                                   # tx, ty, P0, P1, P2
    mo = np.zeros_like(v)
    mo[:, :, :-1] = (v[:, :, 1:] - v[:, :, :-1]) * (f32(1.0) - m[None, :, 1:])
    out = np.concatenate([v[:2], mo[:2], v[2:], mo[2:]], 0)
    assert out.dtype == f32 and out.shape == (10, K, L)
    return out


def edge_counts(xy_norm, mask_absent, input_hw):
    """(points with ix == w, indices clamped at h*w-1, padded slots followed by a present slot)."""
    h, w = int(input_hw[0]), int(input_hw[1])
    t = np.asarray(xy_norm).astype(np.float32)
    m = np.asarray(mask_absent).reshape(t.shape[:2])
    _, raw, ix = pixel_index(t, h, w)
    return int((ix == w).sum()), int((raw > h * w - 1).sum()), int(((m[:, :-1] == 1.0) & (m[:, 1:] == 0.0)).sum())


def seeded_inputs(K, L, input_hw, seed):
    """Case (c)'s recipe at any size: coordinates clip(U(-0.05,1.05), 0, 1) * (1 - mask), 30 % padded, depth iid U[0,1)."""
    rng = np.random.default_rng(seed)
    h, w = input_hw
    mask = (rng.uniform(size=(K, L, 1)) < 0.3).astype(np.float64)
    xy = np.clip(rng.uniform(-0.05, 1.05, size=(K, L, 2)), 0.0, 1.0) * (1.0 - mask)
    depth = rng.uniform(size=(L, h, w))
    return xy, mask, depth
