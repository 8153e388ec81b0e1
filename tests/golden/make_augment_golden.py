#!/usr/bin/env python3
"""Golden vectors for the motion classifier's input step, produced by the REFERENCE's own module: core.network.traj_oa_depth is
imported UNMODIFIED, the real traj_oa_depth(window, input_size) is constructed on the CPU and its augment_traj(depth, traj, mask)
(motion_seg/core/network/traj_oa_depth.py:72-114) is called on tensors built the way motion_seg/main_motion_segmentation.py:71-78
builds them: ToTensor (HWC -> CHW), .float(), stack(-1), unsqueeze(0).

Stand-ins, on top of oracle/ref_shim.load_consumers() (cv2 / cvbase stubs, the `core` package of the reference on the path):
  torch.Tensor.cuda / Module.cuda   identity            ToTensor   HWC ndarray -> CHW tensor (what torchvision's does to an f64 array)
Cases (tests/_augment_np.AUGMENT_CASES):
  (a) two windows -- the first and the last, overlapping one -- that the reference's own load_cut_seq cuts from the CPU checker's
      track() on the seeded psfm_synth sequence of labels_48x64_t23_w10 (real padding patterns), input size (30,50);
  (b) window >= length on the 24x32, T = 27 sequence: L = 27, input size (21,34);
  (c) seeded synthetic: coordinates clip(U(-0.05,1.05),0,1) * (1 - mask), 30 % padded, input size (37,53), K = 300, L = 7 -- asserted to
      hold points with ix == w, indices clamped at h*w-1 and padded slots followed by present ones.
Depth is iid U[0,1) per pixel (f64, as cv2.imread(...) / 65535.0 hands it over): neighbouring pixels differ by far more than an ulp,
so a wrong gather index cannot pass.  Only arrays are stored.  Run in the build container, never on the GPU machine:
    python tests/golden/make_augment_golden.py
"""
import importlib
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "particle-sfm_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import psfm_synth                     # noqa: E402
from _augment_np import augment_np, edge_counts, seeded_inputs     # noqa: E402
from _common import input_hash       # noqa: E402
from oracle import oracle as orc     # noqa: E402
from oracle import ref_shim          # noqa: E402

MAX_BYTES = 847951      # the largest fixture already in tests/golden

# name prefix, T, H, W, ratio, seed, sigma, occluders, flow amplitude (px), window, network input size, windows to keep, depth seed
REAL = [("augment_48x64_t23", 23, 48, 64, 2, 311, 0.3, 2, 3.0, 10, (30, 50), (0, 2), 9101),
        ("augment_24x32_t27", 27, 24, 32, 2, 302, 0.05, 1, 0.5, 28, (21, 34), ("full",), 9102)]
SYNTH = ("augment_synth_37x53", 300, 7, (37, 53), 9103)


def load_reference():
    import torch
    ref = ref_shim.load_consumers()
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.nn.Module.cuda = lambda self, *a, **k: self
    net = importlib.import_module("core.network.traj_oa_depth")       # the reference's file, through the path the shim added
    assert os.path.realpath(net.__file__).startswith(os.path.realpath(ref_shim.REFERENCE_ROOT))
    return ref, net


def to_tensor(a):
    """torchvision.transforms.ToTensor on a float ndarray: HWC -> CHW, values untouched."""
    import torch
    a = np.asarray(a)
    if a.ndim == 2:
        a = a[:, :, None]
    return torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1)))


def reference_augment(net, window, input_size, depths, traj, mask):
    """main_motion_segmentation.py:71-79 up to the model call, then the model's own augment_traj."""
    import torch
    model = net.traj_oa_depth(window, input_size).cuda()
    with torch.no_grad():
        depths_t = torch.stack([to_tensor(d).float().cuda() for d in depths], -1).unsqueeze(0).float().cuda()
        traj_t = to_tensor(traj).unsqueeze(0).float().cuda()
        mask_t = to_tensor(mask).unsqueeze(0).float().cuda()
        out = model.augment_traj(depths_t, traj_t, mask_t)
    K, L = traj.shape[:2]
    assert tuple(out.shape) == (1, 10, K, L) and out.dtype == torch.float32
    return out[0].numpy().copy(), model.K_inv_t[0].numpy().copy()


def save(name, traj, mask, depth, kinv, input_size, out, **extra):
    want = augment_np(traj, mask, depth, input_size, kinv)
    print(name, "K", traj.shape[0], "L", traj.shape[1], "max |reference - unfused fp32 formula|", float(np.abs(out - want).max()),
          "edges (ix == w, clamped, padded -> present)", edge_counts(traj, mask, input_size))
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, traj=traj.astype(np.float64), mask=mask.astype(np.float64), depth=depth, kinv=kinv.astype(np.float32),
                        input_size=np.asarray(input_size), out=out.astype(np.float32), **extra)
    assert os.path.getsize(path) <= MAX_BYTES, (name, os.path.getsize(path))
    print("   ", os.path.getsize(path), "bytes")


def main():
    ref, net = load_reference()
    for prefix, T, H, W, r, seed, sigma, nocc, amp, window, input_size, keep_w, depth_seed in REAL:
        d = psfm_synth.synth_sequence(T, H, W, seed=seed, amp=amp, sigma=sigma, n_occluders=nocc, stride2=False)
        _, occ = orc.flow_check(d["flows_f"], d["flows_b"], 1.0)
        R = orc.track(d["flows_f"], occ, r)
        keep = np.flatnonzero(R.length >= 3)
        ts = ref_shim.TrajectorySet({int(i): ref_shim.Trajectory({"frame_ids": list(range(int(R.birth[i]), int(R.birth[i]) + int(R.length[i]))),
                                                                   "locations": list(R.traj(int(i))[1]), "labels": [False] * int(R.length[i])})
                                     for i in keep})
        ref.cv2.imread = lambda nme, flag=1, H=H, W=W: np.zeros((H, W, 3), np.uint8) if flag != -1 else np.zeros((H, W), np.float64)
        with tempfile.TemporaryDirectory() as tmp:
            img_dir, depth_dir, traj_dir = (os.path.join(tmp, x) for x in ("images", "depths", "traj"))
            for p in (img_dir, depth_dir, traj_dir):
                os.makedirs(p)
            for i in range(T):
                open(os.path.join(img_dir, "%05d.png" % i), "w").close()
                open(os.path.join(depth_dir, "%05d.png" % i), "w").close()
            np.save(os.path.join(traj_dir, "track.npy"), ts, allow_pickle=True)
            cut = ref.load_cut_seq(img_dir, depth_dir, traj_dir, window, input_size, 10 ** 9)
        traj_b, mask_b, time_b = cut[3], cut[4], cut[5]
        rng = np.random.default_rng(depth_seed)
        for wi in keep_w:
            w = 0 if wi == "full" else wi
            traj, mask, tidx = np.asarray(traj_b[w]), np.asarray(mask_b[w]), np.asarray(time_b[w])
            L = len(tidx)
            assert np.array_equal(tidx, np.arange(tidx[0], tidx[0] + L)) and traj.shape[1] == L
            if wi == "full":
                assert len(traj_b) == 1 and L == T and L % 2 == 1 and L != 10
            else:
                assert len(traj_b) == 3 and L == window
            assert 0 < mask.sum() < mask.size          # real padding
            depths = [rng.uniform(size=input_size) for _ in range(L)]          # the cv2 stub's maps are blank: seeded ones instead
            out, kinv = reference_augment(net, window, input_size, depths, traj, mask)
            save("%s_%s" % (prefix, "full" if wi == "full" else "w%d" % wi), traj, mask, np.stack(depths, 0), kinv, input_size, out,
                 T=T, H=H, W=W, ratio=r, seed=seed, sigma=sigma, n_occluders=nocc, amp=amp, window=window, frame0=int(tidx[0]),
                 n_windows=len(traj_b), window_index=w, input_hash=input_hash(d))
    name, K, L, input_size, seed = SYNTH
    traj, mask, depth = seeded_inputs(K, L, input_size, seed)
    n_next_row, n_clamped, n_pad_then_present = edge_counts(traj, mask, input_size)
    assert n_next_row >= 1 and n_clamped >= 1 and n_pad_then_present >= 1, (n_next_row, n_clamped, n_pad_then_present)
    out, kinv = reference_augment(net, 10, input_size, list(depth), traj, mask)
    save(name, traj, mask, depth, kinv, input_size, out, seed=seed)


if __name__ == "__main__":
    main()
