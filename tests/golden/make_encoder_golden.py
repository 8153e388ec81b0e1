#!/usr/bin/env python3
"""Golden vectors for the motion classifier's trajectory transformer, produced by the REFERENCE's own module:
core.network.traj_oa_depth is imported UNMODIFIED (through oracle/ref_shim, as tests/golden/make_augment_golden.py does, with .cuda()
as identity), the real traj_oa_depth(window, input_size) is constructed on the CPU, switched to .eval(), and its
joint_encoder(aug_trajs, masks) (pt_transformer.forward, motion_seg/core/network/traj_oa_depth.py:25-60) is called under no_grad.

Weights: no checkpoint is at hand, so the module's seeded default initialisation plus a seeded N(0, 0.1) perturbation of EVERY
parameter of joint_encoder.  The perturbation matters: the defaults leave every attention bias 0 and every LayerNorm gain 1 and
bias 0, and a kernel that ignored them would pass.
Inputs: the four augment fixtures' `out` ([10,K,L] fp32) and `mask` (L = 10 twice, 27, 7, all with real padding), the mask shaped as
main_motion_segmentation.py:77 shapes it (ToTensor, unsqueeze(0), .float()).
Stored: encoder_weights.npz -- the 68 arrays by packed key (psfm_motion_seg.encoder.ENCODER_KEYS), `e` and `tol`; per case
encoder_<input fixture>.npz -- the input fixture's name, the module's fp32 output out32 and the same module's .double() output
out64, both [16,K].
The tolerance is measured, not chosen: e = max over the cases of max |out32 - out64|, the error of the reference's own fp32 run
against the f64 truth, and tol = 4 e (e is one draw of a maximum over K x 16 outputs; a second, independent rounding pattern of the
same size -- another summation order, another expf -- has to fit under it).
Asserted here: tests/_encoder_np.encoder_np equals out64 to 1e-12, and each of its three misreadings (memory padding masked in
cross-attention, max over valid tokens only, padded positions zeroed) misses tol by at least 100x on every case.
Only arrays are stored.  Run in the build container, never on the GPU machine:
    python tests/golden/make_encoder_golden.py
"""
import copy
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "particle-sfm_amd"), os.path.join(ROOT, "tests"), HERE):
    sys.path.insert(0, p)
from _encoder_np import ENCODER_CASES, WEIGHTS_FIXTURE, encoder_np     # noqa: E402
from make_augment_golden import load_reference, to_tensor              # noqa: E402
from psfm_motion_seg.encoder import ENCODER_KEYS, WEIGHT_COUNT, pack_encoder_weights_host       # noqa: E402

MAX_BYTES = 847951      # make_augment_golden.MAX_BYTES
WINDOW, INPUT_SIZE = 10, (30, 50)
INIT_SEED, PERTURB_SEED, SIGMA = 20260, 20261, 0.1
MARGIN = 4.0


def build_model(net):
    import torch
    torch.manual_seed(INIT_SEED)
    model = net.traj_oa_depth(WINDOW, INPUT_SIZE).cuda().eval()
    gen = torch.Generator().manual_seed(PERTURB_SEED)
    with torch.no_grad():
        for _, p in model.joint_encoder.named_parameters():
            p.add_(torch.randn(p.shape, generator=gen) * SIGMA)
    return model


def main():
    import torch
    _, net = load_reference()
    model = build_model(net)
    enc64 = copy.deepcopy(model.joint_encoder).double()
    sd = {k: v.detach().numpy().copy() for k, v in model.state_dict().items() if k.startswith("joint_encoder.")}
    assert sorted(sd) == sorted("joint_encoder." + k for k, _ in ENCODER_KEYS) and len(sd) == 68
    assert list(k for k in model.state_dict() if k.startswith("joint_encoder.")) == ["joint_encoder." + k for k, _ in ENCODER_KEYS]
    packed = pack_encoder_weights_host(sd)
    assert packed.size == WEIGHT_COUNT == sum(p.numel() for p in model.joint_encoder.parameters())
    W = {k: sd["joint_encoder." + k] for k, _ in ENCODER_KEYS}
    for k, v in W.items():                       # every gain is off 1 and every bias off 0
        if k.endswith("bias"):
            assert (v != 0).all(), k
        if "norm" in k and k.endswith("weight"):
            assert (v != 1).all(), k

    cases, e = [], 0.0
    for name in ENCODER_CASES:
        g = np.load(os.path.join(HERE, name + ".npz"))
        K, L = g["traj"].shape[:2]
        with torch.no_grad():
            aug = torch.from_numpy(g["out"]).unsqueeze(0).float().cuda()
            mask_t = to_tensor(g["mask"]).unsqueeze(0).float().cuda()             # main_motion_segmentation.py:77
            assert tuple(aug.shape) == (1, 10, K, L) and tuple(mask_t.shape) == (1, 1, K, L)
            out32 = model.joint_encoder(aug, mask_t)
            out64 = enc64(aug.double(), mask_t.double())
        assert tuple(out32.shape) == (1, 16, K) and out32.dtype == torch.float32 and out64.dtype == torch.float64
        out32, out64 = out32[0].numpy().copy(), out64[0].numpy().copy()
        assert np.isfinite(out64).all()
        pad = g["mask"].reshape(K, L) > 0.5
        assert 0 < pad.sum() < pad.size and (~pad).sum(1).min() >= 1
        err = float(np.abs(encoder_np(g["out"], g["mask"], W) - out64).max())
        assert err <= 1e-12, (name, err)
        e_case = float(np.abs(out32.astype(np.float64) - out64).max())
        print(name, "K", K, "L", L, "max |restatement - out64|", err, "max |out32 - out64|", e_case)
        e = max(e, e_case)
        cases.append((name, g, out32, out64))
    tol = MARGIN * e
    print("e = %.6e   tol = %g * e = %.6e" % (e, MARGIN, tol))

    for name, g, out32, out64 in cases:
        for quirk in ("mask_memory", "max_valid_only", "zero_padded"):
            miss = float(np.abs(encoder_np(g["out"], g["mask"], W, **{quirk: True}) - out64).max())
            print("   ", name, quirk, "misses by", miss, "= %.0f x tol" % (miss / tol))
            assert miss >= 100 * tol, (name, quirk, miss, tol)
        path = os.path.join(HERE, "encoder_" + name + ".npz")
        np.savez_compressed(path, input=np.asarray(name), out32=out32, out64=out64)
        assert os.path.getsize(path) <= MAX_BYTES, (name, os.path.getsize(path))
        print("   ", os.path.getsize(path), "bytes")
    path = os.path.join(HERE, WEIGHTS_FIXTURE + ".npz")
    np.savez_compressed(path, e=np.float64(e), tol=np.float64(tol), margin=np.float64(MARGIN), init_seed=INIT_SEED, perturb_seed=PERTURB_SEED,
                        sigma=SIGMA, **W)
    assert os.path.getsize(path) <= MAX_BYTES
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
