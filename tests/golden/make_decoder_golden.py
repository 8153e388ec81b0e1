#!/usr/bin/env python3
"""Golden vectors for the motion classifier's OANet decoder, produced by the REFERENCE's own module: core.network.traj_oa_depth is
imported UNMODIFIED (through make_augment_golden.load_reference, as tests/golden/make_encoder_golden.py does), the real
traj_oa_depth(window, input_size) is constructed on the CPU, switched to .eval(), and its decoder (OANBlock, motion_seg/core/network/
oanet.py:161-206) is called under no_grad, once in fp32 and once as a .double() copy.

Weights: no checkpoint is at hand and 2 MB of floats do not fit a fixture, so tests/_decoder_np.seeded_decoder_weights(seed) draws them
(every gain off 1, every bias and running mean off 0) and they are loaded with load_state_dict(strict=True); decoder_meta.npz stores
the sha256 of the packed array.
Cases (tests/_decoder_np.DECODER_CASES): the four encoder fixtures' out32, seeded inputs with the moments of those features at
K = 2 .. 1000 around the kernel's 64-point tile, 50 equal rows (zero variance: eps carries the normalisation), and K = 100 000.
Stored per case, decoder_<case>.npz: the input x (except at K = 100 000, where its sha256 and an 8192-row sample are stored),
logit32 and logit64, e = max |logit32 - logit64| over ALL rows and tol = 4 e (the margin and its reason are the encoder's: another
summation order is a second draw of the same rounding).
Whole model, decoder_full_<window>.npz for the two augment_48x64_t23 windows: the full traj_oa_depth.forward in fp32 (prob32), the
decoder's f64 logits on the encoder's f64 output (logit64), d = max |decoder64(enc out64) - decoder64(enc out32)|.
Asserted here: tests/_decoder_np.decoder_np equals logit64 to 1e-10 on every case; each of its five misreadings misses tol by at
least 100x on every case of K >= 3 where it changes anything; the rows with |logit64| <= tol (and, whole model, <= 4 (e + d)) are at most
0.5 % of a case.
Only arrays are stored.  Run in the build container, never on the GPU machine:
    python tests/golden/make_decoder_golden.py
"""
import copy
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "particle-sfm_amd"), os.path.join(ROOT, "tests"), HERE):
    sys.path.insert(0, p)
from _decoder_np import (BIG_K, BIG_ROWS, DECODER_CASES, META_FIXTURE, WEIGHT_SEED, case_input, decoder_np, packed_sha256,       # noqa: E402
                         seeded_decoder_weights)
from make_augment_golden import load_reference, to_tensor              # noqa: E402
from make_encoder_golden import build_model                            # noqa: E402
from psfm_motion_seg.decoder import DECODER_KEYS, WEIGHT_COUNT, pack_decoder_weights_host       # noqa: E402

MAX_BYTES = 847951      # make_augment_golden.MAX_BYTES
MARGIN = 4.0
BAND_CAP = 0.005
QUIRKS = ("pool_over_clusters", "unbiased_var", "in_eps_1e5", "pool_normalised", "up_shares_down")
FULL_WINDOWS = ["augment_48x64_t23_w0", "augment_48x64_t23_w2"]


def main():
    import torch
    torch.set_num_threads(8)
    _, net = load_reference()
    model = build_model(net)                         # the encoder of encoder_weights.npz
    W = seeded_decoder_weights(WEIGHT_SEED)
    float_keys = [k for k in model.decoder.state_dict() if not k.endswith("num_batches_tracked")]
    assert float_keys == [k for k, _ in DECODER_KEYS] and len(float_keys) == 186
    assert len(model.decoder.state_dict()) == 186 + 30
    model.decoder.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()}, strict=True)
    model.eval()
    packed = pack_decoder_weights_host({k: v for k, v in model.state_dict().items() if k.startswith("decoder.")})
    assert np.array_equal(packed, pack_decoder_weights_host(W))
    n_param = sum(p.numel() for p in model.decoder.parameters())
    assert packed.size == WEIGHT_COUNT == 529497 and n_param == 521785 and WEIGHT_COUNT - n_param == 7712
    for k, v in W.items():
        if k.endswith(("bias", "running_mean")):
            assert (v != 0).all(), k
        elif not k.endswith("running_var") and v.ndim == 1:
            assert (v != 1).all(), k
    dec64 = copy.deepcopy(model.decoder).double()
    enc64 = copy.deepcopy(model.joint_encoder).double()

    def run(x):
        with torch.no_grad():
            t = torch.from_numpy(x)[None, :, :, None]
            l32 = model.decoder(t.float())
            l64 = dec64(t.double())
        assert tuple(l32.shape) == (1, 1, x.shape[1]) and l32.dtype == torch.float32 and l64.dtype == torch.float64
        return l32[0, 0].numpy().copy(), l64[0, 0].numpy().copy()

    failures = []
    es = {}
    for case in DECODER_CASES:
        x = case_input(case)
        K = x.shape[1]
        l32, l64 = run(x)
        assert np.isfinite(l64).all()
        e = float(np.abs(l32.astype(np.float64) - l64).max())
        tol = MARGIN * e
        es[case] = e
        err = float(np.abs(decoder_np(x, W, same_order=case == "equal_k50") - l64).max())
        band = float((np.abs(l64) <= tol).mean())
        wrong = int(((l32 > 0) != (l64 > 0))[np.abs(l64) > tol].sum())
        print("%-28s K %6d  e %.3e  tol %.3e  |restatement - logit64| %.2e  std %.2f  max|logit| %.1f  band %.4f%%  ref labels wrong %d"
              % (case, K, e, tol, err, l64.std(), np.abs(l64).max(), 100 * band, wrong), flush=True)
        assert err <= 1e-10, (case, err)
        assert band <= BAND_CAP and wrong == 0, (case, band, wrong)
        if K < BIG_K:
            for quirk in QUIRKS:
                miss = float(np.abs(decoder_np(x, W, same_order=case == "equal_k50", **{quirk: True}) - l64).max())
                ok = miss >= 100 * tol
                print("      %-20s misses by %.3e = %.0f x tol%s" % (quirk, miss, miss / tol, "" if ok else "   <-- below 100 x"))
                # (50 equal rows: zero variance either way; K = 2: the reference's own fp32 error is 1e-2, nothing stands out 100 x)
                if not ok and not (case == "equal_k50" and quirk == "unbiased_var") and K > 2:
                    failures.append((case, quirk, miss, tol))
        path = os.path.join(HERE, "decoder_" + case + ".npz")
        if K < BIG_K:
            np.savez_compressed(path, x=x, logit32=l32, logit64=l64, e=np.float64(e), tol=np.float64(tol))
        else:
            rows = np.sort(np.random.default_rng(BIG_K).choice(K, size=BIG_ROWS, replace=False)).astype(np.int64)
            np.savez_compressed(path, x_sha256=np.asarray(hashlib.sha256(x.tobytes()).hexdigest()), rows=rows, logit32=l32[rows],
                                logit64=l64[rows], e=np.float64(e), tol=np.float64(tol), band=np.float64(band))
        assert os.path.getsize(path) <= MAX_BYTES, (case, os.path.getsize(path))
    assert not failures, failures

    for name in FULL_WINDOWS:
        g = np.load(os.path.join(HERE, name + ".npz"))
        fx = np.load(os.path.join(HERE, "encoder_" + name + ".npz"))
        K, L = g["traj"].shape[:2]
        with torch.no_grad():
            batch = {"depth": torch.stack([to_tensor(d).float() for d in g["depth"]], -1).unsqueeze(0).float(),
                     "traj": to_tensor(g["traj"]).unsqueeze(0).float(), "mask": to_tensor(g["mask"]).unsqueeze(0).float()}
            prob32 = model(batch)
            aug = model.augment_traj(batch["depth"], batch["traj"], batch["mask"])
            assert np.array_equal(aug[0].numpy(), g["out"])
            out64 = enc64(aug.double(), batch["mask"].double())
            assert np.array_equal(out64[0].numpy(), fx["out64"])
            full64 = dec64(out64.unsqueeze(-1))[0, 0].numpy().copy()
            half64 = dec64(torch.from_numpy(fx["out32"]).double()[None, :, :, None])[0, 0].numpy().copy()
        assert tuple(prob32.shape) == (1, 1, K)
        prob32 = prob32[0, 0].numpy().copy()
        d = float(np.abs(full64 - half64).max())
        e = es["enc_" + name]
        band = MARGIN * (e + d)
        inside = float((np.abs(full64) <= band).mean())
        wrong = int(((prob32 > 0.5) != (full64 > 0))[np.abs(full64) > band].sum())
        print("%-28s whole model: d %.3e  e %.3e  band %.3e holds %.4f%% of rows, reference labels wrong outside it: %d"
              % (name, d, e, band, 100 * inside, wrong))
        assert inside <= BAND_CAP and wrong == 0
        path = os.path.join(HERE, "decoder_full_" + name + ".npz")
        np.savez_compressed(path, prob32=prob32, logit64=full64, d=np.float64(d), e=np.float64(e), band=np.float64(band))
        assert os.path.getsize(path) <= MAX_BYTES

    path = os.path.join(HERE, META_FIXTURE + ".npz")
    np.savez_compressed(path, weights_sha256=np.asarray(packed_sha256(packed)), weight_seed=np.int64(WEIGHT_SEED), margin=np.float64(MARGIN),
                        cases=np.asarray(DECODER_CASES), e=np.asarray([es[c] for c in DECODER_CASES]))
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
