#!/usr/bin/env python3
"""psfm_traj_encode (csrc/psfm_encoder.hip) against torch.nn's own modules for the same network, on the same device, the same
tensors and the same weights.

Workload (defaults): K = 100 000 trajectories (the reference's traj_max_num), L = 10 frames; seeded features with 30 % padded slots
(every row keeps a valid token), the seeded weights of tests/golden/encoder_weights.npz.
  fused   one psfm_traj_encode launch: reads the [10][K][L] f32 features and the f64 mask, writes [16][K] f32
  torch   pt_transformer of motion_seg/core/network/traj_oa_depth.py:25-60 restated with torch.nn: Conv2d(10,16,1), Conv2d(16,16,1),
          nn.Transformer(16, 4, 2, 2, 64, dropout 0.1, relu), the permutes and the max; .eval(), no_grad, fp32, the mask already
          in the reference's [1,1,K,L] f32 form
Both are warmed up, then timed as --reps repetitions between two HIP events on the stream (the span divided by --reps), --rounds
times, alternating; the median round is reported with min and max (rounds x reps >= 20 repetitions).  flop = 2 x 14 752 per-token
FMAs of the linear layers plus 6 attentions of 2 x (2 x 16 L + 16 L) each (scores twice: two passes), times K L tokens; the peak it
is set against is the fp32 vector peak, 157.3 TFLOPS.  Launch counts: --count-launches (torch.profiler kernel events of one call),
or run `--only torch --calls N` / `--only fused --calls N` under `rocprofv3 --kernel-trace --stats` for two values of N and divide
the difference.  The two outputs are compared while both are at hand (reported, not asserted: the tests pin the kernel to the
reference's f64 run).  Prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "particle-sfm_amd"))
PEAK_FP32_VECTOR_TFLOPS = 157.3
LINEAR_FMAS_PER_TOKEN = 160 + 256 + 2 * (768 + 256 + 2048) + 2 * (2 * (768 + 256) + 2048)      # 14 752


def torch_module(weights):
    """The network of pt_transformer from torch.nn's own layers, with the checkpoint's attribute names so the 68 tensors load."""
    import torch
    import torch.nn as nn

    class Encoder(nn.Module):
        def __init__(self):
            super().__init__()
            self.input_fc1 = nn.Conv2d(10, 16, (1, 1))
            self.fc2 = nn.Conv2d(16, 16, (1, 1))
            self.transformer_model = nn.Transformer(d_model=16, nhead=4, num_encoder_layers=2, num_decoder_layers=2, dim_feedforward=64,
                                                    dropout=0.1, activation="relu")

        def forward(self, feat, pad_mask):                       # [1,10,K,L], [1,1,K,L]
            x = torch.relu(self.fc2(torch.relu(self.input_fc1(feat))))
            L = x.shape[-1]
            seq = x.permute(3, 0, 2, 1).reshape(L, -1, 16)
            pad = pad_mask.reshape(-1, L) > 0.5
            y = self.transformer_model(seq, seq, src_key_padding_mask=pad, tgt_key_padding_mask=pad)
            return y.reshape(L, x.shape[0], x.shape[2], -1).max(0)[0].permute(0, 2, 1)       # [1,16,K]

    m = Encoder()
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in weights.items()})
    return m.cuda().eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=100000)
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=["fused", "torch"], default=None, help="run --calls calls of one side and exit (for a kernel trace)")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--count-launches", action="store_true", help="count the kernels of one call of each with torch.profiler")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()

    import torch
    from point_trajectory import _hip
    from psfm_motion_seg.encoder import ENCODER_KEYS, pack_encoder_weights

    assert torch.cuda.is_available(), "encoder.py measures on the GPU"
    K, L = a.tracks, a.frames
    g = np.load(os.path.join(ROOT, "tests", "golden", "encoder_weights.npz"))
    W = {k: g[k] for k, _ in ENCODER_KEYS}
    rng = np.random.default_rng(0)
    pad_h = rng.uniform(size=(K, L)) < 0.3
    pad_h[pad_h.all(1), 0] = False
    f_h = rng.normal(size=(10, K, L)) * np.array([0.3, 0.3, 0.05, 0.05, 0.3, 0.3, 0.5, 0.05, 0.05, 0.05])[:, None, None]
    feat = torch.from_numpy(f_h.astype(np.float32)).cuda()
    mask = torch.from_numpy(pad_h.astype(np.float64)).cuda()                          # (K,L) f64, as psfm_window_sample writes it
    ctx = _hip.context(0)
    lib, sp = _hip.lib(), _hip.current_stream_ptr(0)
    weights = pack_encoder_weights(W)
    out = torch.empty((1, 16, K), dtype=torch.float32, device="cuda")
    model = torch_module(W)
    feat_t, mask_t = feat[None].contiguous(), mask.float()[None, None].contiguous()   # the reference's layout, outside the span

    def fused():
        _hip.check(lib.psfm_traj_encode(ctx.handle, _hip.ptr(feat), _hip.ptr(mask), _hip.ptr(weights), K, L, _hip.ptr(out), sp))
        return out

    def reference():
        with torch.no_grad():
            return model(feat_t, mask_t)

    if a.only:
        fn = fused if a.only == "fused" else reference
        for _ in range(a.calls):
            fn()
        torch.cuda.synchronize()
        print(json.dumps({"only": a.only, "calls": a.calls}))
        return 0

    got, want = fused(), reference()
    max_diff = float((got - want).abs().max())

    def span(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1) / a.reps           # us per call

    for _ in range(a.warmup):
        fused(); reference()
    torch.cuda.synchronize()
    t = np.array([(span(fused), span(reference)) for _ in range(a.rounds)])

    def launches(fn):
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        return len(ev), sorted({e.name for e in ev})
    n_fused = n_ref = names_fused = None
    if a.count_launches:
        n_fused, names_fused = launches(fused)
        n_ref, _ = launches(reference)

    flop = 2.0 * (LINEAR_FMAS_PER_TOKEN + 6 * (2 * 16 * L + 16 * L)) * K * L
    nbytes = (40 + 8) * K * L + 64 * K + 4 * 15872
    med = np.median(t, 0)
    res = {"workload": "K=%d L=%d, 30%% padded" % (K, L), "reps": a.reps, "rounds": a.rounds,
           "fused_us": float(med[0]), "fused_us_min_max": [float(t[:, 0].min()), float(t[:, 0].max())],
           "torch_us": float(med[1]), "torch_us_min_max": [float(t[:, 1].min()), float(t[:, 1].max())],
           "torch_over_fused": float(med[1] / med[0]), "flop": flop, "fused_TFLOPS": float(flop / med[0] / 1e6),
           "fused_fraction_of_fp32_vector_peak": float(flop / med[0] / 1e6 / PEAK_FP32_VECTOR_TFLOPS),
           "algorithmic_bytes": int(nbytes), "fused_launches": n_fused, "fused_kernels": names_fused, "torch_launches": n_ref,
           "outputs_max_abs_diff": max_diff}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fp:
            fp.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
