#!/usr/bin/env python3
"""psfm_traj_decode (csrc/psfm_decoder.hip) against the same formulas written with plain torch operators, on the same device, the
same tensors and the same weights.

Workload (default): K = 100 000 trajectories (the reference's traj_max_num): the K = 100 000 input and the seeded weights of the
tests (tests/_decoder_np.py).
  fused   one psfm_traj_decode call: a fixed sequence of launches, reads [16][K] f32, writes logits, prob and pred
  torch   OANBlock(128, 16, 8, 100) of motion_seg/core/network/oanet.py:161-206 in eval mode, restated with matmul, var_mean, softmax
          and elementwise operators on [C][K] tensors, fp32, no_grad; sigmoid and `> 0.5` included
Both are warmed up, then timed as --reps repetitions between two HIP events on the stream (the span divided by --reps), --rounds
times, alternating; the median round is reported with min and max (rounds x reps >= 20 repetitions).
Floors, derived from the module's shapes and not measured: 729 kflop per trajectory (73 GFLOP at K = 100 000) at the 157.3 TFLOPS
fp32 matrix peak, and 2.5 GB of activation traffic at a 5.2 TB/s copy ceiling: about 0.5 ms each.  Launch counts: --count-launches
(torch.profiler kernel events of one call).  The two logit vectors are compared while both are at hand (reported, not asserted: the
tests pin the kernels to the reference's f64 run).  Prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "particle-sfm_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
PEAK_FP32_MATRIX_TFLOPS = 157.3
COPY_CEILING_TBS = 5.2
# multiply-adds per trajectory: conv1, 7 PointCN(128), down1 and up1 embeddings, the two pooled products, PointCN(256,128), output
FMAS_PER_POINT = 16 * 128 + 7 * 2 * 128 * 128 + 2 * 128 * 100 + 2 * 128 * 100 + (256 * 128 + 128 * 128 + 256 * 128) + 128
# bytes per trajectory that must move at least once: per convolution its [128] input read and [128] output written
BYTES_PER_POINT = 4 * (16 + 128) + 4 * 17 * 2 * 128 + 4 * (3 * 128 + 2 * 100 + 2 * 128 + 128) + 4 * (4 * 128 + 128) + 9


def torch_decoder(W):
    """The decoder from plain operators on [C][K] tensors; W: dict key -> device tensor."""
    import torch

    def inorm(x):
        var, mean = torch.var_mean(x, dim=1, unbiased=False, keepdim=True)
        return (x - mean) * torch.rsqrt(var + 1e-3)

    def bnorm(x, p):
        return (x - W[p + "running_mean"][:, None]) * (W[p + "weight"] * torch.rsqrt(W[p + "running_var"] + 1e-5))[:, None] + W[p + "bias"][:, None]

    def conv(x, p):
        w = W[p + "weight"]
        return w.reshape(w.shape[0], w.shape[1]) @ x + W[p + "bias"][:, None]

    def nbr(x, p):
        return torch.relu(bnorm(inorm(x), p))

    def point_cn(x, p):
        out = conv(nbr(conv(nbr(x, p + "conv.1."), p + "conv.3."), p + "conv.5."), p + "conv.7.")
        return out + (conv(x, p + "shot_cut.") if p + "shot_cut.weight" in W else x)

    def oa_filter(x, p):
        out = conv(nbr(x, p + "conv1.1."), p + "conv1.3.").t()
        out = out + conv(torch.relu(bnorm(out, p + "conv2.0.")), p + "conv2.2.")
        return conv(nbr(out.t(), p + "conv3.2."), p + "conv3.4.") + x

    def forward(enc):                                     # [16][K]
        x1 = conv(enc, "conv1.")
        for i in range(4):
            x1 = point_cn(x1, "l1_1.%d." % i)
        x2 = x1 @ torch.softmax(conv(nbr(x1, "down1.conv.1."), "down1.conv.3."), dim=1).t()
        for i in range(4):
            x2 = oa_filter(x2, "l2.%d." % i)
        out = torch.cat([x1, x2 @ torch.softmax(conv(nbr(x1, "up1.conv.1."), "up1.conv.3."), dim=0)], 0)
        for i in range(4):
            out = point_cn(out, "l1_2.%d." % i)
        logits = conv(out, "output.")[0]
        prob = torch.sigmoid(logits)
        return logits, prob, prob > 0.5
    return forward


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", choices=["fused", "torch"], default=None, help="run --calls calls of one side and exit (for a kernel trace)")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--count-launches", action="store_true", help="count the kernels of one call of each with torch.profiler")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()

    import torch
    from _decoder_np import BIG_SEED, seeded_decoder_inputs, seeded_decoder_weights
    from point_trajectory import _hip
    from psfm_motion_seg.decoder import pack_decoder_weights

    assert torch.cuda.is_available(), "decoder.py measures on the GPU"
    K = a.tracks
    W = seeded_decoder_weights()
    enc = torch.from_numpy(seeded_decoder_inputs(K, BIG_SEED)).cuda()
    ctx = _hip.context(0)
    lib, sp = _hip.lib(), _hip.current_stream_ptr(0)
    weights = pack_decoder_weights(W)
    need = int(lib.psfm_traj_decode_workspace_bytes(K))
    ws = torch.empty((need,), dtype=torch.uint8, device="cuda")
    logits = torch.empty((K,), dtype=torch.float32, device="cuda")
    prob = torch.empty((K,), dtype=torch.float32, device="cuda")
    pred = torch.empty((K,), dtype=torch.uint8, device="cuda")
    model = torch_decoder({k: torch.from_numpy(v).cuda() for k, v in W.items()})

    def fused():
        _hip.check(lib.psfm_traj_decode(ctx.handle, _hip.ptr(enc), _hip.ptr(weights), K, _hip.ptr(ws), need, _hip.ptr(logits), _hip.ptr(prob),
                                        _hip.ptr(pred), sp))
        return logits

    def reference():
        with torch.no_grad():
            return model(enc)[0]

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

    flop = 2.0 * FMAS_PER_POINT * K
    nbytes = float(BYTES_PER_POINT) * K
    med = np.median(t, 0)
    res = {"workload": "K=%d" % K, "reps": a.reps, "rounds": a.rounds,
           "fused_us": float(med[0]), "fused_us_min_max": [float(t[:, 0].min()), float(t[:, 0].max())],
           "torch_us": float(med[1]), "torch_us_min_max": [float(t[:, 1].min()), float(t[:, 1].max())],
           "torch_over_fused": float(med[1] / med[0]), "flop": flop, "fused_TFLOPS": float(flop / med[0] / 1e6),
           "floor_us_fp32_matrix_peak": float(flop / PEAK_FP32_MATRIX_TFLOPS / 1e6),
           "activation_bytes": nbytes, "floor_us_copy_ceiling": float(nbytes / COPY_CEILING_TBS / 1e6),
           "workspace_bytes": need, "fused_launches": n_fused, "fused_kernels": names_fused, "torch_launches": n_ref,
           "logits_max_abs_diff": max_diff}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fp:
            fp.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
