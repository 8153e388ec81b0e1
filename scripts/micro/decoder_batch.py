#!/usr/bin/env python3
"""psfm_traj_decode_batch (csrc/psfm_decoder.hip, psfm_decoder_batch.h) against one psfm_traj_decode per window, and the whole of
stage 2 (the motion classifier over the windows of a sequence) by both routes, on the same device, tensors and weights.

  --mode decoder   --windows N windows of --tracks K trajectories each (seeded inputs and weights of tests/_decoder_np.py):
                   N psfm_traj_decode calls against ONE psfm_traj_decode_batch call, HIP events around --reps repetitions, --rounds
                   rounds, alternating; microseconds per WINDOW, median with min and max.  The outputs are compared bit for bit.
  --mode stage     from "the result is in the context" to finish() returned (host clock around a synchronised region), alternating
                     single   merge_labels.label_trajectories + decoder.device_predictor, one context after the other
                     batched  merge_labels.label_sequences_batched (label_trajectories_batched for one context)
                   --shape a: 16 sequences of 480x854, 50 flows, sample_ratio 4, through run_connect_batch;
                   --shape b: 1080p x 101 frames, sample_ratio 2 (the headline), one context;
                   window 10, traj_max_num 100 000, input size 240x424 (the reference's configs/example_test.yaml), seeded encoder and
                   decoder weights, seeded uniform depth maps made before the clock starts.  The five tensors of every finish() are
                   compared byte for byte between the routes.  `spread` is max - min over the runs of a route.
  --only ROUTE     run ROUTE --calls times and exit (for a kernel trace): decoder: single | batch; stage: single | batched.
Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "particle-sfm_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
INPUT_SIZE = (240, 424)
SHAPES = {"a": dict(n_seq=16, H=480, W=854, frames=51, ratio=4), "b": dict(n_seq=1, H=1080, W=1920, frames=101, ratio=2)}


def decoder_mode(a):
    import ctypes
    import torch
    from _decoder_np import seeded_decoder_inputs, seeded_decoder_weights
    from point_trajectory import _hip
    from psfm_motion_seg.decoder import pack_decoder_weights
    N, K = a.windows, a.tracks
    ctx = _hip.context(0)
    lib, sp, vp = _hip.lib(), _hip.current_stream_ptr(0), ctypes.c_void_p
    weights = pack_decoder_weights(seeded_decoder_weights())
    enc = [torch.from_numpy(seeded_decoder_inputs(K, 100 + b)).cuda() for b in range(N)]
    ks = (ctypes.c_int64 * N)(*[K] * N)
    need1, need = int(lib.psfm_traj_decode_workspace_bytes(K)), int(lib.psfm_traj_decode_batch_workspace_bytes(ks, N))
    ws = torch.empty((need,), dtype=torch.uint8, device="cuda")
    out = {r: [(torch.empty((K,), dtype=torch.float32, device="cuda"), torch.empty((K,), dtype=torch.float32, device="cuda"),
                torch.empty((K,), dtype=torch.uint8, device="cuda")) for _ in range(N)] for r in ("single", "batch")}
    col = lambda ts: (vp * N)(*[t.data_ptr() for t in ts])
    cols = (col(enc),) + tuple(col([o[i] for o in out["batch"]]) for i in range(3))

    def single():
        for e, (lo, pr, pd) in zip(enc, out["single"]):
            _hip.check(lib.psfm_traj_decode(ctx.handle, _hip.ptr(e), _hip.ptr(weights), K, _hip.ptr(ws), need1, _hip.ptr(lo), _hip.ptr(pr), _hip.ptr(pd), sp))

    def batch():
        _hip.check(lib.psfm_traj_decode_batch(ctx.handle, N, cols[0], ks, _hip.ptr(weights), _hip.ptr(ws), need, cols[1], cols[2], cols[3], sp))

    if a.only:
        fn = {"single": single, "batch": batch}[a.only]
        for _ in range(a.calls):
            fn()
        torch.cuda.synchronize()
        return {"only": a.only, "calls": a.calls, "windows": N, "tracks": K}

    def span(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1) / a.reps / N           # us per window

    def wall(fn):                                               # host time to ENQUEUE one repetition, us per window
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        return 1e6 * (t1 - t0) / N

    for _ in range(a.warmup):
        single(); batch()
    torch.cuda.synchronize()
    equal = all(torch.equal(x, y) for s, b in zip(out["single"], out["batch"]) for x, y in zip(s, b))
    t = np.array([(span(single), span(batch)) for _ in range(a.rounds)])
    h = np.array([(wall(single), wall(batch)) for _ in range(a.rounds)])
    med = np.median(t, 0)
    return {"mode": "decoder", "windows": N, "tracks": K, "reps": a.reps, "rounds": a.rounds, "bit_equal": bool(equal),
            "single_us_per_window": float(med[0]), "single_min_max": [float(t[:, 0].min()), float(t[:, 0].max())],
            "batch_us_per_window": float(med[1]), "batch_min_max": [float(t[:, 1].min()), float(t[:, 1].max())],
            "single_over_batch": float(med[0] / med[1]),
            "enqueue_us_per_window": {"single": float(np.median(h[:, 0])), "batch": float(np.median(h[:, 1]))},
            "workspace_bytes": need}


def stage_mode(a):
    import torch
    import psfm_synth
    from _decoder_np import seeded_decoder_weights
    from _encoder_np import fixture_weights
    from point_trajectory import _hip
    from point_trajectory.trajectory import run_connect, run_connect_batch
    from psfm_motion_seg.decoder import device_predictor, pack_decoder_weights
    from psfm_motion_seg.encoder import pack_encoder_weights
    from psfm_motion_seg.load_cut_seq import window_ranges
    from psfm_motion_seg.merge_labels import label_sequences_batched, label_trajectories
    S = SHAPES[a.shape]
    H, W, T, n_seq = S["H"], S["W"], S["frames"], S["n_seq"]
    dec_w = pack_decoder_weights(seeded_decoder_weights())
    enc_w = pack_encoder_weights(fixture_weights()[0])
    seqs = []
    for s in range(n_seq):
        d = psfm_synth.synth_sequence_torch(T, H, W, seed=s, sigma=0.05, n_occluders=2, stride2=False, device="cuda")
        seqs.append((d["flows_f"], d["flows_b"], None, None))
    if n_seq > 1:
        ctxs, infos = run_connect_batch(seqs, 1.0, S["ratio"])
    else:
        infos = [run_connect(seqs[0][0], seqs[0][1], None, None, 1.0, S["ratio"], return_device=True)]
        ctxs = [_hip.context()]
    del seqs
    gen = torch.Generator(device="cuda")
    gen.manual_seed(17)
    depth = {(s, f0): torch.rand((n,) + INPUT_SIZE, generator=gen, device="cuda", dtype=torch.float32)
             for s in range(n_seq) for f0, n in window_ranges(T, a.window)}
    raw_hw = (H, W)
    rows = {}

    def single():
        ms = []
        for s, ctx in enumerate(ctxs):
            predict = device_predictor(enc_w, dec_w, lambda t, s=s: depth[(s, int(t[0]))], INPUT_SIZE, ctx=ctx)
            ms.append(label_trajectories(T, a.window, raw_hw, INPUT_SIZE, a.traj_max_num, predict, seed=a.seed, ctx=ctx))
        return ms

    def batched():
        return label_sequences_batched(ctxs, [T] * n_seq, a.window, raw_hw, INPUT_SIZE, a.traj_max_num, enc_w, dec_w,
                                       lambda s, t: depth[(s, int(t[0]))], seed=a.seed, max_rows=a.max_rows)
    routes = {"single": single, "batched": batched}

    if a.only:
        for _ in range(a.calls):
            routes[a.only]()
        torch.cuda.synchronize()
        return {"only": a.only, "calls": a.calls, "shape": a.shape}

    def sets(ms):
        # (every context's set is read before the next route begins: a context holds one labelled set)
        return [[t.cpu().numpy() for t in m.finish()] for m in ms]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ms = fn()                                               # (the last finish() synchronises the stream)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), ms

    want = None
    equal = True
    for r in ("single", "batched"):
        for _ in range(a.warmup):
            _, ms = timed(routes[r])
        got = sets(ms)
        rows[r] = [[int(i.numel()) for i in m.window_ids] for m in ms]
        if want is None:
            want = got
        else:
            equal = all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for g, w_ in zip(got, want) for x, y in zip(g, w_))
    t = {"single": [], "batched": []}
    for _ in range(a.rounds):
        for r in ("single", "batched"):
            t[r].append(timed(routes[r])[0])
    res = {"mode": "stage", "shape": a.shape, "workload": "%d x %dx%d x %d frames, sample_ratio %d, window %d, traj_max_num %d, input %dx%d"
           % (n_seq, H, W, T, S["ratio"], a.window, a.traj_max_num, INPUT_SIZE[0], INPUT_SIZE[1]),
           "trajectories": [int(i.n_traj) for i in infos], "windows_per_sequence": len(window_ranges(T, a.window)),
           "rows_per_window_seq0": rows["single"][0], "rows_all_windows": int(sum(sum(r) for r in rows["single"])),
           "same_rows": rows["single"] == rows["batched"], "bytes_equal": bool(equal), "rounds": a.rounds}
    for r in ("single", "batched"):
        v = np.array(t[r])
        res[r + "_ms"] = {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "spread": float(v.max() - v.min()),
                          "runs": [float(x) for x in v]}
    res["single_over_batched"] = res["single_ms"]["median"] / res["batched_ms"]["median"]
    res["difference_ms"] = res["single_ms"]["median"] - res["batched_ms"]["median"]
    res["three_spreads_ms"] = 3.0 * max(res["single_ms"]["spread"], res["batched_ms"]["spread"])
    res["batched_is_faster"] = bool(res["difference_ms"] > res["three_spreads_ms"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["decoder", "stage"], default="decoder")
    ap.add_argument("--windows", type=int, default=16)
    ap.add_argument("--tracks", type=int, default=2000)
    ap.add_argument("--shape", choices=sorted(SHAPES), default="a")
    ap.add_argument("--window", type=int, default=10)
    ap.add_argument("--traj-max-num", type=int, default=100000)
    ap.add_argument("--max-rows", type=int, default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default=None, help="run --calls calls of one route and exit (for a kernel trace)")
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "decoder_batch.py measures on the GPU"
    res = decoder_mode(a) if a.mode == "decoder" else stage_mode(a)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fp:
            fp.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
