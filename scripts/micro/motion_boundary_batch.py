#!/usr/bin/env python3
"""The motion-boundary option inside psfm_connect_batch (csrc/psfm_batch.hip, psfm_motion_boundary.hip, psfm_solver_batch_mb.hip).

  a  --seqs-a (16,64) sequences of 480 x 854 x 51 frames, sample_ratio 4, track mode: run_connect_batch(..., motion_boundary=True)
     with mb_engine="loop" (one psfm_connect per sequence: the route before the batched launches carried the option) against
     mb_engine="batch" (psfm_connect_batch with the option on in every context).
  b  16 sequences of 436 x 1024 x 50 frames, sample_ratio 2, with path consistency, the same two routes.
  c  the kill maps alone at 16 x 50 x 480 x 854: ONE psfm_kill_map_batch launch against a loop of psfm_kill_map calls and against a
     device-to-device copy of the same byte count (10 B per pixel: 8 B flow + 1 B occlusion read, 1 B written), between HIP events.
One process, the routes ALTERNATED, --reps rounds after --warmup, wall clock around calls that end in a synchronise (a, b).  Flows
are psfm_synth.synth_realistic_torch without its error terms; a batch holds --distinct different sequences, repeated.  The routes'
results are compared at the timed sizes (a: bit for bit; b: ids and lengths bit for bit, positions to 1e-9 px; c: byte for byte).
Prints one JSON line (--out also writes it to a file)."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "particle-sfm_amd"))


def stats(ms):
    a = np.sort(np.asarray(ms, np.float64))
    return {"median_ms": float(np.median(a)), "min_ms": float(a[0]), "max_ms": float(a[-1])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="abc")
    ap.add_argument("--seqs-a", default="16,64")
    ap.add_argument("--seqs-b", type=int, default=16)
    ap.add_argument("--frames-a", type=int, default=51)
    ap.add_argument("--frames-b", type=int, default=50)
    ap.add_argument("--size-a", default="480x854")
    ap.add_argument("--size-b", default="436x1024")
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--thres", type=float, default=0.02)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    import psfm_synth
    from point_trajectory import _hip
    from point_trajectory.trajectory import run_connect_batch, _result_to_host, kill_map_batch
    from point_trajectory.utils import flow_check_device
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    res = {"thres": a.thres, "reps": a.reps, "warmup": a.warmup}
    synth = dict(psfm_synth.REALISTIC, err_sigma=0.0, outlier_frac=0.0)

    def sequences(n_seq, frames, H, W, opt):
        base = [psfm_synth.synth_realistic_torch(frames, H, W, seed=11 + k, stride2=opt, device="cuda", **synth) for k in range(min(a.distinct, n_seq))]
        return [(d["flows_f"], d["flows_b"], d["flows_f2"] if opt else None, d["flows_b2"] if opt else None) for d in (base[k % len(base)] for k in range(n_seq))]

    def connect(seqs, ratio, engine):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctxs, infos = run_connect_batch(seqs, 1.0, ratio, motion_boundary=True, mb_thres=a.thres, mb_engine=engine)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, ctxs, infos

    def routes(seqs, ratio, opt):
        t = {"loop": [], "batch": []}
        out, modes = {}, {}
        for r in range(a.warmup + a.reps):
            for engine in ("loop", "batch"):
                ms, ctxs, infos = connect(seqs, ratio, engine)
                if r >= a.warmup:
                    t[engine].append(ms)
                if r == a.warmup + a.reps - 1:
                    out[engine] = [_result_to_host(c, i) for c, i in zip(ctxs, infos)]
                    modes[engine] = sorted(set(int(i.chain_mode) for i in infos))
        worst = 0.0
        for A, B in zip(out["loop"], out["batch"]):
            assert np.array_equal(A.birth, B.birth) and np.array_equal(A.length, B.length), "the routes disagree"
            if opt:
                worst = max(worst, float(np.abs(A.xy - B.xy).max()))
                assert worst <= 1e-9, worst
            else:
                assert np.array_equal(A.xy, B.xy), "the routes disagree"
        n = len(seqs)
        sl, sb = stats(t["loop"]), stats(t["batch"])
        spread = max(sl["max_ms"] - sl["min_ms"], sb["max_ms"] - sb["min_ms"])
        return {"n_seq": n, "loop": sl, "batch": sb, "loop_ms_per_seq": sl["median_ms"] / n, "batch_ms_per_seq": sb["median_ms"] / n,
                "speedup_of_medians": sl["median_ms"] / sb["median_ms"], "difference_ms": sl["median_ms"] - sb["median_ms"],
                "larger_spread_ms": spread, "difference_over_spread": (sl["median_ms"] - sb["median_ms"]) / spread if spread > 0 else float("inf"),
                "chain_modes": modes, "max_dxy": worst,
                "trajectories": int(sum(len(R) for R in out["batch"])), "points": int(sum(R.n_points for R in out["batch"]))}

    if "a" in a.parts:
        H, W = (int(x) for x in a.size_a.split("x"))
        res["a"] = {"shape": [a.frames_a, H, W], "sample_ratio": 4, "runs": []}
        for n_seq in (int(x) for x in a.seqs_a.split(",")):
            res["a"]["runs"].append(routes(sequences(n_seq, a.frames_a, H, W, False), 4, False))
            torch.cuda.empty_cache()
    if "b" in a.parts:
        H, W = (int(x) for x in a.size_b.split("x"))
        res["b"] = dict(routes(sequences(a.seqs_b, a.frames_b, H, W, True), 2, True), shape=[a.frames_b, H, W], sample_ratio=2)
        torch.cuda.empty_cache()
    if "c" in a.parts:
        H, W = (int(x) for x in a.size_a.split("x"))
        B, n = 16, a.frames_a - 1
        ctx = _hip.context()
        L, sp = _hip.lib(), _hip.current_stream_ptr(ctx.device)
        fl, oc = [], []
        for k in range(B):
            d = psfm_synth.synth_realistic_torch(n + 1, H, W, seed=31 + k % a.distinct, stride2=False, device="cuda", **synth)
            fl.append(d["flows_f"].clone()); oc.append(flow_check_device(d["flows_f"], d["flows_b"], 1.0)[1].contiguous())
        out_b = [torch.empty_like(o) for o in oc]
        out_l = [torch.empty_like(o) for o in oc]
        nbytes = 10 * B * n * H * W
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)

        def loop():
            for f, o, k in zip(fl, oc, out_l):
                _hip.check(L.psfm_kill_map(ctx.handle, _hip.ptr(f), _hip.ptr(o), n, H, W, a.thres, _hip.ptr(k), sp))
        tb, tl, tc = [], [], []
        for r in range(a.warmup + 1 + 2 * a.reps):
            x, y, z = timed(lambda: kill_map_batch(fl, oc, a.thres, out=out_b)), timed(loop), timed(lambda: dst.copy_(src))
            if r >= a.warmup + 1:
                tb.append(x); tl.append(y); tc.append(z)
        assert all(torch.equal(p, q) for p, q in zip(out_b, out_l)), "the batched launch and the loop disagree"
        res["c"] = {"shape": [B, n, H, W], "bytes": nbytes, "batch": stats(tb), "loop_of_16": stats(tl), "copy_of_half": stats(tc),
                    "batch_over_copy": float(np.median(tb) / np.median(tc)), "loop_over_batch": float(np.median(tl) / np.median(tb)),
                    "batch_gb_per_s": nbytes / np.median(tb) / 1e6,
                    "boundary_density": float(torch.stack([(k >> 1).to(torch.float32).mean() for k in out_b]).mean())}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
