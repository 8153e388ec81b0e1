#!/usr/bin/env python3
"""The motion-boundary option (csrc/psfm_motion_boundary.hip) at the headline size.

  kernels   psfm_motion_boundary (8 B read + 1 B written per pixel) and psfm_kill_map (8 B + 1 B read, 1 B written) over
            --frames flow maps of --width x --height, each between two HIP events, ALTERNATED with a torch copy_ between two device
            buffers of half the kernel's byte count (so that the copy reads + writes that count); --reps rounds after --warmup.
  connect   one psfm_connect call (flow_check + track + finalize) on psfm_synth.synth_realistic_torch flows WITHOUT the error
            terms, option on against option off, both with one launch per frame (chain mode 1), alternated; trajectory and point
            counts beside the times -- the workloads differ (more tracks die, more are born), so this is a cost, not a ratio to meet.
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
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--connect-reps", type=int, default=3)
    ap.add_argument("--thres", type=float, default=0.02)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    import psfm_synth
    from point_trajectory import _hip
    from point_trajectory.trajectory import run_connect
    ctx = _hip.context()
    L, sp = _hip.lib(), _hip.current_stream_ptr(ctx.device)
    n, H, W = a.frames, a.height, a.width
    d = psfm_synth.synth_realistic_torch(n + 1, H, W, seed=3, stride2=False, device="cuda",
                                         **dict(psfm_synth.REALISTIC, err_sigma=0.0, outlier_frac=0.0))
    ff, fb = d["flows_f"], d["flows_b"]
    N = n * H * W
    occ = (torch.rand((n, H, W), device="cuda") < 0.05).to(torch.uint8)
    out = torch.empty((n, H, W), dtype=torch.uint8, device="cuda")
    res = {"shape": [n, H, W], "thres": a.thres}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    kernels = {
        "mask": (9 * N, lambda: _hip.check(L.psfm_motion_boundary(ctx.handle, _hip.ptr(ff), n, H, W, a.thres, _hip.ptr(out), sp))),
        "kill_map": (10 * N, lambda: _hip.check(L.psfm_kill_map(ctx.handle, _hip.ptr(ff), _hip.ptr(occ), n, H, W, a.thres, _hip.ptr(out), sp))),
    }
    for name, (nbytes, fn) in kernels.items():
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        tk, tc = [], []
        for r in range(a.warmup + a.reps):
            k, c = timed(fn), timed(lambda: dst.copy_(src))
            if r >= a.warmup:
                tk.append(k); tc.append(c)
        res[name] = {"bytes": nbytes, "kernel": stats(tk), "copy_of_half": stats(tc),
                     "ratio_of_medians": float(np.median(tk) / np.median(tc)), "gb_per_s": nbytes / np.median(tk) / 1e6}
        del src, dst
    res["mask_density"] = float(out.bitwise_right_shift(1).to(torch.float32).mean())
    del occ, out
    torch.cuda.empty_cache()

    ctx.set_chain_mode(1)
    try:
        t = {False: [], True: []}
        info = {}
        for r in range(1 + a.connect_reps):
            for mb in (False, True):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                i = run_connect(ff, fb, None, None, 1.0, 2, return_device=True, motion_boundary=mb, mb_thres=a.thres)
                torch.cuda.synchronize()
                if r >= 1:
                    t[mb].append((time.perf_counter() - t0) * 1e3)
                info[mb] = {"trajectories": int(i.n_traj), "points": int(i.n_points), "chain_mode": int(i.chain_mode)}
        res["connect_chain_mode_1"] = {"option_off": dict(stats(t[False]), **info[False]), "option_on": dict(stats(t[True]), **info[True])}
    finally:
        ctx.set_chain_mode(0)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
