#!/usr/bin/env python3
"""psfm_track_queries_optimize (csrc/psfm_query_pc.hip) against the composed form on the same input -- all there was before it.

  flows     --frames flow maps of --width x --height with their stride-2 stacks (psfm_synth.synth_realistic_torch), forward direction;
            the occlusion maps of both strides from flow_check_device
  sizes     "grid":   the points of the stride-2 grid at t = 0 (518 400 at 1920 x 1080)
            "random": --random queries uniform in [-1, W] x [-1, H] with t uniform in 0 .. n_flows
  new       one run_track_queries call with the stride-2 stacks, wall time around the synchronising call; from the context's profiler
            (HIP events) the step launches and the solves of the call
  composed  per frame: psfm_grid_sample of the flow and of the occlusion map + the torch elementwise step on the active queries, then
            psfm_grid_sample of flow01, flow02 and occ02 at p0 + torch for refs / scale + psfm_optimize_location on the rows, in query
            order, and a torch scatter (one host round trip per frame for the indices, one per solve)
The two forms are ALTERNATED, --reps runs each after one warm-up pair; both times are reported with their spread (max - min).  Whether
lengths and solve counts are equal, and the largest position difference, are reported per size (the tests assert them at their
sizes).  Prints one JSON line (--out also writes it to a file)."""
import argparse
import ctypes
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
    return {"median_ms": float(np.median(a)), "min_ms": float(a[0]), "max_ms": float(a[-1]), "spread_ms": float(a[-1] - a[0])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--random", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    import psfm_synth
    from point_trajectory import _hip
    from point_trajectory.trajectory import run_track_queries, _result_to_host
    from point_trajectory.utils import flow_check_device
    ctx = _hip.context()
    L = _hip.lib()
    n, H, W = a.frames, a.height, a.width
    d = psfm_synth.synth_realistic_torch(n + 1, H, W, seed=3, stride2=True, device="cuda", **psfm_synth.REALISTIC)
    ff, fb, f2, b2 = d["flows_f"], d["flows_b"], d["flows_f2"], d["flows_b2"]
    occ = flow_check_device(ff, fb, 1.0)[1]
    occ2 = flow_check_device(f2, b2, 1.0)[1]
    del fb, b2
    occ_f32 = occ.to(torch.float32).unsqueeze(-1).contiguous()          # (n,H,W,1): what psfm_grid_sample reads (set-up, not timed)
    occ2_f32 = occ2.to(torch.float32).unsqueeze(-1).contiguous()
    dev = ff.device
    sp = lambda: _hip.current_stream_ptr(ctx.device)

    def sample(m, c, p):
        out = torch.empty((p.shape[0], c), dtype=torch.float32, device=dev)
        _hip.check(L.psfm_grid_sample(ctx.handle, _hip.ptr(m), c, H, W, _hip.ptr(p), p.shape[0], _hip.ptr(out), sp()))
        return out

    def composed(xy, t):
        """(length (Q,), slab (n+1,Q,2), solves) of forward tracking with the solve, one frame at a time."""
        Q = xy.shape[0]
        t64 = t.to(torch.int64)
        slab = torch.zeros((n + 1, Q, 2), dtype=torch.float64, device=dev)
        slab[t64, torch.arange(Q, device=dev)] = xy
        length = torch.ones(Q, dtype=torch.int64, device=dev)
        n_solves = 0
        st = _hip.SolveStats()
        for f in range(n):
            idx = torch.nonzero(t64 + length - 1 == f).squeeze(1)        # (the host round trip of the frame)
            if idx.numel() == 0:
                continue
            p = slab[f, idx].contiguous()
            fs = sample(ff[f], 2, p)
            oc = sample(occ_f32[f], 1, p)
            nxt = p + fs.to(torch.float64)
            alive = (nxt[:, 0] > 0) & (nxt[:, 0] < W - 1) & (nxt[:, 1] > 0) & (nxt[:, 1] < H - 1) & ~(oc[:, 0] > 0.1)
            go = idx[alive]
            slab[f + 1, go] = nxt[alive]
            length[go] += 1
            if f < 1:
                continue
            rows = go[length[go] >= 3]                                    # in query order
            k = int(rows.numel())                                         # (the host round trip of the solve)
            if k == 0:
                continue
            p0 = slab[f - 1, rows].contiguous()
            uv12 = torch.cat([slab[f, rows], slab[f + 1, rows]], 1).contiguous()
            f01, f02, o02 = sample(ff[f - 1], 2, p0), sample(f2[f - 1], 2, p0), sample(occ2_f32[f - 1], 1, p0)[:, 0]
            nrm = torch.sqrt(f02[:, 0] * f02[:, 0] + f02[:, 1] * f02[:, 1])
            scale = ((1.0 - o02) * (nrm < 20.0).to(torch.float32)).to(torch.float64).contiguous()
            ref1, ref2 = (p0 + f01.to(torch.float64)).contiguous(), (p0 + f02.to(torch.float64)).contiguous()
            out = torch.empty((k, 4), dtype=torch.float64, device=dev)
            _hip.check(L.psfm_optimize_location(ctx.handle, _hip.ptr(uv12), _hip.ptr(ref1), _hip.ptr(ref2), _hip.ptr(scale), _hip.ptr(ff[f]),
                                                k, W, H, _hip.ptr(out), ctypes.byref(st), sp()))
            slab[f, rows] = out[:, :2]
            slab[f + 1, rows] = out[:, 2:]
            n_solves += 1
        return length, slab, n_solves

    rng = np.random.default_rng(11)
    yy, xx = np.mgrid[0:H:2, 0:W:2]
    sizes = {
        "grid": (np.stack([xx.ravel(), yy.ravel()], 1).astype(np.float64), np.zeros(xx.size, np.int32)),
        "random": (rng.uniform([-1.0, -1.0], [float(W), float(H)], size=(a.random, 2)), rng.integers(0, n + 1, size=a.random).astype(np.int32)),
    }
    res = {"shape": [n, H, W]}
    for name, (xy_h, t_h) in sizes.items():
        xy, t = torch.from_numpy(xy_h).to(dev), torch.from_numpy(t_h).to(dev)
        t_new, t_old, t_step, t_solve = [], [], [], []
        for r in range(1 + a.reps):
            ctx.set_profiling(1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            info = run_track_queries(xy, t, flows=ff, occ=occ, flows_f2=f2, occ_f2=occ2, return_device=True)
            t1 = time.perf_counter()
            prof = ctx.profile()
            ctx.set_profiling(0)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            length, slab, n_solves = composed(xy, t)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            if r >= 1:
                t_new.append((t1 - t0) * 1e3); t_old.append((t3 - t2) * 1e3)
                t_step.append(prof["chain_step"]["total_ms"]); t_solve.append(prof["solver"]["total_ms"])
        R = _result_to_host(ctx, info)
        same_lengths = bool(np.array_equal(R.length, length.cpu().numpy()) and np.array_equal(R.birth, t_h) and int(info.n_solves) == n_solves)
        err = None
        if same_lengths:
            f_idx = torch.arange(n + 1, device=dev)[None, :]
            inside = (f_idx >= t[:, None]) & (f_idx < (t[:, None] + length[:, None]))          # (Q, n+1)
            err = float((slab.permute(1, 0, 2)[inside] - torch.from_numpy(R.xy).to(dev)).abs().max())
            del inside
        new, old = stats(t_new), stats(t_old)
        res[name] = {"queries": len(t_h), "points": int(info.n_points), "solves": n_solves, "solver_iterations": int(info.solver_iterations),
                     "new_call": new, "composed": old, "ratio_of_medians": old["median_ms"] / new["median_ms"],
                     "beats_by_more_than_three_spreads": bool(old["median_ms"] - new["median_ms"] > 3 * max(new["spread_ms"], old["spread_ms"])),
                     "same_lengths_and_solves": same_lengths, "max_abs_difference_px": err, "step_launches": stats(t_step), "solves_ms": stats(t_solve)}
        del slab
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
