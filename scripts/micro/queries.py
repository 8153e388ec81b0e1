#!/usr/bin/env python3
"""psfm_track_queries (csrc/psfm_query.hip) at the headline size against the composed form -- all there was before it.

  flows     --frames flow maps of --width x --height (psfm_synth.synth_realistic_torch), both directions; the forward stack's
            occlusion maps from flow_check_device
  sizes     "grid":   the points of the stride-2 grid at t = 0 (518 400 at 1920 x 1080)
            "random": --random queries uniform in [-1, W] x [-1, H] with t uniform in 0 .. n_flows
  new       one run_track_queries call (forward), wall time around the synchronising call; the tracking kernel alone from the
            context's profiler (HIP events), as bytes per second against 32 B of taps + 4 mask bytes + a 16 B store per step and
            query -- at sector granularity 4 x 32 B + 4 x 32 B + 16 B when no two taps share a sector
  composed  per frame: psfm_grid_sample of the flow, psfm_grid_sample of the occlusion map, the torch elementwise step, on the
            positions still alive (one host round trip per frame for their indices)
The two forms are ALTERNATED, --reps runs each after one warm-up pair; both times are reported with their spread (max - min).
The composed form gives the same bits, which is asserted once per size.  Prints one JSON line (--out also writes it to a file)."""
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
    return {"median_ms": float(np.median(a)), "min_ms": float(a[0]), "max_ms": float(a[-1]), "spread_ms": float(a[-1] - a[0])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
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
    d = psfm_synth.synth_realistic_torch(n + 1, H, W, seed=3, stride2=False, device="cuda", **psfm_synth.REALISTIC)
    ff, fb = d["flows_f"], d["flows_b"]
    occ = flow_check_device(ff, fb, 1.0)[1]
    del fb
    occ_f32 = occ.to(torch.float32).unsqueeze(-1).contiguous()          # (n,H,W,1): what psfm_grid_sample reads (set-up, not timed)
    dev = ff.device

    def sample(m, c, p):
        out = torch.empty((p.shape[0], c), dtype=torch.float32, device=dev)
        _hip.check(L.psfm_grid_sample(ctx.handle, _hip.ptr(m), c, H, W, _hip.ptr(p), p.shape[0], _hip.ptr(out), _hip.current_stream_ptr(ctx.device)))
        return out

    def composed(xy, t):
        """(length (Q,), slab (n+1,Q,2)) of forward tracking, one frame at a time."""
        Q = xy.shape[0]
        cur, tcur = xy.clone(), t.to(torch.int64).clone()
        live = tcur < n
        slab = torch.zeros((n + 1, Q, 2), dtype=torch.float64, device=dev)
        slab[tcur, torch.arange(Q, device=dev)] = xy
        length = torch.ones(Q, dtype=torch.int32, device=dev)
        for f in range(n):
            idx = torch.nonzero(live & (tcur == f)).squeeze(1)           # (the host round trip of the frame)
            if idx.numel() == 0:
                continue
            p = cur[idx].contiguous()
            fs = sample(ff[f], 2, p)
            oc = sample(occ_f32[f], 1, p)
            nxt = p + fs.to(torch.float64)
            alive = (nxt[:, 0] > 0) & (nxt[:, 0] < W - 1) & (nxt[:, 1] > 0) & (nxt[:, 1] < H - 1) & ~(oc[:, 0] > 0.1)
            go = idx[alive]
            cur[go] = nxt[alive]
            tcur[go] = f + 1
            slab[f + 1, go] = nxt[alive]
            length[go] += 1
            live[idx[~alive]] = False
            live[go] = f + 1 < n
        return length, slab

    rng = np.random.default_rng(11)
    yy, xx = np.mgrid[0:H:2, 0:W:2]
    sizes = {
        "grid": (np.stack([xx.ravel(), yy.ravel()], 1).astype(np.float64), np.zeros(xx.size, np.int32)),
        "random": (rng.uniform([-1.0, -1.0], [float(W), float(H)], size=(a.random, 2)), rng.integers(0, n + 1, size=a.random).astype(np.int32)),
    }
    res = {"shape": [n, H, W], "bytes_per_step": {"algorithmic": 52, "sectors": 4 * 32 + 4 * 32 + 16}}
    for name, (xy_h, t_h) in sizes.items():
        xy, t = torch.from_numpy(xy_h).to(dev), torch.from_numpy(t_h).to(dev)
        t_new, t_old, t_kernel, t_csr = [], [], [], []
        for r in range(1 + a.reps):
            ctx.set_profiling(1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            info = run_track_queries(xy, t, flows=ff, occ=occ, return_device=True)
            t1 = time.perf_counter()
            prof, prof_csr = ctx.profile()["chain_step"], ctx.profile()["finalize"]
            ctx.set_profiling(0)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            length, slab = composed(xy, t)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            if r >= 1:
                t_new.append((t1 - t0) * 1e3); t_old.append((t3 - t2) * 1e3); t_kernel.append(prof["total_ms"]); t_csr.append(prof_csr["total_ms"])
        # the same bits
        R = _result_to_host(ctx, info)
        assert np.array_equal(R.length, length.cpu().numpy()) and np.array_equal(R.birth, t_h)
        f_idx = torch.arange(n + 1, device=dev)[None, :]
        inside = (f_idx >= t[:, None]) & (f_idx < (t[:, None] + length[:, None]))          # (Q, n+1)
        want = slab.permute(1, 0, 2)[inside]
        got = torch.from_numpy(R.xy).to(dev)
        assert want.shape == got.shape and bool((want.view(torch.int64) == got.view(torch.int64)).all())
        steps = int(info.n_points) - len(t_h)                 # alive steps stored; every query that starts also makes one last, dead step
        k_ms = float(np.median(t_kernel))
        new, old = stats(t_new), stats(t_old)
        res[name] = {"queries": len(t_h), "points": int(info.n_points), "new_call": new, "composed": old,
                     "ratio_of_medians": old["median_ms"] / new["median_ms"],
                     "beats_by_more_than_three_spreads": bool(old["median_ms"] - new["median_ms"] > 3 * max(new["spread_ms"], old["spread_ms"])),
                     "track_kernel": dict(stats(t_kernel), alive_steps=steps,
                                          gb_per_s_algorithmic=52 * steps / k_ms / 1e6, gb_per_s_sectors=272 * steps / k_ms / 1e6),
                     "lengths_to_csr": stats(t_csr)}       # plan + scan + offsets + the point count's read-back + gather
        # the open variant "order the queries by tile before the launch", measured from outside: the same queries ordered by
        # (t, 8 x 8 tile) with torch, the tracking kernel alone.  (The grid comes in row order, one t.)
        tile = (xy[:, 1].clamp(0, H - 1).to(torch.int64) // 8) * ((W + 7) // 8) + xy[:, 0].clamp(0, W - 1).to(torch.int64) // 8
        order = torch.argsort(t.to(torch.int64) * (1 << 40) + tile, stable=True)
        xy_s, t_s = xy[order].contiguous(), t[order].contiguous()
        t_sorted = []
        for r in range(1 + a.reps):
            ctx.set_profiling(1)
            info_s = run_track_queries(xy_s, t_s, flows=ff, occ=occ, return_device=True)
            if r >= 1:
                t_sorted.append(ctx.profile()["chain_step"]["total_ms"])
            ctx.set_profiling(0)
        assert int(info_s.n_points) == int(info.n_points)
        res[name]["track_kernel_ordered_by_frame_and_tile"] = stats(t_sorted)
        del slab, want, got, inside
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
