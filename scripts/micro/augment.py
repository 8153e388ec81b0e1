#!/usr/bin/env python3
"""psfm_traj_augment (csrc/psfm_augment.hip) against the reference's own sequence of torch operations, on the same device and the
same tensors.

Workload (defaults): K = 100 000 trajectories (the reference's traj_max_num), L = 10 frames, network input (240,424); seeded
coordinates with 30 % padded slots, iid uniform depth.
  fused   one psfm_traj_augment launch: reads the f64 window tensors psfm_window_sample writes, writes [1,10,K,L] f32
  torch   depth_project + gather_point + augment_traj of motion_seg/core/network/traj_oa_depth.py:84-114 restated as torch calls
          on f32 device tensors already in the reference's layout ([1,2,K,L], [1,1,K,L], [1,1,h,w,L]); --with-glue puts the casts
          and permutes of main_motion_segmentation.py:71-78 from the f64 window tensors inside the span as well
Both are warmed up, then timed as --reps repetitions between two HIP events on the stream (the span divided by --reps), --rounds
times, alternating; the median round is reported with min and max.  Launch counts come from torch.profiler (kernel events of one
call, --count-launches).  Algorithmic bytes = (24 + 4 + 40) * K * L plus the depth maps once; GB/s = those bytes over the call time.  The two outputs
are compared while both are at hand (reported, not asserted: the tests pin the kernel to the reference's CPU run).  Prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "particle-sfm_amd"))


def torch_reference(depth, traj, mask, kinv_t, xy_t):
    """traj_oa_depth.depth_project / gather_point / augment_traj as torch calls; depth [1,1,h,w,L], traj [1,2,N,L], mask [1,1,N,L]."""
    import torch
    b, _, h, w, l = depth.shape
    depth_b = depth.permute(0, 4, 1, 2, 3).reshape(b * l, 1, h * w)
    point_3d = depth_b * kinv_t.bmm(xy_t)
    points = point_3d.reshape(b, l, 3, h, w).permute(0, 2, 3, 4, 1)                   # [B,3,H,W,L]
    points_src = points.permute(0, 4, 1, 2, 3).reshape(b * l, 3, h * w)
    t = traj.permute(0, 3, 1, 2).reshape(b * l, 2, -1)
    idx = (t[:, 1, :] * h).to(torch.int) * w + (t[:, 0, :] * w).to(torch.int)
    idx = idx.unsqueeze(1).repeat(1, 3, 1).to(torch.int64).clamp(0, h * w - 1)
    traj_3d = torch.gather(points_src, dim=-1, index=idx).reshape(b, l, 3, -1).permute(0, 2, 3, 1)
    motion_2d = torch.zeros_like(traj)
    motion_2d[:, :, :, :-1] = (traj[:, :, :, 1:] - traj[:, :, :, :-1]) * (1.0 - mask[:, :, :, 1:])
    motion_3d = torch.zeros_like(traj_3d)
    motion_3d[:, :, :, :-1] = (traj_3d[:, :, :, 1:] - traj_3d[:, :, :, :-1]) * (1.0 - mask[:, :, :, 1:])
    return torch.cat([traj, motion_2d, traj_3d, motion_3d], dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=100000)
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--width", type=int, default=424)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--with-glue", action="store_true")
    ap.add_argument("--count-launches", action="store_true", help="count the kernels of one call of each with torch.profiler")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()

    import torch
    from point_trajectory import _hip
    from psfm_motion_seg.augment import reference_kinv

    assert torch.cuda.is_available(), "augment.py measures on the GPU"
    K, L, h, w = a.tracks, a.frames, a.height, a.width
    rng = np.random.default_rng(0)
    mask_h = (rng.uniform(size=(K, L, 1)) < 0.3).astype(np.float64)
    xy_h = np.clip(rng.uniform(-0.05, 1.05, size=(K, L, 2)), 0.0, 1.0) * (1.0 - mask_h)
    xy, mask = torch.from_numpy(xy_h).cuda(), torch.from_numpy(mask_h).cuda()
    depth = torch.from_numpy(rng.uniform(size=(L, h, w)).astype(np.float32)).cuda()
    kinv = np.ascontiguousarray(reference_kinv((h, w)))
    ctx = _hip.context(0)
    lib, sp = _hip.lib(), _hip.current_stream_ptr(0)
    out = torch.empty((1, 10, K, L), dtype=torch.float32, device="cuda")

    def fused():
        _hip.check(lib.psfm_traj_augment(ctx.handle, _hip.ptr(xy), _hip.ptr(mask), _hip.ptr(depth), K, L, h, w, kinv.ctypes.data,
                                         _hip.ptr(out), sp))
        return out

    # image_grid (:72-82), once, as the reference's constructor does
    xx, yy = np.meshgrid(np.arange(w), np.arange(h))
    grid = np.stack([xx, yy, np.ones((h, w))], axis=-1)
    xy_t = torch.from_numpy(grid).reshape(-1, 3).permute(1, 0).unsqueeze(0).float().cuda()
    kinv_t = torch.from_numpy(kinv.astype(np.float64)).unsqueeze(0).float().cuda()

    def glue():
        return (depth.permute(1, 2, 0)[None, None].float(), xy.permute(2, 0, 1).unsqueeze(0).float(), mask.permute(2, 0, 1).unsqueeze(0).float())
    pre = tuple(t.contiguous() for t in glue())

    def reference():
        return torch_reference(*(glue() if a.with_glue else pre), kinv_t, xy_t)

    # (the fixtures pin the fused kernel to the reference's CPU run; the torch ops on the device need not round like it: rocBLAS's bmm)
    got, want = fused(), reference()
    equal, max_diff = bool(torch.equal(got, want)), float((got - want).abs().max())

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

    nbytes = (24 + 4 + 40) * K * L + 4 * L * h * w
    med = np.median(t, 0)
    res = {"workload": "K=%d L=%d input (%d,%d), 30%% padded" % (K, L, h, w), "reps": a.reps, "rounds": a.rounds,
           "fused_us": float(med[0]), "fused_us_min_max": [float(t[:, 0].min()), float(t[:, 0].max())],
           "torch_us": float(med[1]), "torch_us_min_max": [float(t[:, 1].min()), float(t[:, 1].max())],
           "torch_includes_glue": bool(a.with_glue), "torch_over_fused": float(med[1] / med[0]),
           "algorithmic_bytes": int(nbytes), "fused_GBps_on_algorithmic_bytes": float(nbytes / med[0] / 1e3),
           "torch_GBps_on_algorithmic_bytes": float(nbytes / med[1] / 1e3),
           "torch_point_cloud_bytes": int(4 * 3 * h * w * L), "fused_launches": n_fused, "fused_kernels": names_fused,
           "torch_launches": n_ref, "outputs_bit_equal": equal, "outputs_max_abs_diff": max_diff}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fp:
            fp.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
