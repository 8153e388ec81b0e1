#!/usr/bin/env python3
"""psfm_traj_eval_counts and psfm_traj_vote_labels (csrc/psfm_ground_truth.hip) at the headline size.

Workload: psfm_synth 1080x1920, 101 frames, r = 2 -> psfm_connect -> label_trajectories over windows of 10 frames (--cap 0:
uncapped, every saved point is labelled; seeded random predictions) -> the labelled set in the context.  Ground truth: one u8 map per
frame with moving discs and a soft rim (bytes other than 0 and 255), built on the device.  Timed with HIP events on the stream, after
warm-up, median of --reps repetitions:
  eval      psfm_traj_eval_counts over the context's labelled set (the memset of the counts and the one launch)
  vote      psfm_traj_vote_labels over the window tensors of frames [0, --vote-frames) (uncapped), masks thresholded to 0 / 1;
            the span includes the call's own read-back of its flag
Checks while at it: the counts add up to the number of labelled points, two calls give identical counts, frame 0's counts and the
first --check-rows votes equal the NumPy restatement of the test suite (tests/_ground_truth_np.py).  Prints one JSON line; the
algorithmic bytes are part of it (per labelled point 4 B frame id + 16 B xy + 1 B label read and four byte gathers from its frame's
map; per window element 8 B mask + 16 B xy read, one byte gather per present element).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "particle-sfm_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def disc_maps(T, H, W, device):
    """(T,H,W) u8 on the device: 255 = static, 0 = dynamic, a 3 px ramp at the rim of three moving discs."""
    import torch
    g = torch.Generator(device="cpu")
    g.manual_seed(5)
    c = torch.rand(3, 2, generator=g) * 0.6 + 0.2
    v = (torch.rand(3, 2, generator=g) - 0.5) * 4.0
    rad = (torch.rand(3, generator=g) * 0.1 + 0.12) * min(H, W)
    yy = torch.arange(H, device=device, dtype=torch.float32)[:, None]
    xx = torch.arange(W, device=device, dtype=torch.float32)[None, :]
    out = torch.empty((T, H, W), dtype=torch.uint8, device=device)
    for t in range(T):
        m = torch.zeros((H, W), device=device)
        for b in range(3):
            dist = torch.hypot(xx - (float(c[b, 0]) * W + float(v[b, 0]) * t), yy - (float(c[b, 1]) * H + float(v[b, 1]) * t))
            m = torch.maximum(m, ((float(rad[b]) + 1.5 - dist) / 3.0).clamp(0.0, 1.0))
        out[t] = torch.round(255.0 * (1.0 - m)).to(torch.uint8)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=101)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--window", type=int, default=10)
    ap.add_argument("--cap", type=int, default=0, help="traj_max_num per window; 0 = uncapped")
    ap.add_argument("--vote-frames", type=int, default=10)
    ap.add_argument("--check-rows", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()

    import torch
    import psfm_synth
    from _ground_truth_np import frame_counts_np, vote_np
    from point_trajectory import _hip
    from point_trajectory.trajectory import run_connect
    from psfm_motion_seg import ground_truth as gt
    from psfm_motion_seg.load_cut_seq import sample_window_device
    from psfm_motion_seg.merge_labels import label_trajectories

    assert torch.cuda.is_available(), "ground_truth.py measures on the GPU"
    T, H, W = a.frames, a.height, a.width
    dev = torch.device("cuda", 0)
    d = psfm_synth.synth_sequence_torch(T, H, W, seed=0, sigma=0.05, n_occluders=2, stride2=False, device=dev)
    ctx = _hip.context(0)
    run_connect(d["flows_f"], d["flows_b"], None, None, 1.0, 2, return_device=True)
    del d
    cap = a.cap if a.cap > 0 else 10 ** 9
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    merger = label_trajectories(T, a.window, (H, W), (H, W), cap, lambda raw, nor, mask, t: torch.rand(raw.shape[0], device="cuda", generator=gen) < 0.5,
                                ctx=ctx)
    n_points = merger.n_points
    masks = disc_maps(T, H, W, dev)
    L, sp = _hip.lib(), _hip.current_stream_ptr(0)
    table = np.ascontiguousarray(gt.mask_table())
    counts = torch.empty((T, 4), dtype=torch.int64, device=dev)

    def eval_once():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _hip.check(L.psfm_traj_eval_counts(ctx.handle, None, None, None, 0, _hip.ptr(masks), table.ctypes.data, T, H, W, _hip.ptr(counts), sp))
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)
    for _ in range(a.warmup):
        eval_once()
    first = counts.clone()
    t_eval = np.array([eval_once() for _ in range(a.reps)])
    fr, xy, lab = merger.finish()[2:]
    sel = torch.nonzero(fr == 0)[:, 0]
    frame0 = frame_counts_np(masks[:1].cpu().numpy(), np.zeros(sel.numel(), np.int32), xy[sel].cpu().numpy(), lab[sel].cpu().numpy())[0]

    nv = min(a.vote_frames, T)
    ids, raw, _, mabs = sample_window_device(ctx, 0, nv, (H, W), (H, W), 10 ** 9, 3, 3, 0, normalise=False)
    gts = (masks[:nv] < 128).to(torch.uint8)
    K = int(ids.numel())
    votes = torch.empty((K,), dtype=torch.uint8, device=dev)

    def vote_once():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _hip.check(L.psfm_traj_vote_labels(ctx.handle, _hip.ptr(raw), _hip.ptr(mabs), _hip.ptr(gts), K, nv, H, W, _hip.ptr(votes), sp))
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)
    for _ in range(a.warmup):
        vote_once()
    t_vote = np.array([vote_once() for _ in range(a.reps)])
    rows = min(a.check_rows, K)
    want_votes = vote_np(raw[:rows].cpu().numpy(), mabs[:rows].cpu().numpy(), gts.cpu().numpy())[0]
    present = int((mabs == 0).sum())

    out = {"workload": "%dx%d, %d frames, r=2, window %d, cap %s" % (H, W, T, a.window, a.cap or "none"), "reps": a.reps,
           "n_labelled_points": n_points, "n_frames": T,
           "eval_ms": float(np.median(t_eval)), "eval_ms_min_max": [float(t_eval.min()), float(t_eval.max())],
           "eval_algorithmic_bytes": int(n_points * (4 + 16 + 1 + 4) + T * 32),
           "counts_sum_equals_points": bool(int(counts.sum()) == n_points), "counts_repeatable": bool(torch.equal(first, counts)),
           "frame0_equals_restatement": bool(np.array_equal(counts[0].cpu().numpy(), frame0)),
           "vote_rows": K, "vote_frames": nv, "vote_present": present,
           "vote_ms": float(np.median(t_vote)), "vote_ms_min_max": [float(t_vote.min()), float(t_vote.max())],
           "vote_algorithmic_bytes": int(K * nv * (8 + 16) + present + K),
           "votes_equal_restatement": bool(np.array_equal(votes[:rows].cpu().numpy(), want_votes)), "votes_dynamic": int(votes.sum())}
    out["eval_GBps"] = out["eval_algorithmic_bytes"] / out["eval_ms"] / 1e6
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fp:
            fp.write(line + "\n")
    ok = out["counts_sum_equals_points"] and out["counts_repeatable"] and out["frame0_equals_restatement"] and out["votes_equal_restatement"]
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
