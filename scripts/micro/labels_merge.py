#!/usr/bin/env python3
"""The label merge (csrc/psfm_labels.hip) and the match tables over the labelled set at the headline size, against the host
statement on the same arrays.

Workload: psfm_synth 1080x1920, 101 frames, r = 2 -> psfm_connect -> psfm_result_filter(3); windows of 10 frames from the device
sampler (--cap 100000: the reference's default traj_max_num; --cap 0: uncapped), seeded random predictions.  Timed with HIP events
on the stream, after warm-up, median of --reps repetitions:
  merge     the sum of the psfm_labels_merge_window launches of all windows (behind psfm_labels_begin, which is not in the span)
  finish    psfm_labels_finish (count, sort by first appearance, scan, gather; two host synchronisations inside)
  tables    psfm_labels_to_matches (remove_dynamic as given)
Host comparison (--host all | merge | none): merge_labels_host, match_tables_host on the same saved set, windows and predictions;
the device results are compared with them while at it.  Prints one JSON line; the gather's algorithmic bytes are part of it
(per labelled point 16 B xy + 1 B state read, 4 + 16 + 1 B written; per saved point of a labelled trajectory 1 B state read).
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "particle-sfm_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=101)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--window", type=int, default=10)
    ap.add_argument("--cap", type=int, default=100000, help="traj_max_num per window; 0 = uncapped")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--p-dynamic", type=float, default=0.5)
    ap.add_argument("--keep-dynamic", action="store_true", help="remove_dynamic = False (every labelled point is a keypoint)")
    ap.add_argument("--host", choices=("all", "merge", "none"), default="all")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()

    import torch
    import psfm_synth
    from point_trajectory import _hip
    from point_trajectory.trajectory import run_connect
    from psfm_motion_seg.load_cut_seq import sample_window_device, window_ranges
    from psfm_motion_seg.merge_labels import merge_labels_host
    from psfm_sfm import matches_from_flow as mff

    assert torch.cuda.is_available(), "labels_merge.py measures on the GPU"
    T, H, W = a.frames, a.height, a.width
    d = psfm_synth.synth_sequence_torch(T, H, W, seed=0, sigma=0.05, n_occluders=2, stride2=False, device=torch.device("cuda", 0))
    ctx = _hip.context(0)
    run_connect(d["flows_f"], d["flows_b"], None, None, 1.0, 2, return_device=True)
    del d
    L, sp = _hip.lib(), _hip.current_stream_ptr(0)
    k, n = ctypes.c_int64(0), ctypes.c_int64(0)
    _hip.check(L.psfm_result_filter(ctx.handle, 3, ctypes.byref(k), ctypes.byref(n), sp))
    cap = a.cap if a.cap > 0 else 10 ** 9
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    windows = []
    for w, (f0, nf) in enumerate(window_ranges(T, a.window)):
        ids = sample_window_device(ctx, f0, nf, (H, W), (H, W), cap, 3, 3, seed=w, normalise=False)[0]
        pred = (torch.rand(ids.numel(), device="cuda", generator=gen) < a.p_dynamic).to(torch.uint8)
        windows.append((f0, nf, ids, pred))
    rd = 0 if a.keep_dynamic else 1
    sizes = {}

    def one(timed):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        _hip.check(L.psfm_labels_begin(ctx.handle, sp))
        ev[0].record()
        for f0, nf, ids, pred in windows:
            _hip.check(L.psfm_labels_merge_window(ctx.handle, f0, nf, _hip.ptr(ids), _hip.ptr(pred), ids.numel(), sp))
        ev[1].record()
        m, p = ctypes.c_int64(0), ctypes.c_int64(0)
        _hip.check(L.psfm_labels_finish(ctx.handle, ctypes.byref(m), ctypes.byref(p), sp))
        ev[2].record()
        kp, nm, npair = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        _hip.check(L.psfm_labels_to_matches(ctx.handle, T, mff.SAMPLE_K, rd, ctypes.byref(kp), ctypes.byref(nm), ctypes.byref(npair), sp))
        ev[3].record()
        torch.cuda.synchronize()
        sizes.update(n_labelled=int(m.value), n_labelled_points=int(p.value), n_keypoints=int(kp.value), n_matches=int(nm.value),
                     n_pairs=int(npair.value))
        return [ev[i].elapsed_time(ev[i + 1]) for i in range(3)]
    for _ in range(a.warmup):
        one(False)
    t = np.array([one(True) for _ in range(a.reps)])
    med = np.median(t, 0)

    out = {"workload": "%dx%d, %d frames, r=2, window %d, cap %s, p_dynamic %.2f, remove_dynamic %d" % (H, W, T, a.window, a.cap or "none", a.p_dynamic, rd),
           "n_saved": int(k.value), "n_saved_points": int(n.value), "rows": int(sum(w[2].numel() for w in windows)), "windows": len(windows),
           "reps": a.reps, "merge_ms": float(med[0]), "finish_ms": float(med[1]), "tables_ms": float(med[2]),
           "merge_ms_min_max": [float(t[:, 0].min()), float(t[:, 0].max())], "finish_ms_min_max": [float(t[:, 1].min()), float(t[:, 1].max())],
           "tables_ms_min_max": [float(t[:, 2].min()), float(t[:, 2].max())]}
    out.update(sizes)

    if a.host != "none":
        kk, nn = int(k.value), int(n.value)
        ids, birth, length = np.empty(kk, np.int32), np.empty(kk, np.int32), np.empty(kk, np.int32)
        off, xy = np.zeros(kk + 1, np.int64), np.empty((nn, 2), np.float64)
        vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)
        _hip.check(L.psfm_result_filtered_copy(ctx.handle, vp(ids), vp(birth), vp(length), vp(off), vp(xy), sp))
        hw = [(f0, nf, i.cpu().numpy(), p.cpu().numpy()) for f0, nf, i, p in windows]
        t0 = time.perf_counter()
        hset = merge_labels_host(ids, birth, length, off, xy, hw)
        out["host_merge_ms"] = 1e3 * (time.perf_counter() - t0)
        m, p = sizes["n_labelled"], sizes["n_labelled_points"]
        dset = (np.empty(m, np.int32), np.zeros(m + 1, np.int64), np.empty(p, np.int32), np.empty((p, 2), np.float64), np.empty(p, np.uint8))
        _hip.check(L.psfm_labels_copy(ctx.handle, *[vp(x) for x in dset], sp))
        out["merge_equal_host"] = bool(all(np.array_equal(x, y) for x, y in zip(dset, hset)))
        seen = np.searchsorted(ids, hset[0])
        out["gather_algorithmic_bytes"] = int(p * (16 + 1 + 4 + 16 + 1) + (length[seen].sum() - p) + m * (4 + 8 + 8 + 8 + 4))
        if a.host == "all":
            t0 = time.perf_counter()
            want = mff.match_tables_host(hset[1], hset[2].astype(np.int64), hset[3], hset[4].astype(bool), T, bool(rd))
            out["host_tables_ms"] = 1e3 * (time.perf_counter() - t0)
            got = mff._copy_tables(ctx, T, sizes["n_keypoints"], sizes["n_matches"], sizes["n_pairs"])
            out["tables_equal_host"] = bool(all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(got, want)))
            out["host_over_device"] = (out["host_merge_ms"] + out["host_tables_ms"]) / (out["merge_ms"] + out["finish_ms"] + out["tables_ms"])
        else:
            out["host_merge_over_device_merge_finish"] = out["host_merge_ms"] / (out["merge_ms"] + out["finish_ms"])
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fp:
            fp.write(line + "\n")
    return 0 if out.get("merge_equal_host", True) and out.get("tables_equal_host", True) else 1


if __name__ == "__main__":
    sys.exit(main())
