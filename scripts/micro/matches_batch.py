#!/usr/bin/env python3
"""psfm_result_filter_batch + psfm_traj_to_matches_batch (csrc/psfm_matches_batch.hip) against the loop of psfm_result_filter +
psfm_traj_to_matches per context, on the same device and the same results (profiles/EXPERIMENTS.md section 27).

  --n-seq N        N sequences of --height x --width x --frames at --ratio (default: 480x854 x 51 frames at sample_ratio 4, the
                   README's DAVIS-sized shape), psfm_synth flows (--stacks distinct flow stacks, shared round-robin: every sequence
                   still has its own context and its own result), connected by psfm_connect_batch before the clock starts.
  timed span       host wall clock with a stream synchronisation at both ends, from "results in the contexts" to "tables finished
                   in every context": filter + tables on the --assume_static route (traj_min_len 3, sample_k 20, no labels).
                     single   for every context: psfm_result_filter, psfm_traj_to_matches
                     batch    psfm_result_filter_batch over all contexts, then psfm_traj_to_matches_batch per group of
                              psfm_sfm.matches_from_flow.group_sequences (at most 64 sequences and --max-points points)
                   The two routes alternate; a round that copies every context out and hashes it, one warm-up round, then --runs
                   timed runs each; median and spread (max - min).
  verdict          the batch form is called faster only if the difference of the medians exceeds three times the larger spread.
Also prints the byte-equality of the two routes (sha256 over every context's psfm_result_filtered_copy and psfm_matches_copy) and the
census of the batch calls.  One process, one JSON line; run it under a time limit.
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "particle-sfm_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-seq", type=int, default=16)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=854)
    ap.add_argument("--frames", type=int, default=51)
    ap.add_argument("--ratio", type=int, default=4)
    ap.add_argument("--stacks", type=int, default=4)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--max-points", type=int, default=1 << 25)
    a = ap.parse_args()
    import torch
    import psfm_synth
    from point_trajectory import _hip, trajectory
    from psfm_sfm import matches_from_flow as mff
    L = _hip.lib()
    vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    stacks = []
    for i in range(min(a.stacks, a.n_seq)):
        d = psfm_synth.synth_sequence_torch(a.frames, a.height, a.width, seed=70 + i)
        stacks.append((d["flows_f"], d["flows_b"], None, None))
    B, n_img = a.n_seq, a.frames
    ctxs = []
    for lo in range(0, B, 64):
        part, _ = trajectory.run_connect_batch([stacks[i % len(stacks)] for i in range(lo, min(lo + 64, B))], 1.0, a.ratio)
        ctxs += list(part)
    assert len(ctxs) == B and len({id(c) for c in ctxs}) == B
    dev = ctxs[0].device
    sp = _hip.current_stream_ptr(dev)
    sync = lambda: torch.cuda.synchronize(dev)
    state = {}

    def single():
        sizes = []
        for c in ctxs:
            k, n = ctypes.c_int64(0), ctypes.c_int64(0)
            _hip.check(L.psfm_result_filter(c.handle, 3, ctypes.byref(k), ctypes.byref(n), sp))
            kp, m, p = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
            _hip.check(L.psfm_traj_to_matches(c.handle, n_img, mff.SAMPLE_K, None, ctypes.byref(kp), ctypes.byref(m), ctypes.byref(p), sp))
            sizes.append((int(k.value), int(n.value), int(kp.value), int(m.value), int(p.value)))
        return sizes

    def batch():
        flt = mff.result_filter_batch_device(ctxs, 3)
        state["census_filter"] = census(ctxs[0])
        sizes, groups, cz = [], mff.group_sequences([n for _, n in flt], a.max_points), []
        for lo, hi, alone in groups:
            n = hi - lo
            kp, m, p = (ctypes.c_int64 * n)(), (ctypes.c_int64 * n)(), (ctypes.c_int64 * n)()
            if alone:
                _hip.check(L.psfm_traj_to_matches(ctxs[lo].handle, n_img, mff.SAMPLE_K, None, kp, m, p, sp))
            else:
                hs = (ctypes.c_void_p * n)(*[c.handle.value for c in ctxs[lo:hi]])
                _hip.check(L.psfm_traj_to_matches_batch(hs, n, (ctypes.c_int32 * n)(*[n_img] * n), mff.SAMPLE_K, None, kp, m, p, sp))
                cz.append(census(ctxs[lo]))
            sizes += [flt[lo + i] + (int(kp[i]), int(m[i]), int(p[i])) for i in range(n)]
        state["groups"], state["census_tables"] = [(lo, hi, alone) for lo, hi, alone in groups], cz
        return sizes

    def census(c):
        s, l = ctypes.c_int32(-1), ctypes.c_int32(-1)
        _hip.check(L.psfm_matches_batch_census(c.handle, ctypes.byref(s), ctypes.byref(l)))
        return [int(s.value), int(l.value)]

    def digest(sizes):
        h = hashlib.sha256()
        for c, (k, n, kp, m, p) in zip(ctxs, sizes):
            ids, birth, length = np.empty(k, np.int32), np.empty(k, np.int32), np.empty(k, np.int32)
            off, xy = np.zeros(k + 1, np.int64), np.empty((n, 2), np.float64)
            _hip.check(L.psfm_result_filtered_copy(c.handle, vp(ids), vp(birth), vp(length), vp(off), vp(xy), sp))
            for t in (ids, birth, length, off, xy) + tuple(mff._copy_tables(c, n_img, kp, m, p)):
                h.update(np.ascontiguousarray(t).tobytes())
        return h.hexdigest()

    routes = {"single": single, "batch": batch}
    times, sizes, digests = {r: [] for r in routes}, {}, {}
    # round 0: both routes once, every context copied out and hashed (seconds of host work during which the device idles);
    # round 1: the warm-up, straight in front of the timed rounds
    for it in range(a.runs + 2):
        for r, fn in routes.items():
            sync()
            t0 = time.perf_counter()
            sizes[r] = fn()
            sync()
            dt = (time.perf_counter() - t0) * 1e3
            if it == 0:
                digests[r] = digest(sizes[r])
            elif it >= 2:
                times[r].append(dt)
    med = {r: float(np.median(v)) for r, v in times.items()}
    spread = {r: float(max(v) - min(v)) for r, v in times.items()}
    diff, bar = med["single"] - med["batch"], 3.0 * max(spread.values())
    free, total = torch.cuda.mem_get_info(dev)
    out = {"n_seq": B, "shape": [a.height, a.width, a.frames, a.ratio], "runs": a.runs,
           "points": int(sum(s[1] for s in sizes["single"])), "matches": int(sum(s[3] for s in sizes["single"])),
           "single_ms": {"median": med["single"], "spread": spread["single"], "runs": times["single"]},
           "batch_ms": {"median": med["batch"], "spread": spread["batch"], "runs": times["batch"]},
           "per_sequence_ms": {r: med[r] / B for r in med},
           "difference_ms": diff, "bar_ms": bar, "batch_faster_by_the_bar": bool(diff > bar),
           "sizes_equal": sizes["single"] == sizes["batch"], "bytes_equal": digests["single"] == digests["batch"],
           "groups": state["groups"], "census_filter": state["census_filter"], "census_tables": state["census_tables"],
           "device_memory_in_use_gb": (total - free) / 2 ** 30}
    print(json.dumps(out))
    return 0 if out["sizes_equal"] and out["bytes_equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
