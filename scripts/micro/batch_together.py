#!/usr/bin/env python3
"""psfm_connect_batch with path consistency on flows whose solves reject steps: the sequences that leave the fused batch redone ALONE
(psfm_connect per sequence on host threads: BatchRun::redo_alone) against redone TOGETHER (one set of launches, the frame-mode
multi-problem launch chain: BatchRun::redo_together).  profiles/EXPERIMENTS.md 33.

  variants  a  the parent commit's library (--parent-lib PATH), i.e. redo_alone as it was
            b  this library, psfm_ctx_set_batch_redo(ctx0, 0): must equal (a) within the spread
            c  this library, psfm_ctx_set_batch_redo(ctx0, 1)
  shapes    sintel 436 x 1024, sample_ratio 2, 49 flows, B = 4, 16;  davis 480 x 854, sample_ratio 4, 50 flows, B = 16, 64;
            scannet 640 x 480, sample_ratio 1, 30 flows, B = 4 -- psfm_synth.REALISTIC (synth_realistic_torch) with stride-2 stacks,
            --distinct different sequences per shape, repeated;  mixed: sintel B = 16, every second sequence clean
            (synth_sequence_torch).  Adaptive solver policy, default table factors.
One process, the variants ALTERNATED, --reps rounds after --warmup; wall clock around calls that end in a stream synchronisation.
"faster" only where the difference of the medians exceeds three times the larger spread (max - min).  Reported per shape: ms per
sequence, the census of (c), chain modes, and whether every sequence of (c) that ran in mode 8 holds the bytes of psfm_connect for it
alone on a context pinned to the launch chain (costs apart: they are compared to rounding, and their largest relative difference is
reported).  Prints one JSON line (--out also writes it to a file)."""
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

SHAPES = {"sintel4": (4, 436, 1024, 2, 49, False), "sintel16": (16, 436, 1024, 2, 49, False), "davis16": (16, 480, 854, 4, 50, False),
          "davis64": (64, 480, 854, 4, 50, False), "scannet4": (4, 640, 480, 1, 30, False), "mixed16": (16, 436, 1024, 2, 49, True)}


def stats(ms, B):
    a = np.sort(np.asarray(ms, np.float64)) / B
    return {"median_ms_per_seq": float(np.median(a)), "min": float(a[0]), "max": float(a[-1]), "spread": float(a[-1] - a[0])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="sintel4,sintel16,davis16,davis64,scannet4,mixed16")
    ap.add_argument("--distinct", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--parent-lib", default=None, help="libpsfm_hip.so of the parent commit (variant a)")
    ap.add_argument("--order", default=None, help="the order of the variants inside a round, e.g. b,a,c (default: a,b,c)")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    import psfm_synth
    from point_trajectory import _hip
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    L = _hip.lib()
    vp = ctypes.c_void_p
    libs = {"b": L, "c": L}
    if a.parent_lib:
        LP = ctypes.CDLL(os.path.abspath(a.parent_lib))
        LP.psfm_ctx_create.argtypes = [ctypes.c_int, ctypes.POINTER(vp)]
        LP.psfm_connect_batch.argtypes = L.psfm_connect_batch.argtypes
        LP.psfm_last_error.restype = ctypes.c_char_p
        libs["a"] = LP
    dev_id = torch.cuda.current_device()
    sp = _hip.current_stream_ptr(dev_id)

    def contexts(lib, n):
        out = []
        for _ in range(n):
            h = vp()
            assert lib.psfm_ctx_create(dev_id, ctypes.byref(h)) == 0
            out.append(h)
        return out
    # every variant has contexts of its own: the joint redo leaves its solves' statistics in the contexts' adaptive policy and its
    # tables in their workspaces, and none of that may reach the variant it is measured against
    handles = {"b": contexts(L, 64), "c": contexts(L, 64)}
    if a.parent_lib:
        handles["a"] = contexts(libs["a"], 64)
    ref = contexts(L, 1)[0]
    assert L.psfm_ctx_set_solver(ref, 1, 0) == 0

    def result(handle, info):
        n, npnt = int(info.n_traj), int(info.n_points)
        birth, length, off, xy = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n + 1, np.int64), np.zeros((npnt, 2), np.float64)
        assert L.psfm_result_copy(handle, *[x.ctypes.data_as(vp) for x in (birth, length, off, xy)], sp) == 0
        ss = (_hip.SolveStats * max(int(info.n_solves), 1))()
        got = ctypes.c_int32()
        assert L.psfm_result_solve_stats(handle, ss, int(info.n_solves), ctypes.byref(got)) == 0
        return ((birth.tobytes() + length.tobytes() + off.tobytes(), xy),
                [(s.iterations, s.successful_steps, s.termination, s.dogleg_nonGN) for s in ss[:got.value]],
                [(s.initial_cost, s.final_cost) for s in ss[:got.value]])

    res = {"reps": a.reps, "warmup": a.warmup, "variants": sorted(libs), "runs": []}
    for name in a.shapes.split(","):
        B, H, W, r, n, mixed = SHAPES[name]
        base = []
        for k in range(min(a.distinct, B)):
            d = psfm_synth.synth_realistic_torch(n + 1, H, W, seed=41 + k, stride2=True, device="cuda", **psfm_synth.REALISTIC)
            base.append(tuple(d[key].contiguous() for key in ("flows_f", "flows_b", "flows_f2", "flows_b2")))
            del d
        clean = []
        if mixed:
            d = psfm_synth.synth_sequence_torch(n + 1, H, W, seed=51, stride2=True, device="cuda")
            clean.append(tuple(d[key].contiguous() for key in ("flows_f", "flows_b", "flows_f2", "flows_b2")))
            del d
        seqs = [clean[0] if (mixed and k % 2 == 0) else base[(k // (2 if mixed else 1)) % len(base)] for k in range(B)]
        arr = lambda j: (vp * B)(*[s[j].data_ptr() for s in seqs])
        nf = (ctypes.c_int * B)(*[n] * B)
        infos = {v: (_hip.TrackInfo * B)() for v in libs}

        def call(v):
            if v != "a":
                assert L.psfm_ctx_set_batch_redo(handles[v][0], 1 if v == "c" else 0) == 0
            st = libs[v].psfm_connect_batch((vp * B)(*[h.value for h in handles[v][:B]]), B, arr(0), arr(1), arr(2), arr(3), nf, H, W, 1.0, r,
                                            infos[v], sp)
            assert st == 0, libs[v].psfm_last_error()
        t = {v: [] for v in libs}
        for rep in range(a.warmup + a.reps):
            for v in (a.order.split(",") if a.order else sorted(libs)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call(v)
                torch.cuda.synchronize()
                if rep >= a.warmup:
                    t[v].append((time.perf_counter() - t0) * 1e3)
        # ---- (c) once more, then: census, modes, and every mode-8 sequence against psfm_connect alone on the pinned context ----
        call("c")
        census = [ctypes.c_int32() for _ in range(5)]
        assert L.psfm_connect_batch_census(handles["c"][0], *[ctypes.byref(x) for x in census]) == 0
        modes = [int(i.chain_mode) for i in infos["c"]]
        done, same_bytes, same_ids, same_decisions, worst, worst_xy = {}, True, True, True, 0.0, 0.0
        for k in range(B):
            if modes[k] != 8:
                continue
            key = id(seqs[k])
            if key not in done:
                info = _hip.TrackInfo()
                s = seqs[k]
                assert L.psfm_connect(ref, vp(s[0].data_ptr()), vp(s[1].data_ptr()), vp(s[2].data_ptr()), vp(s[3].data_ptr()), n, H, W, 1.0, r,
                                      None, None, ctypes.byref(info), sp) == 0, L.psfm_last_error()
                done[key] = result(ref, info)
            got = result(handles["c"][k], infos["c"][k])
            same_ids = same_ids and got[0][0] == done[key][0][0]
            same_bytes = same_bytes and got[0][0] == done[key][0][0] and got[0][1].tobytes() == done[key][0][1].tobytes()
            if got[0][1].shape == done[key][0][1].shape and got[0][1].size:
                worst_xy = max(worst_xy, float(np.abs(got[0][1] - done[key][0][1]).max()))
            same_decisions = same_decisions and got[1] == done[key][1]
            for x, y in zip(got[2], done[key][2]):
                for p, q in zip(x, y):
                    worst = max(worst, abs(p - q) / max(abs(q), 1e-300))
        s = {v: stats(t[v], B) for v in libs}
        run = {"shape": name, "n_seq": B, "size": [n, H, W], "sample_ratio": r, "per_variant": s, "modes_c": {str(m): modes.count(m) for m in set(modes)},
               "modes_b": {str(m): [int(i.chain_mode) for i in infos["b"]].count(m) for m in set(int(i.chain_mode) for i in infos["b"])},
               "census_c": dict(zip(("n_left", "n_together", "launches_fixed", "launches_iter", "host_syncs"), (int(x.value) for x in census))),
               "mode8_ids_lengths_positions_bytes_equal_psfm_connect": bool(same_bytes), "mode8_ids_births_lengths_bytes_equal": bool(same_ids),
               "mode8_positions_largest_difference_px": worst_xy, "mode8_solve_decisions_equal": bool(same_decisions),
               "mode8_costs_largest_relative_difference": worst,
               "solves_c": int(sum(int(i.n_solves) for i in infos["c"])), "iterations_c": int(sum(int(i.solver_iterations) for i in infos["c"]))}
        for x, y in (("a", "c"), ("b", "c"), ("a", "b")):
            if x in s and y in s:
                diff = s[x]["median_ms_per_seq"] - s[y]["median_ms_per_seq"]
                spread = max(s[x]["spread"], s[y]["spread"])
                run["%s_minus_%s" % (x, y)] = {"difference": diff, "three_spreads": 3 * spread,
                                               "verdict": "%s faster" % y if diff > 3 * spread else ("%s faster" % x if -diff > 3 * spread else "level")}
        res["runs"].append(run)
        print(name, {v: round(s[v]["median_ms_per_seq"], 3) for v in s}, run["modes_c"], file=sys.stderr, flush=True)
        del base, clean, seqs
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
