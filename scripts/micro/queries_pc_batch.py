#!/usr/bin/env python3
"""psfm_track_queries_optimize_batch (csrc/psfm_query_pc_batch.hip + the multi-problem launch chain of csrc/psfm_solver_multi.hip)
against the loop of psfm_track_queries_optimize calls -- the route there was before it.  The protocol of scripts/micro/queries_batch.py
(profiles/EXPERIMENTS.md 31).

  shapes   a  64 sequences of 480 x 854 x 50 flows, 256 random queries each (uniform in [-1, W] x [-1, H], t uniform in 0 .. n_flows)
           b  16 sequences, the same
           c  8 sequences of 1080 x 1920 x 30 flows, 10 000 queries each
           both directions.  A batch holds --distinct different sequences (psfm_synth.synth_realistic_torch with stride-2 stacks),
           repeated; every sequence has queries of its own.
  routes   loop:  one psfm_track_queries_optimize call per sequence, each into a context of its own
           batch: ONE psfm_track_queries_optimize_batch call into the same number of contexts
           both from "stacks, maps and queries on the device" to "results in every context" (every call ends in a stream
           synchronisation; wall clock around the route).  --loop-lib PATH: the loop runs on another build of the library -- the
           parent commit's -- loaded beside this one, with contexts of its own.
One process, the routes ALTERNATED, --reps rounds after --warmup.  "faster" only where the difference of the medians exceeds three
times the larger spread (max - min).  The two routes' results (and the number of solves and iterations of every sequence) are
compared byte for byte at the timed sizes.  Prints one JSON line (--out also writes it to a file)."""
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

SHAPES = {"a": (64, 480, 854, 50, 256), "b": (16, 480, 854, 50, 256), "c": (8, 1080, 1920, 30, 10000)}


def stats(ms):
    a = np.sort(np.asarray(ms, np.float64))
    return {"median_ms": float(np.median(a)), "min_ms": float(a[0]), "max_ms": float(a[-1]), "spread_ms": float(a[-1] - a[0])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="abc")
    ap.add_argument("--directions", default="both")
    ap.add_argument("--distinct", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--loop-lib", default=None, help="libpsfm_hip.so of another build (the parent commit) for the loop route")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    import psfm_synth
    from point_trajectory import _hip
    from point_trajectory.utils import flow_check_device
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    L = _hip.lib()
    vp = ctypes.c_void_p
    # the loop's library and its contexts
    if a.loop_lib:
        LL = ctypes.CDLL(os.path.abspath(a.loop_lib))
        LL.psfm_ctx_create.argtypes = [ctypes.c_int, ctypes.POINTER(vp)]
        LL.psfm_track_queries_optimize.argtypes = L.psfm_track_queries_optimize.argtypes
        LL.psfm_result_copy.argtypes = L.psfm_result_copy.argtypes
        LL.psfm_last_error.restype = ctypes.c_char_p
    else:
        LL = L
    batch_ctxs = _hip.batch_contexts(64)
    dev_id = batch_ctxs[0].device
    loop_handles = []
    for k in range(64):
        h = vp()
        assert LL.psfm_ctx_create(dev_id, ctypes.byref(h)) == 0
        loop_handles.append(h)
    sp = _hip.current_stream_ptr(dev_id)
    res = {"reps": a.reps, "warmup": a.warmup, "loop_lib": "another build" if a.loop_lib else "this build", "runs": []}

    def copy_out(lib, handle, info):
        n, npnt = int(info.n_traj), int(info.n_points)
        birth, length, off, xy = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n + 1, np.int64), np.zeros((npnt, 2), np.float64)
        assert lib.psfm_result_copy(handle, *[x.ctypes.data_as(vp) for x in (birth, length, off, xy)], sp) == 0
        return birth.tobytes() + length.tobytes() + off.tobytes() + xy.tobytes()

    for name in a.shapes:
        B, H, W, n, Q = SHAPES[name]
        base = []
        for k in range(min(a.distinct, B)):
            d = psfm_synth.synth_realistic_torch(n + 1, H, W, seed=41 + k, stride2=True, device="cuda", **psfm_synth.REALISTIC)
            ff, fb, f2, b2 = (d[key].contiguous() for key in ("flows_f", "flows_b", "flows_f2", "flows_b2"))
            # (stack, its maps) per direction and stride, each direction's maps in its own orientation
            base.append((ff, fb, flow_check_device(ff, fb, 1.0)[1].contiguous(), flow_check_device(fb, ff, 1.0)[1].contiguous(),
                         f2, b2, flow_check_device(f2, b2, 1.0)[1].contiguous(), flow_check_device(b2, f2, 1.0)[1].contiguous()))
            del d
        rng = np.random.default_rng(17)
        q_xy = [torch.from_numpy(rng.uniform([-1.0, -1.0], [float(W), float(H)], size=(Q, 2))).cuda() for _ in range(B)]
        q_t = [torch.from_numpy(rng.integers(0, n + 1, size=Q).astype(np.int32)).cuda() for _ in range(B)]
        seqs = [base[k % len(base)] for k in range(B)]
        for direction in a.directions.split(","):
            fwd, bwd = direction in ("forward", "both"), direction in ("backward", "both")
            infos_l = [_hip.TrackInfo() for _ in range(B)]
            infos_b = (_hip.TrackInfo * B)()
            arr = lambda ptrs: (vp * B)(*ptrs)
            b_args = (arr([c.handle.value for c in batch_ctxs[:B]]), B,
                      arr([s[0].data_ptr() for s in seqs]) if fwd else None, arr([s[2].data_ptr() for s in seqs]) if fwd else None,
                      arr([s[4].data_ptr() for s in seqs]) if fwd else None, arr([s[6].data_ptr() for s in seqs]) if fwd else None,
                      arr([s[1].data_ptr() for s in seqs]) if bwd else None, arr([s[3].data_ptr() for s in seqs]) if bwd else None,
                      arr([s[5].data_ptr() for s in seqs]) if bwd else None, arr([s[7].data_ptr() for s in seqs]) if bwd else None,
                      (ctypes.c_int * B)(*[n] * B), (ctypes.c_int * B)(*[H] * B), (ctypes.c_int * B)(*[W] * B),
                      arr([x.data_ptr() for x in q_xy]), arr([x.data_ptr() for x in q_t]), (ctypes.c_int64 * B)(*[Q] * B), infos_b, sp)

            def loop():
                for k, s in enumerate(seqs):
                    p = lambda j, on: vp(s[j].data_ptr()) if on else None
                    st = LL.psfm_track_queries_optimize(loop_handles[k], p(0, fwd), p(2, fwd), p(4, fwd), p(6, fwd), p(1, bwd), p(3, bwd),
                                                        p(5, bwd), p(7, bwd), n, H, W, vp(q_xy[k].data_ptr()), vp(q_t[k].data_ptr()), Q,
                                                        ctypes.byref(infos_l[k]), sp)
                    assert st == 0, LL.psfm_last_error()

            def batch():
                _hip.check(L.psfm_track_queries_optimize_batch(*b_args))
            t = {"loop": [], "batch": []}
            for r in range(a.warmup + a.reps):
                for route, fn in (("loop", loop), ("batch", batch)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    if r >= a.warmup:
                        t[route].append((time.perf_counter() - t0) * 1e3)
            same = all(copy_out(LL, loop_handles[k], infos_l[k]) == copy_out(L, batch_ctxs[k].handle, infos_b[k]) and
                       (infos_l[k].n_solves, infos_l[k].solver_iterations) == (infos_b[k].n_solves, infos_b[k].solver_iterations) for k in range(B))
            assert same, "the routes disagree"
            sl, sb = stats(t["loop"]), stats(t["batch"])
            spread = max(sl["spread_ms"], sb["spread_ms"])
            diff = sl["median_ms"] - sb["median_ms"]
            res["runs"].append({"shape": name, "n_seq": B, "size": [n, H, W], "queries_per_sequence": Q, "direction": direction,
                                "loop": sl, "batch": sb, "speedup_of_medians": sl["median_ms"] / sb["median_ms"], "difference_ms": diff,
                                "larger_spread_ms": spread, "batch_faster_by_more_than_three_spreads": bool(diff > 3 * spread),
                                "loop_faster_by_more_than_three_spreads": bool(-diff > 3 * spread),
                                "census": batch_ctxs[0].query_pc_batch_census(), "bytes_equal": bool(same),
                                "solves": int(sum(int(i.n_solves) for i in infos_b)), "iterations": int(sum(int(i.solver_iterations) for i in infos_b)),
                                "points": int(sum(int(i.n_points) for i in infos_b))})
            print("%s %s: loop %.3f ms, batch %.3f ms" % (name, direction, sl["median_ms"], sb["median_ms"]), file=sys.stderr, flush=True)
        del base, seqs
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
