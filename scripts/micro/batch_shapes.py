#!/usr/bin/env python3
"""psfm_connect_batch on a directory of clips of several frame sizes: ONE call per size group, as the parent commit has to run them,
against ONE call for all of them (h = w = 0, psfm_ctx_set_frame_size).  profiles/EXPERIMENTS.md 34.

  variants  a  the parent commit's library (--parent-lib PATH): one psfm_connect_batch call per frame size, one after the other
            b  this library, the same calls: must equal (a) within the spread (the same path)
            c  this library, one call with h = w = 0
  shapes    davis16: 16 sequences of 50 flows at sample_ratio 4, four each of 480 x 854, 480 x 910, 480 x 720 and 360 x 640; davis64:
            64 of them; same16: 16 of 480 x 854 (c: h = w = 0 with equal sizes -- the call with that size).
  modes     track (--skip_path_consistency), mb (track with the motion-boundary option, threshold 0.02), opt (path consistency on
            clean flows: synth_sequence_torch, whose solves accept every step -- the sequences stay in the batch).
            track / mb stacks: psfm_synth.REALISTIC (synth_realistic_torch), --distinct different sequences per size, repeated.
One process, the variants ALTERNATED, --reps rounds after --warmup; wall clock around calls that end in a stream synchronisation.
"faster" only where the difference of the medians exceeds three times the larger spread (max - min).  Reported per run: ms per
sequence, whether every sequence of (c) holds the bytes of (b) (track / mb; opt: ids equal and the largest position difference), chain
modes, and the fraction of the blocks of a mixed chain-step launch that return at once: the launch covers the lanes of the LARGEST
grid for every sequence, a smaller sequence's surplus blocks leave at their first test.  Prints one JSON line (--out also writes it)."""
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

SIZES = [(480, 854), (480, 910), (480, 720), (360, 640)]
SHAPES = {"davis16": (16, SIZES), "davis64": (64, SIZES), "same16": (16, SIZES[:1])}
RATIO, N_FLOWS = 4, 50
CHAIN_TILE = 1024      # lanes per block of the batched chain step (PSFM_CHAIN_TILE)


def stats(ms, B):
    a = np.sort(np.asarray(ms, np.float64)) / B
    return {"median_ms_per_seq": float(np.median(a)), "min": float(a[0]), "max": float(a[-1]), "spread": float(a[-1] - a[0])}


def idle_fraction(sizes_of):
    """Blocks of one trimmed chain-step launch over the batch (grid + 1/8 + 2048 lanes of the largest grid, rounded to 8 blocks, per
    sequence) that have no lane of their sequence's grid + 1/8 to step."""
    grids = [-(-h // RATIO) * -(-w // RATIO) for h, w in sizes_of]
    lanes = max(g + g // 8 + 2048 for g in grids)
    gx = (-(-lanes // CHAIN_TILE) + 7) // 8 * 8
    busy = sum(min(gx, -(-(g + g // 8) // CHAIN_TILE)) for g in grids)
    return 1.0 - busy / float(gx * len(grids))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="davis16,davis64,same16")
    ap.add_argument("--modes", default="track,mb,opt")
    ap.add_argument("--distinct", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--parent-lib", default=None, help="libpsfm_hip.so of the parent commit (variant a)")
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
        LP.psfm_ctx_set_motion_boundary.argtypes = L.psfm_ctx_set_motion_boundary.argtypes
        LP.psfm_ctx_set_capacity.argtypes = L.psfm_ctx_set_capacity.argtypes
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
    handles = {v: contexts(libs[v], 64) for v in libs}      # (every variant has contexts of its own)

    def result(handle, info):
        n, npnt = int(info.n_traj), int(info.n_points)
        birth, length, off, xy = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n + 1, np.int64), np.zeros((npnt, 2), np.float64)
        assert L.psfm_result_copy(handle, *[x.ctypes.data_as(vp) for x in (birth, length, off, xy)], sp) == 0
        return birth.tobytes() + length.tobytes() + off.tobytes(), xy

    res = {"reps": a.reps, "warmup": a.warmup, "variants": sorted(libs), "n_flows": N_FLOWS, "sample_ratio": RATIO, "runs": []}
    for name in a.shapes.split(","):
        B, sizes = SHAPES[name]
        for mode in a.modes.split(","):
            opt, mb = mode == "opt", mode == "mb"
            pool = {}
            for (H, W) in sizes:
                for k in range(a.distinct):
                    if opt:
                        d = psfm_synth.synth_sequence_torch(N_FLOWS + 1, H, W, seed=51 + k, stride2=True, device="cuda")
                    else:
                        d = psfm_synth.synth_realistic_torch(N_FLOWS + 1, H, W, seed=41 + k, stride2=False, device="cuda", **psfm_synth.REALISTIC)
                    pool[(H, W, k)] = tuple(d[key].contiguous() for key in (("flows_f", "flows_b", "flows_f2", "flows_b2") if opt else ("flows_f", "flows_b")))
                    del d
            # the directory: sizes interleaved, as a listing of clips would have them
            size_of = [sizes[k % len(sizes)] for k in range(B)]
            seqs = [pool[size_of[k] + ((k // len(sizes)) % a.distinct,)] for k in range(B)]
            groups = [[k for k in range(B) if size_of[k] == s] for s in sizes]
            infos = {v: (_hip.TrackInfo * B)() for v in libs}
            for v in libs:
                for h in handles[v][:B]:
                    assert libs[v].psfm_ctx_set_motion_boundary(h, 1 if mb else 0, 0.02) == 0
                    assert libs[v].psfm_ctx_set_capacity(h, 2.0, 8.0) == 0

            def call(v):
                lib = libs[v]
                if v == "c":
                    ks = list(range(B))
                    for k in ks:
                        assert L.psfm_ctx_set_frame_size(handles[v][k], size_of[k][0], size_of[k][1]) == 0
                    todo = [(ks, 0, 0)]
                else:
                    todo = [(ks, sizes[g][0], sizes[g][1]) for g, ks in enumerate(groups)]
                for ks, h, w in todo:
                    n = len(ks)
                    arr = lambda j: (vp * n)(*[seqs[k][j].data_ptr() for k in ks])
                    out = (_hip.TrackInfo * n)()
                    # (group g runs on the contexts of its sequences: context k holds sequence k's result afterwards in every variant)
                    st = lib.psfm_connect_batch((vp * n)(*[handles[v][k].value for k in ks]), n, arr(0), arr(1), arr(2) if opt else None,
                                                arr(3) if opt else None, (ctypes.c_int * n)(*[N_FLOWS] * n), h, w, 1.0, RATIO, out, sp)
                    if st == _hip.PSFM_ERR_CAPACITY:
                        return st
                    assert st == 0, lib.psfm_last_error()
                    for j, k in enumerate(ks):
                        infos[v][k] = out[j]
                return 0
            # table factors: the defaults, grown for every variant alike (as run_connect_batch grows them) until every call fits -- the
            # motion-boundary option ends tracks at every boundary, more records than 8 x the grid holds
            lane_f, traj_f = 2.0, 8.0
            while any(call(v) != 0 for v in sorted(libs)):
                lane_f, traj_f = lane_f * 2.0, traj_f * 4.0
                assert lane_f <= 64.0
                for v in libs:
                    for h in handles[v][:B]:
                        assert libs[v].psfm_ctx_set_capacity(h, lane_f, traj_f) == 0
            t = {v: [] for v in libs}
            for rep in range(a.warmup + a.reps):
                for v in sorted(libs):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    assert call(v) == 0
                    torch.cuda.synchronize()
                    if rep >= a.warmup:
                        t[v].append((time.perf_counter() - t0) * 1e3)
            same_ids, same_bytes, worst = True, True, 0.0
            for k in range(B):
                x, y = result(handles["c"][k], infos["c"][k]), result(handles["b"][k], infos["b"][k])
                same_ids = same_ids and x[0] == y[0]
                same_bytes = same_bytes and x[0] == y[0] and x[1].tobytes() == y[1].tobytes()
                if x[1].shape == y[1].shape and x[1].size:
                    worst = max(worst, float(np.abs(x[1] - y[1]).max()))
            s = {v: stats(t[v], B) for v in libs}
            run = {"shape": name, "mode": mode, "n_seq": B, "sizes": sizes, "per_variant": s, "table_factors": [lane_f, traj_f],
                   "modes_c": {str(m): [int(i.chain_mode) for i in infos["c"]].count(m) for m in set(int(i.chain_mode) for i in infos["c"])},
                   "modes_b": {str(m): [int(i.chain_mode) for i in infos["b"]].count(m) for m in set(int(i.chain_mode) for i in infos["b"])},
                   "c_ids_births_lengths_equal_b": bool(same_ids), "c_all_bytes_equal_b": bool(same_bytes), "c_positions_largest_difference_px": worst,
                   "chain_step_blocks_that_return_at_once": idle_fraction(size_of)}
            for x, y in (("a", "c"), ("b", "c"), ("a", "b")):
                if x in s and y in s:
                    diff = s[x]["median_ms_per_seq"] - s[y]["median_ms_per_seq"]
                    spread = max(s[x]["spread"], s[y]["spread"])
                    run["%s_minus_%s" % (x, y)] = {"difference": diff, "three_spreads": 3 * spread,
                                                   "verdict": "%s faster" % y if diff > 3 * spread else ("%s faster" % x if -diff > 3 * spread else "level")}
            res["runs"].append(run)
            print(name, mode, {v: round(s[v]["median_ms_per_seq"], 3) for v in s}, run["modes_c"], "bytes equal" if same_bytes else "ids equal" if same_ids else "DIFFERENT",
                  file=sys.stderr, flush=True)
            for v in libs:
                for h in handles[v][:B]:
                    assert libs[v].psfm_ctx_set_motion_boundary(h, 0, 0.02) == 0
                    if v != "a":
                        assert L.psfm_ctx_set_frame_size(h, 0, 0) == 0
            del pool, seqs
            torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
