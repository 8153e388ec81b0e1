#!/usr/bin/env python3
"""The COLMAP database tables (csrc/psfm_database.hip) at a 1080p match table: the row compaction against a device-to-device copy of
the same bytes, and the whole step against the route the package had before it.

Workload: psfm_synth 1080x1920, --frames frames, r = 2 -> psfm_connect -> psfm_result_filter(3) -> psfm_traj_to_matches (every point
kept); COLMAP ids and the iteration order are two seeded random permutations.

  kernel      psfm_database_compact_again (the compaction launch alone) and a torch copy_ between two device buffers of
              8 * n_rows_kept bytes (the same 8 B read + 8 B written per kept row), ALTERNATED, each between two HIP events of its
              own after --warmup rounds; medians and min-max of --reps rounds, and the ratio of the medians.
  end to end  wall clock, alternated, --e2e-reps rounds, from the tables in HBM to what executemany consumes:
                new   psfm_matches_to_database + psfm_database_copy (database_tables_device), the pair list file from pair_key /
                      pair_first, and the offset lists the writer slices the two buffers by
                old   psfm_matches_copy of everything, assemble(as_arrays=True) (which writes the pair list file), then the
                      reference's loop restated: per image np.asarray(np.array(kp) + 0.5, np.float32).tobytes(), per pair the
                      `matched` set, np.asarray(np.array(match)[:, ::-1] if id0 > id1, np.uint32).tobytes()
              sqlite is on neither side.  The blobs of the two routes are compared by id in the first round.
Prints one JSON line (--out also writes it to a file).
"""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "particle-sfm_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=101)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--e2e-reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()

    import torch
    import psfm_synth
    from point_trajectory import _hip
    from point_trajectory.trajectory import run_connect
    from psfm_sfm import database as dbm
    from psfm_sfm import matches_from_flow as mff

    assert torch.cuda.is_available(), "database.py measures on the GPU"
    log = lambda msg: print(msg, file=sys.stderr, flush=True)
    T, H, W = a.frames, a.height, a.width
    d = psfm_synth.synth_sequence_torch(T, H, W, seed=0, sigma=0.05, n_occluders=2, stride2=False, device=torch.device("cuda", 0))
    ctx = _hip.context(0)
    run_connect(d["flows_f"], d["flows_b"], None, None, 1.0, 2, return_device=True)
    del d
    torch.cuda.empty_cache()
    L, sp = _hip.lib(), _hip.current_stream_ptr(0)
    k, n = ctypes.c_int64(0), ctypes.c_int64(0)
    _hip.check(L.psfm_result_filter(ctx.handle, 3, ctypes.byref(k), ctypes.byref(n), sp))
    n_kp, n_m, n_p = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    _hip.check(L.psfm_traj_to_matches(ctx.handle, T, mff.SAMPLE_K, None, ctypes.byref(n_kp), ctypes.byref(n_m), ctypes.byref(n_p), sp))
    n_kp, n_m, n_p = int(n_kp.value), int(n_m.value), int(n_p.value)
    rng = np.random.default_rng(1)
    db_id, db_pos = (rng.permutation(T) + 1).astype(np.int32), rng.permutation(T).astype(np.int32)
    names = ["%05d.png" % i for i in range(T)]
    image_ids = {names[i]: int(db_id[i]) for i in np.argsort(db_pos)}
    vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    kept_p, kept_r = ctypes.c_int64(0), ctypes.c_int64(0)
    _hip.check(L.psfm_matches_to_database(ctx.handle, T, vp(db_id), vp(db_pos), ctypes.byref(kept_p), ctypes.byref(kept_r), sp))
    n_rows = int(kept_r.value)
    log("tables: %d matches in %d pairs, %d rows in %d pairs kept" % (n_m, n_p, n_rows, int(kept_p.value)))
    out = {"workload": "%dx%d, %d frames, r=2, every point kept" % (H, W, T), "n_saved": int(k.value), "n_keypoints": n_kp, "n_matches": n_m,
           "n_pairs": n_p, "n_pairs_kept": int(kept_p.value), "n_rows_kept": n_rows, "chunk_rows": dbm.chunk_rows(),
           "compact_bytes": 16 * n_rows, "keypoint_bytes": 24 * n_kp, "reps": a.reps, "e2e_reps": a.e2e_reps}

    # ---- the compaction launch against a device-to-device copy of the same bytes, alternated ----
    src = torch.empty(8 * n_rows, dtype=torch.uint8, device="cuda")
    dst = torch.empty(8 * n_rows, dtype=torch.uint8, device="cuda")
    src.zero_()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)
    compact = lambda: _hip.check(L.psfm_database_compact_again(ctx.handle, sp))
    copy = lambda: dst.copy_(src)
    tk, tc = [], []
    for r in range(a.warmup + a.reps):
        x, y = timed(compact), timed(copy)
        if r >= a.warmup:
            tk.append(x)
            tc.append(y)
    tk, tc = np.array(tk), np.array(tc)
    out.update(compact_ms=float(np.median(tk)), compact_ms_min_max=[float(tk.min()), float(tk.max())],
               copy_ms=float(np.median(tc)), copy_ms_min_max=[float(tc.min()), float(tc.max())],
               compact_over_copy=float(np.median(tk) / np.median(tc)), compact_GBps=16e-6 * n_rows / float(np.median(tk)))
    del src, dst
    log("kernel: compact %.3f ms, copy %.3f ms" % (np.median(tk), np.median(tc)))
    torch.cuda.empty_cache()

    # ---- end to end, alternated ----
    tmp = tempfile.mkdtemp()

    def new_route():
        pair_key, pair_first = np.empty(n_p, np.int64), np.empty(n_p, np.int64)
        _hip.check(L.psfm_matches_copy(ctx.handle, None, None, vp(pair_key), None, vp(pair_first), None, sp))
        dbm.write_pair_file(os.path.join(tmp, "new.txt"), names, pair_key, pair_first)
        t = dbm.database_tables_device(ctx, T, db_id, db_pos)
        ko, po, pid = (8 * t.kp_off).tolist(), (8 * t.pair_off).tolist(), t.pair_id.tolist()
        return t, ko, po, pid

    def old_route():
        tables = mff._copy_tables(ctx, T, n_kp, n_m, n_p)
        datas = mff.assemble(names, tables, os.path.join(tmp, "old.txt"), as_arrays=True)
        kp, mt, matched = {}, {}, set()
        for name, image_id in image_ids.items():
            kp[image_id] = np.asarray(np.array(datas[name].keypoints) + 0.5, np.float32).tobytes()
        for name, image_id in image_ids.items():
            for pair, match in datas[name].match_pairs.items():
                n0, n1 = pair.split("-")
                id0, id1 = image_ids[n0], image_ids[n1]
                if len({(id0, id1), (id1, id0)} & matched) > 0:
                    continue
                match = np.array(match)
                if id0 > id1:
                    match = match[:, ::-1]
                mt[min(id0, id1) * (2 ** 31 - 1) + max(id0, id1)] = np.asarray(match, np.uint32).tobytes()
                matched |= {(id0, id1), (id1, id0)}
        return kp, mt

    tn, to = [], []
    equal = None
    for r in range(a.e2e_reps):
        t0 = time.perf_counter()
        t, ko, po, pid = new_route()
        t1 = time.perf_counter()
        kp, mt = old_route()
        t2 = time.perf_counter()
        log("end to end round %d: new %.1f ms, old %.1f ms" % (r, 1e3 * (t1 - t0), 1e3 * (t2 - t1)))
        tn.append(1e3 * (t1 - t0))
        to.append(1e3 * (t2 - t1))
        if r == 0:
            rows = t.rows.reshape(-1).view(np.uint8)
            kpb = t.kp_f32.reshape(-1).view(np.uint8)
            equal = (sorted(pid) == sorted(mt) and all(mt[p] == rows[po[g]:po[g + 1]].tobytes() for g, p in enumerate(pid))
                     and all(kp[int(db_id[i])] == kpb[ko[i]:ko[i + 1]].tobytes() for i in range(T))
                     and open(os.path.join(tmp, "new.txt")).read() == open(os.path.join(tmp, "old.txt")).read())
        del t, kp, mt
    tn, to = np.array(tn), np.array(to)
    out.update(new_ms=float(np.median(tn)), new_ms_min_max=[float(tn.min()), float(tn.max())], old_ms=float(np.median(to)),
               old_ms_min_max=[float(to.min()), float(to.max())], old_over_new=float(np.median(to) / np.median(tn)), routes_equal=bool(equal))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fp:
            fp.write(line + "\n")
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
