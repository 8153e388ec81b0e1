#!/usr/bin/env python3
"""A stage that starts from a track.npy: what it costs to get the file's set into a context, and to get from the file to finished
match tables, on one device in one session (host clock around synchronised regions; the page cache is WARM: the file was written by
this process just before and is read once more before the clock starts).

The input is written by save_track_npy (reference layout, with the footer) from the saved set (traj_min_len 3) of a psfm_connect run
on a seeded synthetic sequence of the chosen shape:
  b  1080p x 101 frames, sample_ratio 2 (the headline)
  m  480x854 x 40 frames, sample_ratio 2
  s  480x854 x 24 frames, sample_ratio 4

(i)  file -> result in the context
       file   Context.load_track_npy: psfm_load_track_npy, --threads reader threads through the pinned ring
       host   load_track_npy (NumPy decode of the records, the points memory-mapped) + TrajectorySet.to_device (psfm_result_set
              from pageable host arrays)
     with the byte counts and the implied GB/s, beside psfm_load_flo_stack on .flo files of the same frame size and about the same
     total size, same session, same number of reader threads.
(ii) file -> finished match tables (as_arrays=True)
       device  traj_to_matches(..., device=True): the file into a context, psfm_result_filter(1), psfm_traj_to_matches, one copy
       host    traj_to_matches(..., device=False): the only route before this entry existed
     --tables-shape picks another (smaller) shape for (ii): the host tables hold every match in several int64 arrays.

--warmup runs, then --rounds timed runs per route, alternating between the routes.  `spread` is max - min over a route's runs; a
route is called faster only when the medians differ by more than three times the larger spread.  Routes of a part must give the same
bytes (sha256 over the result / over the tables).  Prints one JSON line."""
import argparse
import ctypes
import hashlib
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SHAPES = {"b": dict(H=1080, W=1920, frames=101, ratio=2), "m": dict(H=480, W=854, frames=40, ratio=2),
          "s": dict(H=480, W=854, frames=24, ratio=4)}


def stats(v):
    v = np.asarray(v, np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "spread": float(v.max() - v.min()),
            "runs": [float(x) for x in v]}


def verdict(a, b, name_a, name_b):
    d = a["median"] - b["median"]
    bar = 3.0 * max(a["spread"], b["spread"])
    return {"difference_ms": d, "three_spreads_ms": bar,
            "verdict": "%s is faster" % name_b if d > bar else "%s is faster" % name_a if -d > bar else "no difference by the bar"}


def alternate(routes, warmup, rounds, sync):
    """{name: fn} -> {name: [ms]}; every fn returns a digest, all digests of all runs must agree."""
    digests = set()

    def timed(fn):
        sync()
        t0 = time.perf_counter()
        out = fn()
        sync()
        return 1e3 * (time.perf_counter() - t0), out
    for name, fn in routes.items():
        for _ in range(warmup):
            timed(fn)
    t = {name: [] for name in routes}
    for _ in range(rounds):
        for name, fn in routes.items():
            ms, finish = timed(fn)
            t[name].append(ms)
            digests.add(finish())            # (outside the clock)
    return t, digests


def make_file(shape, work):
    """psfm_connect on the seeded sequence, its saved set written with the footer.  Returns (traj_dir, T, sizes)."""
    import torch
    import psfm_synth
    from point_trajectory import _hip
    from point_trajectory.trajectory import result_to_trajectory_set, run_connect, save_track_npy, wait_for_reclaims
    S = SHAPES[shape]
    d = psfm_synth.synth_sequence_torch(S["frames"], S["H"], S["W"], seed=0, sigma=0.05, n_occluders=2, stride2=False, device="cuda")
    info = run_connect(d["flows_f"], d["flows_b"], None, None, 1.0, S["ratio"], return_device=True)
    ts = result_to_trajectory_set(_hip.context(), info, 3)
    traj_dir = os.path.join(work, "trajectories_" + shape)
    os.makedirs(traj_dir, exist_ok=True)
    path = os.path.join(traj_dir, "track.npy")
    save_track_npy(path, ts)
    wait_for_reclaims()
    ids, birth, length, off, xy, _ = ts._csr
    sizes = {"file_bytes": os.path.getsize(path), "n_traj": int(len(ids)), "n_points": int(off[-1]), "n_result": int(ids[-1]) + 1,
             "result_trajectories": int(info.n_traj)}
    del d, ts
    torch.cuda.empty_cache()
    with open(path, "rb") as fp:                         # the page cache is warm
        while fp.read(1 << 26):
            pass
    return traj_dir, S["frames"], sizes


def part_ingest(a, work):
    import torch
    from point_trajectory import _hip, reference_pickle
    from point_trajectory.trajectory import load_track_npy
    from point_trajectory.utils import load_flows_device, write_flo
    traj_dir, T, sizes = make_file(a.shape, work)
    path = os.path.join(traj_dir, "track.npy")
    ctx = _hip.Context(torch.cuda.current_device())
    L = _hip.lib()
    rec_size = len(reference_pickle._record_template()[0])
    sizes["record_bytes"] = sizes["n_traj"] * rec_size
    sizes["point_bytes"] = 16 * sizes["n_points"]
    moved = sizes["record_bytes"] + sizes["point_bytes"]

    def digest():
        n, p = sizes["n_result"], sizes["n_points"]
        birth, length, off, xy = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n + 1, np.int64), np.empty((p, 2))
        vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)
        _hip.check(L.psfm_result_copy(ctx.handle, vp(birth), vp(length), vp(off), vp(xy), _hip.current_stream_ptr(ctx.device)))
        h = hashlib.sha256()
        for x in (birth, length, off, xy):
            h.update(x.tobytes())
        return h.hexdigest()[:16]

    def file_route():
        assert ctx.load_track_npy(path, a.threads) == (sizes["n_traj"], sizes["n_points"], sizes["n_result"])
        return digest

    def host_route():
        load_track_npy(path).to_device(ctx)
        return digest
    t, digests = alternate({"file": file_route, "host": host_route}, a.warmup, a.rounds, torch.cuda.synchronize)
    res = {"sizes": sizes, "threads": a.threads, "bytes_equal": len(digests) == 1,
           "routes": {k: dict(stats(v), gb_per_s=moved / 1e6 / float(np.median(v))) for k, v in t.items()}}
    res["file_against_host"] = verdict(res["routes"]["host"], res["routes"]["file"], "host", "file")
    # psfm_load_flo_stack in the same session: frames of the same size, about the points' bytes, the same number of reader threads
    S = SHAPES[a.shape]
    frame = S["H"] * S["W"] * 8
    n_flo = max(2, min(64, sizes["point_bytes"] // frame))
    flo_dir = os.path.join(work, "flo")
    os.makedirs(flo_dir, exist_ok=True)
    rng = np.random.default_rng(1)
    one = rng.standard_normal((S["H"], S["W"], 2)).astype(np.float32)
    for i in range(n_flo):
        write_flo(os.path.join(flo_dir, "%05d.flo" % i), one)
    ms = []
    for i in range(a.warmup + a.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = load_flows_device(flo_dir, n_readers=a.threads)
        torch.cuda.synchronize()
        if i >= a.warmup:
            ms.append(1e3 * (time.perf_counter() - t0))
        del out
    res["load_flo_stack"] = dict(stats(ms), files=int(n_flo), bytes=int(n_flo * (frame + 12)), gb_per_s=n_flo * frame / 1e6 / float(np.median(ms)))
    shutil.rmtree(flo_dir)
    ctx.close()
    return res


def part_tables(a, work):
    import torch
    from psfm_sfm import matches_from_flow as mff
    traj_dir, T, sizes = make_file(a.tables_shape, work)
    img_dir = os.path.join(work, "images_" + a.tables_shape)
    os.makedirs(img_dir, exist_ok=True)
    for i in range(T):
        open(os.path.join(img_dir, "%05d.png" % i), "w").close()
    pairs = os.path.join(work, "pairs.txt")

    def route(device):
        def run():
            datas = mff.traj_to_matches(img_dir, traj_dir, pairs, as_arrays=True, device=device)

            def digest():
                h = hashlib.sha256()
                for name, dm in datas.items():
                    h.update(np.ascontiguousarray(dm.keypoints, np.float64).tobytes())
                    for key, rows in dm.match_pairs.items():
                        h.update(key.encode())
                        h.update(np.ascontiguousarray(rows, np.int32).tobytes())
                h.update(open(pairs, "rb").read())
                return h.hexdigest()[:16]
            return digest
        return run
    t, digests = alternate({"device": route(True), "host": route(False)}, a.warmup, a.rounds, torch.cuda.synchronize)
    res = {"shape": a.tables_shape, "sizes": sizes, "bytes_equal": len(digests) == 1, "routes": {k: stats(v) for k, v in t.items()}}
    res["device_against_host"] = verdict(res["routes"]["host"], res["routes"]["device"], "host", "device")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), default="b", help="part (i)")
    ap.add_argument("--tables-shape", choices=sorted(SHAPES), default=None, help="part (ii); default: --shape")
    ap.add_argument("--parts", default="ingest,tables")
    ap.add_argument("--threads", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--dir", default=None, help="where the files go (default: a temporary directory, removed afterwards)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    a.tables_shape = a.tables_shape or a.shape
    sys.path.insert(0, os.path.join(ROOT, "particle-sfm_amd"))
    import torch
    assert torch.cuda.is_available(), "track_npy_ingest.py measures on the GPU"
    work = a.dir or tempfile.mkdtemp(prefix="psfm_track_npy_")
    os.makedirs(work, exist_ok=True)
    res = {"mode": "track_npy_ingest", "page_cache": "warm", "rounds": a.rounds, "warmup": a.warmup, "shape": a.shape}
    try:
        if "ingest" in a.parts.split(","):
            res["ingest"] = part_ingest(a, work)
        if "tables" in a.parts.split(","):
            res["tables"] = part_tables(a, work)
    finally:
        if not a.dir:
            shutil.rmtree(work, ignore_errors=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fp:
            fp.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
