#!/usr/bin/env python3
"""Stage 2 (the motion classifier over the windows of a sequence) with the front end per window and in one pass, on the same
device, tensors and weights: from "the result is in the context" to finish() returned (host clock around a synchronised region),
as scripts/micro/decoder_batch.py --mode stage measures it.

Routes
  shipped  merge_labels.label_sequences_batched(...) without the `front` argument: what ANY tree runs by default.  With
           --tree PATH the package and its library are taken from another checkout (the parent commit, built there), so the
           comparison is against the parent's library, in a process of its own.
  window   label_sequences_batched(..., front="window") of this tree: per window two psfm_window_sample calls (three host
           synchronisations), four allocations, one psfm_traj_augment and one psfm_traj_encode launch.
  batch    label_sequences_batched(..., front="batch"): per context one psfm_window_sample_batch plan (ONE synchronisation) and
           one fill; one psfm_traj_augment_batch and one psfm_traj_encode_batch launch per 64 windows of all contexts.
Shapes (window 10, traj_max_num 100 000, input 240x424, seeded weights, seeded depth maps made before the clock starts)
  a  16 sequences of 480x854 x 51 frames, sample_ratio 4, through run_connect_batch (section 25's stage-2 shape)
  b  1080p x 101 frames, sample_ratio 2, one context (the headline)
  c  the small-window shape: a with sample_ratio 16 (--ratio overrides); the JSON states the rows per window it gave
--warmup runs, then --rounds timed runs per route, alternating between the routes of the process.  `spread` is max - min over the
runs of a route.  Per context the sha256 over the five tensors of finish() and the window ids is printed, so that routes measured
in different processes can be compared byte for byte:
  --compare A.json B.json ...   reads result files, checks that all digests agree and says per pair of routes whether the
                                difference of the medians exceeds three times the larger spread (the project's bar).
  --only ROUTE --calls N        run ROUTE N times and exit (for a kernel trace).
Prints one JSON line.
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
INPUT_SIZE = (240, 424)
SHAPES = {"a": dict(n_seq=16, H=480, W=854, frames=51, ratio=4), "b": dict(n_seq=1, H=1080, W=1920, frames=101, ratio=2),
          "c": dict(n_seq=16, H=480, W=854, frames=51, ratio=16)}


def compare(paths):
    res = [json.loads(open(p).read().strip().splitlines()[-1]) for p in paths]
    routes = {}
    for r in res:
        for name, v in r["routes"].items():
            routes["%s@%s" % (name, r["tree"])] = dict(v, digests=r["digests"][name], shape=r["shape"])
    names = sorted(routes)
    digests = {json.dumps(routes[n]["digests"]) for n in names}
    out = {"mode": "compare", "routes": {n: {k: routes[n][k] for k in ("median", "min", "max", "spread")} for n in names},
           "bytes_equal": len(digests) == 1 and len({routes[n]["shape"] for n in names}) == 1, "pairs": {}}
    for i, x in enumerate(names):
        for y in names[i + 1:]:
            d = routes[x]["median"] - routes[y]["median"]
            bar = 3.0 * max(routes[x]["spread"], routes[y]["spread"])
            out["pairs"]["%s - %s" % (x, y)] = {"difference_ms": d, "three_spreads_ms": bar,
                                                "verdict": "second is faster" if d > bar else "first is faster" if -d > bar else "no difference by the bar"}
    return out


def measure(a):
    tree = os.path.abspath(a.tree) if a.tree else ROOT
    sys.path.insert(0, os.path.join(tree, "particle-sfm_amd"))
    sys.path.insert(1, os.path.join(ROOT, "tests"))
    import torch
    assert torch.cuda.is_available(), "stage2_front.py measures on the GPU"
    import psfm_synth
    from _decoder_np import seeded_decoder_weights
    from _encoder_np import fixture_weights
    from point_trajectory import _hip
    from point_trajectory.trajectory import run_connect, run_connect_batch
    from psfm_motion_seg.decoder import pack_decoder_weights
    from psfm_motion_seg.encoder import pack_encoder_weights
    from psfm_motion_seg.load_cut_seq import window_ranges
    from psfm_motion_seg.merge_labels import label_sequences_batched
    S = dict(SHAPES[a.shape])
    if a.ratio:
        S["ratio"] = a.ratio
    H, W, T, n_seq = S["H"], S["W"], S["frames"], S["n_seq"]
    dec_w = pack_decoder_weights(seeded_decoder_weights())
    enc_w = pack_encoder_weights(fixture_weights()[0])
    seqs = []
    for s in range(n_seq):
        d = psfm_synth.synth_sequence_torch(T, H, W, seed=s, sigma=0.05, n_occluders=2, stride2=False, device="cuda")
        seqs.append((d["flows_f"], d["flows_b"], None, None))
    if n_seq > 1:
        ctxs, infos = run_connect_batch(seqs, 1.0, S["ratio"])
    else:
        infos = [run_connect(seqs[0][0], seqs[0][1], None, None, 1.0, S["ratio"], return_device=True)]
        ctxs = [_hip.context()]
    del seqs
    gen = torch.Generator(device="cuda")
    gen.manual_seed(17)
    depth = {(s, f0): torch.rand((n,) + INPUT_SIZE, generator=gen, device="cuda", dtype=torch.float32)
             for s in range(n_seq) for f0, n in window_ranges(T, a.window)}
    args = (ctxs, [T] * n_seq, a.window, (H, W), INPUT_SIZE, a.traj_max_num, enc_w, dec_w, lambda s, t: depth[(s, int(t[0]))])
    routes = {"shipped": lambda: label_sequences_batched(*args, seed=a.seed),
              "window": lambda: label_sequences_batched(*args, seed=a.seed, front="window"),
              "batch": lambda: label_sequences_batched(*args, seed=a.seed, front="batch")}
    names = a.routes.split(",")
    if a.only:
        for _ in range(a.calls):
            routes[a.only]()
        torch.cuda.synchronize()
        return {"only": a.only, "calls": a.calls, "shape": a.shape, "tree": os.path.basename(tree)}

    def digest(ms):
        # (every context's set is read before the next route begins: a context holds one labelled set)
        out = []
        for m in ms:
            h = hashlib.sha256()
            for t in list(m.finish()) + list(m.window_ids):
                h.update(t.cpu().numpy().tobytes())
            out.append(h.hexdigest()[:16])
        return out

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ms = fn()                                               # (the last finish() synchronises the stream)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), ms

    digests, rows = {}, {}
    for r in names:
        for _ in range(a.warmup):
            _, ms = timed(routes[r])
        digests[r] = digest(ms)
        rows[r] = [[int(i.numel()) for i in m.window_ids] for m in ms]
    t = {r: [] for r in names}
    for _ in range(a.rounds):
        for r in names:
            t[r].append(timed(routes[r])[0])
    all_rows = [k for seq in rows[names[0]] for k in seq]
    res = {"mode": "stage2_front", "shape": a.shape, "tree": os.path.basename(tree),
           "workload": "%d x %dx%d x %d frames, sample_ratio %d, window %d, traj_max_num %d, input %dx%d"
           % (n_seq, H, W, T, S["ratio"], a.window, a.traj_max_num, INPUT_SIZE[0], INPUT_SIZE[1]),
           "trajectories": [int(i.n_traj) for i in infos], "windows": len(all_rows),
           "rows_per_window": {"min": int(min(all_rows)), "median": float(np.median(all_rows)), "max": int(max(all_rows))},
           "rows_all_windows": int(sum(all_rows)), "rounds": a.rounds, "digests": digests,
           "bytes_equal": len({json.dumps(d) for d in digests.values()}) == 1, "routes": {}}
    for r in names:
        v = np.array(t[r])
        res["routes"][r] = {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "spread": float(v.max() - v.min()),
                            "runs": [float(x) for x in v]}
    if "window" in names and "batch" in names:
        d = res["routes"]["window"]["median"] - res["routes"]["batch"]["median"]
        bar = 3.0 * max(res["routes"]["window"]["spread"], res["routes"]["batch"]["spread"])
        res.update(difference_ms=d, three_spreads_ms=bar, batch_is_faster=bool(d > bar))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), default="a")
    ap.add_argument("--ratio", type=int, default=0, help="override the shape's sample_ratio")
    ap.add_argument("--tree", default=None, help="another checkout (built) whose package and library run the routes")
    ap.add_argument("--routes", default="window,batch")
    ap.add_argument("--window", type=int, default=10)
    ap.add_argument("--traj-max-num", type=int, default=100000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default=None, help="run --calls calls of one route and exit (for a kernel trace)")
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--compare", nargs="+", default=None, help="result files to compare instead of measuring")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    res = compare(a.compare) if a.compare else measure(a)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fp:
            fp.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
