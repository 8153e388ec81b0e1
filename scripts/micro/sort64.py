#!/usr/bin/env python3
"""psfm_sort_records64 on n (key, value) pairs of a long-sequence key layout: checked against numpy's stable argsort, then timed with
device events over `reps` sorts (the figure includes the entry point's four staging copies, 2 x n x 12 B; for the kernels alone run
this script under rocprofv3 --kernel-trace --stats), beside torch.sort(stable=True) on the same int64 keys (a rocPRIM pair sort over
all 64 bits) for orientation.
Usage: sort64.py [layout] [n] [reps]      layout: c3 (1080p x 401, r = 2: 9 + 9 + 19 = 37 bits), c4 (480 x 640 x 1000, r = 1:
10 + 10 + 19 = 39 bits), full (random 64-bit keys)"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "particle-sfm_amd"))
import torch
from point_trajectory import _hip

layout = sys.argv[1] if len(sys.argv) > 1 else "c3"
n = int(sys.argv[2]) if len(sys.argv) > 2 else 8_000_000
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
rng = np.random.default_rng(0)
if layout == "full":
    keys, end_bit = rng.integers(0, 1 << 64, n, dtype=np.uint64), 64
else:
    frames, grid, tbits = {"c3": (401, 540 * 960, 9), "c4": (1000, 480 * 640, 10)}[layout]
    death = np.sort(rng.integers(0, frames + 1, n).reshape(-1, 1)[: (n // 2048) * 2048].reshape(-1, 2048), axis=1).reshape(-1)
    death = np.concatenate([death, rng.integers(0, frames + 1, n - death.size)]).astype(np.uint64)      # segments ordered by death step
    birth = np.minimum((rng.random(n) * (death + 1.0)).astype(np.uint64), death)
    keys = (death << np.uint64(19 + tbits)) | (birth << np.uint64(19)) | rng.integers(0, grid, n).astype(np.uint64)
    end_bit = 19 + 2 * tbits
vals = np.arange(n, dtype=np.int32)
ctx = _hip.context(0)
dk = torch.from_numpy(keys.view(np.int64)).cuda()
dv = torch.from_numpy(vals).cuda()
s = _hip.current_stream_ptr()


def ours():
    k, v = dk.clone(), dv.clone()
    _hip.check(_hip.lib().psfm_sort_records64(ctx.handle, _hip.ptr(k), _hip.ptr(v), n, end_bit, s))
    return k, v


def timed(fn):
    fn(); fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    t = sorted(1e3 * a.elapsed_time(b) for a, b in ev)
    return {"median_us": round(t[len(t) // 2], 1), "min_us": round(t[0], 1)}


k, v = ours()
torch.cuda.synchronize()
order = np.argsort(keys, kind="stable")
ok = bool(np.array_equal(k.cpu().numpy().view(np.uint64), keys[order]) and np.array_equal(v.cpu().numpy(), vals[order]))
out = {"layout": layout, "n": n, "end_bit": end_bit, "passes": (end_bit + 7) // 8, "equal_to_numpy_stable_sort": ok,
       "bytes_per_pass": 2 * n * 12, "psfm_sort_records64_with_clones": timed(ours),
       "clones_alone": timed(lambda: (dk.clone(), dv.clone())), "torch_sort_stable_int64": timed(lambda: torch.sort(dk, stable=True))}
print(json.dumps(out))
sys.exit(0 if ok else 1)
