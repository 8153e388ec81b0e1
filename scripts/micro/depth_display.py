#!/usr/bin/env python3
"""The display images of the sparse depth maps (csrc/psfm_depth_display.hip) at the headline size: the four passes against a
device-to-device copy of the same bytes, the device against the NumPy model, and model files -> output files end to end against the
parent commit.

Workload: the seeded synthetic model of scripts/micro/sparse_depth.py -- --images images of --width x --height, --obs observations.

  kernel      the maps of all images made once (one psfm_sparse_depth call, budget 0); then --reps rounds after --warmup of one
              psfm_depth_display call with the context's timing on -- count, compact, select, colour, each between two HIP events,
              and the call as a whole on the host clock (it ends in a synchronise) -- ALTERNATED with a torch copy_ between two device
              buffers of half the passes' byte count (so that the copy reads + writes that count).  Bytes, from the shapes: count 8 per
              pixel; compact 8 per pixel + 8 per valid pixel written; select 8 rounds x 8 per valid pixel; colour 8 + 4 per pixel.
  check       every image of the device against psfm_sfm.convert.depth_display_host, bit for bit (--check-images limits it).
  end to end  wall clock of write_depth_pose_from_colmap_format, model files -> all output files, each run in a fresh process behind
              one small untimed conversion (HIP start-up, code objects, matplotlib's import): this commit with display="device"
              ALTERNATED with the parent commit (--parent: the particle-sfm_amd directory of a built checkout of it), --e2e-runs
              each; then this commit with display="host", with writers 2 and 4, and with png=False.
  host split  the device route's host side once, on --split-images images: device-to-host copy of the RGBA, plt.imsave, and PIL's
              encode of the same array for comparison.
Prints one JSON line (--out also writes it to a file)."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PACKAGE = os.path.join(ROOT, "particle-sfm_amd")


def run_one(package, warm_model, model_dir, out_dir, kwargs):
    """(in a fresh process) -> seconds of one conversion with the package under `package`."""
    sys.path.insert(0, package)
    os.environ.setdefault("MPLBACKEND", "Agg")
    import torch
    from psfm_sfm import convert
    warm = out_dir + "_warm"
    convert.write_depth_pose_from_colmap_format(warm_model, warm, **kwargs)
    shutil.rmtree(warm, ignore_errors=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    convert.write_depth_pose_from_colmap_format(model_dir, out_dir, **kwargs)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def stats(v):
    v = np.array(v, np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "runs": [float(x) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=101)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--obs", type=int, default=50_000_000)
    ap.add_argument("--points", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--check-images", type=int, default=None)
    ap.add_argument("--e2e-runs", type=int, default=3, help="0: kernel and check only")
    ap.add_argument("--parent", default=None, help="particle-sfm_amd of a built checkout of the parent commit")
    ap.add_argument("--split-images", type=int, default=20)
    ap.add_argument("--tmp", default=None, help="directory for the model and output files (default: a temporary one)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--run-one", nargs=5, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.run_one:
        package, warm_model, model_dir, out_dir, kw = a.run_one
        print(json.dumps({"seconds": run_one(package, warm_model, model_dir, out_dir, json.loads(kw))}))
        return 0
    os.environ.setdefault("MPLBACKEND", "Agg")
    sys.path.insert(0, PACKAGE)
    sys.path.insert(0, HERE)

    import torch
    from point_trajectory import _hip
    from psfm_sfm import convert
    from sparse_depth import synthetic_model, write_model_bin

    assert torch.cuda.is_available(), "depth_display.py measures on the GPU"
    log = lambda msg: print(msg, file=sys.stderr, flush=True)
    t0 = time.perf_counter()
    m = synthetic_model(convert, a.images, a.width, a.height, a.obs, a.points)
    n_pix = a.images * a.width * a.height
    log("model: %d observations, %d points, %.1f s" % (len(m.point3D_ids), len(m.ids), time.perf_counter() - t0))
    ctx = _hip.context(0)
    out = {"workload": "%d images of %dx%d, %d observations, %d points" % (a.images, a.width, a.height, len(m.point3D_ids), len(m.ids)),
           "n_pixels": n_pix, "reps": a.reps, "source_hash": None}
    try:
        sys.path.insert(0, PACKAGE)
        import build as psfm_build
        out["source_hash"] = psfm_build.source_hash()
    except Exception:                                                      # noqa: BLE001 -- a stamp, not a measurement
        pass

    # ---- the four passes against a copy, alternated ----
    ctx.set_sparse_depth(0)
    batch = next(convert.sparse_depth_batches(m, ctx))
    ctx.set_sparse_depth()
    maps = [d for _, d in batch]
    n_valid = int(sum(int(torch.count_nonzero(d > 0)) for d in maps))
    out["n_valid"] = n_valid
    out["bytes"] = {"count": 8 * n_pix, "compact": 8 * n_pix + 8 * n_valid, "select": 8 * 8 * n_valid, "colour": 12 * n_pix}
    total = sum(out["bytes"].values())
    src = torch.zeros(total // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    ctx.set_depth_display(timing=True)
    spans = {k: [] for k in ("count_ms", "compact_ms", "select_ms", "colour_ms", "call_ms", "copy_ms")}
    res = None
    for r in range(a.warmup + a.reps):
        del res
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = convert.depth_display_device(maps, ctx=ctx)
        call_ms = (time.perf_counter() - t0) * 1e3
        ms = ctx.depth_display_ms()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)
        e1.record()
        e1.synchronize()
        if r >= a.warmup:
            for k in ("count_ms", "compact_ms", "select_ms", "colour_ms"):
                spans[k].append(ms[k])
            spans["call_ms"].append(call_ms)
            spans["copy_ms"].append(e0.elapsed_time(e1))
    ctx.set_depth_display()
    del src, dst
    for k, v in spans.items():
        v = np.array(v)
        out[k] = float(np.median(v))
        out[k + "_min_max"] = [float(v.min()), float(v.max())]
    out["passes_ms"] = out["count_ms"] + out["compact_ms"] + out["select_ms"] + out["colour_ms"]
    out["passes_over_copy"] = out["passes_ms"] / out["copy_ms"]
    out["GBps"] = {k: out["bytes"][k] / (out[k + "_ms"] * 1e-3) / 1e9 for k in out["bytes"]}
    log("kernel: count %.3f, compact %.3f, select %.3f, colour %.3f ms; call %.3f ms (host clock, with the allocation of the output); "
        "copy of the same bytes %.3f ms" % tuple(out[k] for k in ("count_ms", "compact_ms", "select_ms", "colour_ms", "call_ms", "copy_ms")))

    # ---- the device against the NumPy model ----
    t0 = time.perf_counter()
    k = a.images if a.check_images is None else min(a.images, a.check_images)
    equal = True
    for d, (rgba, z1, z2) in list(zip(maps, res))[:k]:
        want, w1, w2 = convert.depth_display_host(d.cpu().numpy())
        equal = equal and np.array_equal(rgba.cpu().numpy(), want) and np.array_equal(np.array([z1, z2]).view(np.uint64), np.array([w1, w2]).view(np.uint64))
    out["device_equals_model"], out["checked_images"] = bool(equal), k
    log("check: %d images, equal %s, %.1f s" % (k, equal, time.perf_counter() - t0))

    # ---- the device route's host side, once ----
    from matplotlib import pyplot as plt
    from PIL import Image
    tmp = a.tmp or tempfile.mkdtemp()
    os.makedirs(os.path.join(tmp, "split"), exist_ok=True)
    k = min(a.images, a.split_images)
    split = {"images": k}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host_rgba = [r[0].cpu().numpy() for r in res[:k]]
    split["rgba_to_host_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    host_maps = [d.cpu().numpy() for d in maps[:k]]
    split["maps_to_host_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    for i, d in enumerate(host_maps):
        np.save(os.path.join(tmp, "split", "%05d.npy" % i), d)
    split["np_save_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    for i, x in enumerate(host_rgba):
        plt.imsave(os.path.join(tmp, "split", "%05d.png" % i), x)
    split["imsave_rgba_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    for i, x in enumerate(host_rgba):
        Image.fromarray(x).save(os.path.join(tmp, "split", "pil_%05d.png" % i))
    split["pil_encode_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    for i, d in enumerate(host_maps[:max(1, k // 4)]):
        plt.imsave(os.path.join(tmp, "split", "host_%05d.png" % i), convert.normalize_depth_for_display(d))
    split["host_route_png_s_per_image"] = (time.perf_counter() - t0) / max(1, k // 4)
    out["host_split"] = split
    log("host split: %s" % json.dumps(split))
    shutil.rmtree(os.path.join(tmp, "split"), ignore_errors=True)
    del res, maps, batch, host_rgba, host_maps
    torch.cuda.empty_cache()

    # ---- end to end ----
    if a.e2e_runs > 0:
        model_dir = os.path.join(tmp, "model")
        write_model_bin(m, model_dir)
        warm_model = os.path.join(tmp, "warm_model")
        small = synthetic_model(convert, 2, 64, 48, 2000, 500)
        write_model_bin(small, warm_model)
        del m

        def one(label, package, **kw):
            out_dir = os.path.join(tmp, "out")
            shutil.rmtree(out_dir, ignore_errors=True)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--run-one", package, warm_model, model_dir, out_dir, json.dumps(kw)],
                               stdout=subprocess.PIPE, text=True, check=True)
            s = json.loads(r.stdout.strip().splitlines()[-1])["seconds"]
            n_png = len([n for n in os.listdir(os.path.join(out_dir, "depths")) if n.endswith(".png")])
            shutil.rmtree(out_dir, ignore_errors=True)
            log("end to end, %s: %.2f s (%d PNGs)" % (label, s, n_png))
            return s, n_png

        e2e = {"device": [], "parent": []}
        for _ in range(a.e2e_runs):
            e2e["device"].append(one("this commit, display=device", PACKAGE, display="device")[0])
            if a.parent:
                e2e["parent"].append(one("parent commit", a.parent)[0])
        out["e2e_device_s"] = stats(e2e["device"])
        if a.parent:
            out["e2e_parent_s"] = stats(e2e["parent"])
            spread = max(out["e2e_device_s"]["max"] - out["e2e_device_s"]["min"], out["e2e_parent_s"]["max"] - out["e2e_parent_s"]["min"])
            out["e2e_gain_s"] = out["e2e_parent_s"]["median"] - out["e2e_device_s"]["median"]
            out["e2e_larger_spread_s"] = spread
            out["device_beats_parent_by_3_spreads"] = bool(out["e2e_gain_s"] > 3 * spread)
        out["e2e_host_s"] = one("this commit, display=host", PACKAGE, display="host")[0]
        for w in (2, 4):
            out["e2e_device_writers_%d_s" % w] = one("this commit, display=device, writers=%d" % w, PACKAGE, display="device", writers=w)[0]
        s, n_png = one("this commit, png=False", PACKAGE, png=False)
        out["e2e_png_false_s"], out["png_false_pngs"] = s, n_png
    if not a.tmp:
        shutil.rmtree(tmp, ignore_errors=True)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fp:
            fp.write(line + "\n")
    return 0 if out["device_equals_model"] else 1


if __name__ == "__main__":
    sys.exit(main())
