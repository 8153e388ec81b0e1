#!/usr/bin/env python3
"""The sparse depth maps of a COLMAP model (csrc/psfm_sparse_depth.hip) at the headline size: the three passes against a
device-to-device copy of the same bytes, the device against the NumPy model, and model files -> output files end to end.

Workload: a seeded synthetic model -- --images images of --width x --height, --obs observations in all (30 % with id -1, spread evenly
over the images, uniform over the image), --points 3-D points with sparse ids below 2^32.

  kernel      one psfm_sparse_depth call over all images (budget 0) with the context's timing on: the zero fill (two memsets), the
              winner pass and the store pass, each between two HIP events; ALTERNATED with a torch copy_ between two device buffers
              of half the kernels' byte count (so that the copy reads + writes that count), --reps rounds after --warmup.
  check       every map of the device against psfm_sfm.convert.sparse_depth_host, bit for bit (--check-images limits it).
  end to end  wall clock, the model written to .bin files first (not timed): write_depth_pose_from_colmap_format of the package,
              split into parse / upload + sort / device / device-to-host / np.save / PNG / texts by a second, instrumented walk
              over the same steps; and the reference's algorithm restated (scripts/micro/sparse_depth_restated.py) on the first
              --restated-images images of the same files (all 3-D points: it has to read them all), scaled by images for the ratio.
Prints one JSON line (--out also writes it to a file)."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "particle-sfm_amd"))
sys.path.insert(0, HERE)


def synthetic_model(convert, n_img, w, h, n_obs, n_pts, seed=0):
    rng = np.random.default_rng(seed)
    ids = np.sort(rng.choice(2 ** 32, n_pts, replace=False)).astype(np.int64)
    rng.shuffle(ids)
    xyz = rng.uniform(-3, 3, (n_pts, 3))
    per = n_obs // n_img
    off = np.arange(n_img + 1, dtype=np.int64) * per
    n = int(off[-1])
    xys = np.empty((n, 2))
    xys[:, 0] = rng.uniform(-0.5, w - 0.5, n)
    xys[:, 1] = rng.uniform(-0.5, h - 0.5, n)
    p3d = ids[rng.integers(0, n_pts, n)]
    p3d[rng.random(n) < 0.3] = -1
    images = []
    for i in range(n_img):
        q = rng.normal(size=4)
        images.append(convert.ImageHeader(i + 1, q / np.linalg.norm(q), np.array([0.1, -0.2, rng.uniform(10, 14)]), 1, "%05d.png" % i))
    cams = {1: convert.Camera(1, "SIMPLE_RADIAL", w, h, np.array([1.2 * w, w / 2, h / 2, 0.01]))}
    return convert.ModelArrays(cams, images, off, xys, p3d, ids, xyz)


def write_model_bin(m, path):
    """The three .bin files of the model (every 3-D point with an empty track)."""
    import struct
    os.makedirs(path, exist_ok=True)
    from psfm_sfm.convert import CAMERA_MODELS
    names = {v[0]: k for k, v in CAMERA_MODELS.items()}
    with open(os.path.join(path, "cameras.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(m.cameras)))
        for c in m.cameras.values():
            f.write(struct.pack("<iiQQ", c.id, names[c.model], c.width, c.height) + np.asarray(c.params, "<f8").tobytes())
    with open(os.path.join(path, "images.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(m.images)))
        for i, im in enumerate(m.images):
            a, b = int(m.obs_off[i]), int(m.obs_off[i + 1])
            f.write(struct.pack("<idddddddi", im.id, *im.qvec, *im.tvec, im.camera_id) + im.name.encode() + b"\x00" + struct.pack("<Q", b - a))
            rec = np.empty(b - a, np.dtype([("x", "<f8"), ("y", "<f8"), ("id", "<i8")]))
            rec["x"], rec["y"], rec["id"] = m.xys[a:b, 0], m.xys[a:b, 1], m.point3D_ids[a:b]
            rec.tofile(f)
    rec = np.zeros(len(m.ids), np.dtype([("id", "<u8"), ("xyz", "<f8", 3), ("rgb", "u1", 3), ("err", "<f8"), ("len", "<u8")]))
    assert rec.dtype.itemsize == 51
    rec["id"], rec["xyz"] = m.ids.view(np.uint64), m.xyz
    with open(os.path.join(path, "points3D.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(m.ids)))
        rec.tofile(f)


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
    ap.add_argument("--e2e", type=int, default=1, help="0: kernel and check only")
    ap.add_argument("--restated-images", type=int, default=None, help="default: a tenth of the images")
    ap.add_argument("--tmp", default=None, help="directory for the model and output files (default: a temporary one)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    os.environ.setdefault("MPLBACKEND", "Agg")

    import torch
    from point_trajectory import _hip
    from psfm_sfm import convert
    import sparse_depth_restated as restated

    assert torch.cuda.is_available(), "sparse_depth.py measures on the GPU"
    log = lambda msg: print(msg, file=sys.stderr, flush=True)
    t0 = time.perf_counter()
    m = synthetic_model(convert, a.images, a.width, a.height, a.obs, a.points)
    n_obs, n_pix = len(m.point3D_ids), a.images * a.width * a.height
    n_valid = int(np.count_nonzero(m.point3D_ids != -1))
    log("model: %d observations (%d counted), %d points, %.1f s" % (n_obs, n_valid, len(m.ids), time.perf_counter() - t0))
    ctx = _hip.context(0)
    out = {"workload": "%d images of %dx%d, %d observations (%d with a point), %d points" % (a.images, a.width, a.height, n_obs, n_valid, len(m.ids)),
           "n_obs": n_obs, "n_valid": n_valid, "n_points": len(m.ids), "n_pixels": n_pix, "reps": a.reps}

    # ---- the three passes against a copy, alternated ----
    ctx.set_sparse_depth(0, timing=True)
    maps = None
    spans = {"fill_ms": [], "winner_ms": [], "store_ms": [], "copy_ms": []}
    n_win = None
    src = dst = None
    for r in range(a.warmup + a.reps):
        maps = list(convert.sparse_depth_device(m, ctx))                  # one batch: every map is a view of one buffer
        ms = ctx.sparse_depth_ms()
        if n_win is None:
            n_win = int(sum(int(torch.count_nonzero(d)) for _, d in maps))
            # fill 12 B/pixel; winner 24 B read + 4 B written per observation + a 4-byte atomic per counted one; store 20 B read per
            # observation, 4 B winner read per counted one, 24 B gathered + 8 B written per winner
            out["bytes"] = {"fill": 12 * n_pix, "winner": 28 * n_obs + 4 * n_valid, "store": 20 * n_obs + 4 * n_valid + 32 * n_win}
            total = sum(out["bytes"].values())
            src = torch.zeros(total // 2, dtype=torch.uint8, device="cuda")
            dst = torch.empty_like(src)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)
        e1.record()
        e1.synchronize()
        if r >= a.warmup:
            for k in ("fill_ms", "winner_ms", "store_ms"):
                spans[k].append(ms[k])
            spans["copy_ms"].append(e0.elapsed_time(e1))
        if r + 1 < a.warmup + a.reps:
            del maps
    del src, dst
    out["n_winners"] = n_win
    for k, v in spans.items():
        v = np.array(v)
        out[k] = float(np.median(v))
        out[k + "_min_max"] = [float(v.min()), float(v.max())]
    out["passes_ms"] = out["fill_ms"] + out["winner_ms"] + out["store_ms"]
    out["passes_over_copy"] = out["passes_ms"] / out["copy_ms"]
    log("kernel: fill %.3f, winner %.3f, store %.3f ms; copy of the same bytes %.3f ms" % (out["fill_ms"], out["winner_ms"], out["store_ms"], out["copy_ms"]))

    # ---- the device against the NumPy model ----
    t0 = time.perf_counter()
    k = a.images if a.check_images is None else min(a.images, a.check_images)
    sub = m._replace(images=m.images[:k], obs_off=m.obs_off[:k + 1])
    equal = True
    for (name, want), (_, got) in zip(convert.sparse_depth_host(sub), maps):
        g = got.cpu().numpy()
        equal = equal and np.array_equal(g.view(np.uint64), want.view(np.uint64))
    out["device_equals_model"], out["checked_images"] = bool(equal), k
    log("check: %d images, equal %s, %.1f s" % (k, equal, time.perf_counter() - t0))
    del maps
    torch.cuda.empty_cache()
    ctx.set_sparse_depth()

    # ---- end to end ----
    if a.e2e:
        tmp = a.tmp or tempfile.mkdtemp()
        model_dir = os.path.join(tmp, "model")
        write_model_bin(m, model_dir)
        del m
        t0 = time.perf_counter()
        convert.write_depth_pose_from_colmap_format(model_dir, os.path.join(tmp, "new"))
        out["e2e_new_s"] = time.perf_counter() - t0
        log("end to end, package: %.1f s" % out["e2e_new_s"])
        # the same steps once more, one after the other, each timed (no overlap: the parts add up to more than the run above)
        split = {}
        t0 = time.perf_counter()
        m2 = convert.read_model_arrays(model_dir)
        split["parse_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        host_maps = []
        gen = convert.sparse_depth_device(m2, ctx)
        first = next(gen)                                                 # upload, sort and the first batch
        torch.cuda.synchronize()
        split["upload_sort_first_batch_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        dev_maps = [first] + list(gen)
        torch.cuda.synchronize()
        split["other_batches_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        host_maps = [(n, d.cpu().numpy()) for n, d in dev_maps]
        split["device_to_host_s"] = time.perf_counter() - t0
        del dev_maps
        os.makedirs(os.path.join(tmp, "split"), exist_ok=True)
        t0 = time.perf_counter()
        for n, d in host_maps:
            np.save(os.path.join(tmp, "split", os.path.splitext(n)[0] + ".npy"), d)
        split["np_save_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        from matplotlib import pyplot as plt
        for n, d in host_maps:
            plt.imsave(os.path.join(tmp, "split", os.path.splitext(n)[0] + ".png"), convert.normalize_depth_for_display(d))
        split["png_s"] = time.perf_counter() - t0
        out["e2e_split"] = split
        log("split: %s" % json.dumps(split))
        k = a.restated_images or max(1, a.images // 10)
        t0 = time.perf_counter()
        restated.convert(model_dir, os.path.join(tmp, "old"), limit=k)
        out["e2e_restated_s"], out["restated_images"] = time.perf_counter() - t0, k
        out["e2e_restated_scaled_s"] = out["e2e_restated_s"] * a.images / k
        out["restated_over_new"] = out["e2e_restated_scaled_s"] / out["e2e_new_s"]
        same = all(np.array_equal(np.load(os.path.join(tmp, "old", "depths", "%05d.npy" % i)) != 0, np.load(os.path.join(tmp, "new", "depths", "%05d.npy" % i)) != 0)
                   and np.allclose(np.load(os.path.join(tmp, "old", "depths", "%05d.npy" % i)), np.load(os.path.join(tmp, "new", "depths", "%05d.npy" % i)), rtol=0, atol=1e-13)
                   for i in range(k))
        out["restated_agrees"] = bool(same)
        log("end to end, restated on %d images: %.1f s (agrees: %s)" % (k, out["e2e_restated_s"], same))
        if not a.tmp:
            shutil.rmtree(tmp, ignore_errors=True)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fp:
            fp.write(line + "\n")
    return 0 if out["device_equals_model"] and out.get("restated_agrees", True) else 1


if __name__ == "__main__":
    sys.exit(main())
