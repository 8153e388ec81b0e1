#!/usr/bin/env python3
"""Golden vectors for the sparse depth maps, poses and intrinsics of a COLMAP model (sfm/convert.py:43-104), produced by the
REFERENCE's own functions: sfm/convert.py and sfm/colmap_utils/read_write_model.py are imported UNMODIFIED from the reference checkout
(root: oracle/ref_shim.py), the synthetic models are written by the reference's write_model and converted by its
write_depth_pose_from_colmap_format, with MPLBACKEND=Agg.  Only a `tqdm` stand-in is installed when the real one is missing.

Per case a directory tests/golden/sparse_depth_<case>/ with the three .bin files and expected.npz: the arrays the model was built
from, the reference's .npy maps, its pose and intrinsics texts; case a also keeps one PNG.  Data only.

The reference stops at an image whose map is all zero (its percentile for the display PNG has nothing to work on) -- after that
image's .npy is written, before its pose.  Such images (case d) are therefore converted one model per image, the failure is recorded
(`png_failed`), and their pose text is np.savetxt of the reference's own qvec2rotmat, as the reference would have written it.
Run in the build container, never on the GPU machine:
    python tests/golden/make_sparse_depth_golden.py
"""
import importlib
import os
import shutil
import sys
import tempfile
import types

os.environ["MPLBACKEND"] = "Agg"

import numpy as np      # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import ref_shim          # noqa: E402

MAX_BYTES = 600000
W, H = 37, 23


def load_reference():
    if "tqdm" not in sys.modules:
        try:
            importlib.import_module("tqdm")
        except ImportError:
            m = types.ModuleType("tqdm")
            m.tqdm = lambda it, *a, **k: it
            sys.modules["tqdm"] = m
    sfm = os.path.join(ref_shim.REFERENCE_ROOT, "sfm")
    if not os.path.isdir(sfm):
        raise RuntimeError("reference tree not present at %s" % ref_shim.REFERENCE_ROOT)
    sys.path.insert(0, sfm)
    convert = importlib.import_module("convert")
    rwm = importlib.import_module("colmap_utils.read_write_model")
    return convert, rwm


def pose(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    return q, np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(10, 14)])


def make_points(rwm, rng, ids):
    pts = {}
    for i in ids:
        n = int(rng.integers(0, 6))                                       # variable-length records
        pts[int(i)] = rwm.Point3D(id=int(i), xyz=rng.uniform(-3, 3, 3), rgb=rng.integers(0, 256, 3), error=float(rng.uniform(0, 2)),
                                  image_ids=rng.integers(1, 5, n), point2D_idxs=rng.integers(0, 3000, n))
    return pts


def make_image(rwm, rng, image_id, camera_id, name, xys, p3d):
    q, t = pose(rng)
    return rwm.Image(id=image_id, qvec=q, tvec=t, camera_id=camera_id, name=name, xys=np.asarray(xys, np.float64).reshape(-1, 2),
                     point3D_ids=np.asarray(p3d, np.int64))


def cameras_two(rwm):
    return {1: rwm.Camera(id=1, model="SIMPLE_PINHOLE", width=W, height=H, params=np.array([30.0, 18.5, 11.5])),
            2: rwm.Camera(id=2, model="SIMPLE_RADIAL", width=5, height=4, params=np.array([6.0, 2.5, 2.0, 0.01]))}


def case_a(rwm):
    """3 images x 3 000 observations of 37 x 23 px, 30 % -1, 500 points with ids up to 2^20; a fourth image on a 5 x 4 camera."""
    rng = np.random.default_rng(7100)
    ids = np.sort(rng.choice(2 ** 20, 500, replace=False) + 1)
    ids[-1] = 2 ** 20
    rng.shuffle(ids)                                                      # file order is not id order
    pts = make_points(rwm, rng, ids)
    images = {}
    for k in range(3):
        xys = np.stack([rng.uniform(-2, W + 2, 3000), rng.uniform(-2, H + 2, 3000)], 1)
        p3d = np.where(rng.random(3000) < 0.3, -1, rng.choice(ids, 3000))
        images[k + 1] = make_image(rwm, rng, k + 1, 1, "%05d.png" % k, xys, p3d)
    xys = np.stack([rng.uniform(-1, 6, 200), rng.uniform(-1, 5, 200)], 1)
    images[9] = make_image(rwm, rng, 9, 2, "small.jpg", xys, np.where(rng.random(200) < 0.3, -1, rng.choice(ids, 200)))
    return cameras_two(rwm), images, pts


def case_b(rwm):
    """3 000 valid observations of one image that all round into three pixels."""
    rng = np.random.default_rng(7200)
    ids = rng.permutation(400) + 1
    pts = make_points(rwm, rng, ids)
    centres = np.array([[5.0, 7.0], [6.0, 7.0], [36.0, 22.0]])
    xys = centres[rng.integers(0, 3, 3000)] + rng.uniform(-0.4, 0.4, (3000, 2))
    images = {1: make_image(rwm, rng, 1, 1, "b.png", xys, rng.choice(ids, 3000))}
    return cameras_two(rwm), images, pts


def case_c(rwm):
    """Coordinates exactly on .5 on both parities, negative, at w - 0.5, beyond the far edge, at the ends of the int32 range."""
    rng = np.random.default_rng(7300)
    ids = rng.permutation(300) + 1
    pts = make_points(rwm, rng, ids)
    xs = [0.5, 1.5, 2.5, 3.5, 4.5, -0.5, -0.0, -1.5, -3.2, W - 0.5, W - 1.5, W - 1.0, float(W), W + 3.7, 1e6, -1e6, 2147483647.0,
          -2147483647.5, 0.49999999999999994, 1.5000000000000002, 2.4999999999999996]
    ys = [0.5, 1.5, 2.5, 3.5, -0.5, -2.5, H - 0.5, H - 1.5, float(H), H + 0.5, 1e9, -1e9, 10.5, 11.5]
    xys = np.array([(x, y) for x in xs for y in ys])
    images = {1: make_image(rwm, rng, 1, 1, "c.png", xys, rng.choice(ids, len(xys)))}
    return cameras_two(rwm), images, pts


def case_d(rwm):
    """An ordinary image, an image with only -1 ids, an image with zero points."""
    rng = np.random.default_rng(7400)
    ids = rng.permutation(100) + 1
    pts = make_points(rwm, rng, ids)
    xy = lambda n: np.stack([rng.uniform(0, W, n), rng.uniform(0, H, n)], 1)
    images = {1: make_image(rwm, rng, 1, 1, "d0.png", xy(50), rng.choice(ids, 50)),
              2: make_image(rwm, rng, 2, 1, "d1.png", xy(40), np.full(40, -1)),
              3: make_image(rwm, rng, 3, 2, "d2.png", np.zeros((0, 2)), np.zeros(0, np.int64)),
              4: make_image(rwm, rng, 4, 1, "d3.png", xy(30), rng.choice(ids, 30))}
    return cameras_two(rwm), images, pts


def case_e(rwm):
    """Sparse ids above 2^32 and near 2^62."""
    rng = np.random.default_rng(7500)
    ids = np.concatenate([rng.integers(1, 2 ** 20, 40), 2 ** 32 + rng.integers(0, 2 ** 40, 40), 2 ** 62 - rng.integers(0, 1000, 40),
                          [2 ** 32, 2 ** 32 - 1, 2 ** 62, 2 ** 63 - 1]])
    ids = rng.permutation(np.unique(ids))
    pts = make_points(rwm, rng, ids)
    xys = np.stack([rng.uniform(0, W, 600), rng.uniform(0, H, 600)], 1)
    p3d = np.where(rng.random(600) < 0.2, -1, rng.choice(ids, 600))
    images = {1: make_image(rwm, rng, 1, 1, "e.png", xys, p3d)}
    return cameras_two(rwm), images, pts


def case_f(rwm):
    """One observation names a point the model does not hold."""
    rng = np.random.default_rng(7600)
    ids = rng.permutation(60) * 3 + 5
    pts = make_points(rwm, rng, ids)
    xys = np.stack([rng.uniform(0, W, 80), rng.uniform(0, H, 80)], 1)
    p3d = rng.choice(ids, 80)
    p3d[41] = 4242                                                        # 4242 % 3 == 0: not an id of the model
    images = {1: make_image(rwm, rng, 1, 1, "f.png", xys, p3d)}
    return cameras_two(rwm), images, pts


def stem(name):
    return os.path.splitext(name)[0]


def run_case(convert, rwm, case, cameras, images, pts, keep_png=None, expect_key_error=None):
    out_dir = os.path.join(HERE, "sparse_depth_" + case)
    shutil.rmtree(out_dir, ignore_errors=True)
    os.makedirs(out_dir)
    rwm.write_model(cameras, images, pts, out_dir, ext=".bin")
    exp = dict(
        image_ids=np.array([im.id for im in images.values()], np.int64), names=np.array([im.name for im in images.values()]),
        qvecs=np.stack([im.qvec for im in images.values()]), tvecs=np.stack([im.tvec for im in images.values()]),
        camera_ids=np.array([im.camera_id for im in images.values()], np.int64),
        obs_off=np.concatenate([[0], np.cumsum([len(im.point3D_ids) for im in images.values()])]).astype(np.int64),
        xys=np.concatenate([im.xys for im in images.values()]), point3D_ids=np.concatenate([im.point3D_ids for im in images.values()]),
        ids=np.array(list(pts), np.uint64), xyz=np.stack([p.xyz for p in pts.values()]),
        errors=np.array([p.error for p in pts.values()]), track_len=np.array([len(p.image_ids) for p in pts.values()], np.uint64),
        cam_ids=np.array(list(cameras), np.int64), cam_models=np.array([c.model for c in cameras.values()]),
        cam_wh=np.array([[c.width, c.height] for c in cameras.values()], np.int64),
        cam_params=np.concatenate([c.params for c in cameras.values()]),
        cam_nparams=np.array([len(c.params) for c in cameras.values()], np.int64))
    png_failed = []
    with tempfile.TemporaryDirectory() as tmp:
        if expect_key_error is not None:
            try:
                convert.write_depth_pose_from_colmap_format(out_dir, tmp)
                raise AssertionError("the reference did not fail")
            except KeyError as e:
                assert e.args == (expect_key_error,), e.args
            exp["missing_id"] = np.int64(expect_key_error)
        else:
            try:
                convert.write_depth_pose_from_colmap_format(out_dir, tmp)
            except Exception:
                # an all-zero map stopped the reference: one model per image (read back from the .bin files, the reference's reader)
                cams, ims, p3 = rwm.read_model(out_dir)
                for key, im in ims.items():
                    try:
                        convert.save_depth_pose(tmp, cams, {key: im}, p3)
                    except Exception:
                        png_failed.append(im.name)
                        assert os.path.exists(os.path.join(tmp, "depths", stem(im.name) + ".npy"))
                        np.savetxt(os.path.join(tmp, "poses", stem(im.name) + ".txt"),
                                   np.concatenate([rwm.qvec2rotmat(im.qvec), np.expand_dims(im.tvec, -1)], -1))
            for k, im in enumerate(images.values()):
                exp["depth_%d" % k] = np.load(os.path.join(tmp, "depths", stem(im.name) + ".npy"))
                exp["pose_%d" % k] = np.array(open(os.path.join(tmp, "poses", stem(im.name) + ".txt")).read())
                exp["intr_%d" % k] = np.array(open(os.path.join(tmp, "intrinsics", stem(im.name) + ".txt")).read())
                assert os.path.exists(os.path.join(tmp, "depths", stem(im.name) + ".png")) == (im.name not in png_failed)
            if keep_png:
                shutil.copy(os.path.join(tmp, "depths", stem(keep_png) + ".png"), os.path.join(out_dir, "expected_" + stem(keep_png) + ".png"))
    exp["png_failed"] = np.array(png_failed, dtype="U16")
    np.savez_compressed(os.path.join(out_dir, "expected.npz"), **exp)
    sizes = {f: os.path.getsize(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}
    assert all(s < MAX_BYTES for s in sizes.values()), sizes
    print("sparse_depth_%s: %d images, %d observations, %d points, %s" % (case, len(images), int(exp["obs_off"][-1]), len(pts), sizes))
    return exp


def main():
    convert, rwm = load_reference()
    a = run_case(convert, rwm, "a", *case_a(rwm), keep_png="00000.png")
    assert 0.25 < np.mean(a["point3D_ids"] == -1) < 0.35 and int(a["ids"].max()) == 2 ** 20
    b = run_case(convert, rwm, "b", *case_b(rwm))
    assert np.count_nonzero(b["depth_0"]) == 3
    c = run_case(convert, rwm, "c", *case_c(rwm))
    assert c["depth_0"][0, 0] != 0 and c["depth_0"][H - 1, W - 1] != 0
    d = run_case(convert, rwm, "d", *case_d(rwm))
    assert sorted(d["png_failed"].tolist()) == ["d1.png", "d2.png"] and not d["depth_1"].any() and not d["depth_2"].any()
    assert d["depth_2"].shape == (4, 5) and d["depth_3"].any()
    e = run_case(convert, rwm, "e", *case_e(rwm))
    assert int(e["ids"].max()) == 2 ** 63 - 1 and np.count_nonzero(e["ids"] >= 2 ** 32) > 40
    run_case(convert, rwm, "f", *case_f(rwm), expect_key_error=4242)


if __name__ == "__main__":
    main()
