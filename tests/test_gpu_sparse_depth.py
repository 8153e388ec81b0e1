"""psfm_sparse_depth / psfm_sparse_depth_sort_ids (csrc/psfm_sparse_depth.hip) on the device: against the reference's own maps
(tests/golden/sparse_depth_*/, acceptance in tests/_sparse_depth_np.py) and bit for bit against the NumPy model
psfm_sfm.convert.sparse_depth_host, which tests/test_sparse_depth_host.py pins to the same fixtures.  Reads only tests/golden/."""
import ctypes
import os

import numpy as np
import pytest

from _sparse_depth_np import CASES, assert_map_accepts, case_dir, fixture

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pt():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from point_trajectory import _hip
    from psfm_sfm import convert
    class NS: pass
    ns = NS()
    ns.hip, ns.convert, ns.torch = _hip, convert, torch
    ns.ctx = _hip.context()
    ns.models = {c: convert.read_model_arrays(case_dir(c)) for c in CASES + ["f"]}
    ns.host = {c: [d for _, d in convert.sparse_depth_host(ns.models[c])] for c in CASES}        # computed once, shared, never written
    yield ns
    ns.ctx.set_sparse_depth()                                             # (the default budget, no timing)


def device_maps(pt, model, sort="auto", budget=None):
    if budget is not None:
        pt.ctx.set_sparse_depth(budget)
    out = [(n, d.cpu().numpy()) for n, d in pt.convert.sparse_depth_device(model, pt.ctx, sort=sort)]
    assert [n for n, _ in out] == [im.name for im in model.images]
    return [d for _, d in out]


def bit_equal(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("case", CASES)
def test_device_accepts_reference_fixture_and_equals_model(pt, case):
    f = fixture(case)
    got = device_maps(pt, pt.models[case])
    for i, d in enumerate(got):
        assert_map_accepts(d, f, i)
        assert bit_equal(d, pt.host[case][i])


@pytest.mark.parametrize("case", ["a", "b", "c", "d"])
def test_both_sort_routes_give_identical_bytes(pt, case):
    dev, host = device_maps(pt, pt.models[case], sort="device"), device_maps(pt, pt.models[case], sort="host")
    for x, y, z in zip(dev, host, pt.host[case]):
        assert bit_equal(x, y) and bit_equal(x, z)


def test_large_ids_take_the_host_sort(pt):
    m = pt.models["e"]
    assert int(m.ids.max()) == 2 ** 63 - 1
    with pytest.raises(ValueError):
        device_maps(pt, m, sort="device")
    ids = pt.torch.from_numpy(m.ids.copy()).cuda()
    srt, row = pt.torch.empty_like(ids), pt.torch.empty(len(ids), dtype=pt.torch.int32, device="cuda")
    st = pt.hip.lib().psfm_sparse_depth_sort_ids(pt.ctx.handle, pt.hip.ptr(ids), len(ids), pt.hip.ptr(srt), pt.hip.ptr(row),
                                                 pt.hip.current_stream_ptr(pt.ctx.device))
    assert st == pt.hip.PSFM_ERR_ARG and b"2^32" in pt.hip.lib().psfm_last_error()
    for x, z in zip(device_maps(pt, m, sort="host"), pt.host["e"]):      # the context stays usable
        assert bit_equal(x, z)


def test_device_sort_is_the_stable_argsort(pt):
    rng = np.random.default_rng(11)
    for n in (1, 2, 4095, 4096, 4097, 70001):
        ids = rng.integers(0, 2 ** 32, n).astype(np.int64)
        ids[rng.integers(0, n, n // 3)] = ids[rng.integers(0, n, n // 3)]       # equal ids: file order must survive
        if n > 2:
            ids[:2] = [2 ** 32 - 1, 0]
        srt, row = pt.convert.sort_ids_device(pt.ctx, pt.torch.from_numpy(ids).cuda())
        order = np.argsort(ids, kind="stable")
        assert np.array_equal(srt.cpu().numpy(), ids[order]) and np.array_equal(row.cpu().numpy(), order.astype(np.int32))


def test_budget_of_one_image_equals_all_images(pt):
    m = pt.models["a"]
    desc = pt.convert.image_descriptors(m)
    assert pt.convert.batches(desc, 1) == [(i, i + 1) for i in range(4)] and pt.convert.batches(desc, 0) == [(0, 4)]
    one, every = device_maps(pt, m, budget=1), device_maps(pt, m, budget=0)
    two = device_maps(pt, m, budget=2 * 12 * 37 * 23)                     # two images of the first camera per call
    for x, y, z, w in zip(one, every, two, pt.host["a"]):
        assert bit_equal(x, y) and bit_equal(x, z) and bit_equal(x, w)
    pt.ctx.set_sparse_depth()


def test_two_calls_give_identical_bytes(pt):
    for case in ("a", "b"):
        x, y = device_maps(pt, pt.models[case]), device_maps(pt, pt.models[case])
        assert all(bit_equal(p, q) for p, q in zip(x, y))


def random_model(pt, seed, n_img, w, h, n_obs, n_pts, id_hi):
    rng = np.random.default_rng(seed)
    c = pt.convert
    ids = rng.choice(id_hi, n_pts, replace=False).astype(np.int64)
    cams = {1: c.Camera(1, "SIMPLE_PINHOLE", w, h, np.array([float(w), w / 2, h / 2])),
            2: c.Camera(2, "SIMPLE_RADIAL", w // 2 + 1, h // 3 + 1, np.array([float(w), w / 4, h / 6, 0.0]))}
    images, off = [], [0]
    for i in range(n_img):
        q = rng.normal(size=4)
        images.append(c.ImageHeader(i + 1, q / np.linalg.norm(q), np.array([0.1, -0.2, rng.uniform(8, 12)]), 2 if i % 3 == 2 else 1, "%03d.png" % i))
        off.append(off[-1] + int(n_obs * rng.uniform(0.3, 1.0)))
    n = off[-1]
    xys = np.stack([rng.uniform(-3, w + 3, n), rng.uniform(-3, h + 3, n)], 1)
    tie = rng.random(n) < 0.05
    xys[tie] = rng.integers(0, min(w, h) // 2, (int(tie.sum()), 2)) + 0.5        # exactly between two pixels
    p3d = np.where(rng.random(n) < 0.3, -1, rng.choice(ids, n))
    return c.ModelArrays(cams, images, np.array(off, np.int64), xys, p3d, ids, rng.uniform(-3, 3, (n_pts, 3)))


def test_many_blocks_two_cameras_equal_the_model(pt):
    """5 images of up to 40 000 observations (40 blocks each) on two camera sizes, 20 000 points (5 sort tiles), sparse ids."""
    m = random_model(pt, 21, 5, 200, 150, 40000, 20000, 2 ** 32)
    want = [d for _, d in pt.convert.sparse_depth_host(m)]
    assert sum(int(np.count_nonzero(d)) for d in want) > 30000 and int(np.diff(m.obs_off).max()) > 16 * 1024
    for sort in ("device", "host"):
        for x, z in zip(device_maps(pt, m, sort=sort, budget=0), want):
            assert bit_equal(x, z)
    for x, z in zip(device_maps(pt, m, budget=12 * 200 * 150 + 1), want):
        assert bit_equal(x, z)
    pt.ctx.set_sparse_depth()


def test_equal_ids_resolve_to_the_last_point_in_file_order(pt):
    m = pt.models["d"]
    ids = m.ids.copy()
    ids[20] = ids[3]
    xyz = m.xyz.copy()
    xyz[3] = 1e6                                                           # shadowed by row 20: never used
    m2 = m._replace(ids=ids, point3D_ids=np.where(m.point3D_ids == m.ids[20], -1, m.point3D_ids), xyz=xyz)
    want = [d for _, d in pt.convert.sparse_depth_host(m2)]
    assert max(float(np.abs(d).max()) for d in want) < 1e3
    for sort in ("device", "host"):
        for x, z in zip(device_maps(pt, m2, sort=sort), want):
            assert bit_equal(x, z)


def test_missing_id_raises_key_error_and_the_context_stays_usable(pt):
    for sort in ("device", "host"):
        with pytest.raises(KeyError) as e:
            device_maps(pt, pt.models["f"], sort=sort)
        assert e.value.args == (4242,)
        assert b"4242" in pt.hip.lib().psfm_last_error()
    m = pt.models["f"]
    p3d = m.point3D_ids.copy()
    p3d[7], p3d[60] = 9000, -5                                            # the smallest missing id is reported, as a signed number
    with pytest.raises(KeyError) as e:
        device_maps(pt, m._replace(point3D_ids=p3d))
    assert e.value.args == (-5,)
    for x, z in zip(device_maps(pt, pt.models["d"]), pt.host["d"]):
        assert bit_equal(x, z)


def test_coordinates_outside_the_domain_are_refused(pt):
    m = pt.models["d"]
    for bad in (np.nan, np.inf, 2.0 ** 31, -2.0 ** 31, 2147483647.5):
        xys = m.xys.copy()
        xys[3, 1] = bad
        with pytest.raises(pt.hip.PsfmError) as e:
            device_maps(pt, m._replace(xys=xys))
        assert e.value.status == pt.hip.PSFM_ERR_ARG and "observation 3 " in str(e.value)
    xys = m.xys.copy()
    xys[int(m.obs_off[1]) + 2, 0] = np.nan                                 # id -1: never rounded
    xys[3, 0], xys[4, 1] = 2147483647.0, -2147483647.5
    m2 = m._replace(xys=xys)
    for x, (_, z) in zip(device_maps(pt, m2), pt.convert.sparse_depth_host(m2)):
        assert bit_equal(x, z)


def test_bad_descriptors_are_refused_before_any_launch(pt):
    m = pt.models["d"]
    c, T = pt.convert, pt.torch
    desc = c.image_descriptors(m)
    order = np.argsort(m.ids, kind="stable")
    srt, row = T.from_numpy(m.ids[order]).cuda(), T.from_numpy(order.astype(np.int32)).cuda()
    xyz, xys, ids = T.from_numpy(m.xyz).cuda(), T.from_numpy(m.xys).cuda(), T.from_numpy(m.point3D_ids).cuda()
    out = T.full((int((desc["w"].astype(np.int64) * desc["h"]).sum()),), 5.0, dtype=T.float64, device="cuda")

    def call(d, n_obs=len(m.xys), n_img=None):
        d = np.ascontiguousarray(d)
        return pt.hip.lib().psfm_sparse_depth(pt.ctx.handle, pt.hip.ptr(xys), pt.hip.ptr(ids), n_obs, d.ctypes.data_as(ctypes.c_void_p),
                                              len(d) if n_img is None else n_img, pt.hip.ptr(srt), pt.hip.ptr(row), pt.hip.ptr(xyz), len(m.ids),
                                              pt.hip.ptr(out), None, pt.hip.current_stream_ptr(pt.ctx.device))

    def changed(**kw):
        d = desc.copy()
        for k, (i, v) in kw.items():
            d[k][i] = v
        return d
    for d in (changed(obs_end=(0, len(m.xys) + 1)), changed(obs_begin=(0, -1)), changed(obs_begin=(1, int(desc["obs_end"][1]) + 1)),
              changed(w=(2, 0)), changed(h=(0, -3)), changed(out_off=(1, int(desc["out_off"][1]) + 1)), changed(out_off=(0, 8)),
              changed(out_off=(2, int(desc["out_off"][1]))), changed(t2=(3, np.nan))):
        assert call(d) == pt.hip.PSFM_ERR_ARG
        assert bool((out == 5.0).all())                                   # nothing ran
    assert call(desc, n_obs=len(m.xys) - 1) == pt.hip.PSFM_ERR_ARG and call(desc, n_img=0) == pt.hip.PSFM_ERR_ARG
    assert call(desc) == pt.hip.PSFM_OK
    got = out.cpu().numpy()
    for d, z in zip(desc, pt.host["d"]):
        assert bit_equal(got[int(d["out_off"]):int(d["out_off"]) + z.size].reshape(z.shape), z)


def test_write_depth_pose_from_colmap_format_end_to_end(pt, tmp_path):
    os.environ.setdefault("MPLBACKEND", "Agg")
    from matplotlib import pyplot as plt
    for case in ("a", "d"):
        f = fixture(case)
        out = tmp_path / case
        pt.convert.write_depth_pose_from_colmap_format(case_dir(case), str(out))
        for i, name in enumerate(f["names"].tolist()):
            stem = os.path.splitext(name)[0]
            d = np.load(str(out / "depths" / (stem + ".npy")))
            assert_map_accepts(d, f, i)
            assert bit_equal(d, pt.host[case][i])
            assert open(str(out / "poses" / (stem + ".txt"))).read() == str(f["pose_%d" % i])
            assert open(str(out / "intrinsics" / (stem + ".txt"))).read() == str(f["intr_%d" % i])
            assert os.path.exists(str(out / "depths" / (stem + ".png"))) == (name not in f["png_failed"].tolist())
    got, want = plt.imread(str(tmp_path / "a" / "depths" / "00000.png")), plt.imread(os.path.join(case_dir("a"), "expected_00000.png"))
    assert got.shape == want.shape and np.max(np.abs(np.round(got * 255) - np.round(want * 255))) <= 1


def test_timing_reports_three_spans(pt):
    pt.ctx.set_sparse_depth(0, timing=True)
    device_maps(pt, pt.models["a"])
    ms = pt.ctx.sparse_depth_ms()
    assert set(ms) == {"fill_ms", "winner_ms", "store_ms"} and all(0 < v < 1000 for v in ms.values())
    pt.ctx.set_sparse_depth()
