"""COLMAP models whose point3D ids do not fit 32 bits, sorted on the device: psfm_sfm.convert.sort_ids_device64 (psfm_sort_records64
over the bit length of the largest id) and sparse_depth_device(sort="device64"), against the host route (np.argsort), the NumPy model
and the committed fixture of model "e" (ids up to 2^63 - 1).  Reads only tests/golden/."""
import numpy as np
import pytest

from _sparse_depth_np import assert_map_accepts, case_dir, fixture

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
    ns.model = convert.read_model_arrays(case_dir("e"))
    ns.host = [d for _, d in convert.sparse_depth_host(ns.model)]        # computed once, shared, never written
    yield ns
    ns.ctx.set_sparse_depth()


def device_maps(pt, sort):
    out = [(n, d.cpu().numpy()) for n, d in pt.convert.sparse_depth_device(pt.model, pt.ctx, sort=sort)]
    assert [n for n, _ in out] == [im.name for im in pt.model.images]
    return [d for _, d in out]


def bit_equal(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_large_ids_through_the_device_sort(pt):
    assert int(pt.model.ids.max()) == 2 ** 63 - 1
    f = fixture("e")
    dev, host = device_maps(pt, "device64"), device_maps(pt, "host")
    assert len(dev) == len(host) == len(pt.host) > 0
    for i, (x, y, z) in enumerate(zip(dev, host, pt.host)):
        assert bit_equal(x, y) and bit_equal(x, z)
        assert_map_accepts(x, f, i)


def test_device64_sort_is_the_stable_argsort(pt):
    rng = np.random.default_rng(12)
    for n in (1, 2, 4095, 4096, 4097, 70001):
        ids = np.where(rng.random(n) < 0.5, rng.integers(0, 2 ** 32, n), rng.integers(2 ** 32, 2 ** 63, n)).astype(np.int64)
        ids[rng.integers(0, n, n // 3)] = ids[rng.integers(0, n, n // 3)]       # equal ids: file order must survive
        if n > 4:
            ids[:4] = [2 ** 63 - 1, 0, 2 ** 32, 2 ** 32 - 1]
        srt, row = pt.convert.sort_ids_device64(pt.ctx, pt.torch.from_numpy(ids).cuda())
        order = np.argsort(ids, kind="stable")
        assert srt.dtype == pt.torch.int64 and row.dtype == pt.torch.int32
        assert np.array_equal(srt.cpu().numpy(), ids[order]) and np.array_equal(row.cpu().numpy(), order.astype(np.int32))


def test_small_ids_take_only_the_passes_they_need(pt):
    """ids below 2^20: end_bit is the bit length of the largest id, not 64."""
    rng = np.random.default_rng(13)
    ids = rng.integers(0, 2 ** 20, 70001).astype(np.int64)
    srt, row = pt.convert.sort_ids_device64(pt.ctx, pt.torch.from_numpy(ids).cuda())
    order = np.argsort(ids, kind="stable")
    assert np.array_equal(srt.cpu().numpy(), ids[order]) and np.array_equal(row.cpu().numpy(), order.astype(np.int32))
    zeros = pt.torch.zeros(5, dtype=pt.torch.int64, device="cuda")              # (largest id 0: one pass over one bit)
    srt, row = pt.convert.sort_ids_device64(pt.ctx, zeros)
    assert srt.tolist() == [0] * 5 and row.tolist() == [0, 1, 2, 3, 4]


def test_negative_id_raises(pt):
    ids = pt.torch.tensor([5, -1, 7], dtype=pt.torch.int64, device="cuda")
    with pytest.raises(ValueError):
        pt.convert.sort_ids_device64(pt.ctx, ids)
    for x, z in zip(device_maps(pt, "device64"), pt.host):                        # the context stays usable
        assert bit_equal(x, z)
