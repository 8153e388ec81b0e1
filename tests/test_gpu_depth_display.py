"""psfm_depth_display (csrc/psfm_depth_display.hip) on the device: every case of tests/golden/depth_display.npz -- the reference's own
normalize_depth_for_display followed by matplotlib's byte conversion -- through the C ABI, bytes, valid counts and both percentiles
exact; and save_model with the display images made on the device against the host route.  Reads only tests/golden/."""
import ctypes
import os

import numpy as np
import pytest

from _depth_display_np import case, case_names, fixture, same_bits
from _sparse_depth_np import case_dir, fixture as sd_fixture

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5


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
    return ns


def descriptors(pt, maps):
    d = np.zeros(len(maps), pt.convert.IMAGE_DESC)
    off = 0
    for i, m in enumerate(maps):
        d[i]["h"], d[i]["w"], d[i]["out_off"] = m.shape[0], m.shape[1], off
        off += m.size
    return d


def call(pt, depth, desc, pc, cmap, rgba, n_valid=None, z=None, n_img=None, table=True, bad=True):
    f = fixture()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    t, b = np.ascontiguousarray(f["table_" + cmap]), np.ascontiguousarray(f["bad_" + cmap])
    return pt.hip.lib().psfm_depth_display(pt.ctx.handle, depth, p(desc) if desc is not None else None, len(desc) if n_img is None else n_img,
                                           float(pc), p(t) if table else None, p(b) if bad else None, rgba,
                                           p(n_valid) if n_valid is not None else None, p(z) if z is not None else None,
                                           pt.hip.current_stream_ptr(pt.ctx.device))


def run(pt, maps, pc, cmap):
    """One call over `maps` -> (all output bytes (n_pix, 4) with the sentinel where nothing was written, n_valid, z)."""
    T = pt.torch
    depth = T.from_numpy(np.concatenate([m.reshape(-1) for m in maps])).cuda()
    rgba = T.full((depth.numel(), 4), SENTINEL, dtype=T.uint8, device="cuda")
    desc = descriptors(pt, maps)
    n_valid, z = np.full(len(maps), -1, np.int64), np.full((len(maps), 2), 7.0)
    assert call(pt, pt.hip.ptr(depth), desc, pc, cmap, pt.hip.ptr(rgba), n_valid, z) == pt.hip.PSFM_OK, pt.hip.lib().psfm_last_error()
    return rgba.cpu().numpy(), n_valid, z, desc


def assert_case(got, n_valid, z, desc, maps, want):
    for i, (m, (rgba, zz)) in enumerate(zip(maps, want)):
        o = int(desc[i]["out_off"])
        part = got[o:o + m.size]
        assert int(n_valid[i]) == int(np.count_nonzero(m > 0))
        if rgba is None:
            assert np.all(part == SENTINEL) and np.all(z[i] == 0.0)         # an empty image: untouched, reported by its count
        else:
            assert np.array_equal(part.reshape(m.shape + (4,)), rgba), i
            assert same_bits(z[i], zz), (i, z[i], zz)


@pytest.mark.parametrize("name", case_names())
def test_device_equals_the_reference(pt, name):
    maps, want, pc, cmap = case(name)
    got, n_valid, z, desc = run(pt, maps, pc, cmap)
    assert_case(got, n_valid, z, desc, maps, want)


def test_chunk_of_the_fixture_is_the_library_s(pt):
    assert pt.hip.lib().psfm_depth_display_chunk() == int(fixture()["chunk"])


def test_batch_leaves_bytes_outside_its_images_alone(pt):
    """Images that begin at bytes 60 and 124 of the output; a guard of sentinel bytes in front of and behind the call's range, and the
    empty images of a batch keep theirs."""
    T = pt.torch
    for name in ("batch_misaligned", "batch_with_empty", "batch_widths"):
        maps, want, pc, cmap = case(name)
        desc = descriptors(pt, maps)
        n_pix = sum(m.size for m in maps)
        guard = 8                                                         # pixels: keeps both pointers 16-byte aligned
        depth = T.zeros(n_pix + 2 * guard, dtype=T.float64, device="cuda")
        depth[guard:guard + n_pix] = T.from_numpy(np.concatenate([m.reshape(-1) for m in maps])).cuda()
        depth[:guard], depth[guard + n_pix:] = 3.0, 4.0                   # (valid depths: a stray read would change the counts)
        rgba = T.full((n_pix + 2 * guard, 4), SENTINEL, dtype=T.uint8, device="cuda")
        n_valid, z = np.zeros(len(maps), np.int64), np.zeros((len(maps), 2))
        st = call(pt, depth.data_ptr() + 8 * guard, desc, pc, cmap, rgba.data_ptr() + 4 * guard, n_valid, z)
        assert st == pt.hip.PSFM_OK
        got = rgba.cpu().numpy()
        assert np.all(got[:guard] == SENTINEL) and np.all(got[guard + n_pix:] == SENTINEL)
        assert_case(got[guard:guard + n_pix], n_valid, z, desc, maps, want)
    assert [int(d["out_off"]) * 4 for d in descriptors(pt, case("batch_misaligned")[0])] == [0, 60, 124]


def test_two_calls_give_identical_bytes(pt):
    for name in ("blocks", "batch_widths", "ties"):
        maps, _, pc, cmap = case(name)
        a, b = run(pt, maps, pc, cmap), run(pt, maps, pc, cmap)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and same_bits(a[2], b[2])


def test_null_outputs_are_optional(pt):
    maps, want, pc, cmap = case("mid_pc98")
    T = pt.torch
    depth = T.from_numpy(maps[0].reshape(-1).copy()).cuda()
    rgba = T.full((depth.numel(), 4), SENTINEL, dtype=T.uint8, device="cuda")
    assert call(pt, pt.hip.ptr(depth), descriptors(pt, maps), pc, cmap, pt.hip.ptr(rgba)) == pt.hip.PSFM_OK
    assert np.array_equal(rgba.cpu().numpy().reshape(want[0][0].shape), want[0][0])


def test_bad_arguments_are_refused_and_the_context_stays_usable(pt):
    T = pt.torch
    maps, want, pc, cmap = case("batch_misaligned")
    depth = T.from_numpy(np.concatenate([m.reshape(-1) for m in maps])).cuda()
    rgba = T.full((depth.numel(), 4), SENTINEL, dtype=T.uint8, device="cuda")
    desc = descriptors(pt, maps)
    dp, rp = depth.data_ptr(), rgba.data_ptr()

    def changed(field, i, v):
        d = desc.copy()
        d[field][i] = v
        return d
    bad = [dict(depth=None), dict(rgba=None), dict(desc=None), dict(table=False), dict(bad=False), dict(n_img=0), dict(n_img=-2),
           dict(desc=changed("w", 1, 0)), dict(desc=changed("h", 0, -1)), dict(desc=changed("out_off", 1, 14)),
           dict(desc=changed("out_off", 1, 16)), dict(desc=changed("out_off", 0, 4)), dict(desc=changed("out_off", 2, 15)),
           dict(pc=np.nan), dict(pc=np.inf), dict(pc=-0.5), dict(pc=100.5), dict(depth=dp + 8), dict(rgba=rp + 4)]
    for kw in bad:
        d = kw.get("desc", desc)
        st = call(pt, kw.get("depth", dp), d, kw.get("pc", pc), cmap, kw.get("rgba", rp), n_img=kw.get("n_img", len(desc) if d is not None else 3),
                  table=kw.get("table", True), bad=kw.get("bad", True))
        assert st == pt.hip.PSFM_ERR_ARG, kw
        assert b"psfm_depth_display" in pt.hip.lib().psfm_last_error()
        assert bool((rgba == SENTINEL).all())                             # nothing ran
    assert pt.hip.lib().psfm_depth_display(None, dp, desc.ctypes.data_as(ctypes.c_void_p), 3, 98.0, None, None, rp, None, None, None) == pt.hip.PSFM_ERR_ARG
    got, n_valid, z, desc2 = run(pt, maps, pc, cmap)
    assert_case(got, n_valid, z, desc2, maps, want)


def test_depth_display_device_equals_the_model(pt):
    """The Python entry over the maps of one batch, read where they are."""
    m = pt.convert.read_model_arrays(case_dir("a"))
    pt.ctx.set_sparse_depth(0)
    try:
        batch = next(pt.convert.sparse_depth_batches(m, pt.ctx))
    finally:
        pt.ctx.set_sparse_depth()
    assert len(batch) == 4
    res = pt.convert.depth_display_device([d for _, d in batch], ctx=pt.ctx)
    for (_, d), (rgba, z1, z2) in zip(batch, res):
        want, w1, w2 = pt.convert.depth_display_host(d.cpu().numpy())
        assert np.array_equal(rgba.cpu().numpy(), want) and same_bits([z1, z2], [w1, w2])
    with pytest.raises(ValueError):
        pt.convert.depth_display_device([batch[1][1], batch[0][1]], ctx=pt.ctx)
    assert pt.convert.depth_display_device([], ctx=pt.ctx) == []


def test_save_model_device_display_writes_the_host_route_s_pngs(pt, tmp_path):
    os.environ.setdefault("MPLBACKEND", "Agg")
    from matplotlib import pyplot as plt
    for c in ("a", "d"):
        f = sd_fixture(c)
        m = pt.convert.read_model_arrays(case_dir(c))
        dev, host, off = (str(tmp_path / (c + s)) for s in ("_dev", "_host", "_off"))
        pt.convert.save_model(dev, m, ctx=pt.ctx, display="device", writers=2)
        pt.convert.save_model(host, m, ctx=pt.ctx, display="host")
        pt.convert.save_model(off, m, ctx=pt.ctx, display="device", png=False)
        for name in f["names"].tolist():
            stem = os.path.splitext(name)[0]
            a, b = (os.path.join(p, "depths", stem + ".png") for p in (dev, host))
            assert os.path.exists(a) == os.path.exists(b) == (name not in f["png_failed"].tolist())      # none for the all-zero maps
            if os.path.exists(a):
                x, y = plt.imread(a), plt.imread(b)
                assert x.shape == y.shape and x.shape[2] == 4 and np.array_equal(x, y)
            assert not os.path.exists(os.path.join(off, "depths", stem + ".png"))
            assert np.array_equal(np.load(os.path.join(dev, "depths", stem + ".npy")), np.load(os.path.join(off, "depths", stem + ".npy")))
    assert f["png_failed"].tolist() == ["d1.png", "d2.png"]


def test_timing_reports_four_spans(pt):
    pt.ctx.set_depth_display(timing=True)
    try:
        maps, _, pc, cmap = case("blocks")
        run(pt, maps, pc, cmap)
        ms = pt.ctx.depth_display_ms()
    finally:
        pt.ctx.set_depth_display()
    assert set(ms) == {"count_ms", "compact_ms", "select_ms", "colour_ms"} and all(0 < v < 1000 for v in ms.values())
