"""The motion classifier's input step (motion_seg/core/network/traj_oa_depth.py:72-114) without a GPU, against golden vectors that
the REFERENCE's own traj_oa_depth.augment_traj produced (tests/golden/make_augment_golden.py: the module imported unmodified in the
build container, tensors built as main_motion_segmentation.py:71-78 builds them).

Two statements of the same unfused fp32 formula are pinned to those vectors bit for bit: tests/_augment_np.py (NumPy; the GPU tests
use it where no fixture can exist) and particle-sfm_amd/csrc/psfm_augment.h -- the arithmetic of psfm_traj_augment_kernel --
compiled for the host through tests/host/shim by tests/host/augment_host.cpp, with -ffp-contract=off."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from _augment_np import AUGMENT_CASES, augment_np, edge_counts, seeded_inputs
from _common import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("augment") / "libaugment_host.so")
    cmd = ["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "tests", "host", "shim"),
           "-I", os.path.join(ROOT, "particle-sfm_amd", "csrc"), os.path.join(ROOT, "tests", "host", "augment_host.cpp"), "-o", out]
    subprocess.run(cmd, check=True)
    L = ctypes.CDLL(out)
    vp = ctypes.c_void_p
    L.psfm_host_traj_augment.argtypes = [vp, vp, vp, ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp]
    L.psfm_host_traj_augment.restype = None
    return L


def host_augment(L, xy, mask, depth, input_hw, kinv):
    xy = np.ascontiguousarray(xy, np.float64)
    K, n = xy.shape[:2]
    mask = np.ascontiguousarray(np.asarray(mask, np.float64).reshape(K, n))
    depth = np.ascontiguousarray(depth, np.float32)
    kinv = np.ascontiguousarray(kinv, np.float32)
    assert depth.shape == (n, int(input_hw[0]), int(input_hw[1]))
    out = np.full((10, K, n), np.nan, np.float32)
    L.psfm_host_traj_augment(xy.ctypes.data, mask.ctypes.data, depth.ctypes.data, K, n, int(input_hw[0]), int(input_hw[1]),
                             kinv.ctypes.data, out.ctypes.data)
    return out


@pytest.mark.parametrize("name", AUGMENT_CASES)
def test_numpy_restatement_equals_reference_fixture(name):
    g = golden(name)
    got = augment_np(g["traj"], g["mask"], g["depth"], g["input_size"], g["kinv"])
    assert got.shape == g["out"].shape and np.array_equal(got, g["out"])
    assert np.array_equal(got.view(np.uint32), g["out"].view(np.uint32))        # (the signs of zeros too)


@pytest.mark.parametrize("name", AUGMENT_CASES)
def test_device_header_on_the_host_equals_reference_fixture(host, name):
    g = golden(name)
    got = host_augment(host, g["traj"], g["mask"], g["depth"], g["input_size"], g["kinv"])
    for c in range(10):
        assert np.array_equal(got[c], g["out"][c]), "channel %d" % c


def test_device_header_on_the_host_equals_the_restatement_at_other_shapes(host):
    """L = 1 (no motion, no read past the row), L = 2, a partial last wave's worth of rows, and a kinv that is not image_grid's."""
    from psfm_motion_seg.augment import reference_kinv
    for K, n, hw, seed in [(65, 1, (30, 50), 1), (1, 2, (30, 50), 2), (257, 10, (30, 50), 3), (33, 5, (1, 1), 4), (40, 3, (7, 1), 5)]:
        xy, mask, depth = seeded_inputs(K, n, hw, seed)
        kinv = reference_kinv(hw)
        got = host_augment(host, xy, mask, depth, hw, kinv)
        assert np.array_equal(got, augment_np(xy, mask, depth, hw, kinv)), (K, n, hw)
        if n == 1:
            assert not got[[2, 3, 7, 8, 9]].any()
    xy, mask, depth = seeded_inputs(50, 4, (11, 13), 6)
    kinv = np.random.default_rng(7).normal(size=(3, 3)).astype(np.float32)
    assert np.array_equal(host_augment(host, xy, mask, depth, (11, 13), kinv), augment_np(xy, mask, depth, (11, 13), kinv))


def test_device_header_keeps_every_access_in_bounds_on_nonfinite_coordinates(host):
    """Values are unspecified for NaN / Inf / huge coordinates; the pixel index is not: the depth stack sits between guard pages'
    worth of NaN here, and a finite output in channels 4-6 says the read stayed inside it."""
    K, n, hw = 64, 3, (5, 7)
    rng = np.random.default_rng(8)
    xy = rng.choice(np.array([np.nan, np.inf, -np.inf, 1e300, -1e300, 3e9, -3e9, 1e38, 0.5]), size=(K, n, 2))
    mask = np.zeros((K, n))
    pad = 4096
    buf = np.full(pad + n * hw[0] * hw[1] + pad, np.nan, np.float32)
    depth = buf[pad:pad + n * hw[0] * hw[1]].reshape(n, *hw)
    depth[:] = 1.0
    from psfm_motion_seg.augment import reference_kinv
    with np.errstate(all="ignore"):
        got = host_augment(host, xy, mask, depth, hw, reference_kinv(hw))
    assert np.isfinite(got[4:7]).all()


def test_synthetic_fixture_holds_the_edges_it_is_there_for():
    g = golden(AUGMENT_CASES[3])
    n_next_row, n_clamped, n_pad_then_present = edge_counts(g["traj"], g["mask"], g["input_size"])
    assert n_next_row >= 1 and n_clamped >= 1 and n_pad_then_present >= 1
    t = g["traj"]
    assert (t == 0.0).any() and (t == 1.0).any()
    assert 0.25 < g["mask"].mean() < 0.35
    # the real windows: padding patterns of real trajectories, L = 10 twice and the odd L of the short sequence
    assert [golden(n)["traj"].shape[1] for n in AUGMENT_CASES] == [10, 10, 27, 7]
    for n in AUGMENT_CASES[:3]:
        assert edge_counts(golden(n)["traj"], golden(n)["mask"], golden(n)["input_size"])[2] >= 1
    a, b = golden(AUGMENT_CASES[0]), golden(AUGMENT_CASES[1])
    assert int(a["frame0"]) == 0 and int(b["frame0"]) == 13 and int(b["window_index"]) == int(b["n_windows"]) - 1 == 2


@pytest.mark.parametrize("name", AUGMENT_CASES)
def test_reference_kinv_equals_the_fixture_bit_for_bit(name):
    from psfm_motion_seg.augment import reference_kinv
    g = golden(name)
    k = reference_kinv(tuple(int(x) for x in g["input_size"]))
    assert k.dtype == np.float32 and k.shape == (3, 3)
    assert np.array_equal(k.view(np.uint32), g["kinv"].view(np.uint32))


def test_no_cpu_fallback(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    from psfm_motion_seg.augment import augment_traj_device
    g = golden(AUGMENT_CASES[3])
    with pytest.raises(RuntimeError):
        augment_traj_device(g["traj"], g["mask"], g["depth"], g["input_size"])
