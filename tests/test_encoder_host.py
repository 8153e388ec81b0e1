"""The motion classifier's trajectory transformer (traj_oa_depth.joint_encoder, motion_seg/core/network/traj_oa_depth.py:25-60)
without a GPU, against golden vectors that the REFERENCE's own module produced (tests/golden/make_encoder_golden.py: the module
imported unmodified in the build container, seeded and perturbed weights, the four augment fixtures as inputs).

tests/_encoder_np.py, the f64 restatement, is pinned to the module's .double() output to 1e-12.  particle-sfm_amd/csrc/
psfm_encoder.h -- the arithmetic of psfm_traj_encode_kernel -- is compiled for the host through tests/host/shim by
tests/host/encoder_host.cpp with -ffp-contract=off and compared with that f64 truth within the fixtures' `tol` = 4 e, where e is
the error the reference's own fp32 run shows against it (measured by the generator, stored in encoder_weights.npz)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from _common import golden
from _encoder_np import ENCODER_CASES, encoder_fixture, encoder_np, fixture_weights, seeded_encoder_inputs
from psfm_motion_seg.encoder import ENCODER_KEYS, WEIGHT_COUNT, pack_encoder_weights_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("encoder") / "libencoder_host.so")
    cmd = ["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "tests", "host", "shim"),
           "-I", os.path.join(ROOT, "particle-sfm_amd", "csrc"), os.path.join(ROOT, "tests", "host", "encoder_host.cpp"), "-o", out]
    subprocess.run(cmd, check=True)
    L = ctypes.CDLL(out)
    vp = ctypes.c_void_p
    L.psfm_host_traj_encode.argtypes = [vp, vp, vp, ctypes.c_long, ctypes.c_int, vp]
    L.psfm_host_traj_encode.restype = None
    L.psfm_host_encoder_weight_count.restype = ctypes.c_int
    L.psfm_host_traj_encode_blocks.argtypes = [vp, vp, vp, ctypes.c_long, ctypes.c_int, ctypes.c_int, vp]
    L.psfm_host_traj_encode_blocks.restype = ctypes.c_long
    return L


@pytest.fixture(scope="module")
def weights():
    W, tol = fixture_weights()
    return W, pack_encoder_weights_host(W), tol


def host_encode(L, features, mask, packed):
    f = np.ascontiguousarray(features, np.float32)
    f = f[0] if f.ndim == 4 else f
    _, K, n = f.shape
    m = np.ascontiguousarray(np.asarray(mask, np.float64).reshape(K, n))
    w = np.ascontiguousarray(packed, np.float32)
    out = np.full((16, K), np.nan, np.float32)
    L.psfm_host_traj_encode(f.ctypes.data, m.ctypes.data, w.ctypes.data, K, n, out.ctypes.data)
    return out


def max_err(got, want):
    assert got.shape == want.shape
    err = float(np.abs(got.astype(np.float64) - want).max())
    print("max |got - want| = %.3e" % err)
    return err


def test_the_tolerance_is_the_measured_one(weights):
    """tol = 4 e, e = max |out32 - out64| over the four cases: the reference's own fp32 error against its f64 run."""
    _, _, tol = weights
    e = max(float(np.abs(encoder_fixture(n)["out32"].astype(np.float64) - encoder_fixture(n)["out64"]).max()) for n in ENCODER_CASES)
    g = np.load(os.path.join(ROOT, "tests", "golden", "encoder_weights.npz"))
    assert float(g["e"]) == e and tol == 4.0 * e
    assert 1e-7 < e < 1e-5
    assert [str(encoder_fixture(n)["input"]) for n in ENCODER_CASES] == ENCODER_CASES


@pytest.mark.parametrize("name", ENCODER_CASES)
def test_numpy_restatement_equals_the_reference_in_f64(weights, name):
    W, _, _ = weights
    g, fx = golden(name), encoder_fixture(name)
    assert max_err(encoder_np(g["out"], g["mask"], W), fx["out64"]) <= 1e-12


@pytest.mark.parametrize("name", ENCODER_CASES)
def test_the_fixtures_pin_the_three_quirks(weights, name):
    """Cross-attention sees the padded memory, the max runs over all tokens, nothing is zeroed: each misreading misses by >= 100 tol."""
    W, _, tol = weights
    g, fx = golden(name), encoder_fixture(name)
    for quirk in ("mask_memory", "max_valid_only", "zero_padded"):
        assert np.abs(encoder_np(g["out"], g["mask"], W, **{quirk: True}) - fx["out64"]).max() >= 100 * tol, quirk


@pytest.mark.parametrize("name", ENCODER_CASES)
def test_device_header_on_the_host_equals_the_reference_within_tol(host, weights, name):
    _, packed, tol = weights
    g, fx = golden(name), encoder_fixture(name)
    got = host_encode(host, g["out"], g["mask"], packed)
    assert got.dtype == np.float32 and np.isfinite(got).all()
    assert max_err(got, fx["out64"]) <= tol


def test_device_header_on_the_host_equals_the_restatement_at_other_shapes(host, weights):
    """L = 1 (softmax over one key), L = 2, K = 1, L = 64, and rows with exactly one valid token."""
    W, packed, tol = weights
    for K, n, seed in [(40, 1, 1), (33, 2, 2), (1, 10, 3), (3, 64, 4), (5, 33, 5)]:
        f, m = seeded_encoder_inputs(K, n, seed)
        if n == 1:
            assert not m.any()
        assert max_err(host_encode(host, f, m, packed), encoder_np(f, m, W)) <= tol, (K, n)
    f, m = seeded_encoder_inputs(24, 10, 6)
    for k in range(24):                       # one valid token, at every position in turn
        m[k] = 1.0
        m[k, k % 10] = 0.0
    assert max_err(host_encode(host, f, m, packed), encoder_np(f, m, W)) <= tol


@pytest.mark.parametrize("K,n", [(1, 1), (7, 7), (6 * 4 + 1, 10), (3, 33), (2, 64), (250, 10), (70, 3)])
def test_the_kernels_lane_mapping_emulated_on_the_host(host, weights, K, n):
    """psfm_enc_lane / psfm_enc_pad_bits -- where a lane of the kernel works, which rows it reads and writes, how it cuts its
    trajectory's padding bits out of the wave's ballot -- with blocks of 4 waves emulated thread by thread: every index inside its
    bounds, every output written, and the same bits as the plain loop over trajectories, whatever the packing."""
    _, packed, _ = weights
    f, m = seeded_encoder_inputs(K, n, 300 + K + n)
    want = host_encode(host, f, m, packed)
    mm = np.ascontiguousarray(m.reshape(K, n))
    for waves in (4, 1):
        got = np.full((16, K), np.nan, np.float32)
        assert host.psfm_host_traj_encode_blocks(f.ctypes.data, mm.ctypes.data, packed.ctypes.data, K, n, waves, got.ctypes.data) == 0
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_a_fully_padded_row_changes_no_other_row(host, weights):
    """Its own 16 values are unspecified; every other row keeps its bits."""
    _, packed, _ = weights
    f, m = seeded_encoder_inputs(9, 10, 7)
    want = host_encode(host, f, m, packed)
    m[4] = 1.0
    got = host_encode(host, f, m, packed)
    keep = np.arange(9) != 4
    assert np.array_equal(got[:, keep].view(np.uint32), want[:, keep].view(np.uint32))


def test_pack_encoder_weights(host, weights):
    W, packed, _ = weights
    assert len(ENCODER_KEYS) == len(W) == 68
    assert packed.dtype == np.float32 and packed.size == WEIGHT_COUNT == 15872 == host.psfm_host_encoder_weight_count()
    with_prefix = {"joint_encoder." + k: v for k, v in W.items()}
    with_prefix["decoder.l1_1.conv1.weight"] = np.zeros((128, 16, 1, 1), np.float32)          # the rest of a checkpoint is ignored
    assert np.array_equal(pack_encoder_weights_host(with_prefix), packed)
    assert np.array_equal(pack_encoder_weights_host({"enc." + k: v for k, v in W.items()}, prefix="enc."), packed)
    import torch
    assert np.array_equal(pack_encoder_weights_host({k: torch.from_numpy(v) for k, v in W.items()}), packed)
    # the packed order is the module's own: fc1 first, decoder.norm.bias last
    assert np.array_equal(packed[:160], W["input_fc1.weight"].reshape(-1))
    assert np.array_equal(packed[-16:], W["transformer_model.decoder.norm.bias"])
    missing = dict(W)
    del missing["transformer_model.decoder.layers.1.multihead_attn.in_proj_bias"]
    with pytest.raises(ValueError, match="multihead_attn.in_proj_bias"):
        pack_encoder_weights_host(missing)
    bad = dict(W)
    bad["transformer_model.encoder.layers.0.linear1.weight"] = np.zeros((16, 64), np.float32)
    with pytest.raises(ValueError, match="encoder.layers.0.linear1.weight"):
        pack_encoder_weights_host(bad)


def test_no_cpu_fallback(monkeypatch, weights):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    from psfm_motion_seg.encoder import encode_traj_device, pack_encoder_weights
    W, packed, _ = weights
    with pytest.raises(RuntimeError):
        pack_encoder_weights(W)
    f, m = seeded_encoder_inputs(2, 10, 8)
    with pytest.raises(RuntimeError):
        encode_traj_device(f, m, packed)
