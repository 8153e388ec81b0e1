"""The motion classifier's OANet decoder (traj_oa_depth.decoder, motion_seg/core/network/oanet.py:13-206) without a GPU, against
golden vectors that the REFERENCE's own module produced (tests/golden/make_decoder_golden.py: the module imported unmodified in the
build container, seeded weights, the encoder fixtures' outputs and seeded inputs around the kernel's 64-point tile).

tests/_decoder_np.py, the f64 restatement, is pinned to the module's .double() output to 1e-10.  particle-sfm_amd/csrc/
psfm_decoder.h -- the plan, the folds, the statistics, the softmaxes and the orders of psfm_traj_decode -- is compiled for the host
through tests/host/shim by tests/host/decoder_host.cpp with -ffp-contract=off, the matrix instruction written as the fmaf chain it
equals, and compared with that f64 truth within each case's own tol = 4 e, where e is the error the reference's own fp32 run shows
against it on that case (measured by the generator, stored with the case)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from _decoder_np import (BIG_K, DECODER_CASES, GOLDEN, SMALL_CASES, WEIGHT_SEED, case_input, decoder_fixture, decoder_np, fixture_input,
                         packed_sha256, seeded_decoder_weights, sigmoid, unpack)
from psfm_motion_seg.decoder import DECODER_KEYS, WEIGHT_COUNT, pack_decoder_weights_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG_CASE = DECODER_CASES[-1]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("decoder") / "libdecoder_host.so")
    cmd = ["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "tests", "host", "shim"),
           "-I", os.path.join(ROOT, "particle-sfm_amd", "csrc"), os.path.join(ROOT, "tests", "host", "decoder_host.cpp"), "-o", out]
    subprocess.run(cmd, check=True)
    L = ctypes.CDLL(out)
    vp = ctypes.c_void_p
    L.psfm_host_traj_decode.argtypes = [vp, vp, ctypes.c_long, vp, ctypes.c_size_t, vp, vp, vp]
    L.psfm_host_traj_decode.restype = ctypes.c_int
    L.psfm_host_decoder_weight_count.restype = ctypes.c_int
    L.psfm_host_decoder_workspace_bytes.argtypes = [ctypes.c_long]
    L.psfm_host_decoder_workspace_bytes.restype = ctypes.c_size_t
    L.psfm_host_decoder_tables.argtypes = [ctypes.c_long, vp, vp]
    L.psfm_host_decoder_tables.restype = None
    return L


@pytest.fixture(scope="module")
def weights():
    W = seeded_decoder_weights()
    return W, pack_decoder_weights_host(W)


def host_decode(L, x, packed, fill=0xFF):
    """(logits, prob, pred) of the host build; the workspace starts out as bytes `fill` (0xFF: NaN everywhere)."""
    x = np.ascontiguousarray(x, np.float32)
    K = x.shape[1]
    need = L.psfm_host_decoder_workspace_bytes(K)
    ws = np.full(need, fill, np.uint8)
    lo, pr, pd = np.full(K, np.nan, np.float32), np.full(K, np.nan, np.float32), np.full(K, 77, np.uint8)
    assert L.psfm_host_traj_decode(x.ctypes.data, packed.ctypes.data, K, ws.ctypes.data, need, lo.ctypes.data, pr.ctypes.data, pd.ctypes.data) > 0
    return lo, pr, pd


def test_the_tolerances_and_the_weights_are_the_stored_ones(weights):
    """Per case tol = 4 e, e = max |logit32 - logit64| of the reference's own two runs; the weights are the generator's."""
    _, packed = weights
    meta = np.load(os.path.join(GOLDEN, "decoder_meta.npz"))
    assert int(meta["weight_seed"]) == WEIGHT_SEED and float(meta["margin"]) == 4.0
    assert packed_sha256(packed) == str(meta["weights_sha256"])
    assert [str(c) for c in meta["cases"]] == DECODER_CASES
    for case, e_meta in zip(DECODER_CASES, meta["e"]):
        fx = decoder_fixture(case)
        assert float(fx["e"]) == float(e_meta) and float(fx["tol"]) == 4.0 * float(fx["e"])
        if case != BIG_CASE:
            assert float(fx["e"]) == float(np.abs(fx["logit32"].astype(np.float64) - fx["logit64"]).max())
            assert np.array_equal(fx["x"], case_input(case)), case                # the stored input is the seeded one
            assert (np.abs(fx["logit64"]) <= float(fx["tol"])).mean() <= 0.005
        else:
            assert float(fx["e"]) >= float(np.abs(fx["logit32"].astype(np.float64) - fx["logit64"]).max())      # e is over all rows
            assert float(fx["band"]) <= 0.005 and len(fx["rows"]) == 8192
    e = {c: float(decoder_fixture(c)["e"]) for c in DECODER_CASES}
    assert all(1e-5 < e[c] < 2e-4 for c in DECODER_CASES if c.startswith("enc_"))
    assert e["seeded_k2"] > 1e-3 > e["seeded_k1000"]                              # two points: an ill-conditioned instance variance


def test_pack_decoder_weights(host, weights):
    W, packed = weights
    assert len(DECODER_KEYS) == len(W) == 186
    assert packed.dtype == np.float32 and packed.size == WEIGHT_COUNT == 529497 == host.psfm_host_decoder_weight_count()
    assert sum(int(np.prod(s)) for k, s in DECODER_KEYS if "running_" in k) == 7712
    with_prefix = {"decoder." + k: v for k, v in W.items()}
    with_prefix["joint_encoder.fc2.bias"] = np.zeros(16, np.float32)              # the rest of a checkpoint is ignored
    with_prefix["decoder.l2.0.conv2.0.num_batches_tracked"] = np.zeros((), np.int64)
    assert np.array_equal(pack_decoder_weights_host(with_prefix), packed)
    assert np.array_equal(pack_decoder_weights_host({"dec." + k: v for k, v in W.items()}, prefix="dec."), packed)
    import torch
    assert np.array_equal(pack_decoder_weights_host({k: torch.from_numpy(v) for k, v in W.items()}), packed)
    # the packed order is the module's own: conv1, down1, up1, l1_1, l1_2, l2, output -- and the header's table says the same
    names = ["conv1.weight", "down1.conv.1.weight", "up1.conv.1.weight", "l1_1.0.conv.1.weight", "l1_2.0.shot_cut.weight", "l2.0.conv1.1.weight",
             "output.weight"]
    offsets, o = {}, 0
    for k, s in DECODER_KEYS:
        offsets[k] = o
        o += int(np.prod(s))
    table, ws = (ctypes.c_long * 8)(), (ctypes.c_long * 14)()
    host.psfm_host_decoder_tables(100, table, ws)
    assert list(table) == [offsets[n] for n in names] + [WEIGHT_COUNT]
    assert np.array_equal(packed[:2048], W["conv1.weight"].reshape(-1)) and packed[-1] == W["output.bias"][0]
    assert all(np.array_equal(unpack(packed)[k], W[k]) for k in W)
    missing = dict(W)
    del missing["l2.3.conv2.0.running_var"]
    with pytest.raises(ValueError, match="l2.3.conv2.0.running_var"):
        pack_decoder_weights_host(missing)
    bad = dict(W)
    bad["up1.conv.3.weight"] = np.zeros((128, 100, 1, 1), np.float32)
    with pytest.raises(ValueError, match="up1.conv.3.weight"):
        pack_decoder_weights_host(bad)


@pytest.mark.parametrize("case", SMALL_CASES)
def test_numpy_restatement_equals_the_reference_in_f64(weights, case):
    W, _ = weights
    fx = decoder_fixture(case)
    err = float(np.abs(decoder_np(fx["x"], W, same_order=case == "equal_k50") - fx["logit64"]).max())
    print("max |restatement - logit64| = %.3e" % err)
    assert err <= 1e-10


@pytest.mark.parametrize("case", ["enc_augment_24x32_t27_full", "seeded_k65", "seeded_k3"])
def test_the_fixtures_pin_the_five_readings(weights, case):
    """Softmax over the points, the biased variance, eps 1e-3, the raw x1_1, up1's own weights: each misreading misses by >= 100 tol."""
    W, _ = weights
    fx = decoder_fixture(case)
    for quirk in ("pool_over_clusters", "unbiased_var", "in_eps_1e5", "pool_normalised", "up_shares_down"):
        assert np.abs(decoder_np(fx["x"], W, **{quirk: True}) - fx["logit64"]).max() >= 100 * float(fx["tol"]), quirk


@pytest.mark.parametrize("case", SMALL_CASES)
def test_device_header_on_the_host_equals_the_reference_within_tol(host, weights, case):
    _, packed = weights
    fx = decoder_fixture(case)
    tol, want = float(fx["tol"]), fx["logit64"]
    lo, pr, pd = host_decode(host, fx["x"], packed)
    err = float(np.abs(lo.astype(np.float64) - want).max())
    perr = float(np.abs(pr.astype(np.float64) - sigmoid(want)).max())
    print("max |logit - logit64| = %.3e, max |prob - sigmoid(logit64)| = %.3e, tol = %.3e" % (err, perr, tol))
    assert np.isfinite(lo).all() and err <= tol and perr <= tol
    assert np.array_equal(pd.astype(bool), pr > np.float32(0.5))
    outside = np.abs(want) > tol
    assert (~outside).mean() <= 0.005 and np.array_equal(pd.astype(bool)[outside], (want > 0)[outside])


def test_host_build_ignores_the_workspace_contents_and_refuses_bad_arguments(host, weights):
    _, packed = weights
    x = fixture_input("seeded_k129")
    a, b = host_decode(host, x, packed, fill=0xFF), host_decode(host, x, packed, fill=0x00)
    assert all(np.array_equal(u.view(np.uint8), v.view(np.uint8)) for u, v in zip(a, b))
    ws = np.zeros(host.psfm_host_decoder_workspace_bytes(8), np.uint8)
    out = np.zeros(8, np.float32)
    args = (ws.ctypes.data, ws.size, out.ctypes.data, None, None)
    assert host.psfm_host_traj_decode(x.ctypes.data, packed.ctypes.data, 0, None, 0, None, None, None) == 0
    assert host.psfm_host_traj_decode(x.ctypes.data, packed.ctypes.data, 1, *args) == -1
    assert host.psfm_host_traj_decode(x.ctypes.data, packed.ctypes.data, -1, *args) == -1
    assert host.psfm_host_traj_decode(x.ctypes.data, packed.ctypes.data, 8, ws.ctypes.data, ws.size - 1, out.ctypes.data, None, None) == -1


def test_workspace_layout(host):
    """The byte count is monotone in k, the header's sections are disjoint, in order, 256-byte aligned and each large enough for what
    the plan keeps there; about 2.6 KB per trajectory at the shipped cap."""
    prev = 0
    for k in [2, 3, 63, 64, 65, 511, 512, 513, 1000, 4096, 100000, 2 ** 24 - 1]:
        ws = (ctypes.c_long * 14)()
        host.psfm_host_decoder_tables(k, (ctypes.c_long * 8)(), ws)
        a, t, x1, xup, emb, sp, sf, mp, mf, pp, x2, total, nb, nb2 = list(ws)
        assert total == host.psfm_host_decoder_workspace_bytes(k) > prev
        prev = total
        assert nb == -(-k // 64) and nb2 == -(-k // 512)
        need = [(a, 512 * k), (t, 512 * k), (x1, 512 * k), (xup, 512 * k), (emb, 400 * k), (sp, nb * 128 * 16), (sf, 24 * 256 * 8),
                (mp, nb * 100 * 16), (mf, 800), (pp, nb2 * 51200), (x2, 51200)]
        ends = [o for o, _ in need[1:]] + [total]
        for (o, n), end in zip(need, ends):
            assert o % 256 == 0 and o + n <= end, (k, o, n, end)
    assert 2400 * BIG_K < host.psfm_host_decoder_workspace_bytes(BIG_K) < 2700 * BIG_K


def test_no_cpu_fallback(monkeypatch, weights):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    from psfm_motion_seg.decoder import decode_traj_device, device_predictor, pack_decoder_weights
    W, packed = weights
    with pytest.raises(RuntimeError):
        pack_decoder_weights(W)
    with pytest.raises(RuntimeError):
        decode_traj_device(fixture_input("seeded_k3"), packed)
    predict = device_predictor(packed, packed, lambda t: None, (30, 50))
    with pytest.raises(RuntimeError):
        predict(np.zeros((4, 10, 2)), np.zeros((4, 10, 2)), np.zeros((4, 10, 1)), np.arange(10))
