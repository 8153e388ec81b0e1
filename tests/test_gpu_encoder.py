"""psfm_traj_encode (csrc/psfm_encoder.hip) on the GPU: the motion classifier's trajectory transformer, against the f64 output of
the REFERENCE's own traj_oa_depth.joint_encoder (tests/golden/make_encoder_golden.py) within the fixtures' measured `tol` (4 x the
error of the reference's own fp32 run against that f64 output), through psfm_motion_seg.encoder and through the raw C ABI, and
against the f64 NumPy restatement (tests/_encoder_np.py, pinned to those fixtures by tests/test_encoder_host.py) at the shapes no
fixture covers.  What must be exact is checked bit for bit: a row's result does not depend on where it sits among the K rows, on
how many there are, or on what the other rows hold."""

import numpy as np
import pytest

from _common import golden, regen_inputs
from _encoder_np import ENCODER_CASES, encoder_fixture, encoder_np, fixture_weights, seeded_encoder_inputs

pytestmark = pytest.mark.gpu
SENTINEL = -12345.0
GUARD = 4096


@pytest.fixture(scope="module")
def pt():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from point_trajectory import trajectory, _hip
    from psfm_motion_seg import augment, encoder
    _hip.context()
    class NS: pass
    ns = NS()
    ns.trajectory, ns.hip, ns.augment, ns.encoder = trajectory, _hip, augment, encoder
    ns.W, ns.tol = fixture_weights()
    ns.weights = encoder.pack_encoder_weights({"joint_encoder." + k: v for k, v in ns.W.items()})
    return ns


def raw_call(pt, feat, mask, weights, K, n, out, ctx=None):
    """psfm_traj_encode with device tensors (or None) as they are; returns the status."""
    ctx = ctx or pt.hip.context()
    return pt.hip.lib().psfm_traj_encode(ctx.handle, pt.hip.ptr(feat), pt.hip.ptr(mask), pt.hip.ptr(weights), K, n, pt.hip.ptr(out),
                                         pt.hip.current_stream_ptr(ctx.device))


def raw_encode(pt, feat, mask):
    """Through the C ABI with buffers allocated here: (16,K) result; the guard region behind `out` must come back untouched."""
    import torch
    feat = np.ascontiguousarray(feat, np.float32)
    feat = feat[0] if feat.ndim == 4 else feat
    _, K, n = feat.shape
    d_f = torch.from_numpy(feat).cuda()
    d_m = torch.from_numpy(np.ascontiguousarray(np.asarray(mask, np.float64).reshape(K, n))).cuda()
    out = torch.full((16 * K + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    assert raw_call(pt, d_f, d_m, pt.weights, K, n, out) == pt.hip.PSFM_OK
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert (host[16 * K:] == SENTINEL).all(), "psfm_traj_encode wrote behind its output"
    return host[:16 * K].reshape(16, K)


def max_err(got, want):
    assert got.shape == want.shape and got.dtype == np.float32
    err = float(np.abs(got.astype(np.float64) - want).max())
    print("max |got - want| = %.3e" % err)
    return err


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def rows_250(pt):
    """250 seeded rows at L = 10 and the kernel's result for them: the reference of the exact invariants."""
    f, m = seeded_encoder_inputs(250, 10, 77)
    return f, m, raw_encode(pt, f, m)


def test_weight_count_and_packing(pt):
    import torch
    assert pt.hip.lib().psfm_traj_encode_weight_count() == pt.encoder.WEIGHT_COUNT == 15872
    assert pt.weights.is_cuda and pt.weights.dtype == torch.float32 and tuple(pt.weights.shape) == (15872,)
    assert torch.equal(pt.weights, pt.encoder.pack_encoder_weights({k: torch.from_numpy(v) for k, v in pt.W.items()}))


@pytest.mark.parametrize("name", ENCODER_CASES)
def test_module_equals_reference_fixture(pt, name):
    import torch
    g, fx = golden(name), encoder_fixture(name)
    K = g["traj"].shape[0]
    feat, mask = torch.from_numpy(g["out"]).cuda()[None], torch.from_numpy(g["mask"]).cuda()      # (1,10,K,L) f32, (K,L,1) f64
    out = pt.encoder.encode_traj_device(feat, mask, pt.weights)
    assert tuple(out.shape) == (1, 16, K) and out.dtype == torch.float32 and out.is_contiguous()
    assert max_err(out[0].cpu().numpy(), fx["out64"]) <= pt.tol
    # the other accepted forms: (10,K,L) features, a (K,L) mask, an f32 mask, host arrays
    for f2, m2 in ((feat[0], mask[:, :, 0]), (g["out"], g["mask"].astype(np.float32))):
        assert torch.equal(pt.encoder.encode_traj_device(f2, m2, pt.weights), out)


@pytest.mark.parametrize("name", ENCODER_CASES)
def test_c_abi_equals_reference_fixture(pt, name):
    g, fx = golden(name), encoder_fixture(name)
    assert max_err(raw_encode(pt, g["out"], g["mask"]), fx["out64"]) <= pt.tol


@pytest.mark.parametrize("K,n", [(1, 1),             # one token, softmax over one key
                                 (7, 7),             # 9 trajectories per wave, one idle lane, a partial wave
                                 (6 * 4 + 1, 10),    # one trajectory past a full 256-thread block at L = 10
                                 (3, 33),            # one trajectory per wave
                                 (2, 64),            # a full wave
                                 (100000, 10)])      # the shipped cap of traj_max_num
def test_c_abi_equals_the_restatement(pt, K, n):
    f, m = seeded_encoder_inputs(K, n, 2000 + K + n)
    assert max_err(raw_encode(pt, f, m), encoder_np(f, m, pt.W)) <= pt.tol


def test_rows_with_one_valid_token(pt):
    f, m = seeded_encoder_inputs(30, 10, 9)
    for k in range(30):
        m[k] = 1.0
        m[k, k % 10] = 0.0
    assert max_err(raw_encode(pt, f, m), encoder_np(f, m, pt.W)) <= pt.tol


def test_rows_permuted_in_are_rows_permuted_out(pt, rows_250):
    f, m, want = rows_250
    perm = np.random.default_rng(5).permutation(250)
    got = raw_encode(pt, f[:, perm], m[perm])
    assert np.array_equal(bits(got), bits(want[:, perm]))


@pytest.mark.parametrize("a", [1, 3, 27, 249])       # cuts inside a wave's six trajectories, inside and past the first block's 24
def test_one_call_equals_two_calls_on_the_halves(pt, rows_250, a):
    f, m, want = rows_250
    got = np.concatenate([raw_encode(pt, f[:, :a], m[:a]), raw_encode(pt, f[:, a:], m[a:])], 1)
    assert np.array_equal(bits(got), bits(want))


def test_two_identical_calls_give_identical_bits(pt, rows_250):
    f, m, want = rows_250
    assert np.array_equal(bits(raw_encode(pt, f, m)), bits(want))


def test_a_fully_padded_row_changes_no_other_row(pt, rows_250):
    """Its own 16 values are unspecified; it must not fault, and every other row keeps its bits."""
    f, m, want = rows_250
    m = m.copy()
    m[100] = 1.0
    got = raw_encode(pt, f, m)
    keep = np.arange(250) != 100
    assert np.array_equal(bits(got[:, keep]), bits(want[:, keep]))


def test_k0_is_a_noop(pt):
    import torch
    out = torch.full((GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    assert raw_call(pt, None, None, None, 0, 10, out) == pt.hip.PSFM_OK
    assert raw_call(pt, None, None, None, 0, 10, None) == pt.hip.PSFM_OK
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    empty = pt.encoder.encode_traj_device(np.zeros((1, 10, 0, 10), np.float32), np.zeros((0, 10, 1)), pt.weights)
    assert tuple(empty.shape) == (1, 16, 0)


def test_argument_errors_launch_nothing(pt):
    import torch
    K, n = 8, 3
    f, m = seeded_encoder_inputs(K, n, 5)
    d_f, d_m, w = torch.from_numpy(f).cuda(), torch.from_numpy(m).cuda(), pt.weights
    big = torch.zeros((10 * K * 65,), dtype=torch.float32, device="cuda")           # (enough for n_frames = 65, were it launched)
    big_m = torch.zeros((K * 65,), dtype=torch.float64, device="cuda")
    out = torch.full((16 * K + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    ERR = pt.hip.PSFM_ERR_ARG
    assert raw_call(pt, None, d_m, w, K, n, out) == ERR
    assert raw_call(pt, d_f, None, w, K, n, out) == ERR
    assert raw_call(pt, d_f, d_m, None, K, n, out) == ERR
    assert raw_call(pt, d_f, d_m, w, K, n, None) == ERR
    assert raw_call(pt, d_f, d_m, w, -1, n, out) == ERR
    assert raw_call(pt, d_f, d_m, w, K, 0, out) == ERR
    assert raw_call(pt, d_f, d_m, w, 0, 0, out) == ERR                  # (n_frames < 1 even with k = 0)
    assert raw_call(pt, d_f, d_m, w, (2 ** 31) // 30 + 1, n, out) == ERR            # 10*k*n_frames >= 2^31
    assert b"psfm_traj_encode" in pt.hip.lib().psfm_last_error()
    assert raw_call(pt, big, big_m, w, K, 65, out) == ERR
    msg = pt.hip.lib().psfm_last_error()
    assert b"psfm_traj_encode" in msg and b"64" in msg                  # the message names the limit
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    with pytest.raises(ValueError, match="64"):
        pt.encoder.encode_traj_device(np.zeros((10, K, 65), np.float32), np.zeros((K, 65)), w)
    with pytest.raises(ValueError):
        pt.encoder.encode_traj_device(f[:9], m, w)
    with pytest.raises(ValueError):
        pt.encoder.encode_traj_device(f, m[:, :2], w)
    with pytest.raises(ValueError):
        pt.encoder.encode_traj_device(f, m, w[:-1])


def test_chained_behind_the_window_sampler_and_augment(pt):
    """run_connect on the 48x64, T = 23 sequence, then window_encoding per window: `features` is window_features' tensor, the
    encoding is the restatement fed those device tensors -- and, for the two windows a fixture holds, the reference's own output."""
    import torch
    from psfm_motion_seg.load_cut_seq import window_ranges
    fx = [golden(ENCODER_CASES[0]), None, golden(ENCODER_CASES[1])]
    want = [encoder_fixture(ENCODER_CASES[0]), None, encoder_fixture(ENCODER_CASES[1])]
    g = fx[0]
    d = regen_inputs(g, stride2=False)
    ff, fb = torch.from_numpy(np.stack(d["flows_f"])).cuda(), torch.from_numpy(np.stack(d["flows_b"])).cuda()
    pt.trajectory.run_connect(ff, fb, None, None, 1.0, int(g["ratio"]), return_device=True)
    ctx = pt.hip.context()
    T, raw_hw, hw = int(g["T"]), (int(g["H"]), int(g["W"])), tuple(int(x) for x in g["input_size"])
    rng = np.random.default_rng(17)
    ranges = window_ranges(T, int(g["window"]))
    assert len(ranges) == 3
    for wi, (f0, n) in enumerate(ranges):
        depth = torch.from_numpy(fx[wi]["depth"] if fx[wi] is not None else rng.uniform(size=(n,) + hw)).cuda()
        ids, raw, mask, feat, enc = pt.encoder.window_encoding(ctx, f0, n, raw_hw, hw, depth, pt.weights, traj_max_num=10 ** 9)
        ids2, raw2, mask2, feat2 = pt.augment.window_features(ctx, f0, n, raw_hw, hw, depth, traj_max_num=10 ** 9)
        assert torch.equal(ids, ids2) and torch.equal(raw, raw2) and torch.equal(mask, mask2) and torch.equal(feat, feat2)
        K = ids.numel()
        assert K > 100 and tuple(enc.shape) == (1, 16, K) and enc.dtype == torch.float32
        assert max_err(enc[0].cpu().numpy(), encoder_np(feat.cpu().numpy(), mask.cpu().numpy(), pt.W)) <= pt.tol
        if fx[wi] is not None:
            assert int(fx[wi]["frame0"]) == f0 and np.array_equal(feat[0].cpu().numpy(), fx[wi]["out"])
            assert max_err(enc[0].cpu().numpy(), want[wi]["out64"]) <= pt.tol
