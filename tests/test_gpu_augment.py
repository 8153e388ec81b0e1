"""psfm_traj_augment (csrc/psfm_augment.hip) on the GPU: the motion classifier's 10-channel input, bit for bit against the
fixtures the REFERENCE's own traj_oa_depth.augment_traj produced (tests/golden/make_augment_golden.py), through
psfm_motion_seg.augment and through the raw C ABI, and against the NumPy restatement (tests/_augment_np.py, itself pinned to those
fixtures by tests/test_augment_host.py) at the shapes no fixture covers: L = 1, L = 2, a partial last wave and block, and the
shipped configuration's 100 000 x 10 window at (240,424)."""

import numpy as np
import pytest

from _augment_np import AUGMENT_CASES, augment_np, seeded_inputs
from _common import golden, regen_inputs

pytestmark = pytest.mark.gpu
SENTINEL = -12345.0
GUARD = 4096


@pytest.fixture(scope="module")
def pt():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from point_trajectory import trajectory, _hip
    from psfm_motion_seg import augment
    _hip.context()
    class NS: pass
    ns = NS()
    ns.trajectory, ns.hip, ns.augment = trajectory, _hip, augment
    return ns


def raw_call(pt, xy, mask, depth, K, n, h, w, kinv, out, ctx=None):
    """psfm_traj_augment with device tensors (or None) as they are; returns the status."""
    ctx = ctx or pt.hip.context()
    kinv = None if kinv is None else np.ascontiguousarray(kinv, np.float32)
    return pt.hip.lib().psfm_traj_augment(ctx.handle, pt.hip.ptr(xy), pt.hip.ptr(mask), pt.hip.ptr(depth), K, n, h, w,
                                          None if kinv is None else kinv.ctypes.data, pt.hip.ptr(out), pt.hip.current_stream_ptr(ctx.device))


def raw_augment(pt, xy, mask, depth, hw, kinv):
    """Through the C ABI with buffers allocated here: (10,K,L) result; the guard region behind `out` must come back untouched."""
    import torch
    K, n = xy.shape[:2]
    d_xy = torch.from_numpy(np.ascontiguousarray(xy, np.float64)).cuda()
    d_m = torch.from_numpy(np.ascontiguousarray(np.asarray(mask, np.float64).reshape(K, n))).cuda()
    d_d = torch.from_numpy(np.ascontiguousarray(depth, np.float32)).cuda()
    out = torch.full((10 * K * n + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    assert raw_call(pt, d_xy, d_m, d_d, K, n, int(hw[0]), int(hw[1]), kinv, out) == pt.hip.PSFM_OK
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert (host[10 * K * n:] == SENTINEL).all(), "psfm_traj_augment wrote behind its output"
    return host[:10 * K * n].reshape(10, K, n)


def assert_channels_equal(got, want):
    assert got.shape == want.shape and got.dtype == np.float32
    for c in range(10):
        assert np.array_equal(got[c], want[c]), "channel %d: %d of %d differ" % (c, int((got[c] != want[c]).sum()), got[c].size)


@pytest.mark.parametrize("name", AUGMENT_CASES)
def test_module_equals_reference_fixture(pt, name):
    import torch
    g = golden(name)
    hw = tuple(int(x) for x in g["input_size"])
    xy, mask = torch.from_numpy(g["traj"]).cuda(), torch.from_numpy(g["mask"]).cuda()       # f64 (K,L,2), (K,L,1): the sampler's form
    out = pt.augment.augment_traj_device(xy, mask, torch.from_numpy(g["depth"]).cuda(), hw)     # f64 (L,h,w) depth: rounded on the device
    assert tuple(out.shape) == (1, 10) + g["traj"].shape[:2] and out.dtype == torch.float32 and out.is_contiguous()
    assert_channels_equal(out[0].cpu().numpy(), g["out"])
    # the other accepted forms: a list of maps, the reference's (1,1,h,w,L) tensor, an explicit kinv, a (K,L) mask, host arrays
    ref5 = torch.from_numpy(g["depth"]).float().permute(1, 2, 0)[None, None]
    for depth, m in ((list(g["depth"]), mask[:, :, 0]), (ref5, g["mask"])):
        out2 = pt.augment.augment_traj_device(g["traj"], m, depth, hw, kinv=g["kinv"])
        assert torch.equal(out2, out)


def test_f32_window_tensors_are_widened_exactly(pt):
    import torch
    g = golden(AUGMENT_CASES[3])
    hw = tuple(int(x) for x in g["input_size"])
    xy32, m32 = g["traj"].astype(np.float32), g["mask"].astype(np.float32)
    out = pt.augment.augment_traj_device(torch.from_numpy(xy32).cuda(), torch.from_numpy(m32).cuda(), g["depth"].astype(np.float32), hw)
    assert_channels_equal(out[0].cpu().numpy(), augment_np(xy32, m32, g["depth"], hw, g["kinv"]))


@pytest.mark.parametrize("name", AUGMENT_CASES)
def test_c_abi_equals_reference_fixture(pt, name):
    g = golden(name)
    assert_channels_equal(raw_augment(pt, g["traj"], g["mask"], g["depth"], g["input_size"], g["kinv"]), g["out"])


@pytest.mark.parametrize("K,n,hw", [(65, 1, (30, 50)),          # L = 1: no motion, nothing read past a row
                                    (1, 2, (30, 50)),           # one trajectory, one motion
                                    (257, 10, (30, 50)),        # 2570 elements: a partial last wave and block
                                    (64, 4, (1, 1)),            # every index clamps to the one pixel
                                    (100000, 10, (240, 424))])  # the shipped configuration's resolution and the cap of traj_max_num: 3907 blocks
def test_c_abi_equals_the_restatement(pt, K, n, hw):
    xy, mask, depth = seeded_inputs(K, n, hw, 1000 + K + n)
    kinv = pt.augment.reference_kinv(hw)
    got = raw_augment(pt, xy, mask, depth, hw, kinv)
    assert_channels_equal(got, augment_np(xy, mask, depth, hw, kinv))
    if n == 1:
        assert not got[[2, 3, 7, 8, 9]].any()
    assert not got[[2, 3, 7, 8, 9], :, n - 1].any()          # the last frame's motion is 0


def test_k0_is_a_noop(pt):
    import torch
    out = torch.full((GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    assert raw_call(pt, None, None, None, 0, 10, 30, 50, None, out) == pt.hip.PSFM_OK
    assert raw_call(pt, None, None, None, 0, 10, 30, 50, None, None) == pt.hip.PSFM_OK
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    empty = pt.augment.augment_traj_device(np.zeros((0, 10, 2)), np.zeros((0, 10, 1)), np.zeros((10, 30, 50), np.float32), (30, 50))
    assert tuple(empty.shape) == (1, 10, 0, 10)


def test_argument_errors_launch_nothing(pt):
    import torch
    K, n, hw = 8, 3, (5, 7)
    xy, mask, depth = seeded_inputs(K, n, hw, 5)
    d_xy, d_m = torch.from_numpy(xy).cuda(), torch.from_numpy(mask).cuda()
    d_d = torch.from_numpy(depth.astype(np.float32)).cuda()
    kinv = pt.augment.reference_kinv(hw)
    out = torch.full((10 * K * n + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    ERR = pt.hip.PSFM_ERR_ARG
    assert raw_call(pt, None, d_m, d_d, K, n, 5, 7, kinv, out) == ERR
    assert raw_call(pt, d_xy, None, d_d, K, n, 5, 7, kinv, out) == ERR
    assert raw_call(pt, d_xy, d_m, None, K, n, 5, 7, kinv, out) == ERR
    assert raw_call(pt, d_xy, d_m, d_d, K, n, 5, 7, None, out) == ERR
    assert raw_call(pt, d_xy, d_m, d_d, K, n, 5, 7, kinv, None) == ERR
    assert raw_call(pt, d_xy, d_m, d_d, -1, n, 5, 7, kinv, out) == ERR
    assert raw_call(pt, d_xy, d_m, d_d, K, 0, 5, 7, kinv, out) == ERR
    assert raw_call(pt, d_xy, d_m, d_d, 0, 0, 5, 7, kinv, out) == ERR            # (n_frames < 1 even with k = 0)
    assert raw_call(pt, d_xy, d_m, d_d, K, n, 0, 7, kinv, out) == ERR
    assert raw_call(pt, d_xy, d_m, d_d, K, n, 5, -2, kinv, out) == ERR
    assert raw_call(pt, d_xy, d_m, d_d, K, n, 65536, 32768, kinv, out) == ERR    # h*w = 2^31
    assert raw_call(pt, d_xy, d_m, d_d, (2 ** 31) // 30 + 1, n, 5, 7, kinv, out) == ERR      # 10*k*n_frames >= 2^31
    assert b"psfm_traj_augment" in pt.hip.lib().psfm_last_error()
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    with pytest.raises(ValueError):
        pt.augment.augment_traj_device(xy, mask, depth[:2], hw)
    with pytest.raises(ValueError):
        pt.augment.augment_traj_device(xy[:, :, :1], mask, depth, hw)


def test_chained_behind_the_window_sampler(pt):
    """run_connect on the 48x64, T = 23 sequence, then window_features per window: channels 0-1 are xy_norm.float(), the whole
    tensor is the restatement fed the same device tensors -- and, for the two windows a fixture holds, the reference's own output."""
    import torch
    from psfm_motion_seg.load_cut_seq import sample_window_device, window_ranges
    fx = [golden(AUGMENT_CASES[0]), None, golden(AUGMENT_CASES[1])]
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
        depth = fx[wi]["depth"] if fx[wi] is not None else rng.uniform(size=(n,) + hw)
        ids, raw, mask, feat = pt.augment.window_features(ctx, f0, n, raw_hw, hw, torch.from_numpy(depth).cuda(), traj_max_num=10 ** 9)
        ids2, raw2, nor2, mask2 = sample_window_device(ctx, f0, n, raw_hw, hw, 10 ** 9)
        assert torch.equal(ids, ids2) and torch.equal(raw, raw2) and torch.equal(mask, mask2)
        K = ids.numel()
        assert K > 100 and tuple(feat.shape) == (1, 10, K, n)
        assert torch.equal(feat[0, :2], nor2.float().permute(2, 0, 1))
        assert_channels_equal(feat[0].cpu().numpy(), augment_np(nor2.cpu().numpy(), mask2.cpu().numpy(), depth, hw, pt.augment.reference_kinv(hw)))
        if fx[wi] is not None:
            assert int(fx[wi]["frame0"]) == f0 and np.array_equal(nor2.cpu().numpy(), fx[wi]["traj"])
            assert_channels_equal(feat[0].cpu().numpy(), fx[wi]["out"])
