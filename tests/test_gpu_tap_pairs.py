"""The persistent loop's tap PAIRS (psfm_device.h: the two taps of a row of the backward flow as one 16-byte load, in the fused
flow_check slices) at the smallest shapes at which a pair can go wrong, against the CPU oracle: occlusion masks, ids, lengths and
positions bit for bit, through psfm_track and through the fused psfm_connect, with one launch per frame and with the persistent
frame loop -- and in the second mode the call must report that the persistent loop ran (chain_mode 2), or the slices were not tested.

  * widths 2, 3, 5 x heights 2, 3, 6, sample ratio 1 and 2 (W = 2: every pair is the whole row; W = 3: the two clamped ends
    overlap), with constant flows that put the sampled positions just inside and just outside each border (fractional coordinates
    in (-1, 0) and (W-1, W), the same in y), exactly on it and two pixels outside -- three times: exact, with a distinct offset of a
    few 1/1024 px per pixel, and with a backward field that differs from pixel to pixel by up to 2 px;
  * 24 x 30 (r = 2) and 37 x 53 (r = 3) with random flows of sigma 1.5 px: all four border pick-cases in one run;
  * NaN / +Inf / -Inf in the forward and backward flows at columns 0, 1, W-2, W-1 and rows 0, 1, H-2, H-1.

What these cases can see: the slice's only output is the mask byte (error > 1 px, or sample outside the map).  A sample with a tap
column outside the map is out of bounds whatever its blend, the exact and the 1/1024 px fields have errors far below the threshold, and
a NaN that leaks gives the same verdict as a small error; so a wrong pixel of a pair flips a mask only where neighbouring pixels of
the backward field differ by about the threshold -- the third border variant and the random cases -- or where an Inf leaks.  The
bit-level check of the pick rule is the host test (tests/test_tap_pairs_host.py); this file checks that the device runs it, on the
path that has it, without reading outside the map.

No case is skipped: the oracle runs every shape here, and an error from it fails the test.  The last test prints the count (0)."""
import ctypes

import numpy as np
import pytest

import psfm_synth

pytestmark = pytest.mark.gpu

SMALL = [(H, W, r) for W in (2, 3, 5) for H in (2, 3, 6) for r in (1, 2)]
RANDOM = [(24, 30, 2, 11), (37, 53, 3, 12)]
POISONED = [(6, 5, 1, 21), (24, 30, 2, 22), (37, 53, 3, 23)]

_ref = {}          # case -> (inputs, oracle masks, oracle trajectories): computed once, shared by both chain modes, never modified
_skipped = []      # stays empty: nothing in this file skips


@pytest.fixture(scope="module")
def pt():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from point_trajectory import utils, trajectory, track, _hip
    _hip.context()   # fails loudly if libpsfm_hip.so is missing
    class NS: pass
    ns = NS()
    ns.utils, ns.trajectory, ns.track, ns.hip = utils, trajectory, track.track, _hip
    return ns


@pytest.fixture(autouse=True, params=[1, 2], ids=["per-frame-launches", "persistent-loop"])
def chain_mode(request, pt):
    ctx = pt.hip.context()
    ctx.set_chain_mode(request.param)
    yield request.param
    ctx.set_chain_mode(0)


def border_flows(H, W):
    """One forward / backward pair per constant flow: displacements of 0, a quarter, a half, one, one and three quarters and two
    pixels in both directions along x, along y and along the diagonal.  From the pixels next to a border that is: just inside it,
    exactly on it, just outside (fractional coordinate in (-1, 0) / (size-1, size)) and two pixels outside.  Every constant twice:
    exact, with a distinct offset of a few 1/1024 px per pixel, and with a backward field whose neighbouring pixels differ by up to 2 px
    (errors on both sides of the 1 px threshold: the verdict depends on WHICH pixels are blended)."""
    steps = [0.0, 0.25, -0.25, 0.5, -0.5, 1.0, -1.0, 1.75, -1.75, 2.0, -2.0]
    consts = [(s, 0.0) for s in steps] + [(0.0, s) for s in steps[1:]] + [(s, s) for s in steps[1:]] + [(s, -s) for s in steps[1::2]]
    jit = (np.arange(H * W, dtype=np.float32).reshape(H, W) % 13 - 6.0) / np.float32(1024.0)
    ff, fb = [], []
    rough = ((np.arange(H * W, dtype=np.float32).reshape(H, W) * 7) % 9 - 4.0) / np.float32(4.0)      # -1 .. 1 px, in quarters
    for j in (0, 1, 2):
        for (cx, cy) in consts:
            f = np.empty((H, W, 2), np.float32)
            f[..., 0] = np.float32(cx) + (jit if j == 1 else 0)
            f[..., 1] = np.float32(cy) - (jit.T.reshape(-1)[:H * W].reshape(H, W) if j == 1 else 0)
            ff.append(f)
            b = (-f[::-1, ::-1]).copy() if j == 1 else -f      # (j = 1: a backward field that is no mirror image of the forward one)
            if j == 2:
                b[..., 0] += rough
                b[..., 1] -= rough[::-1, ::-1]
            fb.append(b)
    return ff, fb


def poison_borders(d, seed):
    """NaN / +-Inf into a third of the components of the two outermost columns and rows of every flow field."""
    rng = np.random.default_rng(seed)
    vals = np.array([np.nan, np.inf, -np.inf], np.float32)
    for k in ("flows_f", "flows_b"):
        for a in d[k]:
            H, W = a.shape[:2]
            band = np.zeros((H, W), bool)
            band[:, [0, 1, W - 2, W - 1]] = True
            band[[0, 1, H - 2, H - 1], :] = True
            for (y, x) in np.argwhere(band):
                if rng.uniform() < 1.0 / 3.0:
                    a[y, x, rng.integers(0, 2)] = vals[rng.integers(0, 3)]
    return d


def reference(case, make):
    """(flows_f, flows_b, oracle masks, oracle trajectories) of a case.  An error of the oracle is an error of the test."""
    if case not in _ref:
        from oracle import oracle as orc
        ff, fb = make()
        _, occ = orc.flow_check(ff, fb, 1.0)
        _ref[case] = (ff, fb, occ, orc.track(ff, occ, case[2]))
    return _ref[case]


def connect_with_masks(pt, ff, fb, r, chain_mode):
    """trajectory.run_connect, with the occlusion maps the call computed handed back (psfm_connect's occ_out).  The call must have
    taken the path the fixture asked for: the tap pairs exist only in the persistent loop's slices."""
    import torch
    hip = pt.hip
    ctx = hip.context()
    n, H, W = int(ff.shape[0]), int(ff.shape[1]), int(ff.shape[2])
    occ_out = torch.full((n, H, W), 9, dtype=torch.uint8, device="cuda")
    info = hip.TrackInfo()
    lane_f, traj_f = 2.0, 8.0
    for attempt in range(8):
        ctx.set_capacity(lane_f, traj_f)
        st = hip.lib().psfm_connect(ctx.handle, hip.ptr(ff), hip.ptr(fb), None, None, n, H, W, 1.0, int(r), hip.ptr(occ_out), None,
                                    ctypes.byref(info), hip.current_stream_ptr())
        if st != hip.PSFM_ERR_CAPACITY:
            break
        lane_f, traj_f = lane_f * 2.0, traj_f * 4.0
    hip.check(st)
    assert int(info.chain_mode) == chain_mode, "psfm_connect ran chain mode %d, the test asked for %d" % (int(info.chain_mode), chain_mode)
    R = pt.trajectory._result_to_host(ctx, info)
    ctx.set_capacity(2.0, 8.0)
    return R, occ_out.cpu().numpy()


def check_case(pt, chain_mode, ref, r):
    import torch
    ff, fb, occ, O = ref
    # psfm_track on the oracle's masks: the chain step alone
    R = pt.track(ff, occ, r)
    print("track: %d trajectories, %d points (oracle %d, %d)" % (len(R.birth), len(R.xy), O.n_traj, O.n_points))
    assert np.array_equal(R.birth, O.birth) and np.array_equal(R.length, O.length)
    assert np.array_equal(R.xy.view(np.uint64), O.xy.view(np.uint64))
    # the fused call: masks, then the same trajectories
    dff, dfb = torch.from_numpy(np.stack(ff)).cuda(), torch.from_numpy(np.stack(fb)).cuda()
    C, masks = connect_with_masks(pt, dff, dfb, r, chain_mode)
    ref_masks = np.stack(occ).astype(np.uint8)
    print("connect: %d of %d mask bytes differ" % (int((masks != ref_masks).sum()), masks.size))
    assert np.array_equal(masks, ref_masks)
    assert np.array_equal(C.birth, O.birth) and np.array_equal(C.length, O.length)
    assert np.array_equal(C.xy.view(np.uint64), O.xy.view(np.uint64))
    # the mirror's own entry point gives the same result (and, in track mode, runs the fused persistent loop when asked for it)
    C2 = pt.trajectory.run_connect(dff, dfb, None, None, 1.0, r, return_device=True)
    assert int(C2.n_traj) == O.n_traj and int(C2.n_points) == O.n_points
    assert int(C2.chain_mode) == chain_mode


@pytest.mark.parametrize("H,W,r", SMALL)
def test_border_flows_smallest_shapes(pt, chain_mode, H, W, r):
    ref = reference(("border", H, r, W), lambda: border_flows(H, W))
    check_case(pt, chain_mode, ref, r)


@pytest.mark.parametrize("H,W,r,seed", RANDOM)
def test_random_flows_reach_all_four_borders(pt, chain_mode, H, W, r, seed):
    def make():
        d = psfm_synth.synth_sequence(7, H, W, seed=seed, amp=3.0, sigma=1.5, n_occluders=1, stride2=False)
        return d["flows_f"], d["flows_b"]
    ref = reference(("random", H, r, W, seed), make)
    check_case(pt, chain_mode, ref, r)


@pytest.mark.parametrize("H,W,r,seed", POISONED)
def test_nonfinite_partner_pixels_do_not_leak(pt, chain_mode, H, W, r, seed):
    def make():
        d = poison_borders(psfm_synth.synth_sequence(6, H, W, seed=seed, amp=2.0, sigma=0.5, n_occluders=1, stride2=False), seed + 100)
        return d["flows_f"], d["flows_b"]
    ref = reference(("poisoned", H, r, W, seed), make)
    check_case(pt, chain_mode, ref, r)


def test_zz_report_skipped_cases(pt):
    print("test_gpu_tap_pairs: %d case(s) skipped" % len(_skipped))
    assert _skipped == []
