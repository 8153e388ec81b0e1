"""psfm_traj_eval_counts and psfm_traj_vote_labels (csrc/psfm_ground_truth.hip) on the GPU: exact against the fixtures that the
REFERENCE's own eval_traj_iou.per_img_traj_metrics and prepare_flyingthings3d.find_traj_label produced
(tests/golden/make_ground_truth_golden.py), through psfm_motion_seg.ground_truth and through the raw C ABI (a sentinel guard region
behind every output), and against the NumPy restatement (tests/_ground_truth_np.py, itself pinned to those fixtures by
tests/test_ground_truth_host.py) at the shapes no fixture covers."""
import numpy as np
import pytest

from _common import golden, regen_inputs
from _ground_truth_np import (EVAL_CASES, VOTE_CASES, eval_fixture, frame_counts_np, mask_table, seeded_eval_inputs, seeded_vote_inputs,
                              vote_np)

pytestmark = pytest.mark.gpu
SENTINEL64 = -0x0123456789ABCDEF
SENTINEL8 = 0xA5
GUARD = 4096


@pytest.fixture(scope="module")
def pt():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from point_trajectory import trajectory, _hip
    from psfm_motion_seg import ground_truth
    _hip.context()
    class NS: pass
    ns = NS()
    ns.trajectory, ns.hip, ns.gt = trajectory, _hip, ground_truth
    return ns


def raw_eval_call(pt, fr, xy, lab, n, masks, table, T, h, w, out, ctx=None):
    """psfm_traj_eval_counts with device tensors (or None) as they are; returns the status."""
    ctx = ctx or pt.hip.context()
    table = None if table is None else np.ascontiguousarray(table, np.float32)
    return pt.hip.lib().psfm_traj_eval_counts(ctx.handle, pt.hip.ptr(fr), pt.hip.ptr(xy), pt.hip.ptr(lab), n, pt.hip.ptr(masks),
                                              None if table is None else table.ctypes.data, T, h, w, pt.hip.ptr(out),
                                              pt.hip.current_stream_ptr(ctx.device))


def raw_counts(pt, masks, fr, xy, lab, table=None):
    """Through the C ABI with buffers allocated here (at least one element each, so that no pointer is NULL): (T,4) counts; the guard
    region behind counts_out must come back untouched."""
    import torch
    masks = np.ascontiguousarray(masks, np.uint8)
    T, h, w = masks.shape
    n = len(fr)
    pad = lambda a: np.concatenate([a, np.zeros((1,) + a.shape[1:], a.dtype)])
    d_fr = torch.from_numpy(pad(np.ascontiguousarray(fr, np.int32))).cuda()
    d_xy = torch.from_numpy(pad(np.ascontiguousarray(xy, np.float64).reshape(-1, 2))).cuda()
    d_lab = torch.from_numpy(pad(np.ascontiguousarray(lab, np.uint8))).cuda()
    d_m = torch.from_numpy(masks).cuda()
    out = torch.full((4 * T + GUARD,), SENTINEL64, dtype=torch.int64, device="cuda")
    assert raw_eval_call(pt, d_fr, d_xy, d_lab, n, d_m, mask_table() if table is None else table, T, h, w, out) == pt.hip.PSFM_OK
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert (host[4 * T:] == SENTINEL64).all(), "psfm_traj_eval_counts wrote behind its output"
    return host[:4 * T].reshape(T, 4)


def raw_vote_call(pt, xy, mask, gts, K, L, h, w, out, ctx=None):
    ctx = ctx or pt.hip.context()
    return pt.hip.lib().psfm_traj_vote_labels(ctx.handle, pt.hip.ptr(xy), pt.hip.ptr(mask), pt.hip.ptr(gts), K, L, h, w, pt.hip.ptr(out),
                                              pt.hip.current_stream_ptr(ctx.device))


def raw_vote(pt, xy, mask, gts):
    """Through the C ABI: (status, (K,) labels); the guard region behind labels_out must come back untouched."""
    import torch
    xy = np.ascontiguousarray(xy, np.float64)
    K, L = xy.shape[:2]
    gts = np.ascontiguousarray(gts, np.uint8)
    d_xy = torch.from_numpy(xy).cuda()
    d_m = torch.from_numpy(np.ascontiguousarray(np.asarray(mask, np.float64).reshape(K, L))).cuda()
    d_g = torch.from_numpy(gts).cuda()
    out = torch.full((K + GUARD,), SENTINEL8, dtype=torch.uint8, device="cuda")
    st = raw_vote_call(pt, d_xy, d_m, d_g, K, L, gts.shape[1], gts.shape[2], out)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert (host[K:] == SENTINEL8).all(), "psfm_traj_vote_labels wrote behind its output"
    return st, host[:K]


# ---- the reference's fixtures ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", EVAL_CASES)
def test_eval_module_equals_reference_fixture(pt, name):
    import torch
    g = eval_fixture(name)
    fr, xy, lab = (torch.from_numpy(g[k]).cuda() for k in ("frame_ids", "xy", "labels"))
    counts = pt.gt.frame_counts_device(torch.from_numpy(g["masks"]).cuda(), fr, xy, lab)
    assert counts.dtype == torch.int64 and tuple(counts.shape) == (len(g["masks"]), 4) and counts.is_cuda
    assert np.array_equal(counts.cpu().numpy(), g["counts"])
    # host arrays, a list of maps, bool labels, an explicit table
    counts2 = pt.gt.frame_counts_device(list(g["masks"]), g["frame_ids"], g["xy"], g["labels"].astype(bool), table=mask_table())
    assert torch.equal(counts2, counts)
    # the whole of per_img_traj_metrics: the kept frames and the reference's own metric array
    m = pt.gt.per_img_traj_metrics_device(list(g["masks"]), (fr, xy, lab))
    want = g["metrics"]
    assert m.shape == want.shape and np.array_equal(m[:, 0], want[:, 0]) and np.all(np.abs(m - want) <= 1e-12 * np.abs(want))
    assert np.array_equal(m, pt.gt.seg_metrics_from_counts(g["counts"][g["kept"]]))
    m5 = pt.gt.per_img_traj_metrics_device(list(g["masks"]), (g["ids"], g["off"], g["frame_ids"], g["xy"], g["labels"]))
    assert np.array_equal(m5, m)
    # nothing kept: None (every mask sums to less than 10), whatever the points are
    assert pt.gt.per_img_traj_metrics_device([np.full_like(g["masks"][0], 255)] * len(g["masks"]), (fr, xy, lab)) is None


@pytest.mark.parametrize("name", EVAL_CASES)
def test_eval_c_abi_equals_reference_fixture(pt, name):
    g = eval_fixture(name)
    assert np.array_equal(raw_counts(pt, g["masks"], g["frame_ids"], g["xy"], g["labels"]), g["counts"])


@pytest.mark.parametrize("name", VOTE_CASES)
def test_vote_module_and_c_abi_equal_reference_fixture(pt, name):
    import torch
    g = golden(name)
    out = pt.gt.find_traj_label_device(torch.from_numpy(g["xy"]).cuda(), torch.from_numpy(g["mask"]).cuda(), torch.from_numpy(g["gts"]).cuda())
    assert out.dtype == torch.uint8 and tuple(out.shape) == (len(g["labels"]),) and out.is_cuda
    assert np.array_equal(out.cpu().numpy(), g["labels"])
    out2 = pt.gt.find_traj_label_device(g["xy"], g["mask"][:, :, 0], list(g["gts"]))          # host arrays, a (K,L) mask, a list of maps
    assert torch.equal(out2, out)
    st, got = raw_vote(pt, g["xy"], g["mask"], g["gts"])
    assert st == pt.hip.PSFM_OK and np.array_equal(got, g["labels"])


# ---- the restatement at the shapes no fixture covers -------------------------------------------------------------------------------

@pytest.mark.parametrize("n,T,hw", [(0, 3, (5, 7)),           # no point: zeros
                                    (1, 3, (5, 7)),
                                    (65, 4, (5, 7)),          # a wave and one lane
                                    (257, 5, (6, 4)),         # a partial last wave
                                    (100, 1, (5, 7)),         # n_frames = 1
                                    (90, 3, (2, 2)),          # the smallest map the sampler takes
                                    (9001, 7, (11, 13))])     # three blocks, the last one partial
def test_eval_c_abi_equals_the_restatement(pt, n, T, hw):
    masks, fr, xy, lab = seeded_eval_inputs(n, T, hw, 100 + n + T)
    want = frame_counts_np(masks, fr, xy, lab)
    assert want.sum() == n
    assert np.array_equal(raw_counts(pt, masks, fr, xy, lab), want)
    if n == 0:
        assert not pt.gt.frame_counts_device(masks, fr, xy, lab).cpu().numpy().any()


def test_eval_frame_ids_outside_the_stack_and_an_exact_half(pt):
    masks, fr, xy, lab = seeded_eval_inputs(300, 4, (5, 7), 9)
    fr[::7] = -1
    fr[3::11] = 4
    fr[5::13] = np.iinfo(np.int32).min
    want = frame_counts_np(masks, fr, xy, lab)
    assert want.sum() == int(((fr >= 0) & (fr < 4)).sum()) < 300
    assert np.array_equal(raw_counts(pt, masks, fr, xy, lab), want)
    # table {0, 1}, points midway between a 1-pixel and a 0-pixel: the sample is exactly 0.5f, gt = false
    table = (np.arange(256) != 0).astype(np.float32)
    mask = np.zeros((1, 3, 5), np.uint8)
    mask[0, 1, 1] = 1
    xy = np.array([[1.5, 1.0], [1.0, 1.5], [1.0, 1.0], [1.25, 1.0], [1.75, 1.0]])
    got = raw_counts(pt, mask, np.zeros(5, np.int32), xy, np.array([1, 0, 1, 0, 1], np.uint8), table)
    assert got.tolist() == [[1, 2, 1, 1]]


def test_eval_more_frames_than_the_kernels_tile(pt):
    """1030 frames of 2 x 3 masks: the block's LDS histogram covers 256 of them, the other frames' points go to global memory one by
    one; two blocks, whose tiles differ."""
    T, hw, n = 1030, (2, 3), 6000
    masks, fr, xy, lab = seeded_eval_inputs(n, T, hw, 77, margin=1.0)
    fr[:4096] = np.sort(fr[:4096])                   # the first block starts at frame 0, the second wherever its first point is
    want = frame_counts_np(masks, fr, xy, lab)
    assert want.sum() == n and (want.sum(1) > 0).sum() > 900
    assert np.array_equal(raw_counts(pt, masks, fr, xy, lab), want)
    few = slice(0, 300)
    assert np.array_equal(raw_counts(pt, masks, fr[few], xy[few], lab[few]), frame_counts_np(masks, fr[few], xy[few], lab[few]))


def test_eval_two_identical_calls_give_identical_counts(pt):
    g = eval_fixture(EVAL_CASES[0])
    a = raw_counts(pt, g["masks"], g["frame_ids"], g["xy"], g["labels"])
    b = raw_counts(pt, g["masks"], g["frame_ids"], g["xy"], g["labels"])
    assert np.array_equal(a, b) and np.array_equal(a, g["counts"])


@pytest.mark.parametrize("K,L,hw,maxval", [(1, 1, (5, 7), 1), (1, 10, (5, 7), 255), (65, 1, (5, 7), 1), (257, 10, (9, 6), 1), (64, 3, (1, 1), 255)])
def test_vote_c_abi_equals_the_restatement(pt, K, L, hw, maxval):
    xy, mask, gts = seeded_vote_inputs(K, L, hw, 300 + K + L, maxval)
    want, bad = vote_np(xy, mask, gts)
    assert not bad
    st, got = raw_vote(pt, xy, mask, gts)
    assert st == pt.hip.PSFM_OK and np.array_equal(got, want)


# ---- the labelled set in the context -----------------------------------------------------------------------------------------------

def test_eval_of_the_contexts_labelled_set_equals_its_arrays_passed_explicitly(pt):
    """run_connect on the 48x64, T = 23 sequence, label_trajectories with a stub predictor, then frame_ids = xy = labels = NULL: the
    counts are those of merger.finish()'s arrays passed explicitly, and the fixture's (its labelled set is this one)."""
    import torch
    from psfm_motion_seg.merge_labels import label_trajectories
    e = eval_fixture(EVAL_CASES[0])
    g = golden(str(e["source"]))
    d = regen_inputs(g, stride2=False)
    ff, fb = torch.from_numpy(np.stack(d["flows_f"])).cuda(), torch.from_numpy(np.stack(d["flows_b"])).cuda()
    pt.trajectory.run_connect(ff, fb, None, None, 1.0, int(g["ratio"]), return_device=True)
    ctx = pt.hip.context()
    T, H, W = int(g["T"]), int(g["H"]), int(g["W"])
    masks = torch.from_numpy(e["masks"]).cuda()
    out = torch.full((4 * T + GUARD,), SENTINEL64, dtype=torch.int64, device="cuda")
    # a context that never finished a labelled set: PSFM_ERR_ARG, nothing written
    fresh = pt.hip.Context(ctx.device)
    assert raw_eval_call(pt, None, None, None, 0, masks, mask_table(), T, H, W, out, ctx=fresh) == pt.hip.PSFM_ERR_ARG
    assert b"psfm_traj_eval_counts" in pt.hip.lib().psfm_last_error()
    with pytest.raises(pt.hip.PsfmError):
        pt.gt.frame_counts_device(masks, ctx=fresh)
    fresh.close()
    torch.cuda.synchronize()
    assert bool((out == SENTINEL64).all())
    calls = []

    def predict(raw, nor, mask, time_idx):
        calls.append(1)
        return torch.from_numpy(g["w%d_pred" % (len(calls) - 1)].astype(bool)).cuda()
    m = label_trajectories(T, int(g["window"]), (H, W), tuple(int(x) for x in g["input_size"]), 10 ** 9, predict, ctx=ctx)
    ids, off, fr, xy, lab = m.finish()
    assert raw_eval_call(pt, None, None, None, -5, masks, mask_table(), T, H, W, out) == pt.hip.PSFM_OK        # (n_points is ignored)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert (host[4 * T:] == SENTINEL64).all()
    from_ctx = host[:4 * T].reshape(T, 4)
    explicit = pt.gt.frame_counts_device(masks, fr, xy, lab, ctx=ctx).cpu().numpy()
    assert np.array_equal(from_ctx, explicit) and from_ctx.sum() == m.n_points
    assert np.array_equal(from_ctx, e["counts"])
    assert np.array_equal(pt.gt.frame_counts_device(masks, ctx=ctx).cpu().numpy(), explicit)
    want = e["metrics"]
    for arg in (m, None, (fr, xy, lab)):
        got = pt.gt.per_img_traj_metrics_device(list(e["masks"]), arg, ctx=ctx)
        assert got.shape == want.shape and np.array_equal(got[:, 0], want[:, 0]) and np.all(np.abs(got - want) <= 1e-12 * np.abs(want))


def test_vote_chained_behind_the_window_sampler(pt):
    """psfm_connect on the vote fixture's sequence, one window over all of it, find_traj_label_device on the sampler's tensors as they
    are: the window tensors are the fixture's, and so are the labels for both kinds of mask."""
    import psfm_synth
    import torch
    from psfm_motion_seg.load_cut_seq import sample_window_device
    a, b = golden(VOTE_CASES[0]), golden(VOTE_CASES[1])
    L, H, W = a["gts"].shape
    d = psfm_synth.synth_sequence(L, H, W, seed=int(a["seed"]), amp=3.0, sigma=0.3, n_occluders=2, stride2=False)
    ff, fb = torch.from_numpy(np.stack(d["flows_f"])).cuda(), torch.from_numpy(np.stack(d["flows_b"])).cuda()
    pt.trajectory.run_connect(ff, fb, None, None, 1.0, int(a["ratio"]), return_device=True)
    ctx = pt.hip.context()
    ids, raw, _, mask = sample_window_device(ctx, 0, L, (H, W), (H, W), 10 ** 9)
    assert np.array_equal(ids.cpu().numpy(), a["ids"]) and np.array_equal(raw.cpu().numpy(), a["xy"]) and np.array_equal(mask.cpu().numpy(), a["mask"])
    for g in (a, b):
        assert np.array_equal(pt.gt.find_traj_label_device(raw, mask, g["gts"], ctx=ctx).cpu().numpy(), g["labels"])


# ---- status paths ------------------------------------------------------------------------------------------------------------------

def test_eval_argument_errors_launch_nothing(pt):
    import torch
    masks, fr, xy, lab = seeded_eval_inputs(50, 3, (5, 7), 4)
    d_fr, d_xy, d_lab, d_m = (torch.from_numpy(a).cuda() for a in (fr, xy, lab, masks))
    out = torch.full((12 + GUARD,), SENTINEL64, dtype=torch.int64, device="cuda")
    ERR, t = pt.hip.PSFM_ERR_ARG, mask_table()
    assert raw_eval_call(pt, d_fr, d_xy, d_lab, 50, d_m, t, 3, 5, 1, out) == ERR                # w = 1: the sampler divides by (w-1)/2
    assert b"psfm_traj_eval_counts" in pt.hip.lib().psfm_last_error()
    assert raw_eval_call(pt, d_fr, d_xy, d_lab, 50, d_m, t, 3, 1, 7, out) == ERR
    assert raw_eval_call(pt, d_fr, d_xy, d_lab, 50, d_m, t, 3, 0, 7, out) == ERR
    assert raw_eval_call(pt, d_fr, d_xy, d_lab, 50, d_m, t, 0, 5, 7, out) == ERR
    assert raw_eval_call(pt, d_fr, d_xy, d_lab, -1, d_m, t, 3, 5, 7, out) == ERR
    assert raw_eval_call(pt, d_fr, d_xy, d_lab, 50, d_m, t, 3, 32768, 16384, out) == ERR        # 8*h*w = 2^32: the 32-bit byte offsets
    assert raw_eval_call(pt, None, d_xy, d_lab, 50, d_m, t, 3, 5, 7, out) == ERR                # one of the three arrays missing
    assert raw_eval_call(pt, d_fr, None, None, 50, d_m, t, 3, 5, 7, out) == ERR
    assert raw_eval_call(pt, d_fr, d_xy, d_lab, 50, None, t, 3, 5, 7, out) == ERR
    assert raw_eval_call(pt, d_fr, d_xy, d_lab, 50, d_m, None, 3, 5, 7, out) == ERR
    assert raw_eval_call(pt, d_fr, d_xy, d_lab, 50, d_m, t, 3, 5, 7, None) == ERR
    torch.cuda.synchronize()
    assert bool((out == SENTINEL64).all())
    with pytest.raises(ValueError):
        pt.gt.frame_counts_device(masks, fr, xy, None)
    with pytest.raises(ValueError):
        pt.gt.frame_counts_device(masks.astype(np.float32), fr, xy, lab)
    with pytest.raises(ValueError):
        pt.gt.frame_counts_device(masks, fr, xy[:10], lab)


def test_vote_errors_and_the_empty_call(pt):
    """An out-of-image point is a status check only: the kernel compares in f64 before it forms an index, so nothing is read or
    written out of bounds -- the guard region stays as it was."""
    import torch
    K, L, hw = 70, 3, (5, 7)
    xy, mask, gts = seeded_vote_inputs(K, L, hw, 5)
    for point in ((7.5, 2.0), (2.0, -1.0), (np.nan, 1.0), (3e9, 1.0)):
        bad = xy.copy()
        mask[4, 1] = 0.0
        bad[4, 1] = point
        st, _ = raw_vote(pt, bad, mask, gts)
        assert st == pt.hip.PSFM_ERR_ARG and b"psfm_traj_vote_labels" in pt.hip.lib().psfm_last_error()
        with pytest.raises(pt.hip.PsfmError):
            pt.gt.find_traj_label_device(bad, mask, gts)
    mask[4, 1] = 1.0                                  # the same coordinates in a padded slot are never looked at
    st, got = raw_vote(pt, bad, mask, gts)
    assert st == pt.hip.PSFM_OK and np.array_equal(got, vote_np(bad, mask, gts)[0])
    # k = 0 is a no-op; argument errors launch nothing
    out = torch.full((GUARD,), SENTINEL8, dtype=torch.uint8, device="cuda")
    d_xy, d_m, d_g = torch.from_numpy(xy).cuda(), torch.from_numpy(mask).cuda(), torch.from_numpy(gts).cuda()
    OK, ERR = pt.hip.PSFM_OK, pt.hip.PSFM_ERR_ARG
    assert raw_vote_call(pt, None, None, None, 0, L, 5, 7, out) == OK
    assert raw_vote_call(pt, None, None, None, 0, L, 5, 7, None) == OK
    assert raw_vote_call(pt, d_xy, d_m, d_g, -1, L, 5, 7, out) == ERR
    assert raw_vote_call(pt, d_xy, d_m, d_g, K, 0, 5, 7, out) == ERR
    assert raw_vote_call(pt, d_xy, d_m, d_g, K, L, 0, 7, out) == ERR
    assert raw_vote_call(pt, d_xy, d_m, d_g, K, L, 65536, 32768, out) == ERR          # h*w = 2^31
    assert raw_vote_call(pt, None, d_m, d_g, K, L, 5, 7, out) == ERR
    assert raw_vote_call(pt, d_xy, None, d_g, K, L, 5, 7, out) == ERR
    assert raw_vote_call(pt, d_xy, d_m, None, K, L, 5, 7, out) == ERR
    assert raw_vote_call(pt, d_xy, d_m, d_g, K, L, 5, 7, None) == ERR
    torch.cuda.synchronize()
    assert bool((out == SENTINEL8).all())
    assert tuple(pt.gt.find_traj_label_device(np.zeros((0, L, 2)), np.zeros((0, L, 1)), gts).shape) == (0,)
    with pytest.raises(ValueError):
        pt.gt.find_traj_label_device(xy, mask, gts[:2])
    with pytest.raises(ValueError):
        pt.gt.find_traj_label_device(xy[:, :, :1], mask, gts)
