"""The batched front end of the motion classifier on the GPU: psfm_window_sample_batch (csrc/psfm_window_batch.hip),
psfm_traj_augment_batch (csrc/psfm_augment.hip) and psfm_traj_encode_batch (csrc/psfm_encoder.hip).  No new rule: every window's
tensors are compared BYTE FOR BYTE with the single calls on that window alone (sample_window_device, augment_traj_device,
encode_traj_device), the sampled ids also with the NumPy statement tests/_window_batch_np.py; then the stage:
label_trajectories_batched / label_sequences_batched with front="batch" against front="window".
Sequences: (i) 48x64, T = 23 (connect_t23 of tests/test_gpu_decoder.py), (ii) 60x84, T = 18, ratio 2 (psfm_synth, the sequence of
test_device_window_sample_above_the_cap)."""
import ctypes

import numpy as np
import pytest

import _window_batch_np as wb
from test_gpu_decoder import FULL_WINDOWS, connect_t23, pt, window_depths  # noqa: F401 (pt: fixture)
from test_window_sample_cap import _sequence

pytestmark = pytest.mark.gpu
SENT = -12345.0
GUARD = 64              # rows behind every output that must come back untouched
RAW_II, INP_II = (60, 84), (32, 48)


def host(ts):
    return [None if t is None else t.cpu().numpy() for t in ts]


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_window_equal(got, want, what=""):
    assert len(got) == len(want) == 4
    for g, w in zip(got, want):
        assert same_bytes(g, w), what


def raw_sample(pt, ctx, windows, seeds, cap, raw_hw, inp, capacity=None, outputs=True, n_win=None):
    """One call through the C ABI.  Returns (status, k, rows, (ids, raw, nor, mask) device tensors with GUARD sentinel rows behind
    the capacity).  capacity None: plan first (a call of its own) to learn the rows."""
    import torch
    lib, sp = pt.hip.lib(), pt.hip.current_stream_ptr(ctx.device)
    n = len(windows) if n_win is None else n_win
    L = windows[0][1]
    frame0 = (ctypes.c_int * max(len(windows), 1))(*[f0 for f0, _ in windows])
    seed = (ctypes.c_uint64 * max(len(windows), 1))(*seeds)
    k = (ctypes.c_int64 * max(len(windows), 1))(*([-7] * len(windows)))
    args = (n, frame0, L, 3, 3, int(cap), seed, raw_hw[0], raw_hw[1], inp[0], inp[1])
    if not outputs:
        st = lib.psfm_window_sample_batch(ctx.handle, *args, 0, None, None, None, None, k, sp)
        return st, list(k), None, None
    if capacity is None:
        assert lib.psfm_window_sample_batch(ctx.handle, *args, 0, None, None, None, None, k, sp) == pt.hip.PSFM_OK, lib.psfm_last_error()
        capacity = sum(k)
    rows = capacity + GUARD
    ids = torch.full((rows,), -99, dtype=torch.int32, device="cuda")
    raw = torch.full((rows, L, 2), SENT, dtype=torch.float64, device="cuda")
    nor = torch.full((rows, L, 2), SENT, dtype=torch.float64, device="cuda")
    mask = torch.full((rows, L, 1), SENT, dtype=torch.float64, device="cuda")
    st = lib.psfm_window_sample_batch(ctx.handle, *args, capacity, pt.hip.ptr(ids), pt.hip.ptr(raw), pt.hip.ptr(nor), pt.hip.ptr(mask), k, sp)
    torch.cuda.synchronize()
    return st, list(k), capacity, (ids, raw, nor, mask)


def split(k, tensors):
    """The concatenated outputs -> per window host arrays; everything behind the last row must be sentinels."""
    ids, raw, nor, mask = host(tensors)
    total = sum(k)
    assert (ids[total:] == -99).all() and (raw[total:] == SENT).all() and (nor[total:] == SENT).all() and (mask[total:] == SENT).all()
    out, at = [], 0
    for kb in k:
        out.append((ids[at:at + kb], raw[at:at + kb], nor[at:at + kb], mask[at:at + kb]))
        at += kb
    return out


def singles(ctx, windows, seeds, cap, raw_hw, inp):
    from psfm_motion_seg.load_cut_seq import sample_window_device
    return [host(sample_window_device(ctx, f0, n, raw_hw, inp, cap, seed=s)) for (f0, n), s in zip(windows, seeds)]


def connect_ii(pt):
    import torch
    d = _sequence(T=18, H=60, W=84, seed=5)
    ff = torch.from_numpy(np.stack(d["flows_f"])).cuda()
    fb = torch.from_numpy(np.stack(d["flows_b"])).cuda()
    info = pt.trajectory.run_connect(ff, fb, None, None, 1.0, 2, return_device=True)
    return pt.hip.context(), info


WINDOWS_I = [(0, 10), (10, 10), (13, 10), (40, 10)]        # window_ranges(23, 10) and one outside the sequence
WINDOWS_II = [(0, 9), (4, 9), (9, 9)]
SEEDS_II = [0, 1, 1]


def test_sampler_uncapped_equals_the_single_calls(pt):
    from psfm_motion_seg.load_cut_seq import sample_windows_device, window_ranges
    g, ctx = connect_t23(pt)
    raw_hw, hw = (int(g["H"]), int(g["W"])), tuple(int(x) for x in g["input_size"])
    assert window_ranges(int(g["T"]), 10) == WINDOWS_I[:3]
    want = singles(ctx, WINDOWS_I, [0] * 4, 10 ** 9, raw_hw, hw)
    st, k, _, tensors = raw_sample(pt, ctx, WINDOWS_I, [0] * 4, 10 ** 9, raw_hw, hw)
    assert st == pt.hip.PSFM_OK, pt.hip.lib().psfm_last_error()
    assert k[3] == 0 and all(kb > 100 for kb in k[:3]) and k == [len(w[0]) for w in want]
    got = split(k, tensors)
    for b in range(4):
        assert_window_equal(got[b], want[b], "window %d" % b)
    assert len({tuple(w[0].tolist()) for w in got[:3]}) == 3              # the windows' id sets differ
    views = sample_windows_device(ctx, WINDOWS_I, raw_hw, hw, traj_max_num=10 ** 9, seeds=[0] * 4)
    for b, v in enumerate(views):
        assert all(t.is_contiguous() for t in v)
        assert_window_equal(host(v), want[b], "module, window %d" % b)
    ids, raw, nor, mask = sample_windows_device(ctx, WINDOWS_I[:1], raw_hw, hw, traj_max_num=10 ** 9, normalise=False)[0]
    assert nor is None and same_bytes(ids.cpu().numpy(), want[0][0]) and same_bytes(mask.cpu().numpy(), want[0][3])


def test_sampler_capped_equals_the_single_calls_and_the_numpy_statement(pt):
    ctx, info = connect_ii(pt)
    R = pt.trajectory._result_to_host(ctx, info)
    uncapped = singles(ctx, WINDOWS_II, SEEDS_II, 10 ** 9, RAW_II, INP_II)
    counts = [len(w[0]) for w in uncapped]
    K_min = min(counts)
    assert K_min // 4 > 25 and max(counts) > 300
    for cap in (K_min // 4, 25, 1, counts[0]):
        want = singles(ctx, WINDOWS_II, SEEDS_II, cap, RAW_II, INP_II)
        st, k, _, tensors = raw_sample(pt, ctx, WINDOWS_II, SEEDS_II, cap, RAW_II, INP_II)
        assert st == pt.hip.PSFM_OK, pt.hip.lib().psfm_last_error()
        assert k == [min(c, cap) for c in counts]
        got = split(k, tensors)
        k_np, row0, ids_np, raw_np, mask_np, nor_np = wb.sample_windows_np(R.birth, R.length, R.off, R.xy, WINDOWS_II, SEEDS_II, cap,
                                                                         raw_hw=RAW_II, input_size=INP_II)
        assert k_np.tolist() == k
        for b in range(3):
            assert_window_equal(got[b], want[b], "cap %d window %d" % (cap, b))
            lo, hi = row0[b], row0[b + 1]
            assert np.array_equal(got[b][0], ids_np[lo:hi])
            assert np.array_equal(got[b][1], raw_np[lo:hi]) and np.array_equal(got[b][3][:, :, 0], mask_np[lo:hi])
            assert np.array_equal(got[b][2], nor_np[lo:hi])
        if cap == counts[0]:                                             # at the cap, not above it: untouched, ascending
            assert np.array_equal(got[0][0], uncapped[0][0]) and np.array_equal(got[0][0], np.sort(got[0][0]))
            assert any(c > cap for c in counts[1:]) or all(np.array_equal(got[b][0], uncapped[b][0]) for b in (1, 2))
        elif cap > 1:
            assert not np.array_equal(got[0][0], np.sort(got[0][0]))    # a shuffle, not the first rows
    # the same window with another seed picks another subset
    st, k, _, tensors = raw_sample(pt, ctx, [WINDOWS_II[1]] * 2, [1, 2], K_min // 4, RAW_II, INP_II)
    a, b = split(k, tensors)
    assert set(a[0].tolist()) != set(b[0].tolist())


def test_plan_and_fill_protocol(pt):
    import torch
    from psfm_motion_seg.load_cut_seq import sample_window_device
    lib = pt.hip.lib()
    g, ctx = connect_t23(pt)
    raw_hw, hw = (int(g["H"]), int(g["W"])), tuple(int(x) for x in g["input_size"])
    wins, seeds, cap = WINDOWS_I, [3, 4, 5, 6], 150                      # (window 0 has more than 150: one capped window in the plan)
    st, k_plan, _, _ = raw_sample(pt, ctx, wins, seeds, cap, raw_hw, hw, outputs=False)
    assert st == pt.hip.PSFM_OK and k_plan[3] == 0 and max(k_plan) == cap
    total = sum(k_plan)
    st, k1, _, t1 = raw_sample(pt, ctx, wins, seeds, cap, raw_hw, hw, capacity=total)           # fill from the kept plan
    st2, k2, _, t2 = raw_sample(pt, ctx, wins, seeds, cap, raw_hw, hw, capacity=total)          # and again
    assert st == st2 == pt.hip.PSFM_OK and k1 == k2 == k_plan
    for a, b in zip(host(t1), host(t2)):
        assert same_bytes(a, b)
    want = singles(ctx, wins, seeds, cap, raw_hw, hw)                    # (single calls in between do not disturb the kept plan)
    st3, k3, _, t3 = raw_sample(pt, ctx, wins, seeds, cap, raw_hw, hw, capacity=total)
    assert st3 == pt.hip.PSFM_OK
    for got in (split(k1, t1), split(k3, t3)):
        for b in range(4):
            assert_window_equal(got[b], want[b], "window %d" % b)
    # one row too few: refused, nothing written
    st, k, _, t = raw_sample(pt, ctx, wins, seeds, cap, raw_hw, hw, capacity=total - 1)
    assert st == pt.hip.PSFM_ERR_CAPACITY, lib.psfm_last_error()
    ids, raw, nor, mask = host(t)
    assert (ids == -99).all() and (raw == SENT).all() and (nor == SENT).all() and (mask == SENT).all()
    # a new result on the context: the old arguments, the NEW result
    ctx2, _ = connect_ii(pt)
    assert ctx2.handle == ctx.handle
    st, k, _, t = raw_sample(pt, ctx, wins, seeds, cap, raw_hw, hw, capacity=4 * cap)
    assert st == pt.hip.PSFM_OK, lib.psfm_last_error()
    want_new = singles(ctx, wins, seeds, cap, raw_hw, hw)
    assert k == [len(w[0]) for w in want_new] and not same_bytes(want_new[0][1], want[0][1])       # (the results differ)
    got = split(k, t)
    for b in range(4):
        assert_window_equal(got[b], want_new[b], "new result, window %d" % b)
    # one seed changed: a plan of its own
    seeds2 = [3, 4, 5, 6]
    seeds2[0] = 77
    st, k, _, t = raw_sample(pt, ctx, wins, seeds2, cap, raw_hw, hw, capacity=4 * cap)
    assert st == pt.hip.PSFM_OK
    want2 = singles(ctx, wins, seeds2, cap, raw_hw, hw)
    got = split(k, t)
    assert len(want2[0][0]) == cap and not np.array_equal(want2[0][0], want_new[0][0])        # (the changed seed matters here)
    for b in range(4):
        assert_window_equal(got[b], want2[b], "changed seed, window %d" % b)


def test_64_windows_in_one_call_and_more_through_the_module(pt):
    from psfm_motion_seg.load_cut_seq import sample_windows_device
    lib = pt.hip.lib()
    g, ctx = connect_t23(pt)
    raw_hw, hw = (int(g["H"]), int(g["W"])), tuple(int(x) for x in g["input_size"])
    wins = [(b % 14, 10) for b in range(65)]
    want = singles(ctx, wins[:14], [0] * 14, 10 ** 9, raw_hw, hw)
    st, k, _, tensors = raw_sample(pt, ctx, wins[:64], [0] * 64, 10 ** 9, raw_hw, hw)
    assert st == pt.hip.PSFM_OK, lib.psfm_last_error()
    got = split(k, tensors)
    for b in range(64):
        assert_window_equal(got[b], want[b % 14], "window %d" % b)
    st, _, _, _ = raw_sample(pt, ctx, wins, [0] * 65, 10 ** 9, raw_hw, hw, outputs=False)
    assert st == pt.hip.PSFM_ERR_ARG and b"n_win=65" in lib.psfm_last_error()
    views = sample_windows_device(ctx, wins, raw_hw, hw, traj_max_num=10 ** 9)
    assert len(views) == 65
    for b in (0, 13, 14, 63, 64):
        assert_window_equal(host(views[b]), want[b % 14], "module, window %d" % b)


@pytest.fixture(scope="module")
def front_tensors(pt):
    """Windows of (i) as (nor, mask) device tensors, all of L = 10 (one call takes one n_frames): the three windows of hundreds of
    rows and the empty one, two windows capped at 25 rows (one more than an encoder block of 24 trajectories) and one capped at 1;
    and (i) as ONE window of 23 frames (two trajectories per wave)."""
    import torch
    from psfm_motion_seg.load_cut_seq import sample_windows_device
    g, ctx = connect_t23(pt)
    raw_hw, hw = (int(g["H"]), int(g["W"])), tuple(int(x) for x in g["input_size"])
    wins = [(n, m) for _, _, n, m in sample_windows_device(ctx, WINDOWS_I, raw_hw, hw, traj_max_num=10 ** 9)]
    wins += [(n, m) for _, _, n, m in sample_windows_device(ctx, [(5, 10), (11, 10)], raw_hw, hw, traj_max_num=25, seeds=[1, 2])]
    wins += [(n, m) for _, _, n, m in sample_windows_device(ctx, [(8, 10)], raw_hw, hw, traj_max_num=1, seeds=[9])]
    whole = [(n, m) for _, _, n, m in sample_windows_device(ctx, [(0, 23)], raw_hw, hw, traj_max_num=10 ** 9)]
    ks = [int(n.shape[0]) for n, _ in wins]
    assert ks[3] == 0 and ks[4:] == [25, 25, 1] and min(ks[:3]) > 100 and whole[0][0].shape[0] > 100
    rng = np.random.default_rng(29)
    _, depth_of = window_depths(hw)
    depths = [depth_of(b, 10) if b < 3 else torch.from_numpy(rng.uniform(0.1, 4.0, size=(10,) + hw).astype(np.float32)).cuda() for b in range(len(wins))]
    depth23 = torch.from_numpy(rng.uniform(0.1, 4.0, size=(23,) + hw).astype(np.float32)).cuda()
    return hw, wins, depths, whole, depth23


def bits(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_augment_and_encoder_batches_equal_the_single_calls(pt, front_tensors, order):
    hw, wins, depths, whole, depth23 = front_tensors
    idx = list(range(len(wins)))[::-1] if order == "reversed" else list(range(len(wins)))
    nors, masks, deps = [wins[i][0] for i in idx], [wins[i][1] for i in idx], [depths[i] for i in idx]
    feats = pt.augment.augment_windows_device(nors, masks, deps, hw)
    encs = pt.encoder.encode_windows_device(feats, masks, pt.enc_weights)
    for n, m, d, f, e in zip(nors, masks, deps, feats, encs):
        K = int(n.shape[0])
        assert tuple(f.shape) == (1, 10, K, 10) and tuple(e.shape) == (1, 16, K) and f.is_contiguous() and e.is_contiguous()
        f1 = pt.augment.augment_traj_device(n, m, d, hw)
        e1 = pt.encoder.encode_traj_device(f1, m, pt.enc_weights)
        assert np.array_equal(bits(f), bits(f1)) and np.array_equal(bits(e), bits(e1)), K
        assert K == 0 or np.isfinite(e.cpu().numpy()).all()
    # one window alone, and the window of 23 frames (window >= length)
    for (n, m), d in ((wins[0], depths[0]), (wins[5], depths[5]), (whole[0], depth23)):
        f, = pt.augment.augment_windows_device([n], [m], [d], hw)
        e, = pt.encoder.encode_windows_device([f], [m], pt.enc_weights)
        f1 = pt.augment.augment_traj_device(n, m, d, hw)
        assert np.array_equal(bits(f), bits(f1)) and np.array_equal(bits(e), bits(pt.encoder.encode_traj_device(f1, m, pt.enc_weights)))


def raw_front_call(pt, which, n_win, a, b, c, ks, L, outs, hw=(30, 50)):
    """psfm_traj_augment_batch (a, b, c = xy, mask, depth) or psfm_traj_encode_batch (a, b = features, mask; c = weights) as it stands:
    lists of tensors (None: a NULL entry) or None (a NULL array)."""
    vp = ctypes.c_void_p
    col = lambda ts: None if ts is None else (vp * max(len(ts), 1))(*[None if t is None else t.data_ptr() for t in ts])
    ctx = pt.hip.context()
    k = (ctypes.c_int64 * max(len(ks), 1))(*ks)
    sp = pt.hip.current_stream_ptr(ctx.device)
    if which == "augment":
        kinv = np.ascontiguousarray(pt.augment.reference_kinv(hw))
        return pt.hip.lib().psfm_traj_augment_batch(ctx.handle, n_win, col(a), col(b), col(c), k, L, hw[0], hw[1], kinv.ctypes.data, col(outs), sp)
    return pt.hip.lib().psfm_traj_encode_batch(ctx.handle, n_win, col(a), col(b), pt.hip.ptr(c), k, L, col(outs), sp)


def test_empty_batches_and_refusals_launch_nothing(pt, front_tensors):
    import torch
    hw, wins, depths, _, _ = front_tensors
    lib, OK, ERR = pt.hip.lib(), pt.hip.PSFM_OK, pt.hip.PSFM_ERR_ARG
    n, m, d = wins[4][0], wins[4][1], depths[4]                          # k = 25, L = 10
    K = int(n.shape[0])
    feat = pt.augment.augment_traj_device(n, m, d, hw)[0].contiguous()
    out_a = torch.full((10 * K * 10 + 64,), SENT, dtype=torch.float32, device="cuda")
    out_e = torch.full((16 * K + 64,), SENT, dtype=torch.float32, device="cuda")
    w = pt.enc_weights
    for which, a, b, c, out in (("augment", n, m, d, out_a), ("encode", feat, m, w, out_e)):
        third = (lambda cnt: [c] * cnt) if which == "augment" else (lambda cnt: c)
        assert raw_front_call(pt, which, 0, None, None, third(0) if which == "encode" else None, [], 10, None, hw) == OK
        assert raw_front_call(pt, which, 0, [a], [b], third(1), [K], 10, [out], hw) == OK
        assert raw_front_call(pt, which, 3, [None] * 3, [None] * 3, third(3), [0, 0, 0], 10, [out] * 3, hw) == OK
        assert raw_front_call(pt, which, 64, [a] * 64, [b] * 64, third(64), [0] * 64, 10, [out] * 64, hw) == OK
        assert raw_front_call(pt, which, 65, [a] * 65, [b] * 65, third(65), [K] * 65, 10, [out] * 65, hw) == ERR
        assert b"n_win=65" in lib.psfm_last_error()
        assert raw_front_call(pt, which, -1, [a], [b], third(1), [K], 10, [out], hw) == ERR
        assert raw_front_call(pt, which, 3, [a, None, a], [b, b, b], third(3), [K, K, K], 10, [out] * 3, hw) == ERR
        assert b"window 1" in lib.psfm_last_error()
        assert raw_front_call(pt, which, 3, [a, a, a], [b, b, b], third(3), [K, K, K], 10, [out, out, None], hw) == ERR
        assert b"window 2" in lib.psfm_last_error()
        assert raw_front_call(pt, which, 2, [a, a], [b, b], third(2), [K, -1], 10, [out, out], hw) == ERR
        assert b"window 1" in lib.psfm_last_error()
        assert raw_front_call(pt, which, 1, [a], [b], third(1), [K], 0, [out], hw) == ERR
    assert raw_front_call(pt, "encode", 1, [feat], [m], w, [K], 65, [out_e], hw) == ERR
    assert b"n_frames=65" in lib.psfm_last_error()
    assert raw_front_call(pt, "encode", 1, [feat], [m], None, [K], 10, [out_e], hw) == ERR
    assert raw_front_call(pt, "augment", 1, [n], [m], [None], [K], 10, [out_a], hw) == ERR
    torch.cuda.synchronize()
    assert bool((out_a == SENT).all()) and bool((out_e == SENT).all())
    assert pt.augment.augment_windows_device([], [], [], hw) == [] and pt.encoder.encode_windows_device([], [], w) == []
    # a window that is skipped leaves its output alone; its neighbours are written
    assert raw_front_call(pt, "encode", 3, [feat, None, feat], [m, None, m], w, [K, 0, K], 10, [out_e[:16 * K], out_e, out_e[:16 * K]], hw) == OK
    torch.cuda.synchronize()
    assert bool((out_e[16 * K:] == SENT).all()) and np.array_equal(bits(out_e[:16 * K]), bits(pt.encoder.encode_traj_device(feat, m, w)).ravel())


def finished(m):
    return [t.cpu().numpy() for t in m.finish()]


def assert_sets_equal(got, want):
    assert len(got) == len(want) == 5
    for a, b in zip(got, want):
        assert same_bytes(a, b)


@pytest.mark.parametrize("traj_max_num", [10 ** 9, 100])
def test_label_trajectories_batched_front_batch_equals_front_window(pt, traj_max_num):
    from psfm_motion_seg.load_cut_seq import window_ranges
    from psfm_motion_seg.merge_labels import label_trajectories_batched
    g, ctx = connect_t23(pt)
    T, raw_hw, hw, window = int(g["T"]), (int(g["H"]), int(g["W"])), tuple(int(x) for x in g["input_size"]), int(g["window"])
    _, depth_of = window_depths(hw)
    depth = {f0: depth_of(wi, n) for wi, (f0, n) in enumerate(window_ranges(T, window))}
    calls = []

    def depth_for_window(time_idx):
        calls.append(int(time_idx[0]))
        return depth[int(time_idx[0])]
    args = (T, window, raw_hw, hw, traj_max_num, pt.enc_weights, pt.weights, depth_for_window)
    mw = label_trajectories_batched(*args, seed=3, ctx=ctx)
    want, want_ids, calls_w = finished(mw), [t.cpu().numpy() for t in mw.window_ids], list(calls)
    del calls[:]
    mb = label_trajectories_batched(*args, seed=3, ctx=ctx, front="batch")
    assert calls == calls_w == [f0 for f0, _ in window_ranges(T, window)]
    assert_sets_equal(finished(mb), want)
    got_ids = [t.cpu().numpy() for t in mb.window_ids]
    assert len(got_ids) == len(want_ids) == 3 and all(same_bytes(a, b) for a, b in zip(got_ids, want_ids))
    rows = [len(i) for i in want_ids]
    assert len(want[0]) > 0 and (rows == [100] * 3 if traj_max_num == 100 else min(rows) > 100)
    with pytest.raises(ValueError):
        label_trajectories_batched(*args, seed=3, ctx=ctx, front="rows")


def test_label_sequences_batched_front_batch_equals_front_window(pt):
    import torch
    from _common import golden, regen_inputs
    from psfm_motion_seg.merge_labels import label_sequences_batched
    g = golden(FULL_WINDOWS[0])
    d = regen_inputs(g, stride2=False)
    ff, fb = torch.from_numpy(np.stack(d["flows_f"])).cuda(), torch.from_numpy(np.stack(d["flows_b"])).cuda()
    raw_hw, hw, window = (int(g["H"]), int(g["W"])), tuple(int(x) for x in g["input_size"]), int(g["window"])
    lengths = [int(g["T"]), 16]
    ctxs, infos = pt.trajectory.run_connect_batch([(ff, fb, None, None), (ff[:15].contiguous(), fb[:15].contiguous(), None, None)], 1.0,
                                                  int(g["ratio"]))
    rng = np.random.default_rng(23)
    depth = {}

    def depth_for_window(seq, time_idx):
        key = (seq, int(time_idx[0]))
        if key not in depth:
            depth[key] = torch.from_numpy(rng.uniform(size=(len(time_idx),) + hw).astype(np.float32)).cuda()
        return depth[key]
    args = (ctxs, lengths, window, raw_hw, hw, 10 ** 9, pt.enc_weights, pt.weights, depth_for_window)
    want = [(finished(m), [t.cpu().numpy() for t in m.window_ids]) for m in label_sequences_batched(*args, seed=5)]
    got = [(finished(m), [t.cpu().numpy() for t in m.window_ids]) for m in label_sequences_batched(*args, seed=5, front="batch")]
    assert [len(ids) for _, ids in got] == [3, 2]
    for (gs, gi), (ws, wi) in zip(got, want):
        assert_sets_equal(gs, ws)
        assert all(same_bytes(a, b) for a, b in zip(gi, wi))
    assert len(got[0][0][0]) > 0 and not np.array_equal(got[0][0][0], got[1][0][0])
