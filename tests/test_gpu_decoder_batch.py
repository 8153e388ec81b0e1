"""psfm_traj_decode_batch (csrc/psfm_decoder.hip, psfm_decoder_batch.h) on the GPU: the windows of a sequence through ONE sequence of
decoder launches.  Pinned twice: to the REFERENCE (every SMALL_CASES fixture as one window of one batch, each within its own stored
tol of the reference module's f64 output, the per-case check of tests/test_gpu_decoder.py) and, bit for bit, to psfm_traj_decode on
each window alone.  Then the stage: label_trajectories_batched / label_sequences_batched against label_trajectories with
device_predictor, byte for byte."""
import ctypes

import numpy as np
import pytest

from _decoder_np import SMALL_CASES, fixture_input, seeded_decoder_inputs
from test_gpu_decoder import FULL_WINDOWS, GUARD, SENTINEL, bits, check_case, connect_t23, pt, window_depths  # noqa: F401 (pt: fixture)

pytestmark = pytest.mark.gpu
MIXED = [65, 2, 0, 513, 64, 735]        # a tile boundary, the smallest window, an empty one, a slice boundary, a full tile, many tiles


def seeded_windows(ks, seed=4100):
    return [np.ascontiguousarray(seeded_decoder_inputs(k, seed + 7 * i + k)) for i, k in enumerate(ks)]


def batch_need(pt, ks):
    return int(pt.hip.lib().psfm_traj_decode_batch_workspace_bytes((ctypes.c_int64 * max(len(ks), 1))(*ks), len(ks)))


def raw_batch_call(pt, n_win, encs, ks, weights, ws, ws_bytes, los, prs, pds):
    """The C ABI as it stands: encs / los / prs / pds are lists of tensors (None: a NULL entry) or None (a NULL array)."""
    vp = ctypes.c_void_p
    col = lambda ts: None if ts is None else (vp * max(len(ts), 1))(*[None if t is None else t.data_ptr() for t in ts])
    ctx = pt.hip.context()
    return pt.hip.lib().psfm_traj_decode_batch(ctx.handle, n_win, col(encs), (ctypes.c_int64 * max(len(ks), 1))(*ks), pt.hip.ptr(weights),
                                               pt.hip.ptr(ws), ws_bytes, col(los), col(prs), col(pds), pt.hip.current_stream_ptr(ctx.device))


def raw_batch(pt, xs, fill=0xA5, arrays=(True, True, True), entries=None):
    """One call through the C ABI with buffers allocated here; guard regions behind every output and behind the workspace must come
    back untouched.  arrays: which of the three pointer arrays are passed at all; entries: per window which of its three outputs are
    non-NULL (default: all).  Returns per window (logits, prob, pred) as host arrays, None where not asked for."""
    import torch
    ks = [x.shape[1] for x in xs]
    d_x = [torch.from_numpy(x).cuda() if x.shape[1] else None for x in xs]
    need = batch_need(pt, ks)
    assert need == sum(int(pt.hip.lib().psfm_traj_decode_workspace_bytes(k)) for k in ks)
    ws = torch.full((need + GUARD,), fill, dtype=torch.uint8, device="cuda")
    ws[need:] = 0x5A
    entries = entries or [(True, True, True)] * len(xs)
    bufs = []
    for k, e in zip(ks, entries):
        bufs.append((torch.full((k + GUARD,), SENTINEL, dtype=torch.float32, device="cuda") if e[0] and arrays[0] else None,
                     torch.full((k + GUARD,), SENTINEL, dtype=torch.float32, device="cuda") if e[1] and arrays[1] else None,
                     torch.full((k + GUARD,), 77, dtype=torch.uint8, device="cuda") if e[2] and arrays[2] else None))
    cols = [[b[i] for b in bufs] if arrays[i] else None for i in range(3)]
    assert raw_batch_call(pt, len(xs), d_x, ks, pt.weights, ws, need, *cols) == pt.hip.PSFM_OK, pt.hip.lib().psfm_last_error()
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0x5A).all()), "psfm_traj_decode_batch wrote behind its workspace"
    out = []
    for k, b in zip(ks, bufs):
        row = []
        for t, s in zip(b, (SENTINEL, SENTINEL, 77)):
            if t is None:
                row.append(None)
                continue
            h = t.cpu().numpy()
            assert (h[k:] == s).all(), "psfm_traj_decode_batch wrote behind an output"
            row.append(h[:k].copy())
        out.append(tuple(row))
    return out


def single(pt, x):
    """psfm_traj_decode on one window alone, as host arrays."""
    import torch
    lo, pr, pd = pt.decoder.decode_traj_device(torch.from_numpy(x).cuda(), pt.weights)
    return lo[0, 0].cpu().numpy(), pr[0, 0].cpu().numpy(), pd.cpu().numpy().astype(np.uint8)


def assert_same_bits(got, want, what=""):
    for a, b in zip(got, want):
        assert a.shape == b.shape and np.array_equal(bits(a), bits(b)), what


def test_every_fixture_case_as_one_batch_equals_the_reference(pt):
    """All SMALL_CASES as the windows of ONE call (19 windows, K from 2 to 1000): each passes the single call's per-case check."""
    import torch
    xs = [fixture_input(case) for case in SMALL_CASES]
    outs = pt.decoder.decode_windows_device([torch.from_numpy(x).cuda()[None] for x in xs], pt.weights)
    assert len(outs) == len(SMALL_CASES) <= pt.decoder.BATCH_MAX
    for case, x, (logits, prob, pred) in zip(SMALL_CASES, xs, outs):
        K = x.shape[1]
        assert tuple(logits.shape) == (1, 1, K) and tuple(prob.shape) == (1, 1, K) and tuple(pred.shape) == (K,)
        assert logits.dtype == torch.float32 and prob.dtype == torch.float32 and pred.dtype == torch.bool
        check_case(case, logits[0, 0].cpu().numpy(), prob[0, 0].cpu().numpy(), pred.cpu().numpy())


@pytest.mark.parametrize("ks", [MIXED, MIXED[::-1]], ids=["mixed", "reversed"])
def test_bit_equal_to_the_single_call_per_window(pt, ks):
    import torch
    xs = seeded_windows(ks)
    got = raw_batch(pt, xs)
    for b, (x, g) in enumerate(zip(xs, got)):
        if ks[b] == 0:
            assert all(a.size == 0 for a in g)
            continue
        want = single(pt, x)
        assert_same_bits(g, want, "window %d (k = %d)" % (b, ks[b]))
        assert np.isfinite(g[0]).all()
    # the module, with mixed input forms, and torch.equal on its tensors
    outs = pt.decoder.decode_windows_device([torch.from_numpy(x).cuda() if b % 2 else x[None] for b, x in enumerate(xs)], pt.weights)
    for x, (lo, pr, pd) in zip(xs, outs):
        l1, p1, d1 = pt.decoder.decode_traj_device(x, pt.weights)
        assert torch.equal(lo, l1) and torch.equal(pr, p1) and torch.equal(pd, d1)


def test_one_window_equals_the_single_call(pt):
    for k in (2, 129):
        x = seeded_windows([k], seed=4200)[0]
        assert_same_bits(raw_batch(pt, [x])[0], single(pt, x))


def test_more_than_64_windows_are_split(pt):
    import torch
    ks = [2 + (b % 5) for b in range(70)]
    xs = seeded_windows(ks, seed=4300)
    outs = pt.decoder.decode_windows_device([torch.from_numpy(x).cuda() for x in xs], pt.weights)
    assert len(outs) == 70
    for b in (0, 63, 64, 69):
        l1, p1, d1 = pt.decoder.decode_traj_device(xs[b], pt.weights)
        assert torch.equal(outs[b][0], l1) and torch.equal(outs[b][1], p1) and torch.equal(outs[b][2], d1), b


def test_no_window_and_empty_windows_launch_nothing(pt):
    import torch
    lib = pt.hip.lib()
    lo = torch.full((GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    pd = torch.full((GUARD,), 77, dtype=torch.uint8, device="cuda")
    ws = torch.full((GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    OK = pt.hip.PSFM_OK
    assert raw_batch_call(pt, 0, None, [], None, None, 0, None, None, None) == OK
    assert raw_batch_call(pt, 0, [lo], [5], pt.weights, ws, GUARD, [lo], [lo], [pd]) == OK
    assert raw_batch_call(pt, 3, [None] * 3, [0, 0, 0], None, None, 0, [lo] * 3, [lo] * 3, [pd] * 3) == OK
    assert raw_batch_call(pt, 64, [lo] * 64, [0] * 64, pt.weights, ws, GUARD, [lo] * 64, [lo] * 64, [pd] * 64) == OK
    torch.cuda.synchronize()
    assert bool((lo == SENTINEL).all()) and bool((pd == 77).all()) and bool((ws == 0xA5).all())
    assert batch_need(pt, []) == 0 and batch_need(pt, [0, 0]) == 0
    assert pt.decoder.decode_windows_device([], pt.weights) == []
    (logits, prob, pred), = pt.decoder.decode_windows_device([np.zeros((1, 16, 0), np.float32)], pt.weights)
    assert tuple(logits.shape) == (1, 1, 0) and tuple(prob.shape) == (1, 1, 0) and tuple(pred.shape) == (0,)


def test_repetition_and_workspace_contents_do_not_matter(pt):
    xs = seeded_windows(MIXED, seed=4400)
    want = raw_batch(pt, xs, fill=0xA5)
    for fill in (0xA5, 0x00):
        got = raw_batch(pt, xs, fill=fill)
        for b, (g, w) in enumerate(zip(got, want)):
            assert_same_bits(g, w, "fill %#x window %d" % (fill, b))


def test_any_subset_of_the_outputs_per_array_and_per_entry(pt):
    ks = [65, 2, 130]
    xs = seeded_windows(ks, seed=4500)
    want = raw_batch(pt, xs)

    def check(got, arrays, entries):
        for g, w, e in zip(got, want, entries):
            for i in range(3):
                if arrays[i] and e[i]:
                    assert np.array_equal(bits(g[i]), bits(w[i])), (arrays, entries)
                else:
                    assert g[i] is None
    full = [(True, True, True)] * 3
    for mask in range(8):                                   # whole arrays NULL
        arrays = (bool(mask & 1), bool(mask & 2), bool(mask & 4))
        check(raw_batch(pt, xs, arrays=arrays), arrays, full)
    for mask in range(8):                                   # single entries NULL: window b drops the outputs of mask rotated by b
        entries = [tuple(bool(((mask >> ((i + b) % 3)) & 1)) for i in range(3)) for b in range(3)]
        check(raw_batch(pt, xs, entries=entries), (True, True, True), entries)


def test_refusals_launch_nothing(pt):
    import torch
    lib = pt.hip.lib()
    ks = [8, 8, 8, 8]
    K = 8
    x = [torch.from_numpy(v).cuda() for v in seeded_windows(ks, seed=4600)]
    need = batch_need(pt, ks)
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda")
    lo = [torch.full((K + GUARD,), SENTINEL, dtype=torch.float32, device="cuda") for _ in ks]
    pr = [torch.full((K + GUARD,), SENTINEL, dtype=torch.float32, device="cuda") for _ in ks]
    pd = [torch.full((K + GUARD,), 77, dtype=torch.uint8, device="cuda") for _ in ks]
    ERR, w = pt.hip.PSFM_ERR_ARG, pt.weights
    assert raw_batch_call(pt, 65, x * 17, ks * 17, w, ws, need, lo * 17, pr * 17, pd * 17) == ERR
    assert b"n_win=65" in lib.psfm_last_error()
    assert raw_batch_call(pt, -1, x, ks, w, ws, need, lo, pr, pd) == ERR
    assert raw_batch_call(pt, 4, x, [8, 8, 8, 1], w, ws, need, lo, pr, pd) == ERR
    msg = lib.psfm_last_error()
    assert b"window 3" in msg and b"k=1" in msg and b"InstanceNorm" in msg, msg
    assert raw_batch_call(pt, 4, x, [8, -2, 8, 1], w, ws, need, lo, pr, pd) == ERR
    assert b"window 1" in lib.psfm_last_error()                                         # the FIRST refused window
    assert raw_batch_call(pt, 4, x, [8, 8, (2 ** 31) // 128, 8], w, ws, need, lo, pr, pd) == ERR
    assert b"window 2" in lib.psfm_last_error()
    assert raw_batch_call(pt, 4, [x[0], None, x[2], x[3]], ks, w, ws, need, lo, pr, pd) == ERR
    assert b"window 1" in lib.psfm_last_error()
    assert raw_batch_call(pt, 4, None, ks, w, ws, need, lo, pr, pd) == ERR
    assert raw_batch_call(pt, 4, x, ks, None, ws, need, lo, pr, pd) == ERR
    assert raw_batch_call(pt, 4, x, ks, w, None, need, lo, pr, pd) == ERR
    assert raw_batch_call(pt, 4, x, ks, w, ws, need - 1, lo, pr, pd) == ERR
    msg = lib.psfm_last_error()
    assert b"workspace" in msg and str(need).encode() in msg, msg                       # the message names the needed size
    assert batch_need(pt, [8, 1]) == 0 and batch_need(pt, [2] * 65) == 0
    torch.cuda.synchronize()
    for t in lo + pr:
        assert bool((t == SENTINEL).all())
    assert all(bool((t == 77).all()) for t in pd) and bool((ws == 0xA5).all())
    with pytest.raises(ValueError, match="window 2.*K = 1"):
        pt.decoder.decode_windows_device([x[0], x[1], np.zeros((16, 1), np.float32)], w)
    with pytest.raises(ValueError, match="window 1"):
        pt.decoder.decode_windows_device([x[0], np.zeros((15, K), np.float32)], w)
    with pytest.raises(ValueError):
        pt.decoder.decode_windows_device(x, w[:-1])
    with pytest.raises(ValueError, match=str(need)):
        pt.decoder.decode_windows_device(x, w, workspace=ws[:-1])


def finished(m):
    return [t.cpu().numpy() for t in m.finish()]


def assert_bytes_equal(got, want):
    assert len(got) == len(want) == 5
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_label_trajectories_batched_equals_the_per_window_route(pt):
    """The 48x64, T = 23 sequence (three windows): the same five tensors out of finish(), byte for byte, with groups of one window, of
    two and of all three."""
    from psfm_motion_seg.load_cut_seq import window_ranges
    from psfm_motion_seg.merge_labels import decode_groups, label_trajectories, label_trajectories_batched
    g, ctx = connect_t23(pt)
    T, raw_hw, hw, window = int(g["T"]), (int(g["H"]), int(g["W"])), tuple(int(x) for x in g["input_size"]), int(g["window"])
    _, depth_of = window_depths(hw)
    depth = {f0: depth_of(wi, n) for wi, (f0, n) in enumerate(window_ranges(T, window))}
    depth_for_window = lambda time_idx: depth[int(time_idx[0])]
    predict = pt.decoder.device_predictor(pt.enc_weights, pt.weights, depth_for_window, hw, ctx=ctx)
    m = label_trajectories(T, window, raw_hw, hw, 10 ** 9, predict, seed=3, ctx=ctx)
    want, want_ids = finished(m), [t.cpu().numpy() for t in m.window_ids]
    rows = [len(i) for i in want_ids]
    assert len(rows) == 3 and min(rows) > 100 and len(want[0]) > 0 and 0 < want[4].sum() < len(want[4])
    for max_rows, groups in ((1, 3), (rows[0] + rows[1], 2), (None, 1)):
        assert len(decode_groups(rows, max_rows)) == groups
        mb = label_trajectories_batched(T, window, raw_hw, hw, 10 ** 9, pt.enc_weights, pt.weights, depth_for_window, seed=3, ctx=ctx,
                                        max_rows=max_rows)
        assert_bytes_equal(finished(mb), want)
        assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(mb.window_ids, want_ids))


def test_label_sequences_batched_equals_the_batched_route_per_context(pt):
    """Two sequences of different length from run_connect_batch (T = 23: three windows, T = 16: two): the windows of both go through
    one decode group, and every context's labelled set is the one it gets alone."""
    import torch
    from _common import golden, regen_inputs
    from psfm_motion_seg.merge_labels import label_sequences_batched, label_trajectories_batched
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
    ms = label_sequences_batched(ctxs, lengths, window, raw_hw, hw, 10 ** 9, pt.enc_weights, pt.weights, depth_for_window, seed=5)
    assert [len(m.window_ids) for m in ms] == [3, 2]
    got = [finished(m) for m in ms]
    assert all(len(s[0]) > 0 for s in got) and not np.array_equal(got[0][0], got[1][0])
    for i, (ctx, length) in enumerate(zip(ctxs, lengths)):
        alone = label_trajectories_batched(length, window, raw_hw, hw, 10 ** 9, pt.enc_weights, pt.weights,
                                           lambda t, i=i: depth_for_window(i, t), seed=5, ctx=ctx)
        assert_bytes_equal(finished(alone), got[i])
