"""psfm_traj_decode (csrc/psfm_decoder.hip) on the GPU: the motion classifier's OANet decoder, sigmoid and threshold, against the f64
output of the REFERENCE's own traj_oa_depth.decoder (tests/golden/make_decoder_golden.py) within each case's measured tol (4 x the
error of the reference's own fp32 run against that f64 output, per case), through psfm_motion_seg.decoder and through the raw C ABI.
Labels must equal `logit64 > 0` on every row outside the band |logit64| <= tol (at most 0.5 % of a case), pred must equal
prob > 0.5 exactly, prob must be within tol of sigmoid(logit64).  What must be exact is checked bit for bit: two calls, a workspace
full of NaN or of zeros, any subset of the outputs."""
import ctypes

import numpy as np
import pytest

from _common import golden, regen_inputs
from _decoder_np import (BIG_K, DECODER_CASES, SMALL_CASES, decoder_fixture, decoder_np, fixture_input, packed_sha256,
                         seeded_decoder_weights, sigmoid)
from _encoder_np import fixture_weights as encoder_fixture_weights

pytestmark = pytest.mark.gpu
SENTINEL = -12345.0
GUARD = 4096
BAND_CAP = 0.005
BIG_CASE = DECODER_CASES[-1]
FULL_WINDOWS = ["augment_48x64_t23_w0", None, "augment_48x64_t23_w2"]


@pytest.fixture(scope="module")
def pt():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from point_trajectory import trajectory, _hip
    from psfm_motion_seg import augment, decoder, encoder
    _hip.context()
    class NS: pass
    ns = NS()
    ns.trajectory, ns.hip, ns.augment, ns.encoder, ns.decoder = trajectory, _hip, augment, encoder, decoder
    ns.W = seeded_decoder_weights()
    ns.weights = decoder.pack_decoder_weights({"decoder." + k: v for k, v in ns.W.items()})
    meta = np.load(golden_path("decoder_meta"))
    assert packed_sha256(ns.weights.cpu().numpy()) == str(meta["weights_sha256"]), "the seeded weights are not the generator's"
    ns.enc_W, _ = encoder_fixture_weights()
    ns.enc_weights = encoder.pack_encoder_weights(ns.enc_W)
    return ns


def golden_path(name):
    import os
    from _decoder_np import GOLDEN
    return os.path.join(GOLDEN, name + ".npz")


def raw_call(pt, enc, weights, K, ws, ws_bytes, logits, prob, pred):
    ctx = pt.hip.context()
    return pt.hip.lib().psfm_traj_decode(ctx.handle, pt.hip.ptr(enc), pt.hip.ptr(weights), K, pt.hip.ptr(ws), ws_bytes, pt.hip.ptr(logits),
                                         pt.hip.ptr(prob), pt.hip.ptr(pred), pt.hip.current_stream_ptr(ctx.device))


def raw_decode(pt, x, fill=0xA5, want=(True, True, True)):
    """Through the C ABI with buffers allocated here; guard regions behind the three outputs and the workspace must come back
    untouched.  The workspace starts out as bytes `fill`.  Returns (logits, prob, pred) as host arrays (None where not asked for)."""
    import torch
    x = np.ascontiguousarray(x, np.float32)
    K = x.shape[1]
    d_x = torch.from_numpy(x).cuda()
    need = int(pt.hip.lib().psfm_traj_decode_workspace_bytes(K))
    ws = torch.full((need + GUARD,), fill, dtype=torch.uint8, device="cuda")
    ws[need:] = 0x5A
    lo = torch.full((K + GUARD,), SENTINEL, dtype=torch.float32, device="cuda") if want[0] else None
    pr = torch.full((K + GUARD,), SENTINEL, dtype=torch.float32, device="cuda") if want[1] else None
    pd = torch.full((K + GUARD,), 77, dtype=torch.uint8, device="cuda") if want[2] else None
    assert raw_call(pt, d_x, pt.weights, K, ws, need, lo, pr, pd) == pt.hip.PSFM_OK, pt.hip.lib().psfm_last_error()
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0x5A).all()), "psfm_traj_decode wrote behind its workspace"
    out = []
    for t, s in ((lo, SENTINEL), (pr, SENTINEL), (pd, 77)):
        if t is None:
            out.append(None)
            continue
        h = t.cpu().numpy()
        assert (h[K:] == s).all(), "psfm_traj_decode wrote behind an output"
        out.append(h[:K].copy())
    return tuple(out)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def check_case(case, logits, prob, pred):
    """The rules of the module docstring for one fixture case; prints each figure before it asserts."""
    fx = decoder_fixture(case)
    tol, want = float(fx["tol"]), fx["logit64"]
    assert tol == 4.0 * float(fx["e"])
    assert logits.dtype == np.float32 and prob.dtype == np.float32
    assert np.array_equal(pred.astype(bool), prob > np.float32(0.5)), "pred is not prob > 0.5"
    if "rows" in fx.files:
        rows = fx["rows"]
        logits, prob, pred = logits[rows], prob[rows], pred[rows]
    err = float(np.abs(logits.astype(np.float64) - want).max())
    perr = float(np.abs(prob.astype(np.float64) - sigmoid(want)).max())
    outside = np.abs(want) > tol
    wrong = int((pred.astype(bool) != (want > 0))[outside].sum())
    print("%s: max |logit - logit64| = %.3e, max |prob - sigmoid(logit64)| = %.3e, tol = %.3e, rows in the band %d of %d, labels wrong "
          "outside it %d" % (case, err, perr, tol, int((~outside).sum()), len(want), wrong))
    assert np.isfinite(logits).all() and np.isfinite(prob).all()
    assert err <= tol
    assert perr <= tol
    assert (~outside).mean() <= BAND_CAP
    assert wrong == 0


def test_weight_count_and_packing(pt):
    import torch
    assert pt.hip.lib().psfm_traj_decode_weight_count() == pt.decoder.WEIGHT_COUNT == 529497
    assert pt.weights.is_cuda and pt.weights.dtype == torch.float32 and tuple(pt.weights.shape) == (529497,)
    assert torch.equal(pt.weights, pt.decoder.pack_decoder_weights({k: torch.from_numpy(v) for k, v in pt.W.items()}))
    assert pt.hip.lib().psfm_version() == 141


@pytest.mark.parametrize("case", SMALL_CASES)
def test_module_equals_reference_fixture(pt, case):
    import torch
    x = fixture_input(case)
    K = x.shape[1]
    logits, prob, pred = pt.decoder.decode_traj_device(torch.from_numpy(x).cuda()[None], pt.weights)
    assert tuple(logits.shape) == (1, 1, K) and tuple(prob.shape) == (1, 1, K) and tuple(pred.shape) == (K,)
    assert logits.dtype == torch.float32 and prob.dtype == torch.float32 and pred.dtype == torch.bool
    check_case(case, logits[0, 0].cpu().numpy(), prob[0, 0].cpu().numpy(), pred.cpu().numpy())
    # the other accepted forms: (16,K), a host array, a workspace of the caller's
    need = int(pt.hip.lib().psfm_traj_decode_workspace_bytes(K))
    ws = torch.empty((need,), dtype=torch.uint8, device="cuda")
    for l2, p2, d2 in (pt.decoder.decode_traj_device(x, pt.weights), pt.decoder.decode_traj_device(torch.from_numpy(x).cuda(), pt.weights, workspace=ws)):
        assert torch.equal(l2, logits) and torch.equal(p2, prob) and torch.equal(d2, pred)


@pytest.mark.parametrize("case", SMALL_CASES)
def test_c_abi_equals_reference_fixture(pt, case):
    check_case(case, *raw_decode(pt, fixture_input(case)))


def test_c_abi_at_the_shipped_cap(pt):
    """K = 100 000 against the stored 8192-row sample; a second identical call gives identical bits."""
    import hashlib
    x = fixture_input(BIG_CASE)
    assert x.shape == (16, BIG_K) and hashlib.sha256(x.tobytes()).hexdigest() == str(decoder_fixture(BIG_CASE)["x_sha256"])
    got = raw_decode(pt, x)
    check_case(BIG_CASE, *got)
    again = raw_decode(pt, x, fill=0)
    for a, b in zip(got, again):
        assert np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("case", ["seeded_k2", "seeded_k129", "seeded_k1000"])
def test_workspace_contents_and_repetition_do_not_matter(pt, case):
    """A workspace full of NaN, one full of zeros, a second identical call: the same bits."""
    x = fixture_input(case)
    want = raw_decode(pt, x, fill=0xFF)                 # (0xFFFFFFFF is a NaN, as fp32 and as f64)
    for fill in (0x00, 0xFF):
        got = raw_decode(pt, x, fill=fill)
        for a, b in zip(got, want):
            assert np.array_equal(bits(a), bits(b)), fill


def test_any_subset_of_the_outputs(pt):
    x = fixture_input("seeded_k257")
    want = raw_decode(pt, x)
    for mask in range(7):
        sel = (bool(mask & 1), bool(mask & 2), bool(mask & 4))
        got = raw_decode(pt, x, want=sel)
        for s, a, b in zip(sel, got, want):
            assert (a is None) if not s else np.array_equal(bits(a), bits(b)), sel


def test_rows_permuted_in_are_rows_permuted_out(pt):
    """Within tol, not bit for bit: the statistics are sums over all rows."""
    case = "seeded_k257"
    x, tol = fixture_input(case), float(decoder_fixture(case)["tol"])
    lo, pr, _ = raw_decode(pt, x)
    perm = np.random.default_rng(5).permutation(x.shape[1])
    lo2, pr2, pd2 = raw_decode(pt, x[:, perm])
    err = float(np.abs(lo2.astype(np.float64) - lo[perm]).max())
    print("max |permuted - original| = %.3e, tol = %.3e" % (err, tol))
    assert err <= tol and np.abs(pr2.astype(np.float64) - pr[perm]).max() <= tol
    check_case(case, lo2[np.argsort(perm)], pr2[np.argsort(perm)], pd2[np.argsort(perm)])


def test_k0_is_a_noop(pt):
    import torch
    out = torch.full((GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    pd = torch.full((GUARD,), 77, dtype=torch.uint8, device="cuda")
    assert raw_call(pt, None, None, 0, None, 0, out, out, pd) == pt.hip.PSFM_OK
    assert raw_call(pt, None, None, 0, None, 0, None, None, None) == pt.hip.PSFM_OK
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((pd == 77).all())
    assert pt.hip.lib().psfm_traj_decode_workspace_bytes(0) == 0
    logits, prob, pred = pt.decoder.decode_traj_device(np.zeros((1, 16, 0), np.float32), pt.weights)
    assert tuple(logits.shape) == (1, 1, 0) and tuple(prob.shape) == (1, 1, 0) and tuple(pred.shape) == (0,)


def test_argument_errors_launch_nothing(pt):
    import torch
    K = 8
    x = torch.from_numpy(fixture_input("seeded_k63")[:, :K].copy()).cuda()
    lib = pt.hip.lib()
    need = int(lib.psfm_traj_decode_workspace_bytes(K))
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda")
    lo = torch.full((K + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    pr = torch.full((K + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    pd = torch.full((K + GUARD,), 77, dtype=torch.uint8, device="cuda")
    ERR, w = pt.hip.PSFM_ERR_ARG, pt.weights
    assert raw_call(pt, None, w, K, ws, need, lo, pr, pd) == ERR
    assert raw_call(pt, x, None, K, ws, need, lo, pr, pd) == ERR
    assert raw_call(pt, x, w, K, None, need, lo, pr, pd) == ERR
    assert raw_call(pt, x, w, -1, ws, need, lo, pr, pd) == ERR
    assert raw_call(pt, x, w, (2 ** 31) // 128, ws, need, lo, pr, pd) == ERR            # 128 k >= 2^31
    assert b"psfm_traj_decode" in lib.psfm_last_error()
    assert raw_call(pt, x, w, 1, ws, need, lo, pr, pd) == ERR
    msg = lib.psfm_last_error()
    assert b"k=1" in msg and b"InstanceNorm" in msg, msg
    assert raw_call(pt, x, w, K, ws, need - 1, lo, pr, pd) == ERR
    msg = lib.psfm_last_error()
    assert b"workspace" in msg and str(need).encode() in msg, msg                       # the message names the needed size
    torch.cuda.synchronize()
    assert bool((lo == SENTINEL).all()) and bool((pr == SENTINEL).all()) and bool((pd == 77).all()) and bool((ws == 0xA5).all())
    with pytest.raises(ValueError, match="K = 1"):
        pt.decoder.decode_traj_device(np.zeros((16, 1), np.float32), w)
    with pytest.raises(ValueError):
        pt.decoder.decode_traj_device(np.zeros((15, K), np.float32), w)
    with pytest.raises(ValueError):
        pt.decoder.decode_traj_device(x, w[:-1])
    with pytest.raises(ValueError, match=str(need)):
        pt.decoder.decode_traj_device(x, w, workspace=ws[:-1])


def connect_t23(pt):
    import torch
    g = golden(FULL_WINDOWS[0])
    d = regen_inputs(g, stride2=False)
    ff, fb = torch.from_numpy(np.stack(d["flows_f"])).cuda(), torch.from_numpy(np.stack(d["flows_b"])).cuda()
    pt.trajectory.run_connect(ff, fb, None, None, 1.0, int(g["ratio"]), return_device=True)
    return g, pt.hip.context()


def window_depths(hw):
    """The fixtures' depth maps for windows 0 and 2, seeded maps for window 1."""
    import torch
    fx = [golden(n) if n else None for n in FULL_WINDOWS]
    rng = np.random.default_rng(17)
    return fx, lambda wi, n: torch.from_numpy(fx[wi]["depth"] if fx[wi] is not None else rng.uniform(size=(n,) + hw).astype(np.float32)).cuda()


def test_chained_behind_the_window_sampler_the_augment_and_the_encoder(pt):
    """run_connect on the 48x64, T = 23 sequence, then window_prediction per window: the logits are the restatement fed the device's
    own encoding; for the two windows a fixture holds, the labels are the reference's full-model labels outside 4 (e + d)."""
    from psfm_motion_seg.load_cut_seq import window_ranges
    g, ctx = connect_t23(pt)
    T, raw_hw, hw = int(g["T"]), (int(g["H"]), int(g["W"])), tuple(int(x) for x in g["input_size"])
    fx, depth_of = window_depths(hw)
    ranges = window_ranges(T, int(g["window"]))
    assert len(ranges) == 3
    for wi, (f0, n) in enumerate(ranges):
        ids, raw, mask, enc, logits, prob, pred = pt.decoder.window_prediction(ctx, f0, n, raw_hw, hw, depth_of(wi, n), pt.enc_weights,
                                                                               pt.weights, traj_max_num=10 ** 9)
        K = ids.numel()
        assert K > 100 and tuple(enc.shape) == (1, 16, K) and tuple(logits.shape) == (1, 1, K) and tuple(pred.shape) == (K,)
        near = decoder_fixture("enc_" + (FULL_WINDOWS[wi] or FULL_WINDOWS[0]))          # (window 1: the nearest fixture, K = 735)
        tol = float(near["tol"])
        want = decoder_np(enc[0].cpu().numpy(), pt.W)
        got, p = logits[0, 0].cpu().numpy(), prob[0, 0].cpu().numpy()
        err = float(np.abs(got.astype(np.float64) - want).max())
        print("window %d: K = %d, max |logit - restatement(device encoding)| = %.3e, tol = %.3e" % (wi, K, err, tol))
        assert err <= tol
        assert np.array_equal(pred.cpu().numpy(), p > np.float32(0.5))
        if fx[wi] is not None:
            full = np.load(golden_path("decoder_full_" + FULL_WINDOWS[wi]))
            assert int(fx[wi]["frame0"]) == f0 and K == len(full["logit64"])
            band = float(full["band"])
            assert band == 4.0 * (float(full["e"]) + float(full["d"]))
            outside = np.abs(full["logit64"]) > band
            assert (~outside).mean() <= BAND_CAP
            assert np.array_equal(pred.cpu().numpy()[outside], (full["prob32"] > 0.5)[outside])
            assert np.array_equal(pred.cpu().numpy()[outside], (full["logit64"] > 0)[outside])


def test_label_trajectories_with_the_device_predictor(pt):
    """The whole labelled set from device code: label_trajectories(predict=device_predictor(...)) equals merge_labels_host fed the
    same per-window predictions."""
    from psfm_motion_seg.merge_labels import label_trajectories, merge_labels_host
    from test_labels_merge import assert_set_equal, saved_set_host
    g, ctx = connect_t23(pt)
    T, raw_hw, hw = int(g["T"]), (int(g["H"]), int(g["W"])), tuple(int(x) for x in g["input_size"])
    _, depth_of = window_depths(hw)
    seen = []

    def depth_for_window(time_idx):
        return depth_of(len(seen), len(time_idx))
    inner = pt.decoder.device_predictor(pt.enc_weights, pt.weights, depth_for_window, hw, ctx=ctx)

    def predict(raw, nor, mask, time_idx):
        pred = inner(raw, nor, mask, time_idx)
        seen.append([int(time_idx[0]), len(time_idx), None, pred.cpu().numpy().astype(np.uint8)])
        return pred
    m = label_trajectories(T, int(g["window"]), raw_hw, hw, 10 ** 9, predict, ctx=ctx)
    assert len(seen) == 3 and all(0 < w[3].sum() < len(w[3]) for w in seen)             # both labels occur in every window
    for w, ids in zip(seen, m.window_ids):
        w[2] = ids.cpu().numpy()
    got = [t.cpu().numpy() for t in m.finish()]
    assert_set_equal(got, merge_labels_host(*saved_set_host(pt, ctx), [tuple(w) for w in seen]))
