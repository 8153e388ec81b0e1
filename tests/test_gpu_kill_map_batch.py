"""psfm_kill_map_batch (csrc/psfm_motion_boundary.hip): the kill maps of up to 64 same-shape stacks in ONE launch, restricted to a
range of frames -- what psfm_connect_batch enqueues behind every chunk of flow_check when its contexts have the motion-boundary
option on.  Every byte must be psfm_kill_map's on that stack alone (itself pinned to the reference's masks by
tests/test_gpu_motion_boundary.py; where a mask fixture of the frame size exists its frames are part of the stacks here and bit 1 is
compared with it again), and the RANGE is a contract: occlusion bytes of frames outside it are never read (they hold 0xA5 here, where
the batch would hold bytes flow_check has not written yet) and kill bytes outside it are never written."""
import ctypes

import numpy as np
import pytest

from _motion_boundary_np import mask_case, motion_boundary_np

pytestmark = pytest.mark.gpu
SENTINEL8 = 0xA5
GUARD = 4096
# (n, H, W): P mod 4 = 3, 1, 0, 2, 1, 1, 2 -- odd P (one pixel per thread), one-row-pair frames, more than one block per frame, >= 64 chunks
SHAPES = [(2, 3, 5), (7, 37, 53), (8, 48, 64), (2, 259, 254), (2, 259, 255), (3, 33, 129), (1, 2, 2051)]
FIXTURE_OF = {(3, 5): "stack2_3x5", (37, 53): "m37x53", (48, 64): "m48x64"}       # mask fixtures of these frame sizes: their frames lead the stack
RANGES = ["whole", "pair0=1,n_pairs=2", "beyond_the_shortest"]


@pytest.fixture(scope="module")
def pt():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from point_trajectory import trajectory, _hip
    _hip.context()
    class NS: pass
    ns = NS()
    ns.trajectory, ns.hip, ns.torch = trajectory, _hip, torch
    return ns


_bases = {}


def base(pt, shape, thres=0.02):
    """(flows (n,H,W,2) f32, occ (n,H,W) u8, psfm_kill_map of the whole stack) of a shape: built once, never changed.  The kill map of
    the first k frames of a stack is the first k frames of its kill map (the rule looks at one frame), so every member of a batch is a
    prefix of this stack."""
    key = (shape, thres)
    if key not in _bases:
        n, h, w = shape
        rng = np.random.default_rng(n * 1000 + w)
        yy, xx = np.mgrid[0:h, 0:w]
        b = np.stack([np.sin(xx / 17.0) + (xx > w // 2) * 0.4, np.cos(yy / 13.0) - (yy > h // 3) * 0.3], -1)
        flows = (b[None] * rng.uniform(0.5, 2.0, size=(n, 1, 1, 1)) + rng.normal(0, 0.004, size=(n, h, w, 2))).astype(np.float32)
        if (h, w) in FIXTURE_OF:
            fx = mask_case(FIXTURE_OF[(h, w)])[0]
            flows[:len(fx)] = fx
        occ = ((rng.uniform(size=(n, h, w)) < 0.3) * rng.integers(1, 256, size=(n, h, w))).astype(np.uint8)
        torch = pt.torch
        ctx = pt.hip.context()
        df, do = torch.from_numpy(flows).cuda(), torch.from_numpy(occ).cuda()
        out = torch.empty((n, h, w), dtype=torch.uint8, device="cuda")
        pt.hip.check(pt.hip.lib().psfm_kill_map(ctx.handle, pt.hip.ptr(df), pt.hip.ptr(do), n, h, w, float(thres), pt.hip.ptr(out),
                                                pt.hip.current_stream_ptr(ctx.device)))
        want = out.cpu().numpy()
        assert np.array_equal(want & 1, (occ != 0).astype(np.uint8)) and int(want.max()) <= 3
        _bases[key] = (flows, occ, want)
    return _bases[key]


def run_batch(pt, shape, ns, thres, pair0, n_pairs, flow_shift=0, byte_shift=0, expect=None):
    """One psfm_kill_map_batch call over prefixes (ns[i] frames) of the shape's stack.  Occlusion bytes of frames outside
    [pair0, pair0 + n_pairs) are 0xA5, the outputs are 0xA5 everywhere beforehand (and in a guard behind them); flow_shift (floats) /
    byte_shift (bytes) move the buffers off their natural alignment.  Returns the outputs, (ns[i],H,W) u8 each."""
    torch = pt.torch
    _, h, w = shape
    P = h * w
    keep, fl, oc, ou, raws = [], [], [], [], []
    for i, n in enumerate(ns):
        flows, occ, _ = base(pt, shape)
        fbuf = torch.zeros(n * P * 2 + 16, dtype=torch.float32, device="cuda")
        f = fbuf[flow_shift:flow_shift + n * P * 2]
        f.copy_(torch.from_numpy(flows[:n].reshape(-1)))
        o_host = np.full((n, P), SENTINEL8, np.uint8)
        lo, hi = min(pair0, n), min(pair0 + n_pairs, n)
        o_host[lo:hi] = occ[lo:hi].reshape(-1, P)
        obuf = torch.zeros(byte_shift + n * P, dtype=torch.uint8, device="cuda")
        obuf[byte_shift:].copy_(torch.from_numpy(o_host.reshape(-1)))
        raw = torch.full((byte_shift + n * P + GUARD,), SENTINEL8, dtype=torch.uint8, device="cuda")
        keep += [fbuf, obuf]
        fl.append(f); oc.append(obuf[byte_shift:]); ou.append(raw[byte_shift:]); raws.append(raw)
    vp = ctypes.c_void_p
    B = len(ns)
    ctx = pt.hip.context()
    th = thres if isinstance(thres, (list, tuple)) else [thres] * B
    st = pt.hip.lib().psfm_kill_map_batch(ctx.handle, (vp * B)(*[x.data_ptr() for x in fl]), (vp * B)(*[x.data_ptr() for x in oc]),
                                          (ctypes.c_int * B)(*ns), B, h, w, (ctypes.c_float * B)(*th), pair0, n_pairs,
                                          (vp * B)(*[x.data_ptr() for x in ou]), pt.hip.current_stream_ptr(ctx.device))
    if expect is not None:
        assert st == expect, (st, pt.hip.lib().psfm_last_error())
    else:
        pt.hip.check(st)
    torch.cuda.synchronize()
    outs = []
    for n, raw in zip(ns, raws):
        host = raw.cpu().numpy()
        assert (host[:byte_shift] == SENTINEL8).all() and (host[byte_shift + n * P:] == SENTINEL8).all(), "wrote outside its output"
        outs.append(host[byte_shift:byte_shift + n * P].reshape(n, h, w))
    return outs


def check_range(pt, shape, ns, outs, pair0, n_pairs, thres=0.02):
    for i, (n, got) in enumerate(zip(ns, outs)):
        want = base(pt, shape, thres)[2]
        lo, hi = min(pair0, n), min(pair0 + n_pairs, n)
        assert np.array_equal(got[lo:hi], want[lo:hi]), (i, n, int((got[lo:hi] != want[lo:hi]).sum()))
        assert (got[:lo] == SENTINEL8).all() and (got[hi:] == SENTINEL8).all(), (i, n, "kill bytes outside the range were written")


def members(n, B):
    """B prefix lengths in [1, n], not all equal when n > 1, the whole stack among them."""
    return [n] if B == 1 else [1 + (5 * i + n - 1) % n for i in range(B)]


@pytest.mark.parametrize("rng", RANGES)
@pytest.mark.parametrize("B", [1, 3, 64])
@pytest.mark.parametrize("shape", SHAPES)
def test_batch_equals_the_single_call_inside_the_range_and_touches_nothing_outside(pt, shape, B, rng):
    n = shape[0]
    ns = members(n, B)
    assert max(ns) == n and (n == 1 or B == 1 or len(set(ns)) > 1)
    if rng == "whole":
        pair0, n_pairs = 0, n
    elif rng == "pair0=1,n_pairs=2":
        pair0, n_pairs = 1, 2
    else:
        pair0, n_pairs = 0, min(ns) + 1          # ends one frame beyond the shortest stack (beyond all of them in a batch of equals)
    outs = run_batch(pt, shape, ns, 0.02, pair0, n_pairs)
    check_range(pt, shape, ns, outs, pair0, n_pairs)
    if rng == "whole" and shape[1:] in FIXTURE_OF:
        mb = mask_case(FIXTURE_OF[shape[1:]])[1]["mb002"].astype(np.uint8)
        k = ns.index(n)
        assert np.array_equal(outs[k][:len(mb)] >> 1, mb)


def test_a_lane_never_straddles_a_frame_end(pt):
    """37 x 53 = 1961 pixels, 1 mod 4, odd: no frame of the stack starts where a run of four pixels does.  Frames 1 and 2 of seven:
    the occlusion bytes of frames 0 and 3 are 0xA5 and the kill bytes of frame 3 must stay 0xA5 -- also with an even pixel count that
    is no multiple of 4 (259 x 254 = 2 mod 4), where the four-pixels-per-lane kernel runs and the frames' bytes alternate between
    4-byte aligned and not."""
    for shape, pair0, n_pairs in (((7, 37, 53), 1, 2), ((2, 259, 254), 0, 1), ((2, 259, 254), 1, 1)):
        ns = [shape[0]] * 2
        check_range(pt, shape, ns, run_batch(pt, shape, ns, 0.02, pair0, n_pairs), pair0, n_pairs)


@pytest.mark.parametrize("shape", [(2, 3, 5), (7, 37, 53), (8, 48, 64), (2, 259, 254)])
def test_buffers_off_their_alignment(pt, shape):
    """Flow stacks one pixel (8 bytes: the one-pixel-per-thread kernel) and two pixels (16 bytes) off, byte buffers 1, 2 and 3 bytes off a
    4-byte boundary (the bytes leave one by one), both at once."""
    n = shape[0]
    ns = members(n, 3)
    for fs, bs in ((2, 0), (4, 0), (0, 1), (0, 2), (0, 3), (2, 3), (4, 2)):
        for pair0, n_pairs in ((0, n), (1, 2)):
            check_range(pt, shape, ns, run_batch(pt, shape, ns, 0.02, pair0, n_pairs, flow_shift=fs, byte_shift=bs), pair0, n_pairs)


@pytest.mark.parametrize("shape", [(8, 48, 64), (7, 37, 53)])
def test_every_row_has_its_own_threshold(pt, shape):
    flows = base(pt, shape)[0]
    a = np.stack([motion_boundary_np(f, 0.02) for f in flows])
    b = np.stack([motion_boundary_np(f, 0.05) for f in flows])
    assert not np.array_equal(a, b), "the two thresholds give the same masks on this stack: pick another"
    n = shape[0]
    outs = run_batch(pt, shape, [n, n, n], [0.02, 0.05, 0.02], 0, n)
    assert np.array_equal(outs[0], base(pt, shape, 0.02)[2]) and np.array_equal(outs[2], outs[0])
    assert np.array_equal(outs[1], base(pt, shape, 0.05)[2])
    assert not np.array_equal(outs[0], outs[1])
    assert np.array_equal(outs[0] >> 1, a.astype(np.uint8)) and np.array_equal(outs[1] >> 1, b.astype(np.uint8))


def test_python_helper(pt):
    shape = (8, 48, 64)
    flows, occ, want = base(pt, shape)
    t = pt.torch
    fl = [t.from_numpy(flows).cuda(), t.from_numpy(flows[:3]).cuda()]
    oc = [t.from_numpy(occ).cuda(), t.from_numpy(occ[:3]).cuda()]
    out = pt.trajectory.kill_map_batch(fl, oc, 0.02)
    assert np.array_equal(out[0].cpu().numpy(), want) and np.array_equal(out[1].cpu().numpy(), want[:3])
    out = pt.trajectory.kill_map_batch(fl, oc, [0.02, 0.02], pair0=2, n_pairs=3)
    assert np.array_equal(out[0][2:5].cpu().numpy(), want[2:5]) and int(out[0][:2].max()) == 0 and int(out[0][5:].max()) == 0
    assert np.array_equal(out[1][2:].cpu().numpy(), want[2:3]) and int(out[1][:2].max()) == 0


def test_refusals_leave_every_output_untouched(pt):
    shape = (2, 3, 5)
    E = pt.hip.PSFM_ERR_ARG
    for kw in (dict(thres=[0.02, -0.5]), dict(thres=[float("nan"), 0.02]), dict(thres=[0.02, float("inf")]), dict(pair0=-1), dict(n_pairs=-1)):
        a = dict(thres=0.02, pair0=0, n_pairs=2)
        a.update(kw)
        outs = run_batch(pt, shape, [2, 2], a["thres"], a["pair0"], a["n_pairs"], expect=E)
        assert all((o == SENTINEL8).all() for o in outs), kw
        assert b"psfm_kill_map_batch" in pt.hip.lib().psfm_last_error()
    # the arguments run_batch cannot spoil: NULL arrays, a NULL entry, n_seq outside [1, 64], a bad frame size
    torch = pt.torch
    flows, occ, _ = base(pt, shape)
    n, h, w = shape
    f, o = torch.from_numpy(flows).cuda(), torch.from_numpy(occ).cuda()
    out = torch.full((n, h, w), SENTINEL8, dtype=torch.uint8, device="cuda")
    vp = ctypes.c_void_p
    L, ctx = pt.hip.lib(), pt.hip.context()
    sp = pt.hip.current_stream_ptr(ctx.device)
    F, O, K = (vp * 1)(f.data_ptr()), (vp * 1)(o.data_ptr()), (vp * 1)(out.data_ptr())
    N, T, Z = (ctypes.c_int * 1)(n), (ctypes.c_float * 1)(0.02), (vp * 1)(None)
    assert L.psfm_kill_map_batch(None, F, O, N, 1, h, w, T, 0, n, K, sp) == E
    assert L.psfm_kill_map_batch(ctx.handle, None, O, N, 1, h, w, T, 0, n, K, sp) == E
    assert L.psfm_kill_map_batch(ctx.handle, F, None, N, 1, h, w, T, 0, n, K, sp) == E
    assert L.psfm_kill_map_batch(ctx.handle, F, O, None, 1, h, w, T, 0, n, K, sp) == E
    assert L.psfm_kill_map_batch(ctx.handle, F, O, N, 1, h, w, None, 0, n, K, sp) == E
    assert L.psfm_kill_map_batch(ctx.handle, F, O, N, 1, h, w, T, 0, n, None, sp) == E
    assert L.psfm_kill_map_batch(ctx.handle, Z, O, N, 1, h, w, T, 0, n, K, sp) == E
    assert L.psfm_kill_map_batch(ctx.handle, F, Z, N, 1, h, w, T, 0, n, K, sp) == E
    assert L.psfm_kill_map_batch(ctx.handle, F, O, N, 1, h, w, T, 0, n, Z, sp) == E
    assert L.psfm_kill_map_batch(ctx.handle, F, O, N, 0, h, w, T, 0, n, K, sp) == E
    assert L.psfm_kill_map_batch(ctx.handle, F, O, N, 65, h, w, T, 0, n, K, sp) == E
    assert L.psfm_kill_map_batch(ctx.handle, F, O, N, 1, 0, w, T, 0, n, K, sp) == E
    assert L.psfm_kill_map_batch(ctx.handle, F, O, N, 1, h, -3, T, 0, n, K, sp) == E
    torch.cuda.synchronize()
    assert int(out.min()) == SENTINEL8 and int(out.max()) == SENTINEL8
    pt.hip.check(L.psfm_kill_map_batch(ctx.handle, F, O, N, 1, h, w, T, 0, n, K, sp))      # ... and the same arrays, unspoilt, are taken
    assert np.array_equal(out.cpu().numpy(), base(pt, shape)[2])
