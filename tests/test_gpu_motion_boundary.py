"""The motion-boundary option on the GPU (csrc/psfm_motion_boundary.hip, psfm_ctx_set_motion_boundary), against the fixtures that the
REFERENCE's own point_trajectory Python produced (tests/golden/make_motion_boundary_golden.py): psfm_motion_boundary byte for byte on
every mask fixture; psfm_connect / psfm_track with the option on against the reference's track / track_optimize run with the
motion-boundary form of step_forward, and with the option off against its shipped form, on the same inputs.  Where no fixture
exists (the multi-block shapes of the mask kernel) the NumPy statement stands in, itself pinned to the fixtures by
tests/test_motion_boundary_host.py."""
import ctypes

import numpy as np
import pytest

import psfm_synth
from _common import golden, input_hash
from _motion_boundary_np import MASK_CASES, MASK_THRES, SEQ_OPT, SEQ_SYNTH, SEQ_TRACK, mask_case, motion_boundary_np
from test_gpu_whole_sequence import TOL          # track_optimize positions against the oracle: the suite's bar, not a new one

pytestmark = pytest.mark.gpu
SENTINEL8 = 0xA5
GUARD = 4096


@pytest.fixture(scope="module")
def pt():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from point_trajectory import trajectory, utils, _hip
    _hip.context()
    class NS: pass
    ns = NS()
    ns.trajectory, ns.utils, ns.hip, ns.torch = trajectory, utils, _hip, torch
    return ns


def device_mask(pt, stack, thres, flow_shift=0, out_shift=0, occ=None):
    """psfm_motion_boundary (occ given: psfm_kill_map) through the C ABI: (n,H,W) u8.  flow_shift (floats) / out_shift (bytes) move the
    buffers off their natural alignment (the occlusion maps move with the output); the guard region behind the output must come
    back untouched."""
    torch = pt.torch
    stack = np.ascontiguousarray(stack, np.float32)
    n, h, w = stack.shape[:3]
    buf = torch.zeros(stack.size + 16, dtype=torch.float32, device="cuda")
    flows = buf[flow_shift:flow_shift + stack.size]
    flows.copy_(torch.from_numpy(stack.reshape(-1)))
    raw = torch.full((out_shift + n * h * w + GUARD,), SENTINEL8, dtype=torch.uint8, device="cuda")
    out = raw[out_shift:]
    ctx = pt.hip.context()
    if occ is not None:
        occ_raw = torch.zeros(out_shift + n * h * w, dtype=torch.uint8, device="cuda")
        occ_raw[out_shift:].copy_(torch.from_numpy(np.ascontiguousarray(occ, np.uint8).reshape(-1)))
        pt.hip.check(pt.hip.lib().psfm_kill_map(ctx.handle, pt.hip.ptr(flows), pt.hip.ptr(occ_raw[out_shift:]), n, h, w, float(thres),
                                                pt.hip.ptr(out), pt.hip.current_stream_ptr(ctx.device)))
    else:
        pt.hip.check(pt.hip.lib().psfm_motion_boundary(ctx.handle, pt.hip.ptr(flows), n, h, w, float(thres), pt.hip.ptr(out),
                                                       pt.hip.current_stream_ptr(ctx.device)))
    torch.cuda.synchronize()
    host = raw.cpu().numpy()
    assert (host[:out_shift] == SENTINEL8).all() and (host[out_shift + n * h * w:] == SENTINEL8).all(), "wrote outside its output"
    return host[out_shift:out_shift + n * h * w].reshape(n, h, w)


@pytest.mark.parametrize("name", MASK_CASES)
def test_mask_equals_reference_fixture_byte_for_byte(pt, name):
    stack, want = mask_case(name)
    for key, thres in MASK_THRES.items():
        got = device_mask(pt, stack, thres)
        assert np.array_equal(got, want[key].astype(np.uint8)), (key, int((got != want[key]).sum()))
        assert np.array_equal(device_mask(pt, stack, thres), got)                      # identical calls, identical bytes


@pytest.mark.parametrize("name", ["stack2_3x5", "m37x53", "nonfinite_12x13"])
def test_mask_on_buffers_off_their_alignment(pt, name):
    """A flow stack 8 bytes off a 16-byte boundary takes the one-pixel-per-thread kernel; an output 1-3 bytes off a 4-byte boundary
    leaves as single bytes."""
    stack, want = mask_case(name)
    w8 = want["mb002"].astype(np.uint8)
    assert np.array_equal(device_mask(pt, stack, 0.02, flow_shift=2), w8)
    for s in (1, 2, 3):
        assert np.array_equal(device_mask(pt, stack, 0.02, out_shift=s), w8)
    assert np.array_equal(device_mask(pt, stack, 0.02, flow_shift=2, out_shift=3), w8)


@pytest.mark.parametrize("n,h,w", [(2, 259, 254), (2, 259, 255), (3, 33, 129), (1, 2, 2051)])
def test_mask_at_multi_block_shapes_equals_the_numpy_statement(pt, n, h, w):
    """More than one block per frame, frames whose pixel count is no multiple of 4 (a lane's pixels cross the frame end), odd and even
    widths (the row below as 8-byte / 16-byte loads), >= 64 chunks per frame (the banded block order)."""
    rng = np.random.default_rng(n * 1000 + w)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([np.sin(xx / 17.0) + (xx > w // 2) * 0.4, np.cos(yy / 13.0) - (yy > h // 3) * 0.3], -1)
    stack = (base[None] * rng.uniform(0.5, 2.0, size=(n, 1, 1, 1)) + rng.normal(0, 0.004, size=(n, h, w, 2))).astype(np.float32)
    want = np.stack([motion_boundary_np(f, 0.02) for f in stack]).astype(np.uint8)
    assert 0.02 < want.mean() < 0.98
    assert np.array_equal(device_mask(pt, stack, 0.02), want)


@pytest.mark.parametrize("name,flow_shift,out_shift", [("m37x53", 0, 0), ("stack2_3x5", 0, 0), ("m48x64", 0, 0), ("m37x53", 2, 0), ("stack2_3x5", 0, 1),
                                                       ("m2x2", 0, 0)])
def test_kill_map_holds_both_masks_in_their_bits(pt, name, flow_shift, out_shift):
    """Bit 0 = occlusion (any non-zero byte of the map), bit 1 = the fixture's mask, nothing else."""
    stack, want = mask_case(name)
    rng = np.random.default_rng(len(name) + out_shift)
    occ = (rng.uniform(size=stack.shape[:3]) < 0.3).astype(np.uint8) * rng.integers(1, 256, size=stack.shape[:3]).astype(np.uint8)
    kill = device_mask(pt, stack, 0.02, flow_shift=flow_shift, out_shift=out_shift, occ=occ)
    assert np.array_equal(kill, (occ != 0).astype(np.uint8) | (want["mb002"].astype(np.uint8) << 1))


def test_python_motion_boundary_on_a_device_tensor(pt):
    stack, want = mask_case("m48x64")
    got = pt.trajectory.motion_boundary(pt.torch.from_numpy(stack[0]).cuda(), 0.3)
    assert got.is_cuda and got.dtype == pt.torch.bool and np.array_equal(got.cpu().numpy(), want["mb03"][0])


@pytest.mark.parametrize("thres", [float("nan"), float("inf"), -0.5])
def test_option_refuses_a_bad_threshold(pt, thres):
    ctx = pt.hip.context()
    with pytest.raises(pt.hip.PsfmError) as e:
        ctx.set_motion_boundary(True, thres)
    assert e.value.status == pt.hip.PSFM_ERR_ARG


# ---- whole sequences ---------------------------------------------------------------------------------------------------------------

_inputs = {}


def sequence(pt, name, optimize):
    """The fixture, its inputs on the device (re-synthesised from the seed, checked against the fixture's hash) and the device's
    occlusion maps; built once per case."""
    if name not in _inputs:
        g = golden(name)
        d = psfm_synth.synth_realistic(int(g["T"]), int(g["H"]), int(g["W"]), seed=int(g["seed"]), stride2=optimize,
                                       **dict(psfm_synth.REALISTIC, **SEQ_SYNTH))
        assert input_hash(d) == str(g["input_hash"]), "psfm_synth.synth_realistic no longer reproduces this fixture's inputs"
        dev = {k: pt.torch.from_numpy(np.stack(v)).cuda() for k, v in d.items()}
        dev["occ"] = pt.utils.flow_check_device(dev["flows_f"], dev["flows_b"], 1.0)[1]
        if optimize:
            dev["occ2"] = pt.utils.flow_check_device(dev["flows_f2"], dev["flows_b2"], 1.0)[1]
        _inputs[name] = (g, dev)
    return _inputs[name]


def assert_equals(R, g, key, tol):
    assert len(R) == len(g[key + "_birth"]) and R.n_points == len(g[key + "_xy"])
    assert np.array_equal(R.birth, g[key + "_birth"]) and np.array_equal(R.length, g[key + "_length"])
    if tol == 0.0:
        assert np.array_equal(R.xy, g[key + "_xy"])
    else:
        err = float(np.abs(R.xy - g[key + "_xy"]).max())
        print(key, "max |dxy|", err)
        assert err <= tol, err
        for k in ("iterations", "successful_steps", "termination", "dogleg_nonGN"):
            assert [s[k] for s in R.solve_stats] == g["%s_solve_%s" % (key, k)].tolist(), k


@pytest.mark.parametrize("name", SEQ_TRACK)
def test_track_with_and_without_the_option(pt, name):
    g, d = sequence(pt, name, False)
    r = int(g["ratio"])
    assert not np.array_equal(g["mb_length"], g["shipped_length"])
    for R in (pt.trajectory.run_connect(d["flows_f"], d["flows_b"], None, None, 1.0, r, motion_boundary=True),
              pt.trajectory.run_track(d["flows_f"], d["occ"], None, None, r, motion_boundary=True)):
        assert R.info["chain_mode"] == 1
        assert_equals(R, g, "mb", 0.0)
    for R in (pt.trajectory.run_connect(d["flows_f"], d["flows_b"], None, None, 1.0, r),
              pt.trajectory.run_track(d["flows_f"], d["occ"], None, None, r)):
        assert_equals(R, g, "shipped", 0.0)


def test_persistent_mode_with_the_option_runs_per_frame(pt):
    g, d = sequence(pt, SEQ_TRACK[0], False)
    r = int(g["ratio"])
    ctx = pt.hip.context()
    try:
        ctx.set_chain_mode(2)
        for R in (pt.trajectory.run_connect(d["flows_f"], d["flows_b"], None, None, 1.0, r, motion_boundary=True),
                  pt.trajectory.run_track(d["flows_f"], d["occ"], None, None, r, motion_boundary=True)):
            assert R.info["chain_mode"] == 1
            assert_equals(R, g, "mb", 0.0)
        assert pt.trajectory.run_track(d["flows_f"], d["occ"], None, None, r).info["chain_mode"] == 2       # off again: the loop
    finally:
        ctx.set_chain_mode(0)


@pytest.mark.parametrize("solver", [0, 1, 2])
def test_track_optimize_with_and_without_the_option(pt, solver):
    """solver 0 adaptive, 1 launch chain, 2 fused solve: every form that follows a separate chain step."""
    g, d = sequence(pt, SEQ_OPT[0], True)
    r = int(g["ratio"])
    ctx = pt.hip.context()
    try:
        ctx.set_solver(solver, 0)
        for R in (pt.trajectory.run_connect(d["flows_f"], d["flows_b"], d["flows_f2"], d["flows_b2"], 1.0, r, motion_boundary=True),
                  pt.trajectory.run_track(d["flows_f"], d["occ"], d["flows_f2"], d["occ2"], r, motion_boundary=True)):
            assert R.info["chain_mode"] == 1
            assert_equals(R, g, "mb", TOL)
        if solver == 0:
            assert_equals(pt.trajectory.run_connect(d["flows_f"], d["flows_b"], d["flows_f2"], d["flows_b2"], 1.0, r), g, "shipped", TOL)
    finally:
        ctx.set_solver(0, 0)


def test_occ_returned_by_connect_stays_zero_one(pt):
    torch = pt.torch
    g, d = sequence(pt, SEQ_TRACK[1], False)
    n, H, W = (int(x) for x in d["flows_f"].shape[:3])
    ctx = pt.hip.context()
    occ = torch.full((n, H, W), SENTINEL8, dtype=torch.uint8, device="cuda")
    info = pt.hip.TrackInfo()
    ctx.set_motion_boundary(True, 0.02)
    try:
        pt.hip.check(pt.hip.lib().psfm_connect(ctx.handle, pt.hip.ptr(d["flows_f"]), pt.hip.ptr(d["flows_b"]), None, None, n, H, W, 1.0,
                                               int(g["ratio"]), pt.hip.ptr(occ), None, ctypes.byref(info),
                                               pt.hip.current_stream_ptr(ctx.device)))
    finally:
        ctx.set_motion_boundary(False)
    assert int(info.n_traj) == len(g["mb_birth"]) and int(info.chain_mode) == 1
    assert torch.equal(occ, d["occ"]) and int(occ.max()) == 1


def test_batch_and_sharded_engines_refuse_the_option(pt):
    torch = pt.torch
    g, d = sequence(pt, SEQ_TRACK[0], False)
    n, H, W = (int(x) for x in d["flows_f"].shape[:3])
    r = int(g["ratio"])
    L = pt.hip.lib()
    ctxs = pt.hip.batch_contexts(2)
    vp = ctypes.c_void_p
    handles = (vp * 2)(*[c.handle for c in ctxs])
    ff = (vp * 2)(d["flows_f"].data_ptr(), d["flows_f"].data_ptr())
    fb = (vp * 2)(d["flows_b"].data_ptr(), d["flows_b"].data_ptr())
    nf = (ctypes.c_int * 2)(n, n)
    infos = (pt.hip.TrackInfo * 2)()
    ctxs[1].set_motion_boundary(True, 0.02)
    try:
        st = L.psfm_connect_batch(handles, 2, ff, fb, None, None, nf, H, W, 1.0, r, infos, pt.hip.current_stream_ptr(ctxs[0].device))
        assert st == pt.hip.PSFM_ERR_ARG and b"psfm_ctx_set_motion_boundary" in L.psfm_last_error()
        G = ((H + r - 1) // r) * ((W + r - 1) // r)
        maps = torch.zeros(2 * (G + 128), dtype=torch.uint8, device="cuda")
        st = L.psfm_shard_begin(ctxs[1].handle, n, H, W, r, 0, G, 0, pt.hip.ptr(maps), G + 128, pt.hip.current_stream_ptr(ctxs[1].device))
        assert st == pt.hip.PSFM_ERR_ARG and b"psfm_ctx_set_motion_boundary" in L.psfm_last_error()
    finally:
        ctxs[1].set_motion_boundary(False)
    # the Python driver of a batch loops over psfm_connect instead
    seqs = [(d["flows_f"], d["flows_b"], None, None), (d["flows_f"][:5], d["flows_b"][:5], None, None)]
    cs, infos = pt.trajectory.run_connect_batch(seqs, 1.0, r, motion_boundary=True)
    assert_equals(pt.trajectory._result_to_host(cs[0], infos[0]), g, "mb", 0.0)
    short = pt.trajectory.run_connect(d["flows_f"][:5], d["flows_b"][:5], None, None, 1.0, r, motion_boundary=True)
    R1 = pt.trajectory._result_to_host(cs[1], infos[1])
    assert np.array_equal(R1.birth, short.birth) and np.array_equal(R1.length, short.length) and np.array_equal(R1.xy, short.xy)
    # ... and the batch engine itself still takes these contexts with the option off
    cs, infos = pt.trajectory.run_connect_batch(seqs[:1] * 2, 1.0, r)
    assert_equals(pt.trajectory._result_to_host(cs[1], infos[1]), g, "shipped", 0.0)
