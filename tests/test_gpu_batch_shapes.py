"""psfm_connect_batch over sequences of DIFFERENT frame sizes in one call (h = w = 0, every context carrying its sequence's size:
psfm_ctx_set_frame_size; run_connect_batch does that by itself when the shapes differ): the frame launches read every dimension from
the sequence's row, flow_check and the kill maps run over a grid flattened over the sequences (psfm_flow_check_x2v_shapes_kernel,
psfm_kill_map_shapes_kernel; index rules: tests/test_batch_shapes_host.py), and the one segmented finalize sorts the records of all
sequences with the index bits of the widest grid.  Every sequence must be what it is alone: the oracle's result bit for bit in track
mode; ids, lengths and every solve's decisions exact and positions within the suite's 1e-4 px with path consistency; the bytes of the
same sequences grouped by size; the bytes of one psfm_connect each with the motion-boundary option.

Shapes: small frames whose pixel counts are 0 and 2 mod 4, with W odd, of fewer than 8 and of more than 8 flow_check chunks, one frame
far larger than its neighbours (480 x 854: banded over the XCDs), grids of 1 200 to 7 875 points (11 to 13 index bits), sequences of
1 to 13 flows; a frame of 960 pixels or of an odd pixel count sends every stack of its batch through the per-stack launches up front."""
import ctypes

import numpy as np
import pytest

import psfm_synth
from test_gpu_batch import TOL, _dev, _oracle

pytestmark = pytest.mark.gpu
ROUNDING = 1e-9          # px: what include/psfm.h promises between two runs of one path-consistency sequence
STATS = ("iterations", "successful_steps", "termination", "dogleg_nonGN")


@pytest.fixture(scope="module")
def pt():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from point_trajectory import trajectory, _hip
    first = _hip.context()

    class NS:
        pass
    ns = NS()
    ns.trajectory, ns.hip, ns.torch = trajectory, _hip, torch
    # test 7's reference: psfm_connect for a sequence ALONE on a context of its own, pinned to the launch chain
    ns.ref = _hip.Context(first.device)
    ns.ref.set_solver(1, 0)
    yield ns
    ns.ref.close()
    # the sequences built here go back to the driver with the module: the tests behind this one in a session find the caching
    # allocator as they would without it
    _seqs.clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def sizes_left_clear(pt):
    """After every test no batch context of the thread carries a frame size: a call with h = w = 0 on them is refused."""
    yield
    ctxs = pt.hip.batch_contexts(2)
    st, _, _ = call_c(pt, [seq(pt, 64, 96, 3, 900, 0.05, 0, False)["dev"]] * 2, 2, 0, 0, ctxs=ctxs)
    assert st == pt.hip.PSFM_ERR_ARG and b"context 0 has no frame size" in pt.hip.lib().psfm_last_error()


_seqs = {}


def seq(pt, H, W, T, seed, sigma, occluders, opt, realistic=False):
    """One synthetic sequence (T frames: T - 1 flows), on the host and on the device; its oracle result on demand.  Built once."""
    key = (H, W, T, seed, sigma, occluders, opt, realistic)
    if key not in _seqs:
        if realistic:
            d = psfm_synth.synth_realistic(T, H, W, seed=seed, stride2=opt, **psfm_synth.REALISTIC)
        else:
            d = psfm_synth.synth_sequence(T, H, W, seed=seed, sigma=sigma, n_occluders=occluders, stride2=opt)
        _seqs[key] = dict(host=d, dev=_dev(pt, d, opt), opt=opt, oracle={})
    return _seqs[key]


def oracle(s, r):
    if r not in s["oracle"]:
        s["oracle"][r] = _oracle(s["host"], 1.0, r, s["opt"])
    return s["oracle"][r]


def shape_of(s):
    return int(s["dev"][0].shape[1]), int(s["dev"][0].shape[2])


def results(pt, ctxs, infos):
    """Every sequence's result on the host (the batch contexts are reused by the thread's next batch)."""
    return [pt.trajectory._result_to_host(c, i) for c, i in zip(ctxs, infos)]


def same_bytes(A, B, what):
    for k in ("birth", "length", "off", "xy"):
        a, b = np.asarray(getattr(A, k)), np.asarray(getattr(B, k))
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), (what, k)


def same_to_rounding(A, B, what, tol=ROUNDING):
    """Path consistency between two device runs: ids, births, lengths, offsets and every solve's decisions exact, positions to tol."""
    for k in ("birth", "length", "off"):
        assert np.array_equal(np.asarray(getattr(A, k)), np.asarray(getattr(B, k))), (what, k)
    assert len(A.solve_stats) == len(B.solve_stats), what
    for k in STATS:
        assert [s[k] for s in A.solve_stats] == [s[k] for s in B.solve_stats], (what, k)
    err = float(np.abs(A.xy - B.xy).max()) if A.xy.size else 0.0
    print("%s: max |dxy| %.3g px" % (what, err))
    assert err <= tol, (what, err)


def check_oracle(R, O, opt, what):
    assert len(R) == O.n_traj, (what, len(R), O.n_traj)
    assert np.array_equal(R.birth, O.birth) and np.array_equal(R.length, O.length), what
    assert np.array_equal(R.off, np.concatenate([[0], np.cumsum(O.length)])), what
    if not opt:
        assert np.array_equal(R.xy, O.xy), (what, float(np.abs(R.xy - O.xy).max()))
        return
    err = float(np.abs(R.xy - O.xy).max()) if R.xy.size else 0.0
    print("%s: max |dxy| against the oracle %.3g px" % (what, err))
    assert err <= TOL, (what, err)
    for k in STATS[:3]:
        assert [s[k] for s in R.solve_stats] == [s[k] for s in O.solves], (what, k)


def call_c(pt, seqs, r, h, w, sizes=None, mb=None, ctxs=None):
    """psfm_connect_batch through the C ABI: context i gets psfm_ctx_set_frame_size(sizes[i]) (None: none) and
    psfm_ctx_set_motion_boundary(1, mb[i]) (None: off); both are cleared again.  Returns (status, contexts, infos)."""
    B = len(seqs)
    vp = ctypes.c_void_p
    opt = seqs[0][2] is not None
    keep = []

    def ptrs(k):
        out = []
        for s in seqs:
            t = s[k]
            if t.numel() == 0:       # (a one-flow sequence has no stride-2 stack: never read, but not NULL)
                t = pt.torch.zeros((1,) + tuple(s[0].shape[1:]), dtype=pt.torch.float32, device="cuda")
                keep.append(t)
            out.append(t.data_ptr())
        return (vp * B)(*out)
    ctxs = ctxs or pt.hip.batch_contexts(B)
    infos = (pt.hip.TrackInfo * B)()
    nf = (ctypes.c_int * B)(*[int(s[0].shape[0]) for s in seqs])
    try:
        for c, sz in zip(ctxs, sizes or [None] * B):
            if sz is not None:
                c.set_frame_size(*sz)
        for c, t in zip(ctxs, mb or [None] * B):
            if t is not None:
                c.set_motion_boundary(True, t)
        st = pt.hip.lib().psfm_connect_batch((vp * B)(*[c.handle for c in ctxs]), B, ptrs(0), ptrs(1), ptrs(2) if opt else None,
                                             ptrs(3) if opt else None, nf, h, w, 1.0, r, infos, pt.hip.current_stream_ptr(ctxs[0].device))
    finally:
        for c in ctxs:
            c.set_frame_size(0, 0)
            c.set_motion_boundary(False)
    return st, ctxs, [infos[i] for i in range(B)]


# ---- 1. track mode against the oracle ----
# (sample_ratio, [(H, W, frames, seed, sigma, occluders)])
SIX = [(120, 200, 9, 201, 0.05, 1), (96, 130, 6, 202, 0.3, 3), (75, 102, 12, 203, 0.1, 2), (64, 97, 5, 204, 0.05, 0), (81, 100, 2, 205, 0.05, 0),
       (150, 210, 7, 206, 0.2, 2)]
TRACK_BATCHES = {
    "six-shapes": (2, SIX),                                               # every stack passes the vector test; 11 to 13 index bits
    "with-960-pixels": (2, SIX + [(24, 40, 5, 207, 0.05, 1)]),            # fewer than 1024 pixels: every stack up front
    "with-an-odd-pixel-count": (2, SIX[:3] + [(75, 101, 6, 208, 0.1, 1)]),
    "one-far-larger": (4, [(480, 854, 7, 211, 0.05, 2), (120, 200, 9, 212, 0.3, 3), (60, 80, 12, 213, 0.1, 1)]),
    "dense": (1, [(96, 130, 8, 221, 0.05, 1), (64, 96, 5, 222, 0.35, 2)]),
    "generic-ratio": (3, [(135, 240, 10, 231, 0.05, 1), (90, 140, 6, 232, 0.25, 2)]),
}


def track_batch(pt, name):
    r, spec = TRACK_BATCHES[name]
    return r, [seq(pt, H, W, T, seed, sg, no, False) for (H, W, T, seed, sg, no) in spec]


@pytest.mark.parametrize("name", sorted(TRACK_BATCHES))
def test_track_mode_against_the_oracle(pt, name):
    """flow_check + track of sequences of different frame sizes in one call: every sequence bit for bit the oracle's, every one still
    in the batch (chain_mode 3); then once more on the warm contexts in reversed order, so that every context holds another shape."""
    r, S = track_batch(pt, name)
    assert len({shape_of(s) for s in S}) == len(S)
    for order in (list(range(len(S))), list(range(len(S)))[::-1]):
        ctxs, infos = pt.trajectory.run_connect_batch([S[k]["dev"] for k in order], 1.0, r)
        assert [int(i.chain_mode) for i in infos] == [3] * len(S)
        for pos, (k, R) in enumerate(zip(order, results(pt, ctxs, infos))):
            check_oracle(R, oracle(S[k], r), False, (name, "sequence", k, "at", pos))


# ---- 2. 64 sequences ----
TINY = [(32, 40), (36, 44), (40, 51), (33, 48)]


def test_sixty_four_sequences_and_a_batch_of_one(pt):
    """64 sequences of 3 flows that cycle four tiny shapes: the first and the last against the oracle, every one against psfm_connect for
    it alone, byte for byte.  And n_seq = 1 with h = w = 0: the context's size is the call's."""
    r = 2
    S = [seq(pt, TINY[k % 4][0], TINY[k % 4][1], 4, 300 + k, 0.05 + 0.05 * (k % 5), k % 3, False) for k in range(64)]
    ctxs, infos = pt.trajectory.run_connect_batch([s["dev"] for s in S], 1.0, r)
    assert [int(i.chain_mode) for i in infos] == [3] * 64
    got = results(pt, ctxs, infos)
    for k in (0, 63):
        check_oracle(got[k], oracle(S[k], r), False, ("sequence", k))
    for k, s in enumerate(S):
        a, b, _, _ = s["dev"]
        same_bytes(got[k], pt.trajectory.run_connect(a, b, None, None, 1.0, r), ("sequence", k))
    st, ctxs, infos = call_c(pt, [S[2]["dev"]], r, 0, 0, sizes=[TINY[2]])
    assert st == pt.hip.PSFM_OK, pt.hip.lib().psfm_last_error()
    same_bytes(results(pt, ctxs, infos)[0], got[2], "a batch of one")


# ---- 3. path consistency against the oracle ----
# (sample_ratio, [(H, W, frames, seed, sigma, occluders)], solver policy of the contexts: 0 adaptive, 2 fused solve)
# The noise levels are those of tests/test_gpu_batch.py::OPT_BATCHES.  A sequence whose solves reject steps leaves its batch under the
# adaptive policy, whatever the frame sizes of its neighbours, and whether they do depends on the noise the seed draws:
#   * dense: 20 seed pairs tried at sigma 0.05, both sequences stay with 4 of them (these seeds among them), one of the two with 7;
#   * five-shapes: the 64 x 96 x 14 sequence at sigma 0.08 left with every one of 26 seeds tried (13 seeds, with and without an
#     occluder) while its four neighbours stayed every time -- it is the noise level that rejects steps there, not the seed.  That
#     batch therefore runs on contexts set to the fused solve (psfm_ctx_set_solver(ctx, 2, 0): "keeps a sequence in", psfm_batch.hip),
#     where a solve that rejects steps is redone by the launch chain at the checkpoint and the sequence goes on in the batch -- the
#     batched solves over rows of different frame sizes are what runs, for all five, and the assert below stays what it is.
OPT_BATCHES = {
    "five-shapes": (2, [(120, 200, 9, 261, 0.05, 2), (64, 96, 14, 262, 0.08, 1), (96, 130, 7, 263, 0.03, 1), (150, 210, 2, 264, 0.05, 0),
                        (80, 120, 3, 265, 0.05, 1)], 2),
    "dense": (1, [(64, 96, 10, 283, 0.05, 1), (48, 80, 8, 284, 0.05, 1)], 0),
}


@pytest.mark.parametrize("name", sorted(OPT_BATCHES))
def test_path_consistency_against_the_oracle(pt, name):
    """flow_check x 2 + track_optimize of sequences of different frame sizes in one call: ids, lengths and every solve's iterations,
    termination and successful steps exact, positions within the suite's 1e-4 px -- and every sequence still in the batch (chain_mode
    3): one that left would have run alone and say nothing about the batched solves."""
    r, spec, policy = OPT_BATCHES[name]
    S = [seq(pt, H, W, T, seed, sg, no, True) for (H, W, T, seed, sg, no) in spec]
    for c in pt.hip.batch_contexts(len(S)):
        c.set_solver(policy, 0)
    # (the adaptive policy carries the iterations per fused launch from a context's last call -- whatever test that was -- into this
    # one, and a K too small for a sequence's first solve sends it out of the batch: the first call settles every context's K, as in
    # tests/test_gpu_batch_together.py; both calls are held to the oracle, the second to the batch as well)
    try:
        for attempt in ("settling", "settled"):
            ctxs, infos = pt.trajectory.run_connect_batch([s["dev"] for s in S], 1.0, r)
            modes = [int(i.chain_mode) for i in infos]
            print(name, attempt, "modes", modes)
            for k, R in enumerate(results(pt, ctxs, infos)):
                check_oracle(R, oracle(S[k], r), True, (name, attempt, "sequence", k))
    finally:
        for c in pt.hip.batch_contexts(len(S)):
            c.set_solver(0, 0)
    assert modes == [3] * len(S), modes


# ---- 4. equal to the sequences grouped by size ----
@pytest.mark.parametrize("opt", [False, True])
def test_equal_to_one_call_per_frame_size(pt, opt):
    """Two shapes with three sequences each, interleaved: one call for all six against one call per shape.  Track mode: every byte.
    Path consistency: ids, births, lengths, offsets and the solves' decisions exact, positions to 1e-9 px."""
    r = 2
    shapes = [(96, 130), (75, 102)]
    S = [seq(pt, shapes[k % 2][0], shapes[k % 2][1], 6 + k, 400 + k, 0.04, k % 2, opt) for k in range(6)]
    ctxs, infos = pt.trajectory.run_connect_batch([s["dev"] for s in S], 1.0, r)
    modes = [int(i.chain_mode) for i in infos]
    mixed = results(pt, ctxs, infos)
    for g in range(2):
        ks = [k for k in range(6) if k % 2 == g]
        ctxs, infos = pt.trajectory.run_connect_batch([S[k]["dev"] for k in ks], 1.0, r)
        for k, R in zip(ks, results(pt, ctxs, infos)):
            (same_to_rounding if opt else same_bytes)(mixed[k], R, ("opt" if opt else "track", "sequence", k))
    print("modes of the call for all six", modes)
    if not opt:
        assert modes == [3] * 6


# ---- 5. one frame size through h = w = 0 ----
@pytest.mark.parametrize("opt", [False, True])
def test_equal_sizes_through_the_contexts_are_the_call_with_that_size(pt, opt):
    H, W, r = 96, 130, 2
    S = [seq(pt, H, W, 6 + k, 500 + k, 0.05, 1, opt) for k in range(3)]
    st, ctxs, infos = call_c(pt, [s["dev"] for s in S], r, H, W, sizes=[(40, 40)] * 3)      # (h, w > 0: the stored sizes are ignored)
    assert st == pt.hip.PSFM_OK, pt.hip.lib().psfm_last_error()
    want, census = results(pt, ctxs, infos), ctxs[0].connect_batch_census()
    st, ctxs, infos = call_c(pt, [s["dev"] for s in S], r, 0, 0, sizes=[(H, W)] * 3)
    assert st == pt.hip.PSFM_OK, pt.hip.lib().psfm_last_error()
    assert ctxs[0].connect_batch_census() == census
    for k, (A, B) in enumerate(zip(results(pt, ctxs, infos), want)):
        (same_to_rounding if opt else same_bytes)(A, B, ("sequence", k))
        check_oracle(A, oracle(S[k], r), opt, ("sequence", k))


# ---- 6. motion boundary ----
MB_SHAPES = [(64, 97), (75, 102), (96, 130), (60, 80)]       # W odd with P even; P = 2 mod 4; P = 0 mod 4 twice
MB_THRES = [0.02, 0.05, 0.01, 0.03, 0.02]


@pytest.mark.parametrize("extra", [None, (24, 40), (75, 101)], ids=["side-stream", "with-960-pixels", "with-an-odd-pixel-count"])
@pytest.mark.parametrize("opt", [False, True])
def test_motion_boundary_batch_against_one_connect_each(pt, opt, extra):
    """The option on every context, each with its own threshold: the batched launches (kill maps of all shapes in one launch per chunk)
    against one psfm_connect per sequence -- every byte in track mode; with path consistency as between two runs."""
    r = 2
    shapes = MB_SHAPES + ([extra] if extra else [])
    S = [seq(pt, H, W, 7 + k % 3, 600 + k, 0.0, 0, opt, realistic=True) for k, (H, W) in enumerate(shapes)]
    thres = MB_THRES[:len(S)]
    if opt:
        for c in pt.hip.batch_contexts(len(S)):
            c.set_solver(2, 0)         # (realistic flows: solves that reject steps are redone at the checkpoint, the sequence stays)
    try:
        ctxs, infos = pt.trajectory.run_connect_batch([s["dev"] for s in S], 1.0, r, motion_boundary=True, mb_thres=thres, mb_engine="batch")
        modes = [int(i.chain_mode) for i in infos]
        got = results(pt, ctxs, infos)
    finally:
        for c in pt.hip.batch_contexts(len(S)):
            c.set_solver(0, 0)
    assert modes == [3] * len(S), modes
    ctxs, infos = pt.trajectory.run_connect_batch([s["dev"] for s in S], 1.0, r, motion_boundary=True, mb_thres=thres, mb_engine="loop")
    for k, R in enumerate(results(pt, ctxs, infos)):
        (same_to_rounding if opt else same_bytes)(got[k], R, ("sequence", k))
    off = pt.trajectory.run_connect(S[0]["dev"][0], S[0]["dev"][1], S[0]["dev"][2], S[0]["dev"][3], 1.0, r)
    assert not (len(off) == len(got[0]) and np.array_equal(off.length, got[0].length)), "the batch ran without the second verdict"


# ---- 7. the joint redo ----
def test_sequences_that_leave_are_redone_together(pt):
    """Contexts pinned to the launch chain and redo="together": every sequence goes through the joint redo (chain_mode 8) -- the batched
    chain step and the frame-mode multi-problem launch chain over rows of different frame sizes, on the maps the flattened launches
    made -- and equals psfm_connect for it alone on a pinned context, under the criteria of tests/test_gpu_batch_together.py."""
    from test_gpu_batch_together import assert_equal_to_references, reference, solver_modes
    r = 2
    spec = [(120, 200, 6, 701), (64, 97, 9, 702), (75, 102, 3, 703)]
    S = [seq(pt, H, W, T, seed, psfm_synth.HARD["sigma"], psfm_synth.HARD["n_occluders"], True) for (H, W, T, seed) in spec]
    with solver_modes(pt, [(1, 0)] * len(S)) as ctxs0:
        ctxs, infos = pt.trajectory.run_connect_batch([s["dev"] for s in S], 1.0, r, redo="together")
        modes, census = [int(i.chain_mode) for i in infos], ctxs[0].connect_batch_census()
        got = results(pt, ctxs, infos)
        capacity = ctxs0[0]._capacity.get(("batch", tuple(sorted({shape_of(s) for s in S})), r, True), (2.0, 8.0))
    print("modes", modes, "census", census)
    assert modes == [8] * len(S) and census["n_left"] == census["n_together"] == len(S)
    for k, R in enumerate(got):
        check_oracle(R, oracle(S[k], r), True, ("sequence", k))
    assert_equal_to_references(got, [reference(pt, s["host"], r, capacity=capacity) for s in S])


# ---- 8. refusals ----
def test_refusals_and_a_valid_call_behind_them(pt):
    L, ERR = pt.hip.lib(), pt.hip.PSFM_ERR_ARG
    r = 2
    S = [seq(pt, H, W, 5, 800 + k, 0.05, 1, False) for k, (H, W) in enumerate([(64, 96), (48, 80), (60, 90)])]
    devs, sizes = [s["dev"] for s in S], [shape_of(s) for s in S]
    ctxs = pt.hip.batch_contexts(3)
    assert call_c(pt, devs, r, 0, 96, sizes=sizes)[0] == ERR and call_c(pt, devs, r, 64, 0, sizes=sizes)[0] == ERR
    st, _, _ = call_c(pt, devs, r, 0, 0, sizes=[sizes[0], None, None])
    assert st == ERR and b"context 1 has no frame size" in L.psfm_last_error(), L.psfm_last_error()
    assert L.psfm_ctx_set_frame_size(ctxs[0].handle, -1, 5) == ERR and L.psfm_ctx_set_frame_size(ctxs[0].handle, 1, 5) == ERR
    st, _, _ = call_c(pt, devs, r, 0, 0, sizes=sizes, mb=[0.02, None, 0.02])
    assert st == ERR and b"psfm_ctx_set_motion_boundary" in L.psfm_last_error(), L.psfm_last_error()
    st, ctxs, infos = call_c(pt, devs, r, 0, 0, sizes=sizes)
    assert st == pt.hip.PSFM_OK, L.psfm_last_error()
    for k, R in enumerate(results(pt, ctxs, infos)):
        check_oracle(R, oracle(S[k], r), False, ("sequence", k))


# ---- 9. a non-default stream ----
def test_on_a_non_default_stream(pt):
    r, S = track_batch(pt, "six-shapes")
    ctxs, infos = pt.trajectory.run_connect_batch([s["dev"] for s in S], 1.0, r)
    want = results(pt, ctxs, infos)
    stream = pt.torch.cuda.Stream()
    stream.wait_stream(pt.torch.cuda.current_stream())
    with pt.torch.cuda.stream(stream):
        ctxs, infos = pt.trajectory.run_connect_batch([s["dev"] for s in S], 1.0, r)
        got = results(pt, ctxs, infos)
    stream.synchronize()
    for k, (A, B) in enumerate(zip(got, want)):
        same_bytes(A, B, ("sequence", k))
