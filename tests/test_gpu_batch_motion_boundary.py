"""psfm_connect_batch with the motion-boundary option on in every context of the batch: the batched frame launches form the second
verdict (the MB forms of psfm_chain_step_batch_kernel / psfm_seq_batch_kernel) from kill maps that ONE launch per flow_check chunk
builds for all sequences (psfm_kill_map_batch_kernel).  The fixture sequences must equal the REFERENCE's own track / track_optimize
run with the motion-boundary form of step_forward (tests/golden/make_motion_boundary_golden.py), every other sequence psfm_connect
with the option on that sequence alone; every test leaves the option off on the thread's batch contexts."""
import ctypes

import numpy as np
import pytest

import psfm_synth
from _motion_boundary_np import SEQ_OPT, SEQ_SYNTH, SEQ_TRACK
from test_gpu_motion_boundary import assert_equals, sequence
from test_gpu_whole_sequence import TOL          # track_optimize positions: the suite's bar, as tests/test_gpu_motion_boundary.py uses it

pytestmark = pytest.mark.gpu
STATS = ("iterations", "successful_steps", "termination", "dogleg_nonGN")


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


@pytest.fixture(autouse=True)
def option_left_clean(pt):
    """After every test: the option is off on the thread's batch contexts -- a plain batch on them stays in the batch and equals the
    shipped fixture."""
    yield
    g, d = sequence(pt, SEQ_TRACK[0], False)
    seq = (d["flows_f"], d["flows_b"], None, None)
    ctxs, infos = pt.trajectory.run_connect_batch([seq, seq], 1.0, int(g["ratio"]))
    for c, i in zip(ctxs, infos):
        assert int(i.chain_mode) == 3
        assert_equals(pt.trajectory._result_to_host(c, i), g, "shipped", 0.0)


_others = {}


def other(pt, H, W, T, seed, opt):
    """Another seed of the fixtures' scene model, on the device (built once)."""
    key = (H, W, T, seed, opt)
    if key not in _others:
        d = psfm_synth.synth_realistic(T, H, W, seed=seed, stride2=opt, **dict(psfm_synth.REALISTIC, **SEQ_SYNTH))
        _others[key] = {k: pt.torch.from_numpy(np.stack(v)).cuda() for k, v in d.items()}
    return _others[key]


def cut(d, n, opt):
    """The first n flows of a sequence (and the n - 1 stride-2 flows that go with them)."""
    return (d["flows_f"][:n], d["flows_b"][:n], d["flows_f2"][:max(n - 1, 0)] if opt else None, d["flows_b2"][:max(n - 1, 0)] if opt else None)


_singles = {}


def single(pt, key, seq, r, mb, thres=0.02):
    """psfm_connect on one sequence alone (option on / off), on the thread's own context: computed once per sequence."""
    k = (key, r, mb, thres)
    if k not in _singles:
        _singles[k] = pt.trajectory.run_connect(seq[0], seq[1], seq[2], seq[3], 1.0, r, motion_boundary=mb, mb_thres=thres)
    return _singles[k]


def connect_batch_c(pt, seqs, r, mb_thres):
    """psfm_connect_batch through the C ABI with psfm_ctx_set_motion_boundary(1, mb_thres[i]) on context i (None: off).  Returns
    (status, contexts, infos); the option is off again afterwards."""
    B = len(seqs)
    vp = ctypes.c_void_p
    opt = seqs[0][2] is not None
    H, W = int(seqs[0][0].shape[1]), int(seqs[0][0].shape[2])
    keep = []

    def ptrs(k):
        out = []
        for s in seqs:
            t = s[k]
            if t.numel() == 0:       # (a one-flow sequence has no stride-2 stack: never read, but not NULL)
                t = pt.torch.zeros((1, H, W, 2), dtype=pt.torch.float32, device="cuda")
                keep.append(t)
            out.append(t.data_ptr())
        return (vp * B)(*out)
    ctxs = pt.hip.batch_contexts(B)
    infos = (pt.hip.TrackInfo * B)()
    nf = (ctypes.c_int * B)(*[int(s[0].shape[0]) for s in seqs])
    try:
        for c, t in zip(ctxs, mb_thres):
            if t is not None:
                c.set_motion_boundary(True, t)
        st = pt.hip.lib().psfm_connect_batch((vp * B)(*[c.handle for c in ctxs]), B, ptrs(0), ptrs(1), ptrs(2) if opt else None,
                                             ptrs(3) if opt else None, nf, H, W, 1.0, r, infos, pt.hip.current_stream_ptr(ctxs[0].device))
    finally:
        for c in ctxs:
            c.set_motion_boundary(False)
    return st, ctxs, [infos[i] for i in range(B)]


def same(A, B, tol):
    assert len(A) == len(B) and np.array_equal(A.birth, B.birth) and np.array_equal(A.length, B.length)
    if tol == 0.0:
        assert np.array_equal(A.xy, B.xy)
    else:
        err = float(np.abs(A.xy - B.xy).max()) if A.n_points else 0.0
        print("max |dxy|", err)
        assert err <= tol, err
        for k in STATS:
            assert [s[k] for s in A.solve_stats] == [s[k] for s in B.solve_stats], k


def track_batch(pt, name):
    """The fixture's sequence, its first 5 flows, its first flow only, and two other seeds."""
    g, d = sequence(pt, name, False)
    H, W, T = int(g["H"]), int(g["W"]), int(g["T"])
    n = int(d["flows_f"].shape[0])
    seqs = [cut(d, n, False), cut(d, 5, False), cut(d, 1, False),
            cut(other(pt, H, W, T, 101, False), n, False), cut(other(pt, H, W, T - 2, 102, False), n - 2, False)]
    keys = [(name, n), (name, 5), (name, 1), (name, "seed101"), (name, "seed102")]
    return g, seqs, keys


def check_track_batch(pt, g, seqs, keys, ctxs, infos, order):
    r = int(g["ratio"])
    for pos, k in enumerate(order):
        assert int(infos[pos].chain_mode) == 3, (k, int(infos[pos].chain_mode))
        R = pt.trajectory._result_to_host(ctxs[pos], infos[pos])
        if k == 0:
            assert_equals(R, g, "mb", 0.0)                                        # the reference's own run, bit for bit
        same(R, single(pt, keys[k], seqs[k], r, True), 0.0)
        if int(seqs[k][0].shape[0]) > 1:      # (with one flow nothing is looked at after a track died)
            off = single(pt, keys[k], seqs[k], r, False)
            assert not (len(off) == len(R) and np.array_equal(off.length, R.length)), "the batch ran the shipped rule"


@pytest.mark.parametrize("fc_chunk", [None, "2", "0"])
@pytest.mark.parametrize("name", SEQ_TRACK)
def test_track_batch_with_the_option(pt, monkeypatch, name, fc_chunk):
    """fc_chunk None: the default flow_check pipeline; "2": kill maps built two frames at a time behind their flow_check chunk on the
    side stream (48 x 64; the 37 x 53 frames have an odd pixel count, which the 16-byte-load flow_check cannot take: those stacks go
    up front whatever the chunk); "0": everything up front on the launch stream."""
    if fc_chunk is not None:
        monkeypatch.setenv("PSFM_BATCH_FC_CHUNK", fc_chunk)
    g, seqs, keys = track_batch(pt, name)
    r = int(g["ratio"])
    order = list(range(len(seqs)))
    st, ctxs, infos = connect_batch_c(pt, seqs, r, [0.02] * len(seqs))
    assert st == pt.hip.PSFM_OK, pt.hip.lib().psfm_last_error()
    check_track_batch(pt, g, seqs, keys, ctxs, infos, order)
    if fc_chunk is None:      # ... and again on the warm contexts, in reverse order
        order = order[::-1]
        st, ctxs, infos = connect_batch_c(pt, [seqs[k] for k in order], r, [0.02] * len(seqs))
        assert st == pt.hip.PSFM_OK, pt.hip.lib().psfm_last_error()
        check_track_batch(pt, g, seqs, keys, ctxs, infos, order)


def test_chunked_kill_maps_across_frame_ends(pt, monkeypatch):
    """46 x 65 = 2990 pixels: even, so the chunked flow_check pipeline takes the stacks, and 2 mod 4, so every second frame starts
    in the middle of a 4-byte word of the kill maps.  Chunks of two frames, and of three (chunk ends at odd frames): while the kill
    maps of a chunk are built, the occlusion maps of the next frame are not written yet."""
    H, W, r = 46, 65, 2
    ds = [other(pt, H, W, 8, 111, False), other(pt, H, W, 6, 112, False), other(pt, H, W, 8, 113, False)]
    seqs = [cut(ds[0], 7, False), cut(ds[1], 5, False), cut(ds[2], 2, False)]
    for chunk in ("2", "3"):
        monkeypatch.setenv("PSFM_BATCH_FC_CHUNK", chunk)
        st, ctxs, infos = connect_batch_c(pt, seqs, r, [0.02] * 3)
        assert st == pt.hip.PSFM_OK, pt.hip.lib().psfm_last_error()
        for k in range(3):
            assert int(infos[k].chain_mode) == 3
            R = pt.trajectory._result_to_host(ctxs[k], infos[k])
            same(R, single(pt, ("46x65", k), seqs[k], r, True), 0.0)
            assert not np.array_equal(single(pt, ("46x65", k), seqs[k], r, False).length, R.length)


def opt_batch(pt):
    """mb_opt_48x64x8_r2, its first 5 flows, its first 2 flows, and one other seed."""
    name = SEQ_OPT[0]
    g, d = sequence(pt, name, True)
    H, W, T = int(g["H"]), int(g["W"]), int(g["T"])
    n = int(d["flows_f"].shape[0])
    seqs = [cut(d, n, True), cut(d, 5, True), cut(d, 2, True), cut(other(pt, H, W, T, 103, True), n, True)]
    keys = [(name, n), (name, 5), (name, 2), (name, "seed103")]
    return g, seqs, keys


def check_opt_batch(pt, g, seqs, keys, ctxs, infos):
    r = int(g["ratio"])
    # the fixture's seven solves are all clean (iterations = successful steps + 1 <= 3, no dogleg): the adaptive solver keeps the
    # sequence in the batch, where the merged MB kernel runs its chain steps
    assert int(infos[0].chain_mode) == 3, int(infos[0].chain_mode)
    for k in range(len(seqs)):
        R = pt.trajectory._result_to_host(ctxs[k], infos[k])
        if k == 0:
            assert_equals(R, g, "mb", TOL)
        same(R, single(pt, keys[k], seqs[k], r, True), TOL)
        off = single(pt, keys[k], seqs[k], r, False)
        assert not (len(off) == len(R) and np.array_equal(off.length, R.length)), "the batch ran the shipped rule"


def test_track_optimize_batch_with_the_option(pt):
    g, seqs, keys = opt_batch(pt)
    iters, steps = g["mb_solve_iterations"], g["mb_solve_successful_steps"]
    assert (iters == steps + 1).all() and int(iters.max()) <= 3 and not g["mb_solve_dogleg_nonGN"].any()
    st, ctxs, infos = connect_batch_c(pt, seqs, int(g["ratio"]), [0.02] * len(seqs))
    assert st == pt.hip.PSFM_OK, pt.hip.lib().psfm_last_error()
    check_opt_batch(pt, g, seqs, keys, ctxs, infos)


def test_track_optimize_batch_with_the_option_rerun_untrimmed(pt, monkeypatch):
    """PSFM_BATCH_GRID_LANES=512 (as test_gpu_batch.py sets it): launches that cover 512 lanes of grids of 768 points raise overflow
    bit 16 and the batch -- kill maps included -- runs again with launches that cover the tables."""
    g, seqs, keys = opt_batch(pt)
    monkeypatch.setenv("PSFM_BATCH_GRID_LANES", "512")
    st, ctxs, infos = connect_batch_c(pt, seqs, int(g["ratio"]), [0.02] * len(seqs))
    assert st == pt.hip.PSFM_OK, pt.hip.lib().psfm_last_error()
    check_opt_batch(pt, g, seqs, keys, ctxs, infos)


def test_every_context_has_its_own_threshold(pt):
    name = SEQ_TRACK[0]
    g, d = sequence(pt, name, False)
    r = int(g["ratio"])
    seq = cut(d, int(d["flows_f"].shape[0]), False)
    # (the layered scene's boundaries are sharp: its masks at 0.02 and 0.05 are the same 780 pixels, at 1.0 they are 472 -- the third
    # context is the one that shows whose threshold a row's kill maps were built with)
    st, ctxs, infos = connect_batch_c(pt, [seq, seq, seq], r, [0.02, 0.05, 1.0])
    assert st == pt.hip.PSFM_OK, pt.hip.lib().psfm_last_error()
    A, B, C = (pt.trajectory._result_to_host(c, i) for c, i in zip(ctxs, infos))
    assert_equals(A, g, "mb", 0.0)
    same(B, single(pt, (name, "t005"), seq, r, True, 0.05), 0.0)
    same(C, single(pt, (name, "t1"), seq, r, True, 1.0), 0.0)
    assert not (len(A) == len(C) and np.array_equal(A.length, C.length)), "0.02 and 1.0 kill the same tracks here: pick another threshold"
    off = single(pt, (name, int(seq[0].shape[0])), seq, r, False)
    assert not (len(off) == len(C) and np.array_equal(off.length, C.length))


def test_contexts_that_disagree_are_refused(pt):
    g, d = sequence(pt, SEQ_TRACK[0], False)
    seq = cut(d, 3, False)
    for thr in ([0.02, None], [None, 0.02], [0.02, 0.02, None]):
        st, _, _ = connect_batch_c(pt, [seq] * len(thr), int(g["ratio"]), thr)
        assert st == pt.hip.PSFM_ERR_ARG and b"psfm_ctx_set_motion_boundary" in pt.hip.lib().psfm_last_error()


def test_consumers_on_a_member(pt):
    """result_to_trajectory_set on a batch context equals the one from run_connect."""
    name = SEQ_TRACK[0]
    g, seqs, keys = track_batch(pt, name)
    r = int(g["ratio"])
    ctxs, infos = pt.trajectory.run_connect_batch(seqs, 1.0, r, motion_boundary=True, mb_engine="batch")
    assert int(infos[1].chain_mode) == 3
    got = pt.trajectory.result_to_trajectory_set(ctxs[1], infos[1], 3)
    info = pt.trajectory.run_connect(seqs[1][0], seqs[1][1], None, None, 1.0, r, return_device=True, motion_boundary=True)
    want = pt.trajectory.result_to_trajectory_set(pt.hip.context(), info, 3)
    for x, y in zip(want._to_csr()[:4], got._to_csr()[:4]):
        assert np.array_equal(np.asarray(x), np.asarray(y))


@pytest.mark.parametrize("opt", [False, True])
def test_python_engines_agree(pt, opt):
    if opt:
        g, seqs, _ = opt_batch(pt)
    else:
        g, seqs, _ = track_batch(pt, SEQ_TRACK[0])
    r = int(g["ratio"])
    thr = [0.02, 0.05] + [0.02] * (len(seqs) - 2)
    res = {}
    for engine in ("batch", "loop"):
        ctxs, infos = pt.trajectory.run_connect_batch(seqs, 1.0, r, motion_boundary=True, mb_thres=thr, mb_engine=engine)
        res[engine] = [pt.trajectory._result_to_host(c, i) for c, i in zip(ctxs, infos)]
    assert all(R.info["chain_mode"] == 1 for R in res["loop"])
    assert res["batch"][0].info["chain_mode"] == 3
    for A, B in zip(res["batch"], res["loop"]):
        same(A, B, TOL if opt else 0.0)
    assert_equals(res["batch"][0], g, "mb", TOL if opt else 0.0)
    with pytest.raises(ValueError):
        pt.trajectory.run_connect_batch(seqs, 1.0, r, motion_boundary=True, mb_engine="fastest")
    with pytest.raises(ValueError):
        pt.trajectory.run_connect_batch(seqs, 1.0, r, motion_boundary=True, mb_thres=[0.02])


def test_a_bad_threshold_leaves_the_option_off(pt):
    g, seqs, _ = track_batch(pt, SEQ_TRACK[0])
    with pytest.raises(pt.hip.PsfmError):
        pt.trajectory.run_connect_batch(seqs[:2], 1.0, int(g["ratio"]), motion_boundary=True, mb_thres=[0.02, -1.0], mb_engine="batch")
    # (the autouse fixture then runs a plain batch on these contexts)


@pytest.mark.parametrize("opt", [False, True])
def test_connect_sequences_with_the_option_writes_the_same_files(pt, tmp_path, opt):
    """connect_sequences(..., motion_boundary=True, batch=2) disk to disk, as test_connect_sequences_in_batches_writes_the_same_files:
    every track.npy holds what main_connect_point_trajectories(..., motion_boundary=True) writes for that sequence alone -- and not
    what it writes without the option."""
    import os
    from point_trajectory.batch import connect_sequences
    from point_trajectory.main_connect_point_trajectories import main_connect_point_trajectories
    from point_trajectory.trajectory import load_track_npy
    from point_trajectory.utils import write_flo
    H, W, r = 48, 64, 2
    fdirs, tdirs, sdirs = [], [], []
    for k in range(3):
        d = psfm_synth.synth_realistic(6 + k, H, W, seed=141 + k, stride2=opt, **dict(psfm_synth.REALISTIC, **SEQ_SYNTH))
        fd = tmp_path / ("seq%d" % k) / "flows"
        for name, key in (("flow_f", "flows_f"), ("flow_b", "flows_b"), ("flow_f2", "flows_f2"), ("flow_b2", "flows_b2")):
            if key not in d:
                continue
            os.makedirs(fd / name)
            for i, a in enumerate(d[key]):
                write_flo(str(fd / name / ("%05d.flo" % i)), a)
        fdirs.append(str(fd)); tdirs.append(str(tmp_path / ("seq%d" % k) / "traj")); sdirs.append(str(tmp_path / ("seq%d" % k) / "single"))
    for engine in ("batch", "loop"):
        connect_sequences(fdirs, tdirs, sample_ratio=r, skip_path_consistency=not opt, concurrency=2, rank=0, world=1, layout="reference", batch=2,
                          motion_boundary=True, mb_thres=0.02, mb_engine=engine)
        for fd, td, sd in zip(fdirs, tdirs, sdirs):
            if engine == "batch":
                main_connect_point_trajectories(fd, sd, sample_ratio=r, skip_path_consistency=not opt, motion_boundary=True)
                main_connect_point_trajectories(fd, sd + "_off", sample_ratio=r, skip_path_consistency=not opt)
            a, b = load_track_npy(os.path.join(td, "track.npy")), load_track_npy(os.path.join(sd, "track.npy"))
            for x, y in zip(a._to_csr()[:4], b._to_csr()[:4]):
                if np.asarray(x).dtype == np.float64 and opt:
                    assert float(np.abs(np.asarray(x) - np.asarray(y)).max()) <= 1e-9
                else:
                    assert np.array_equal(np.asarray(x), np.asarray(y))
            got = open(os.path.join(td, "track.npy"), "rb").read()
            if not opt:
                assert got == open(os.path.join(sd, "track.npy"), "rb").read()
            assert got != open(os.path.join(sd + "_off", "track.npy"), "rb").read(), "the file of the shipped rule"
            os.remove(os.path.join(td, "track.npy"))
