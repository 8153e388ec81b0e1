"""The label merge of motion segmentation (motion_seg/main_motion_segmentation.py:89-129) and the match tables built from its
output, against golden vectors that the REFERENCE's own main_motion_segmentation + traj_to_matches produced
(tests/golden/make_labels_golden.py: both imported unmodified in the build container, a stub network with seeded scores).

CPU part (runs anywhere): psfm_motion_seg.merge_labels.merge_labels_host -- the NumPy statement of the data model -- on the CPU
checker's trajectories, and the host match tables over its result.
GPU part (-m gpu): psfm_labels_* (csrc/psfm_labels.hip) through LabelMerger / label_trajectories and psfm_labels_to_matches, bit for
bit against the fixtures, and against the host statement where no fixture can exist (gaps, the sampler's cap).
"""
import ctypes
import functools
import hashlib

import numpy as np
import pytest

from _common import check_match_tables, golden, regen_inputs

CASES = ["labels_48x64_t23_w10",      # three windows of 10 over 23 frames, the last overlaps the one before it
         "labels_48x64_t23_full",     # window >= length: the single-window branch (load_cut_seq.py:51-58)
         "labels_24x32_t27_w10"]      # slow flow: trajectories keep more than K = 20 points (the strided branch of traj_to_matches)
SET_KEYS = ("ids", "off", "frame_ids", "xy", "labels")


def fixture_windows(g):
    return [(int(g["w%d_frame0" % w]), int(g["w%d_n_frames" % w]), g["w%d_ids" % w], g["w%d_pred" % w]) for w in range(int(g["n_windows"]))]


def tables_view(g, remove_dynamic):
    tag = "rd1_" if remove_dynamic else "rd0_"
    return {k[len(tag):]: g[k] for k in g.files if k.startswith(tag)}


@functools.lru_cache(maxsize=None)
def checker_saved_set(name):
    """The saved set (length >= 3) of the fixture's sequence from the CPU checker: (ids, birth, length, off, xy)."""
    from oracle import oracle as orc
    g = golden(name)
    d = regen_inputs(g, stride2=False)
    _, occ = orc.flow_check(d["flows_f"], d["flows_b"], 1.0)
    R = orc.track(d["flows_f"], occ, int(g["ratio"]))
    keep = np.flatnonzero(R.length >= 3)
    assert len(keep) == int(g["n_saved"])
    off = np.zeros(len(keep) + 1, np.int64)
    np.cumsum(R.length[keep], out=off[1:])
    xy = np.concatenate([R.traj(int(i))[1] for i in keep], 0)
    return keep.astype(np.int32), R.birth[keep].astype(np.int32), R.length[keep].astype(np.int32), off, xy


def assert_set_equal(got, want):
    """Every array of the labelled set, np.array_equal (xy bit for bit)."""
    for key, a in zip(SET_KEYS, got):
        b = want[key] if not isinstance(want, tuple) else want[SET_KEYS.index(key)]
        assert np.asarray(a).shape == np.asarray(b).shape, (key, np.asarray(a).shape, np.asarray(b).shape)
        assert np.array_equal(a, b), key


def gap_windows(windows, seed=5):
    """The fixture's windows with every id divisible by 3 dropped from the middle windows and all rows permuted (seeded), seeded
    random predictions: trajectories left out of a middle window get a gap in their frames."""
    rng = np.random.default_rng(seed)
    out = []
    for w, (f0, n, ids, _) in enumerate(windows):
        ids = np.asarray(ids, np.int32)
        if 0 < w < len(windows) - 1:
            ids = ids[ids % 3 != 0]
        ids = ids[rng.permutation(len(ids))]
        out.append((f0, n, ids, (rng.uniform(size=len(ids)) < 0.5).astype(np.uint8)))
    return out


def has_gap(off, frame_ids):
    d = np.diff(frame_ids.astype(np.int64))
    inner = np.ones(len(d), bool)
    inner[off[1:-1] - 1] = False          # the step from one trajectory's last point to the next one's first
    return bool(np.any(d[inner] > 1))


# ---- CPU -------------------------------------------------------------------------------------------------------------------------

def test_fixture_pins_what_the_saved_set_cannot_express():
    """Case (a): fewer labelled than saved trajectories and points, a trajectory with both labels, a key order that is not
    ascending -- a fixture without these would pin nothing beyond a label array over the saved set."""
    g = golden(CASES[0])
    assert len(g["ids"]) < int(g["n_saved"])
    assert len(g["frame_ids"]) < int(g["n_saved_points"])
    off, lab = g["off"], g["labels"]
    assert any(len(set(lab[off[i]:off[i + 1]].tolist())) == 2 for i in range(len(off) - 1))
    assert not np.all(np.diff(g["ids"]) > 0)
    assert int(g["n_windows"]) == 3
    assert int(golden(CASES[1])["n_windows"]) == 1
    c = golden(CASES[2])
    kept = [int((c["labels"][c["off"][i]:c["off"][i + 1]] == 0).sum()) for i in range(len(c["ids"]))]
    assert max(kept) > 20      # the strided branch (matches_from_flow.py:92-101) runs after the labels dropped points


@pytest.mark.parametrize("name", CASES)
def test_host_merge_equals_reference_fixture(name):
    from psfm_motion_seg.merge_labels import merge_labels_host
    g = golden(name)
    assert_set_equal(merge_labels_host(*checker_saved_set(name), fixture_windows(g)), g)


@pytest.mark.parametrize("remove_dynamic", [True, False])
@pytest.mark.parametrize("name", CASES)
def test_host_tables_over_the_labelled_dict_equal_reference_fixture(name, remove_dynamic, tmp_path):
    """labelled_as_dict -- the dict the reference saves -- through the host traj_to_matches path (track.npy and all)."""
    from psfm_motion_seg.merge_labels import labelled_as_dict, merge_labels_host
    from psfm_sfm import matches_from_flow as mff
    g = golden(name)
    trajs = labelled_as_dict(*merge_labels_host(*checker_saved_set(name), fixture_windows(g)))
    assert list(trajs) == g["ids"].tolist()
    T = int(g["T"])
    names = ["%05d.png" % i for i in range(T)]
    img_dir, traj_dir = tmp_path / "images", tmp_path / "traj"
    img_dir.mkdir(); traj_dir.mkdir()
    for n in names:
        (img_dir / n).touch()
    np.save(str(traj_dir / "track.npy"), trajs, allow_pickle=True)
    datas = mff.traj_to_matches(str(img_dir), str(traj_dir), str(tmp_path / "pairs.txt"), remove_dynamic=remove_dynamic)
    want = tables_view(g, remove_dynamic)
    check_match_tables(datas, names, want)
    assert hashlib.sha256(open(str(tmp_path / "pairs.txt")).read().encode()).hexdigest() == str(want["pair_file_hash"])
    # and straight from the CSR
    ids, off, fr, xy, lab = merge_labels_host(*checker_saved_set(name), fixture_windows(g))
    tables = mff.match_tables_host(off, fr.astype(np.int64), xy, lab.astype(bool), T, remove_dynamic)
    check_match_tables(mff.assemble(names, tables, str(tmp_path / "pairs2.txt")), names, want)


def test_host_merge_toy_gap_first_seen_order_and_first_window_wins():
    """Three trajectories, three windows, written out by hand.  Trajectory 2 is absent from the middle window (a gap at frames
    3, 4); the set lists 5, 2, 9 (order of first appearance, not of id); window 2 overlaps window 1 at frame 5, where the labels of
    window 1 stay."""
    from psfm_motion_seg.merge_labels import labelled_as_dict, merge_labels_host
    ids = np.array([2, 5, 9]); birth = np.array([0, 1, 4]); length = np.array([9, 7, 5])
    off = np.array([0, 9, 16, 21])
    xy = np.stack([np.arange(21.0), 100.0 + np.arange(21.0)], 1)
    windows = [(0, 3, np.array([5, 2]), np.array([1, 0])),
               (3, 3, np.array([9, 5]), np.array([True, False])),
               (5, 4, np.array([2, 9, 5]), np.array([1, 0, 1]))]
    o_ids, o_off, o_fr, o_xy, o_lab = merge_labels_host(ids, birth, length, off, xy, windows)
    assert o_ids.tolist() == [5, 2, 9]
    assert o_off.tolist() == [0, 7, 14, 19]
    assert o_fr.tolist() == [1, 2, 3, 4, 5, 6, 7,   0, 1, 2, 5, 6, 7, 8,   4, 5, 6, 7, 8]
    assert o_lab.tolist() == [1, 1, 0, 0, 0, 1, 1,   0, 0, 0, 1, 1, 1, 1,   1, 1, 0, 0, 0]
    src = [9, 10, 11, 12, 13, 14, 15,   0, 1, 2, 5, 6, 7, 8,   16, 17, 18, 19, 20]
    assert np.array_equal(o_xy, xy[src])
    assert has_gap(o_off, o_fr)
    d = labelled_as_dict(o_ids, o_off, o_fr, o_xy, o_lab)
    assert list(d) == [5, 2, 9] and d[2]["frame_ids"].tolist() == [0, 1, 2, 5, 6, 7, 8] and d[2]["labels"].dtype == bool
    # a row without a point in its window is ignored; an id outside the saved set is an error
    same = merge_labels_host(ids, birth, length, off, xy, [(0, 3, np.array([9, 5, 2]), np.array([1, 1, 0]))] + windows[1:])
    assert same[0].tolist() == [5, 2, 9] and same[2].tolist() == o_fr.tolist()
    with pytest.raises(ValueError):
        merge_labels_host(ids, birth, length, off, xy, [(0, 3, np.array([5, 7]), np.array([1, 0]))])
    empty = merge_labels_host(ids, birth, length, off, xy, [])
    assert empty[0].shape == (0,) and empty[1].tolist() == [0] and empty[3].shape == (0, 2)


def test_gap_windows_leave_a_gap():
    """The windows of the GPU gap test (fixture ids = what the device sampler returns, pinned by the driver test): the host
    statement over them has a trajectory with a gap in its frames."""
    from psfm_motion_seg.merge_labels import merge_labels_host
    name = CASES[0]
    ids, off, fr, xy, lab = merge_labels_host(*checker_saved_set(name), gap_windows(fixture_windows(golden(name))))
    assert has_gap(off, fr)
    assert not np.all(np.diff(ids) > 0)


# ---- GPU -------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pt():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from point_trajectory import utils, trajectory, _hip
    _hip.context()
    class NS: pass
    ns = NS()
    ns.utils, ns.trajectory, ns.hip = utils, trajectory, _hip
    return ns


def connect(pt, d, ratio):
    import torch
    ff = torch.from_numpy(np.stack(d["flows_f"])).cuda()
    fb = torch.from_numpy(np.stack(d["flows_b"])).cuda()
    pt.trajectory.run_connect(ff, fb, None, None, 1.0, int(ratio), return_device=True)
    return pt.hip.context()


def result_filter(pt, ctx, traj_min_len=3):
    k, n = ctypes.c_int64(0), ctypes.c_int64(0)
    pt.hip.check(pt.hip.lib().psfm_result_filter(ctx.handle, traj_min_len, ctypes.byref(k), ctypes.byref(n), pt.hip.current_stream_ptr(ctx.device)))
    return int(k.value), int(n.value)


def saved_set_host(pt, ctx):
    k, n = result_filter(pt, ctx)
    ids, birth, length = np.empty(k, np.int32), np.empty(k, np.int32), np.empty(k, np.int32)
    off, xy = np.zeros(k + 1, np.int64), np.empty((n, 2), np.float64)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    pt.hip.check(pt.hip.lib().psfm_result_filtered_copy(ctx.handle, vp(ids), vp(birth), vp(length), vp(off), vp(xy), pt.hip.current_stream_ptr(ctx.device)))
    return ids, birth, length, off, xy


def merge_on_device(pt, ctx, windows, pred_dtype=None):
    import torch
    from psfm_motion_seg.merge_labels import LabelMerger
    m = LabelMerger(ctx)
    for f0, n, ids, pred in windows:
        p = torch.from_numpy(np.asarray(pred, np.uint8)).cuda()
        m.add_window(f0, n, torch.from_numpy(np.asarray(ids, np.int32)).cuda(), p.to(pred_dtype) if pred_dtype else p)
    return m, [t.cpu().numpy() for t in m.finish()]


def assert_tables_equal_host(pt, ctx, lset, T, remove_dynamic):
    from psfm_sfm import matches_from_flow as mff
    ids, off, fr, xy, lab = lset
    want = mff.match_tables_host(off, fr.astype(np.int64), xy, lab.astype(bool), T, remove_dynamic)
    got = mff.match_tables_labelled_device(ctx, T, remove_dynamic)
    for key, a, b in zip(("kp_off", "kp_xy", "pair_key", "pair_off", "pair_first", "rows"), got, want):
        assert a.shape == b.shape, (key, a.shape, b.shape)
        assert np.array_equal(a, b), key


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_device_merge_and_tables_equal_reference_fixture(pt, name, tmp_path):
    """run_connect -> psfm_result_filter(3) -> LabelMerger fed the fixture's ids and predictions per window: every array of the
    labelled set bit-equal to what the reference saved; traj_to_matches_labelled_device for both remove_dynamic values equal to the
    reference's traj_to_matches over that file, the pair list file included."""
    import torch
    from psfm_sfm import matches_from_flow as mff
    g = golden(name)
    ctx = connect(pt, regen_inputs(g, stride2=False), g["ratio"])
    k, n = result_filter(pt, ctx)
    assert (k, n) == (int(g["n_saved"]), int(g["n_saved_points"]))
    m, got = merge_on_device(pt, ctx, fixture_windows(g), torch.bool if name == CASES[1] else None)
    assert_set_equal(got, g)
    assert (m.n_traj, m.n_points) == (len(g["ids"]), len(g["frame_ids"]))
    d = m.as_dict()
    assert list(d) == g["ids"].tolist()
    names = ["%05d.png" % i for i in range(int(g["T"]))]
    for rd in (True, False):
        want = tables_view(g, rd)
        datas = mff.traj_to_matches_labelled_device(ctx, names, str(tmp_path / "pairs.txt"), remove_dynamic=rd)
        check_match_tables(datas, names, want)
        assert hashlib.sha256(open(str(tmp_path / "pairs.txt")).read().encode()).hexdigest() == str(want["pair_file_hash"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_label_trajectories_driver_equals_reference_fixture(pt, name):
    """The whole loop (window sampler -> predict -> merge): the sampled ids are the fixture's, and with the fixture's predictions
    looked up by window index the labelled set is the reference's."""
    import torch
    from psfm_motion_seg.merge_labels import label_trajectories
    g = golden(name)
    ctx = connect(pt, regen_inputs(g, stride2=False), g["ratio"])
    T, H, W = int(g["T"]), int(g["H"]), int(g["W"])
    calls = []

    def predict(raw, nor, mask, time_idx):
        w = len(calls)
        calls.append((raw.shape, time_idx))
        assert raw.shape == nor.shape == (len(g["w%d_ids" % w]), int(g["w%d_n_frames" % w]), 2) and mask.shape[:2] == raw.shape[:2]
        assert time_idx[0] == int(g["w%d_frame0" % w]) and len(time_idx) == int(g["w%d_n_frames" % w])
        return torch.from_numpy(g["w%d_pred" % w].astype(bool)).cuda()
    m = label_trajectories(T, int(g["window"]), (H, W), tuple(int(x) for x in g["input_size"]), 10 ** 9, predict, ctx=ctx)
    assert len(calls) == int(g["n_windows"])
    for w, ids in enumerate(m.window_ids):
        assert np.array_equal(ids.cpu().numpy(), g["w%d_ids" % w])
    assert_set_equal([t.cpu().numpy() for t in m.finish()], g)


@pytest.mark.gpu
def test_gaps_and_shuffled_rows_equal_host_statement(pt):
    """Window ids from the device sampler, every id divisible by 3 dropped from the middle window, rows permuted: trajectories
    with a gap in their frames, rows in no particular order.  The device set equals merge_labels_host on the same windows and the
    tables equal match_tables_host over it."""
    from psfm_motion_seg.load_cut_seq import cut_trajectory_windows, window_ranges
    from psfm_motion_seg.merge_labels import merge_labels_host
    g = golden(CASES[0])
    ctx = connect(pt, regen_inputs(g, stride2=False), g["ratio"])
    T, H, W = int(g["T"]), int(g["H"]), int(g["W"])
    idx_b = cut_trajectory_windows(T, int(g["window"]), (H, W), (30, 50), 10 ** 9, as_numpy=True, ctx=ctx)[4]
    windows = gap_windows([(f0, n, ids, None) for (f0, n), ids in zip(window_ranges(T, int(g["window"])), idx_b)])
    saved = saved_set_host(pt, ctx)
    want = merge_labels_host(*saved, windows)
    assert has_gap(want[1], want[2])
    _, got = merge_on_device(pt, ctx, windows)
    assert_set_equal(got, want)
    for rd in (True, False):
        assert_tables_equal_host(pt, ctx, got, T, rd)


@pytest.mark.gpu
def test_midsize_with_the_samplers_cap_equals_host_statement(pt):
    """480x854, 40 frames, r = 2, window 10, the reference's default traj_max_num = 100000 (the sampler's cap branch runs: a
    seeded random subset in shuffled order per window, so trajectories come and go between windows), seeded random predictions.
    The merge is checked in full against the host statement.  The tables are checked with remove_dynamic on predictions that are
    85 % dynamic: the host tables hold every match in several int64 arrays, and with ~4e6 points of trajectories longer than K = 20
    the unfiltered case would need ~8e7 matches (several GB) on the host; remove_dynamic=False is covered by the small cases."""
    import psfm_synth
    import torch
    from psfm_motion_seg.merge_labels import label_trajectories, merge_labels_host
    T, H, W = 40, 480, 854
    d = psfm_synth.synth_sequence(T, H, W, seed=77, sigma=0.3, n_occluders=2, stride2=False)
    ctx = connect(pt, d, 2)
    rng = np.random.default_rng(78)
    windows = []

    def predict(raw, nor, mask, time_idx):
        p = rng.uniform(size=raw.shape[0]) < 0.85
        windows.append([int(time_idx[0]), len(time_idx), None, p.astype(np.uint8)])
        return torch.from_numpy(p).cuda()
    m = label_trajectories(T, 10, (H, W), (240, 432), 100000, predict, seed=3, ctx=ctx)
    for w, ids in zip(windows, m.window_ids):
        w[2] = ids.cpu().numpy()
    assert any(len(w[2]) == 100000 for w in windows), [len(w[2]) for w in windows]      # the cap branch ran
    got = [t.cpu().numpy() for t in m.finish()]
    saved = saved_set_host(pt, ctx)          # (a new psfm_result_filter: the labelled set in the context stays valid)
    want = merge_labels_host(*saved, [tuple(w) for w in windows])
    assert_set_equal(got, want)
    assert has_gap(want[1], want[2]) and len(want[0]) < len(saved[0])
    assert_tables_equal_host(pt, ctx, got, T, True)


@pytest.mark.gpu
def test_label_merge_errors_and_the_empty_set(pt):
    import torch
    from psfm_motion_seg.merge_labels import LabelMerger
    from psfm_sfm import matches_from_flow as mff
    g = golden(CASES[0])
    T = int(g["T"])
    ctx = connect(pt, regen_inputs(g, stride2=False), g["ratio"])
    L, sp = pt.hip.lib(), pt.hip.current_stream_ptr(ctx.device)
    ids = torch.from_numpy(g["w0_ids"]).cuda()
    pred = torch.from_numpy(g["w0_pred"]).cuda()
    # merge without begin: psfm_connect voided whatever an earlier test left in the context
    with pytest.raises(pt.hip.PsfmError):
        pt.hip.check(L.psfm_labels_merge_window(ctx.handle, 0, 10, pt.hip.ptr(ids), pt.hip.ptr(pred), ids.numel(), sp))
    result_filter(pt, ctx)
    # zero windows: the empty set, tables with kp_off all zero
    m = LabelMerger(ctx)
    out = m.finish()
    assert (m.n_traj, m.n_points) == (0, 0) and out[0].numel() == 0 and out[1].cpu().tolist() == [0] and tuple(out[3].shape) == (0, 2)
    tables = mff.match_tables_labelled_device(ctx, T, True)
    assert tables[0].tolist() == [0] * (T + 1) and len(tables[1]) == 0 and len(tables[5]) == 0
    m.add_window(0, 10, ids[:0], pred[:0])           # k = 0 is a no-op
    assert m.finish()[0].numel() == 0
    # an id outside the saved set: the window call stays asynchronous, finish reports it
    saved_ids = saved_set_host(pt, ctx)[0]
    missing = int(np.setdiff1d(np.arange(saved_ids.max() + 2), saved_ids)[0])
    m = LabelMerger(ctx)
    bad = ids.clone(); bad[3] = missing
    m.add_window(0, 10, bad, pred)
    with pytest.raises(pt.hip.PsfmError):
        m.finish()
    # merge / finish after a new psfm_result_filter
    m = LabelMerger(ctx)
    m.add_window(0, 10, ids, pred)
    result_filter(pt, ctx)
    with pytest.raises(pt.hip.PsfmError):
        m.add_window(10, 10, ids[:1], pred[:1])
    with pytest.raises(pt.hip.PsfmError):
        m.finish()
    # frames beyond n_img
    m = LabelMerger(ctx)
    m.add_window(0, 10, ids, pred)
    m.finish()
    with pytest.raises(pt.hip.PsfmError):
        mff.match_tables_labelled_device(ctx, 5, False)
    mff.match_tables_labelled_device(ctx, 10, False)


@pytest.mark.gpu
def test_saved_set_tables_unchanged_after_a_labelled_run(pt, tmp_path):
    """traj_to_matches_device on matches_24x32_t27_dyn still equals its fixture after a labelled run on the same context (the two
    entries share the pipeline and the context's tables)."""
    import torch
    from psfm_sfm import matches_from_flow as mff
    g = golden("matches_24x32_t27_dyn")
    gl = golden(CASES[2])
    assert str(gl["input_hash"]) == str(g["input_hash"])
    ctx = connect(pt, regen_inputs(g, stride2=False), g["ratio"])
    result_filter(pt, ctx)
    merge_on_device(pt, ctx, fixture_windows(gl))
    T = int(g["T"])
    names = ["%05d.png" % i for i in range(T)]
    check_match_tables(mff.traj_to_matches_labelled_device(ctx, names, str(tmp_path / "p0.txt"), remove_dynamic=True), names, tables_view(gl, True))
    labels = torch.from_numpy(np.unpackbits(g["labels"])[:int(g["n_points"])].astype(np.uint8)).cuda()
    datas = mff.traj_to_matches_device(ctx, names, str(tmp_path / "pairs.txt"), traj_min_len=3, labels=labels)
    check_match_tables(datas, names, g)
    assert hashlib.sha256(open(str(tmp_path / "pairs.txt")).read().encode()).hexdigest() == str(g["pair_file_hash"])
