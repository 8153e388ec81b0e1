"""psfm_result_set / psfm_load_track_npy (csrc/psfm_result_set.hip) and the Python routes on top of them, on the device: a trajectory
set from elsewhere -- arrays, or a track.npy -- becomes a context's result, and the kernels that exist run on it.  The new calls move
data; every equality here is byte equality.

Round trip against a tracker's own saved set; the reference's fixtures (windows, label merge, match tables, database rows) on a
context that never ran a tracker; file ingest at block boundaries of the record decode, HOST and DEVICE pointers, a non-default
stream behind a gate (tests/_stream_gate.py); refusals that leave the context as it was; the file-signature entry points with
device=True against device=False on the same files."""
import ctypes
import hashlib
import os
import pickle

import numpy as np
import pytest

import _stream_gate as sg
from _common import check_match_tables, golden, regen_inputs
from test_gpu_decoder import pt  # noqa: F401  (fixture: the package, the seeded encoder and decoder weights)
from test_labels_merge import assert_set_equal, checker_saved_set, fixture_windows, tables_view

pytestmark = pytest.mark.gpu
WINDOWS, LABELS_A, LABELS_C = "windows_48x64_t23", "labels_48x64_t23_w10", "labels_24x32_t27_w10"
SIZES = [0, 1, 255, 256, 257, 1025]          # records: none, one, a block less one, a block, a block and one, four blocks and one


def vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def sp(pt, ctx, stream=None):
    return pt.hip.current_stream_ptr(ctx.device) if stream is None else stream


def result_filter(pt, ctx, m, stream=None):
    k, n = ctypes.c_int64(0), ctypes.c_int64(0)
    pt.hip.check(pt.hip.lib().psfm_result_filter(ctx.handle, m, ctypes.byref(k), ctypes.byref(n), sp(pt, ctx, stream)))
    return int(k.value), int(n.value)


def filtered_copy(pt, ctx, k, n, stream=None):
    ids, birth, length = np.full(k, -1, np.int32), np.full(k, -1, np.int32), np.full(k, -1, np.int32)
    off, xy = np.full(k + 1, -1, np.int64), np.full((n, 2), np.nan)
    pt.hip.check(pt.hip.lib().psfm_result_filtered_copy(ctx.handle, vp(ids), vp(birth), vp(length), vp(off), vp(xy), sp(pt, ctx, stream)))
    return ids, birth, length, off, xy


def saved_set(pt, ctx, m, stream=None):
    return filtered_copy(pt, ctx, *result_filter(pt, ctx, m, stream), stream=stream)


def result_copy(pt, ctx, n_result, n_points, stream=None):
    birth, length = np.full(n_result, -1, np.int32), np.full(n_result, -1, np.int32)
    off, xy = np.full(n_result + 1, -1, np.int64), np.full((n_points, 2), np.nan)
    pt.hip.check(pt.hip.lib().psfm_result_copy(ctx.handle, vp(birth), vp(length), vp(off), vp(xy), sp(pt, ctx, stream)))
    return birth, length, off, xy


def same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def expanded(ids, birth, length, xy):
    """What psfm_result_copy must return behind set_result: index == id, absent ids as empty entries."""
    n = int(ids[-1]) + 1 if len(ids) else 0
    b, l = np.zeros(n, np.int32), np.zeros(n, np.int32)
    b[ids], l[ids] = birth, length
    off = np.zeros(n + 1, np.int64)
    np.cumsum(l, out=off[1:])
    return b, l, off, np.ascontiguousarray(xy, np.float64).reshape(-1, 2)


def cut(s, k):
    ids, birth, length, off, xy = s
    return ids[:k].copy(), birth[:k].copy(), length[:k].copy(), off[:k + 1].copy(), xy[:int(off[k])].copy()


def as_set(s):
    from point_trajectory.optimize.build import particlesfm
    ids, birth, length, off, xy = s
    return particlesfm.TrajectorySet._from_csr(ids.astype(np.int64), birth, length, off, xy)


@pytest.fixture(scope="module")
def seq(pt):
    """ONE tracker run for the module: the 48x64x23 sample_ratio 2 sequence on the thread's context; its result and saved sets."""
    import torch
    g = golden(WINDOWS)
    d = regen_inputs(g, stride2=False)
    ff, fb = torch.from_numpy(np.stack(d["flows_f"])).cuda(), torch.from_numpy(np.stack(d["flows_b"])).cuda()
    ctx = pt.hip.context()
    info = pt.trajectory.run_connect(ff, fb, None, None, 1.0, int(g["ratio"]), return_device=True)
    class NS: pass
    ns = NS()
    ns.g, ns.ctx, ns.ff, ns.fb = g, ctx, ff, fb
    ns.n_traj, ns.n_points = int(info.n_traj), int(info.n_points)
    ns.full = result_copy(pt, ctx, ns.n_traj, ns.n_points)
    ns.saved5 = saved_set(pt, ctx, 5)
    ns.saved1 = saved_set(pt, ctx, 1)
    ns.saved3 = saved_set(pt, ctx, 3)              # (last: the context's saved set is this one)
    assert len(ns.saved1[0]) == ns.n_traj >= 1025 and 0 < len(ns.saved5[0]) < len(ns.saved3[0]) < ns.n_traj
    ns.base = ns.saved3 if len(ns.saved3[0]) >= 1025 else ns.saved1       # what the file tests cut their sets from
    return ns


def rerun_tracker(pt, seq):
    pt.trajectory.run_connect(seq.ff, seq.fb, None, None, 1.0, int(seq.g["ratio"]), return_device=True, ctx=seq.ctx)
    assert same(saved_set(pt, seq.ctx, 3), seq.saved3)


# ---- round trip ------------------------------------------------------------------------------------------------------------------

def test_round_trip_of_a_trackers_saved_set(pt, seq):
    ids, birth, length, off, xy = seq.saved3
    ctx2 = pt.hip.Context(0)
    n_result = ctx2.set_result(ids, birth, length, xy)
    assert n_result == int(ids[-1]) + 1
    assert same(saved_set(pt, ctx2, 1), seq.saved3)                    # filter(1) gives the set back, off included
    assert same(saved_set(pt, ctx2, 3), seq.saved3)
    assert same(saved_set(pt, ctx2, 5), seq.saved5)                    # ... and filter(m) its trajectories of length >= m
    got = result_copy(pt, ctx2, n_result, len(xy))
    assert same(got, expanded(ids, birth, length, xy))
    absent = np.setdiff1d(np.arange(n_result), ids)
    assert len(absent) > 0 and np.all(got[1][absent] == 0) and np.all(got[1][ids] == length) and np.all(got[0][ids] == seq.full[0][ids])
    # the host view: empty entries are trajectories without points
    tl = pt.trajectory.TrajectoryList(*got)
    assert tl[int(absent[0])].length() == 0 and tl[int(ids[0])].length() == int(length[0])
    assert same(tuple(np.asarray(a) for a in tl.to_trajectory_set(1)._csr[:5]),
                (ids.astype(np.int64), birth, length, off, xy))
    ctx2.close()


def test_host_and_device_pointers_and_the_empty_set(pt, seq):
    import torch
    ids, birth, length, off, xy = cut(seq.saved3, 700)
    want = expanded(ids, birth, length, xy)
    a, b = pt.hip.Context(0), pt.hip.Context(0)
    n = a.set_result(ids, birth, length, xy)
    assert b.set_result(*[torch.from_numpy(x).cuda() for x in (ids, birth, length, xy)]) == n
    # mixed: metadata on the host, points on the device
    assert same(result_copy(pt, a, n, len(xy)), want) and same(result_copy(pt, b, n, len(xy)), want)
    assert a.set_result(ids, birth, length, torch.from_numpy(xy).cuda()) == n and same(result_copy(pt, a, n, len(xy)), want)
    # an empty set is legal and leaves an empty result
    assert a.set_result(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 2))) == 0
    assert result_filter(pt, a, 1) == (0, 0) and result_copy(pt, a, 0, 0)[2].tolist() == [0]
    # a single trajectory with a high id: one entry in front of which everything is empty
    assert a.set_result([41], [7], [2], [[1.0, 2.0], [3.0, 4.0]]) == 42
    got = result_copy(pt, a, 42, 2)
    assert got[1].tolist() == [0] * 41 + [2] and got[0].tolist() == [0] * 41 + [7] and got[2].tolist() == [0] * 42 + [2]
    assert saved_set(pt, a, 1)[0].tolist() == [41]
    a.close(); b.close()


def test_set_result_on_a_non_default_stream_behind_a_gate(pt, seq):
    """psfm_result_set reads DEVICE arrays that a side stream fills behind a delay: the call, made with that stream's pointer, must
    see the real arrays (a copy on any other stream reads the decoy: another valid set of the same shape)."""
    import torch
    ids, birth, length, off, xy = cut(seq.saved3, 600)
    real = [ids, birth, length, xy]
    decoy = [ids + 1, birth + 1, length.copy(), xy[::-1].copy()]
    ctx = pt.hip.Context(0)
    n = ctx.set_result(*decoy)
    assert not same(result_copy(pt, ctx, n, len(xy)), expanded(*real))
    bufs = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in decoy]
    reals = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in real]
    n_result = ctypes.c_int64(0)
    with sg.gated_inputs(list(zip(bufs, reals)), "psfm_result_set") as g:
        g.enqueued()
        st = pt.hip.lib().psfm_result_set(ctx.handle, len(ids), len(xy), *[pt.hip.ptr(t) for t in bufs], ctypes.byref(n_result), g.ptr)
    assert st == 0 and n_result.value == int(ids[-1]) + 1
    assert same(result_copy(pt, ctx, n_result.value, len(xy), stream=g.ptr), expanded(*real))
    assert same(saved_set(pt, ctx, 1, stream=g.ptr), (ids, birth, length, off, xy))
    ctx.close()


# ---- pinned by the reference's fixtures, on a context that never ran a tracker --------------------------------------------------------

@pytest.fixture(scope="module")
def oracle_ctx(pt):
    """The saved set of the 48x64x23 sequence rebuilt on the CPU by the checker, put into a fresh context with set_result."""
    assert str(golden(WINDOWS)["input_hash"]) == str(golden(LABELS_A)["input_hash"])
    ctx = pt.hip.Context(0)
    ids, birth, length, off, xy = checker_saved_set(LABELS_A)
    ctx.set_result(ids, birth, length, xy)
    return ctx


def test_window_tensors_equal_reference_fixture(pt, oracle_ctx):
    from psfm_motion_seg.load_cut_seq import cut_trajectory_windows, sample_windows_device, window_ranges
    g = golden(WINDOWS)
    T, H, W = int(g["T"]), int(g["H"]), int(g["W"])
    input_size = tuple(int(x) for x in g["input_size"])
    for tag, win in (("w", int(g["window"])), ("full", T + 5)):
        raw_b, nor_b, mask_b, time_b, idx_b = cut_trajectory_windows(T, win, (H, W), input_size, traj_max_num=10 ** 9, as_numpy=True, ctx=oracle_ctx)
        ranges = window_ranges(T, win)
        batch = sample_windows_device(oracle_ctx, ranges, (H, W), input_size, 10 ** 9, 3, 3, list(range(len(ranges))))
        assert len(raw_b) == len(batch) == int(g[tag + "_n"])
        for w in range(len(raw_b)):
            for got in ((idx_b[w], raw_b[w], nor_b[w], mask_b[w]), tuple(t.cpu().numpy() for t in batch[w])):
                assert np.array_equal(got[0].astype(np.int64), g["%s%d_ids" % (tag, w)])
                assert np.array_equal(got[1], g["%s%d_raw" % (tag, w)]) and np.array_equal(got[2], g["%s%d_nor" % (tag, w)])
                assert np.array_equal(got[3], g["%s%d_mask" % (tag, w)])
            assert np.array_equal(time_b[w], g["%s%d_time" % (tag, w)])


@pytest.mark.parametrize("name", [LABELS_A, LABELS_C])
def test_label_merge_and_its_tables_equal_reference_fixture(pt, name, tmp_path):
    import torch
    from psfm_motion_seg.merge_labels import LabelMerger
    from psfm_sfm import matches_from_flow as mff
    g = golden(name)
    ctx = pt.hip.Context(0)
    ids, birth, length, off, xy = checker_saved_set(name)
    ctx.set_result(ids, birth, length, xy)
    assert result_filter(pt, ctx, 1) == (int(g["n_saved"]), int(g["n_saved_points"]))
    m = LabelMerger(ctx)
    for f0, n, wids, pred in fixture_windows(g):
        m.add_window(f0, n, torch.from_numpy(np.asarray(wids, np.int32)).cuda(), torch.from_numpy(np.asarray(pred, np.uint8)).cuda())
    assert_set_equal([t.cpu().numpy() for t in m.finish()], g)
    names = ["%05d.png" % i for i in range(int(g["T"]))]
    for rd in (True, False):
        want = tables_view(g, rd)
        check_match_tables(mff.traj_to_matches_labelled_device(ctx, names, str(tmp_path / "pairs.txt"), remove_dynamic=rd), names, want)
        assert hashlib.sha256(open(str(tmp_path / "pairs.txt")).read().encode()).hexdigest() == str(want["pair_file_hash"])
    # a new result voids the merger (res_gen)
    ctx.set_result(ids, birth, length, xy)
    with pytest.raises(pt.hip.PsfmError):
        m.finish()
    ctx.close()


def test_saved_set_match_tables_equal_reference_fixture(pt, tmp_path):
    from oracle import oracle as orc
    from psfm_sfm import matches_from_flow as mff
    g = golden("matches_40x56_t12")
    d = regen_inputs(g, stride2=False)
    _, occ = orc.flow_check(d["flows_f"], d["flows_b"], 1.0)
    R = orc.track(d["flows_f"], occ, int(g["ratio"]))
    keep = np.flatnonzero(R.length >= 3)
    assert len(keep) == int(g["n_saved"]) and not np.unpackbits(g["labels"])[:int(g["n_points"])].any()
    xy = np.concatenate([R.traj(int(i))[1] for i in keep], 0)
    ctx = pt.hip.Context(0)
    ctx.set_result(keep, R.birth[keep], R.length[keep], xy)
    names = ["%05d.png" % i for i in range(int(g["T"]))]
    datas = mff.traj_to_matches_device(ctx, names, str(tmp_path / "pairs.txt"), traj_min_len=1)
    check_match_tables(datas, names, g)
    assert hashlib.sha256(open(str(tmp_path / "pairs.txt")).read().encode()).hexdigest() == str(g["pair_file_hash"])
    ctx.close()


def dirs(tmp_path, names, tag):
    img_dir, traj_dir = tmp_path / tag / "images", tmp_path / tag / "traj"
    img_dir.mkdir(parents=True); traj_dir.mkdir(parents=True)
    for n in names:
        (img_dir / n).touch()
    return img_dir, traj_dir


def test_database_rows_equal_reference_fixture_from_the_labelled_file(pt, tmp_path):
    """database_a_permuted: the labelled dict as stage 2 saves it -> import_keypoints_matches(device=True) -> the reference's rows."""
    from _database_np import assert_database_equals_fixture, create_tables, fixture
    from psfm_sfm.database import import_keypoints_matches
    f = fixture("database_a_permuted")
    img_dir, traj_dir = dirs(tmp_path, f["names"], "a")
    np.save(str(traj_dir / "track.npy"), f["trajs"], allow_pickle=True)
    got = {}
    for device in (True, False):
        path = tmp_path / ("database_%d.db" % device)
        create_tables(path)
        import_keypoints_matches(f["image_ids"], str(img_dir), str(path), str(tmp_path / "pairs.txt"), str(traj_dir),
                                 skip_geometric_verification=True, device=device)
        assert_database_equals_fixture(path, f)
        got[device] = open(str(tmp_path / "pairs.txt")).read()
        assert hashlib.sha256(got[device].encode()).hexdigest() == f["pair_file_hash"]
    assert got[True] == got[False]


# ---- file ingest -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", SIZES)
def test_file_ingest_equals_the_to_device_route(pt, seq, k, tmp_path):
    s = cut(seq.base, k)
    ts = as_set(s)
    path = str(tmp_path / "track.npy")
    pt.trajectory.save_track_npy(path, ts)
    a, b = pt.hip.Context(0), pt.hip.Context(0)
    ctx, kind, sizes = pt.trajectory.load_track_npy_device(path, a)
    n_result = int(s[0][-1]) + 1 if k else 0
    assert ctx is a and kind == "set" and sizes == {"n_traj": k, "n_points": len(s[4]), "n_result": n_result, "route": "file"}
    assert ts.to_device(b) is b
    want = expanded(s[0], s[1], s[2], s[4])
    assert same(result_copy(pt, a, n_result, len(s[4])), want) and same(result_copy(pt, b, n_result, len(s[4])), want)
    if k:
        assert same(saved_set(pt, a, 1), s)
    # the same file again over the result it left, with one reader thread and with many
    for threads in (1, 9):
        assert a.load_track_npy(path, threads) == (k, len(s[4]), n_result)
        assert same(result_copy(pt, a, n_result, len(s[4])), want)
    a.close(); b.close()


def test_file_ingest_on_a_non_default_stream(pt, seq, tmp_path):
    """psfm_load_track_npy takes no device input of the caller's: it is made with a side stream's pointer while torch's current
    stream stays the default one, and its consumers follow on that stream."""
    s = cut(seq.base, 513)
    path = str(tmp_path / "track.npy")
    pt.trajectory.save_track_npy(path, as_set(s))
    from point_trajectory import reference_pickle as rp
    rec, at = rp._record_template()
    tmpl = np.frombuffer(rec, np.uint8).copy()
    field_at = np.asarray([at[n] for n in ("id", "b", "bn", "s", "e", "n")], np.int32)
    ctx = pt.hip.Context(0)
    g = sg.gate()
    n, p, r = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    st = pt.hip.lib().psfm_load_track_npy(ctx.handle, os.fsencode(path), tmpl.ctypes.data, len(rec), field_at.ctypes.data, 4, ctypes.byref(n),
                                          ctypes.byref(p), ctypes.byref(r), g.ptr)
    assert st == 0 and (n.value, p.value, r.value) == (513, len(s[4]), int(s[0][-1]) + 1)
    assert same(saved_set(pt, ctx, 1, stream=g.ptr), s)
    ctx.close()


def test_other_layouts_load_through_the_fallback_to_the_same_bytes(pt, seq, tmp_path):
    s = cut(seq.base, 300)
    ts = as_set(s)
    want = expanded(s[0], s[1], s[2], s[4])
    n_result = int(s[0][-1]) + 1
    csr = str(tmp_path / "csr.npy")
    pt.trajectory.save_track_npy(csr, ts, layout="csr")
    plain = str(tmp_path / "plain.npy")
    ts.pickle_layout = "reference"
    arr = np.empty((), dtype=object)
    arr[()] = ts
    with open(plain, "wb") as fp:                   # the generic pickler's file of the same set: the reference's state, no footer
        np.lib.format.write_array_header_1_0(fp, np.lib.format.header_data_from_array_1_0(arr))
        pickle.dump(arr, fp, protocol=3)
    for path in (csr, plain):
        ctx = pt.hip.Context(0)
        with pytest.raises(pt.hip.PsfmError) as e:
            ctx.load_track_npy(path)
        assert e.value.status == pt.hip.PSFM_ERR_ARG
        _, kind, sizes = pt.trajectory.load_track_npy_device(path, ctx)
        assert kind == "set" and sizes == {"n_traj": 300, "n_points": len(s[4]), "n_result": n_result, "route": "host", "true_labels": False}
        assert same(result_copy(pt, ctx, n_result, len(s[4])), want)
        ctx.close()


def test_a_set_with_a_gap_in_its_frames_is_refused_by_name(pt):
    from point_trajectory.optimize.build import particlesfm
    ts = particlesfm.TrajectorySet({4: {"frame_ids": [0, 1, 2], "locations": np.zeros((3, 2)), "labels": [False] * 3},
                                    9: {"frame_ids": [3, 5, 6], "locations": np.ones((3, 2)), "labels": [False] * 3}})
    ctx = pt.hip.Context(0)
    with pytest.raises(ValueError, match="trajectory 9"):
        ts.to_device(ctx)
    ts = particlesfm.TrajectorySet({9: {"frame_ids": [3, 4], "locations": np.ones((2, 2)), "labels": [False] * 2},
                                    4: {"frame_ids": [0, 1, 2], "locations": np.zeros((3, 2)), "labels": [False] * 3}})
    ts.to_device(ctx)                                # map-backed, keys out of order: sorted by id
    got = saved_set(pt, ctx, 1)
    assert got[0].tolist() == [4, 9] and got[1].tolist() == [0, 3] and got[2].tolist() == [3, 2] and got[4][:, 0].tolist() == [0, 0, 0, 1, 1]
    ctx.close()


@pytest.mark.parametrize("name", [LABELS_A])
def test_a_labelled_file_loads_as_labelled(pt, name, tmp_path):
    from psfm_motion_seg.merge_labels import labelled_as_dict, merge_labels_host
    from psfm_sfm import matches_from_flow as mff
    g = golden(name)
    lset = merge_labels_host(*checker_saved_set(name), fixture_windows(g))
    path = str(tmp_path / "track.npy")
    np.save(path, labelled_as_dict(*lset), allow_pickle=True)
    ctx = pt.hip.Context(0)
    _, kind, sizes = pt.trajectory.load_track_npy_device(path, ctx)
    assert kind == "labelled" and sizes == {"n_traj": len(lset[0]), "n_points": len(lset[2]), "route": "host"}
    T = int(g["T"])
    off, frames, xy, labels = mff._flatten(np.load(path, allow_pickle=True).item())
    for rd in (True, False):
        want = mff.match_tables_host(off, frames, xy, labels, T, rd)
        got = mff.match_tables_labelled_device(ctx, T, rd)
        assert len(got) == len(want) == 6 and len(want[5]) > 0
        for a, b in zip(got, want):
            assert a.shape == b.shape and np.array_equal(a, b)
    ctx.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_context_as_it_was(pt, seq, tmp_path):
    rerun_tracker(pt, seq)
    ctx, L = seq.ctx, pt.hip.lib()
    k3, n3 = len(seq.saved3[0]), len(seq.saved3[4])
    ids, birth, length, off, xy = cut(seq.saved3, 400)

    def refused(index, what, ids=ids, birth=birth, length=length, xy=xy):
        with pytest.raises(pt.hip.PsfmError) as e:
            ctx.set_result(ids, birth, length, xy)
        assert e.value.status == pt.hip.PSFM_ERR_ARG, str(e.value)
        assert what in str(e.value) and (index is None or "trajectory %d " % index in str(e.value)), str(e.value)

    def changed(a, where, value):
        a = a.copy()
        a[where] = value
        return a
    refused(7, "ascend", ids=changed(ids, 7, ids[6]))
    refused(1, "ascend", ids=changed(ids, 0, ids[1]))                          # (lane 1 reads ids[0])
    refused(0, "2^28", ids=changed(ids, 0, -1))
    refused(399, "2^28", ids=changed(ids, 399, 1 << 28))
    refused(0, "len", length=changed(length, 0, 0))
    refused(399, "len", length=changed(length, 399, -3))
    refused(12, "birth", birth=changed(birth, 12, -1))
    refused(399, "2^30", birth=changed(birth, 399, (1 << 30) - 1))
    refused(5, "birth", birth=changed(birth, 5, -1), length=changed(length, 300, 0))     # two bad entries: the lower one is named
    refused(None, "add up", xy=xy[:-1])
    refused(None, "add up", length=changed(length, 3, length[3] + 1))
    n_result = ctypes.c_int64(-5)
    s0 = pt.hip.current_stream_ptr(ctx.device)
    for args in ((-1, 0, vp(ids), vp(birth), vp(length), vp(xy)), (400, -1, vp(ids), vp(birth), vp(length), vp(xy)),
                 (400, len(xy), None, vp(birth), vp(length), vp(xy)), (400, len(xy), vp(ids), vp(birth), vp(length), None)):
        assert L.psfm_result_set(ctx.handle, *args, ctypes.byref(n_result), s0) == pt.hip.PSFM_ERR_ARG
    # a file whose record 256 differs from the template in one byte, and a truncated one
    from point_trajectory import reference_pickle as rp
    path = str(tmp_path / "track.npy")
    pt.trajectory.save_track_npy(path, as_set(cut(seq.base, 300)))
    data = bytearray(open(path, "rb").read())
    _, xy_data, n_points, rec_start, n, R, end, _ = rp._FOOTER.unpack(bytes(data[-64:]))
    rec, at = rp._record_template()
    plain = [j for j in range(R) if not any(a <= j < a + 4 for a in at.values())]
    data[rec_start + 256 * R + plain[len(plain) // 2]] ^= 0x01
    bad = str(tmp_path / "bad.npy")
    open(bad, "wb").write(bytes(data))
    with pytest.raises(pt.hip.PsfmError) as e:
        ctx.load_track_npy(bad)
    assert e.value.status == pt.hip.PSFM_ERR_ARG and "trajectory 256 " in str(e.value) and "template" in str(e.value)
    open(bad, "wb").write(open(path, "rb").read()[:-7])
    with pytest.raises(pt.hip.PsfmError) as e:
        ctx.load_track_npy(bad)
    assert e.value.status == pt.hip.PSFM_ERR_ARG and "footer" in str(e.value)
    with pytest.raises(pt.hip.PsfmError) as e:
        ctx.load_track_npy(str(tmp_path / "missing.npy"))
    assert e.value.status == pt.hip.PSFM_ERR_ARG
    # nothing of all that touched the tracker's result or its saved set
    assert same(result_copy(pt, ctx, seq.n_traj, seq.n_points), seq.full)
    assert same(filtered_copy(pt, ctx, k3, n3), seq.saved3)
    # ... which still takes traj_min_len = 0 and gives its keys
    import torch
    assert result_filter(pt, ctx, 0) == (seq.n_traj, seq.n_points)
    keys = torch.empty((seq.n_traj,), dtype=torch.int64, device="cuda")
    pt.hip.check(L.psfm_result_keys(ctx.handle, int(seq.g["ratio"]), int(seq.g["W"]), pt.hip.ptr(keys), s0))
    torch.cuda.synchronize()


def test_a_set_result_refuses_keys_and_traj_min_len_below_one(pt, seq):
    import torch
    from psfm_motion_seg.load_cut_seq import sample_window_device, sample_windows_device
    from psfm_sfm import matches_from_flow as mff
    ids, birth, length, off, xy = cut(seq.saved3, 400)
    ctx, L = pt.hip.Context(0), pt.hip.lib()
    ctx.set_result(ids, birth, length, xy)
    s0 = pt.hip.current_stream_ptr(ctx.device)
    keys = torch.empty((int(ids[-1]) + 1,), dtype=torch.int64, device="cuda")
    assert L.psfm_result_keys(ctx.handle, 2, 64, pt.hip.ptr(keys), s0) == pt.hip.PSFM_ERR_ARG
    assert result_filter(pt, ctx, 1)[0] == 400
    k, n = ctypes.c_int64(0), ctypes.c_int64(0)
    for m in (0, -1):
        assert L.psfm_result_filter(ctx.handle, m, ctypes.byref(k), ctypes.byref(n), s0) == pt.hip.PSFM_ERR_ARG
        assert "traj_min_len" in L.psfm_last_error().decode()
        with pytest.raises(pt.hip.PsfmError):
            mff.result_filter_batch_device([ctx], m)
        with pytest.raises(pt.hip.PsfmError):
            sample_window_device(ctx, 0, 10, (48, 64), (30, 50), 10 ** 9, 3, m)
        with pytest.raises(pt.hip.PsfmError):
            sample_windows_device(ctx, [(0, 10), (10, 10)], (48, 64), (30, 50), 10 ** 9, 3, m)
    assert same(filtered_copy(pt, ctx, 400, len(xy)), (ids, birth, length, off, xy))      # the refused filters left the saved set alone
    assert sample_window_device(ctx, 0, 10, (48, 64), (30, 50), 10 ** 9, 3, 1)[0].numel() > 0
    # a tracker's result on the same context is a tracker's result again
    pt.trajectory.run_connect(seq.ff, seq.fb, None, None, 1.0, int(seq.g["ratio"]), return_device=True, ctx=ctx)
    assert result_filter(pt, ctx, 0) == (seq.n_traj, seq.n_points)
    assert L.psfm_result_keys(ctx.handle, 2, 64, pt.hip.ptr(torch.empty((seq.n_traj,), dtype=torch.int64, device="cuda")), s0) == 0
    torch.cuda.synchronize()
    ctx.close()


# ---- the entry points ------------------------------------------------------------------------------------------------------------

def assert_same_matches(a, b, names):
    assert list(a) == list(b) == names
    for n in names:
        assert np.array_equal(np.asarray(a[n].keypoints, np.float64).reshape(-1, 2), np.asarray(b[n].keypoints, np.float64).reshape(-1, 2))
        assert list(a[n].match_pairs) == list(b[n].match_pairs)
        for key in a[n].match_pairs:
            assert np.array_equal(np.asarray(a[n].match_pairs[key]), np.asarray(b[n].match_pairs[key])), (n, key)


def test_traj_to_matches_device_equals_host_on_the_same_files(pt, seq, tmp_path):
    from psfm_motion_seg.merge_labels import labelled_as_dict, merge_labels_host
    from psfm_sfm import matches_from_flow as mff
    g = golden(LABELS_A)
    names = ["%05d.png" % i for i in range(int(g["T"]))]
    # a TrajectorySet file of this package (through psfm_load_track_npy) ...
    img_dir, traj_dir = dirs(tmp_path, names, "set")
    pt.trajectory.save_track_npy(str(traj_dir / "track.npy"), as_set(seq.saved3))
    out = {}
    for device in (False, True):
        out[device] = mff.traj_to_matches(str(img_dir), str(traj_dir), str(tmp_path / ("p%d.txt" % device)), as_arrays=True, device=device)
    assert_same_matches(out[True], out[False], names)
    assert open(str(tmp_path / "p1.txt")).read() == open(str(tmp_path / "p0.txt")).read() != ""
    # ... and the labelled dict stage 2 writes, for both values of remove_dynamic, against the host route and the reference's tables
    img_dir, traj_dir = dirs(tmp_path, names, "labelled")
    np.save(str(traj_dir / "track.npy"), labelled_as_dict(*merge_labels_host(*checker_saved_set(LABELS_A), fixture_windows(g))), allow_pickle=True)
    for rd in (True, False):
        for device in (False, True):
            out[device] = mff.traj_to_matches(str(img_dir), str(traj_dir), str(tmp_path / ("q%d.txt" % device)), remove_dynamic=rd, device=device)
        assert_same_matches(out[True], out[False], names)
        check_match_tables(out[True], names, tables_view(g, rd))
        assert open(str(tmp_path / "q1.txt")).read() == open(str(tmp_path / "q0.txt")).read()


def test_import_keypoints_matches_device_equals_host_on_a_set_file(pt, seq, tmp_path):
    from _database_np import create_tables, read_tables
    from psfm_sfm.database import import_keypoints_matches
    T = int(seq.g["T"])
    names = ["%05d.png" % i for i in range(T)]
    rng = np.random.default_rng(12)
    image_ids = {names[i]: int(v) for i, v in zip(rng.permutation(T), rng.permutation(T) + 3)}
    img_dir, traj_dir = dirs(tmp_path, names, "db")
    pt.trajectory.save_track_npy(str(traj_dir / "track.npy"), as_set(seq.saved3))
    got = {}
    for device in (False, True):
        path = tmp_path / ("d%d.db" % device)
        create_tables(path)
        import_keypoints_matches(image_ids, str(img_dir), str(path), str(tmp_path / ("p%d.txt" % device)), str(traj_dir),
                                 skip_geometric_verification=True, device=device)
        got[device] = read_tables(path)
    assert got[True] == got[False] and len(got[True][1]) > 0
    assert open(str(tmp_path / "p1.txt")).read() == open(str(tmp_path / "p0.txt")).read() != ""


def test_label_track_npy_equals_the_in_process_route(pt, seq, tmp_path):
    """Stage 2 from file to file against label_trajectories_batched on the tracker's own context: seeded weights, constant depth."""
    import torch
    from psfm_motion_seg.merge_labels import label_track_npy, label_trajectories_batched
    rerun_tracker(pt, seq)
    g = seq.g
    T, raw_hw, hw, window = int(g["T"]), (int(g["H"]), int(g["W"])), tuple(int(x) for x in g["input_size"]), int(g["window"])
    depth_for_window = lambda time_idx: torch.full((len(time_idx),) + hw, 0.5, dtype=torch.float32, device="cuda")
    want = label_trajectories_batched(T, window, raw_hw, hw, 10 ** 9, pt.enc_weights, pt.weights, depth_for_window, seed=3, ctx=seq.ctx).as_dict()
    assert len(want) > 100
    src, dst = tmp_path / "trajectories", tmp_path / "trajectories_labeled"
    src.mkdir()
    pt.trajectory.save_track_npy(str(src / "track.npy"), as_set(seq.saved3))
    for front in ("window", "batch"):
        label_track_npy(str(src), str(dst), T, raw_hw, hw, pt.enc_weights, pt.weights, depth_for_window, window=window, traj_max_num=10 ** 9,
                        seed=3, front=front)
        got = np.load(str(dst / "track.npy"), allow_pickle=True).item()
        assert list(got) == list(want)
        for key in want:
            for name in ("frame_ids", "locations", "labels"):
                a, b = np.asarray(got[key][name]), np.asarray(want[key][name])
                assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (key, name)


def test_a_labelled_file_is_scored_like_the_labelled_set(pt, tmp_path):
    from psfm_motion_seg.ground_truth import frame_counts_device, frame_counts_file_device
    from psfm_motion_seg.merge_labels import labelled_as_dict, merge_labels_host
    g = golden(LABELS_A)
    lset = merge_labels_host(*checker_saved_set(LABELS_A), fixture_windows(g))
    path = str(tmp_path / "track.npy")
    np.save(path, labelled_as_dict(*lset), allow_pickle=True)
    T, H, W = int(g["T"]), int(g["H"]), int(g["W"])
    masks = (np.random.default_rng(3).uniform(size=(T, H, W)) < 0.4).astype(np.uint8) * 255
    ctx = pt.hip.Context(0)
    got = frame_counts_file_device(path, masks, ctx=ctx).cpu().numpy()
    want = frame_counts_device(masks, lset[2], lset[3], lset[4], ctx=ctx).cpu().numpy()
    assert np.array_equal(got, want) and int(got.sum()) == len(lset[2])
    ctx.close()


def test_a_set_file_with_true_labels_takes_the_host_tables(pt, seq, tmp_path):
    """A result holds no labels: a TrajectorySet file that carries True labels (csr layout: CSR-backed; the generic pickle of fewer
    than 1024 trajectories: map-backed) must not lose them under remove_dynamic -- device=True returns what device=False returns."""
    from _database_np import create_tables, read_tables
    from point_trajectory.optimize.build import particlesfm
    from psfm_sfm import matches_from_flow as mff
    from psfm_sfm.database import import_keypoints_matches
    T = int(seq.g["T"])
    names = ["%05d.png" % i for i in range(T)]
    ids, birth, length, off, xy = cut(seq.saved3, 300)
    labels = np.random.default_rng(8).uniform(size=len(xy)) < 0.3
    ts = particlesfm.TrajectorySet._from_csr(ids.astype(np.int64), birth, length, off, xy, labels)
    for tag, layout in (("csr", "csr"), ("map", "reference")):
        img_dir, traj_dir = dirs(tmp_path, names, tag)
        pt.trajectory.save_track_npy(str(traj_dir / "track.npy"), ts, layout=layout)
        _, kind, sizes = pt.trajectory.load_track_npy_device(str(traj_dir / "track.npy"), pt.hip.Context(0))
        assert kind == "set" and sizes["route"] == "host" and sizes["true_labels"] is True
        for rd in (True, False):
            out = {d: mff.traj_to_matches(str(img_dir), str(traj_dir), str(tmp_path / ("%s%d.txt" % (tag, d))), remove_dynamic=rd, as_arrays=True,
                                          device=d) for d in (False, True)}
            assert_same_matches(out[True], out[False], names)
            assert sum(len(out[True][n].keypoints) for n in names) == (int((~labels).sum()) if rd else len(xy))
        got = {}
        for d in (False, True):
            path = tmp_path / ("%s_%d.db" % (tag, d))
            create_tables(path)
            import_keypoints_matches({n: i + 1 for i, n in enumerate(names)}, str(img_dir), str(path), str(tmp_path / "p.txt"), str(traj_dir),
                                     skip_geometric_verification=True, device=d)
            got[d] = read_tables(path)
        assert got[True] == got[False] and len(got[True][1]) > 0


def test_an_empty_labelled_file(pt, tmp_path):
    from psfm_motion_seg.ground_truth import frame_counts_file_device
    from psfm_motion_seg.merge_labels import set_labelled
    from psfm_sfm import matches_from_flow as mff
    ctx = pt.hip.Context(0)
    assert set_labelled(ctx, {}) == (0, 0)
    path = str(tmp_path / "track.npy")
    np.save(path, {}, allow_pickle=True)
    _, kind, sizes = pt.trajectory.load_track_npy_device(path, ctx)
    assert kind == "labelled" and sizes == {"n_traj": 0, "n_points": 0, "route": "host"}
    tables = mff.match_tables_labelled_device(ctx, 4, True)
    assert tables[0].tolist() == [0] * 5 and len(tables[5]) == 0
    assert int(frame_counts_file_device(path, np.zeros((3, 8, 8), np.uint8), ctx=ctx).sum()) == 0
    ctx.close()
