"""psfm_matches_to_database / psfm_database_copy (csrc/psfm_database.hip) on the device, bit for bit against the NumPy model
psfm_sfm.database.database_tables_host, which tests/test_database_host.py pins to the reference's own import_keypoints_matches
(tests/golden/database_*.npz).  Labelled sets enter the context through psfm_labels_set (the fixtures' dict order, frame gaps and
non-ascending frames included); the saved-set producer runs on a small psfm_connect result."""
import ctypes
import hashlib

import numpy as np
import pytest

from _common import golden, regen_inputs
from _database_np import (CASES, assert_database_equals_fixture, assert_tables_bit_equal, assert_tables_equal_fixture, create_tables,
                          fixture, ids_pos, match_tables)

pytestmark = pytest.mark.gpu


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


def vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def labels_set(pt, ctx, off, frames, xy, labels):
    off = np.ascontiguousarray(off, np.int64)
    frames = np.ascontiguousarray(frames, np.int32)
    xy = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
    labels = np.ascontiguousarray(labels, np.uint8)
    ids = np.arange(len(off) - 1, dtype=np.int32)
    pt.hip.check(pt.hip.lib().psfm_labels_set(ctx.handle, len(off) - 1, len(frames), vp(ids), vp(off), vp(frames), vp(xy), vp(labels),
                                              pt.hip.current_stream_ptr(ctx.device)))


def labelled_tables(pt, ctx, n_img, remove_dynamic=True):
    """psfm_labels_to_matches only: the match tables stay in the context."""
    from psfm_sfm import matches_from_flow as mff
    a, b, c = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    pt.hip.check(pt.hip.lib().psfm_labels_to_matches(ctx.handle, n_img, mff.SAMPLE_K, 1 if remove_dynamic else 0, ctypes.byref(a),
                                                     ctypes.byref(b), ctypes.byref(c), pt.hip.current_stream_ptr(ctx.device)))
    return int(a.value), int(b.value), int(c.value)


def device_vs_model(pt, ctx, off, frames, xy, labels, n_img, db_id, db_pos, remove_dynamic=True):
    """Labelled set -> match tables -> database tables on the device; the NumPy model of the same input; both returned, compared."""
    from psfm_sfm import matches_from_flow as mff
    from psfm_sfm.database import database_tables_device, database_tables_host
    labels_set(pt, ctx, off, frames, xy, labels)
    labelled_tables(pt, ctx, n_img, remove_dynamic)
    got = database_tables_device(ctx, n_img, db_id, db_pos)
    want = database_tables_host(mff.match_tables_host(np.asarray(off, np.int64), np.asarray(frames, np.int64), np.asarray(xy, np.float64).reshape(-1, 2),
                                                      np.asarray(labels).astype(bool), n_img, remove_dynamic), db_id, db_pos)
    assert_tables_bit_equal(got, want)
    return got, want


def pairs_set(pairs_with_counts):
    """[((frame_a, frame_b), n)] -> a labelled set of n two-point trajectories per entry: directed pairs (a,b) and (b,a), n rows each."""
    frames = np.concatenate([np.tile(np.array(p, np.int32), n) for p, n in pairs_with_counts])
    n_traj = len(frames) // 2
    off = 2 * np.arange(n_traj + 1, dtype=np.int64)
    rng = np.random.default_rng(n_traj)
    xy = rng.uniform(0, 1000, size=(2 * n_traj, 2))
    return off, frames, xy, np.zeros(2 * n_traj, np.uint8)


# ---- the fixtures ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CASES)
def test_labelled_producer_equals_model_and_reference_fixture(pt, name):
    f = fixture(name)
    db_id, db_pos = ids_pos(f)
    ctx = pt.hip.context()
    got, _ = device_vs_model(pt, ctx, f["off"], f["frames"], f["xy"], f["labels"], len(f["names"]), db_id, db_pos)
    assert_tables_equal_fixture(got, f)
    # all points kept: other tables, the same agreement
    device_vs_model(pt, ctx, f["off"], f["frames"], f["xy"], f["labels"], len(f["names"]), db_id, db_pos, remove_dynamic=False)


def test_saved_set_producer_equals_model(pt):
    """psfm_connect -> psfm_result_filter -> psfm_traj_to_matches -> psfm_matches_to_database against database_tables_host of
    match_tables_host over the saved set copied to the host."""
    import torch
    from psfm_sfm import matches_from_flow as mff
    from psfm_sfm.database import database_tables_device, database_tables_host
    g = golden("matches_24x32_t27_dyn")
    d = regen_inputs(g, stride2=False)
    ff = torch.from_numpy(np.stack(d["flows_f"])).cuda()
    fb = torch.from_numpy(np.stack(d["flows_b"])).cuda()
    ctx = pt.hip.context()
    pt.trajectory.run_connect(ff, fb, None, None, 1.0, int(g["ratio"]), return_device=True)
    T = int(g["T"])
    L, sp = pt.hip.lib(), pt.hip.current_stream_ptr(ctx.device)
    k, n = ctypes.c_int64(0), ctypes.c_int64(0)
    pt.hip.check(L.psfm_result_filter(ctx.handle, 3, ctypes.byref(k), ctypes.byref(n), sp))
    k, n = int(k.value), int(n.value)
    ids, birth, length = np.empty(k, np.int32), np.empty(k, np.int32), np.empty(k, np.int32)
    off, xy = np.zeros(k + 1, np.int64), np.empty((n, 2), np.float64)
    pt.hip.check(L.psfm_result_filtered_copy(ctx.handle, vp(ids), vp(birth), vp(length), vp(off), vp(xy), sp))
    frames = (np.repeat(birth, length) + np.arange(n) - np.repeat(off[:-1], length)).astype(np.int64)
    rng = np.random.default_rng(77)
    db_id, db_pos = (rng.permutation(T) + 5).astype(np.int32), rng.permutation(T).astype(np.int32)
    mff.match_tables_device(ctx, T)                                     # (filter + psfm_traj_to_matches; its copy is not needed here)
    got = database_tables_device(ctx, T, db_id, db_pos)
    tables = mff.match_tables_host(off, frames, xy, np.zeros(n, bool), T)
    assert_tables_bit_equal(got, database_tables_host(tables, db_id, db_pos))
    assert length.max() > 20 and 0 < len(got.rows) < len(tables[5])       # the two directions differ, and one of them is dropped


# ---- edges of the compaction -----------------------------------------------------------------------------------------------------

def test_two_images_one_trajectory(pt):
    ctx = pt.hip.context()
    got, _ = device_vs_model(pt, ctx, [0, 2], [0, 1], [[1.5, 2.5], [3.0, 4.0]], [0, 0], 2, np.array([8, 3]), np.array([1, 0]))
    assert got.pair_key.tolist() == [2] and got.rows.tolist() == [[0, 0]] and got.pair_off.tolist() == [0, 1]     # (1,0) is written
    assert got.pair_id.tolist() == [3 * (2 ** 31 - 1) + 8] and got.kp_f32.tolist() == [[2.0, 3.0], [3.5, 4.5]]


@pytest.mark.parametrize("delta", [-1, 0, 1])
@pytest.mark.parametrize("swap_first", [False, True])
def test_pair_boundaries_around_the_chunk(pt, delta, swap_first):
    """chunk - 1, chunk, chunk + 1 rows in a first kept pair followed by a 1-row pair: the boundary falls at the last row of a chunk,
    on the chunk boundary and one row behind it, at both parities; with and without the column swap on the first pair."""
    from psfm_sfm.database import chunk_rows
    chunk = chunk_rows()
    assert chunk >= 2 and chunk % 2 == 0
    off, frames, xy, labels = pairs_set([((0, 1), chunk + delta), ((2, 3), 1)])
    ids = np.array([9, 4, 1, 2] if swap_first else [4, 9, 2, 1])
    got, _ = device_vs_model(pt, pt.hip.context(), off, frames, xy, labels, 4, ids, np.arange(4))
    assert got.pair_key.tolist() == [1, 11] and got.pair_off.tolist() == [0, chunk + delta, chunk + delta + 1]


def test_a_pair_that_spans_several_chunks_at_an_odd_source_offset(pt):
    """Dropped pairs in front of a kept one shift its source offset; here (1,0) is written, not (0,1), behind an odd number of rows."""
    from psfm_sfm.database import chunk_rows
    chunk = chunk_rows()
    off, frames, xy, labels = pairs_set([((0, 1), 2 * chunk + 2), ((1, 2), 5), ((0, 2), 1)])
    got, want = device_vs_model(pt, pt.hip.context(), off, frames, xy, labels, 3, np.array([1, 2, 3]), np.array([2, 1, 0]))
    assert got.pair_key.tolist() == [3, 6, 7]                             # (1,0) from source row 2 chunk + 3, (2,0), (2,1)
    assert got.pair_off.tolist() == [0, 2 * chunk + 2, 2 * chunk + 3, 2 * chunk + 8]


def test_more_kept_pairs_than_one_scan_block(pt):
    """40 images, short trajectories over random frame triples: several hundred kept pairs of a few rows each."""
    rng = np.random.default_rng(5)
    n_img, n_traj = 40, 1500
    frames = np.concatenate([np.sort(rng.choice(n_img, 3, replace=False)) for _ in range(n_traj)]).astype(np.int32)
    off = 3 * np.arange(n_traj + 1, dtype=np.int64)
    xy = rng.uniform(-1, 2000, size=(3 * n_traj, 2))
    labels = (rng.random(3 * n_traj) < 0.1).astype(np.uint8)
    got, _ = device_vs_model(pt, pt.hip.context(), off, frames, xy, labels, n_img, rng.permutation(n_img) + 1, rng.permutation(n_img))
    assert len(got.pair_id) > 600                                         # more than two blocks of 256 pairs


def test_all_points_dynamic(pt):
    f = fixture(CASES[3])
    db_id, db_pos = ids_pos(f)
    ctx = pt.hip.context()
    got, _ = device_vs_model(pt, ctx, f["off"], f["frames"], f["xy"], np.ones(len(f["frames"]), np.uint8), 4, db_id, db_pos)
    assert got.kp_off.tolist() == [0] * 5 and got.kp_f32.shape == (0, 2)
    assert got.pair_id.shape == (0,) and got.pair_off.tolist() == [0] and got.rows.shape == (0, 2)


def test_every_pair_one_directional(pt):
    """Trajectories of 21 points, the first 20 (the only targets) in image 0, the 21st in image 1 + i: the pairs are the self pair
    (0,0) and the sources (1 + i, 0), none of which has a reverse -- nothing is dropped, whatever the order."""
    n_extra = 5
    frames = np.concatenate([np.array([0] * 20 + [1 + i], np.int32) for i in range(n_extra)])
    off = 21 * np.arange(n_extra + 1, dtype=np.int64)
    xy = np.random.default_rng(2).uniform(0, 100, size=(21 * n_extra, 2))
    n_img = 1 + n_extra
    for pos in (np.arange(n_img), np.arange(n_img)[::-1].copy()):
        got, _ = device_vs_model(pt, pt.hip.context(), off, frames, xy, np.zeros(len(frames), np.uint8), n_img, np.arange(n_img, 0, -1), pos)
        assert got.pair_key.tolist() == [0] + [(1 + i) * n_img for i in range(n_extra)]
        assert np.diff(got.pair_off).tolist() == [20 * 19 * n_extra] + [20] * n_extra


# ---- the interface ---------------------------------------------------------------------------------------------------------------

def test_two_calls_give_identical_bytes_and_device_copy_equals_host_copy(pt):
    import torch
    from psfm_sfm.database import database_tables_device
    f = fixture(CASES[0])
    db_id, db_pos = ids_pos(f)
    ctx = pt.hip.context()
    labels_set(pt, ctx, f["off"], f["frames"], f["xy"], f["labels"])
    labelled_tables(pt, ctx, len(f["names"]))
    a = database_tables_device(ctx, len(f["names"]), db_id, db_pos)
    b = database_tables_device(ctx, len(f["names"]), db_id, db_pos)
    assert_tables_bit_equal(a, b)
    dev = torch.device("cuda", ctx.device)
    kp = torch.empty((len(a.kp_f32), 2), dtype=torch.float32, device=dev)
    pid, key = (torch.empty(len(a.pair_id), dtype=torch.int64, device=dev) for _ in range(2))
    poff = torch.empty(len(a.pair_off), dtype=torch.int64, device=dev)
    rows = torch.empty((len(a.rows), 2), dtype=torch.int32, device=dev)
    p = pt.hip.ptr
    pt.hip.check(pt.hip.lib().psfm_database_copy(ctx.handle, p(kp), p(pid), p(key), p(poff), p(rows), pt.hip.current_stream_ptr(ctx.device)))
    assert kp.cpu().numpy().tobytes() == a.kp_f32.tobytes() and pid.cpu().numpy().tobytes() == a.pair_id.tobytes()
    assert key.cpu().numpy().tobytes() == a.pair_key.tobytes() and poff.cpu().numpy().tobytes() == a.pair_off.tobytes()
    assert rows.cpu().numpy().tobytes() == a.rows.tobytes()
    # every pointer may be NULL
    pt.hip.check(pt.hip.lib().psfm_database_copy(ctx.handle, None, None, None, None, None, pt.hip.current_stream_ptr(ctx.device)))


def test_tables_survive_a_rebuild_of_the_match_tables(pt):
    from psfm_sfm.database import DatabaseTables
    f, small = fixture(CASES[0]), fixture(CASES[3])
    db_id, db_pos = ids_pos(f)
    ctx = pt.hip.context()
    got, _ = device_vs_model(pt, ctx, f["off"], f["frames"], f["xy"], f["labels"], len(f["names"]), db_id, db_pos)
    labels_set(pt, ctx, small["off"], small["frames"], small["xy"], small["labels"])
    labelled_tables(pt, ctx, 4)                                            # other match tables, other n_img
    kp, pid, key = np.empty_like(got.kp_f32), np.empty_like(got.pair_id), np.empty_like(got.pair_key)
    poff, rows = np.empty_like(got.pair_off), np.empty_like(got.rows)
    pt.hip.check(pt.hip.lib().psfm_database_copy(ctx.handle, vp(kp), vp(pid), vp(key), vp(poff), vp(rows), pt.hip.current_stream_ptr(ctx.device)))
    assert_tables_bit_equal(DatabaseTables(got.kp_off, kp, pid, key, poff, rows), got)


def test_argument_errors_leave_the_context_usable(pt):
    from psfm_sfm.database import database_tables_device
    fresh = pt.hip.Context(pt.hip.context().device)
    try:
        with pytest.raises(pt.hip.PsfmError) as e:                        # no match tables yet
            database_tables_device(fresh, 4, np.array([1, 2, 3, 4]), np.arange(4))
        assert e.value.status == pt.hip.PSFM_ERR_ARG
        f = fixture(CASES[3])
        db_id, db_pos = ids_pos(f)
        labels_set(pt, fresh, f["off"], f["frames"], f["xy"], f["labels"])
        labelled_tables(pt, fresh, 4)
        bad = [(4, [3, 7, 7, 2], db_pos), (4, [0, 7, 9, 2], db_pos), (4, [3, 7, 9, 2 ** 31 - 1], db_pos), (4, db_id, [0, 0, 2, 3]),
               (4, db_id, [1, 2, 3, 4]), (4, db_id, [0, 1, 2, -1]), (3, db_id[:3], [0, 1, 2]), (5, [1, 2, 3, 4, 5], [0, 1, 2, 3, 4])]
        for n_img, ids, pos in bad:
            with pytest.raises(pt.hip.PsfmError) as e:
                database_tables_device(fresh, n_img, np.array(ids, np.int64).astype(np.int32), np.array(pos, np.int32))
            assert e.value.status == pt.hip.PSFM_ERR_ARG
            assert_tables_equal_fixture(database_tables_device(fresh, 4, db_id, db_pos), f)      # a correct call afterwards
        t = database_tables_device(fresh, 4, np.array([1, 2 ** 31 - 2, 9, 2], np.int32), db_pos)      # the ends of the id range are ids
        assert (2 ** 31 - 1) + (2 ** 31 - 2) in t.pair_id.tolist()
    finally:
        fresh.close()


def test_labels_set_refuses_a_broken_off(pt):
    ctx = pt.hip.Context(pt.hip.context().device)
    try:
        for off in ([1, 2, 4], [0, 3, 2, 4], [0, 2, 5]):
            with pytest.raises(pt.hip.PsfmError) as e:
                labels_set(pt, ctx, off, [0, 1, 2, 3], np.zeros((4, 2)), np.zeros(4, np.uint8))
            assert e.value.status == pt.hip.PSFM_ERR_ARG
            with pytest.raises(pt.hip.PsfmError):                         # ... and the context holds no labelled set
                labelled_tables(pt, ctx, 4)
        labels_set(pt, ctx, [0, 2, 4], [0, 1, 2, 3], np.zeros((4, 2)), np.zeros(4, np.uint8))
        assert labelled_tables(pt, ctx, 4) == (4, 4, 4)
    finally:
        ctx.close()


# ---- end to end ------------------------------------------------------------------------------------------------------------------

def test_import_keypoints_matches_device_equals_reference_fixture(pt, tmp_path):
    from psfm_sfm.database import import_keypoints_matches_device
    f = fixture(CASES[0])
    ctx = pt.hip.context()
    labels_set(pt, ctx, f["off"], f["frames"], f["xy"], f["labels"])
    path = tmp_path / "database.db"
    create_tables(path)
    import_keypoints_matches_device(ctx, f["image_ids"], f["names"], str(path), str(tmp_path / "pairs.txt"), skip_geometric_verification=True,
                                    labelled=True)
    assert_database_equals_fixture(path, f)
    assert hashlib.sha256(open(str(tmp_path / "pairs.txt")).read().encode()).hexdigest() == f["pair_file_hash"]
    with pytest.raises(ValueError):
        import_keypoints_matches_device(ctx, dict(f["image_ids"], other=999), f["names"], str(path), str(tmp_path / "pairs.txt"), labelled=True)
