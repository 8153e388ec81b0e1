"""Match tables -> the keypoints / matches / two_view_geometries rows of the COLMAP database: the consumer
sfm/import_feature_matches.py:76-104 (import_keypoints_matches) of the reference, which writes through
sfm/colmap_utils/database.py:181-225, as array work on tables instead of its per-image np.array() / per-pair np.array().tobytes()
loops over dicts.

Two producers feed ONE writer:
  * `import_keypoints_matches(image_ids, image_dir, database_path, match_list_file, traj_dir, ...)` -- the reference's signature;
    reads track.npy, builds the match tables (matches_from_flow.match_tables_host) and the database tables in NumPy;
  * `import_keypoints_matches_device(ctx, image_ids, image_names, database_path, match_list_file, ...)` -- the database tables
    computed by psfm_matches_to_database (csrc/psfm_database.hip) from the match tables in HBM; only the kept rows as u32 and the
    keypoints as f32 cross PCIe (the reference's route moves both directions of every pair as i32 and the keypoints as f64, and
    then throws half of the rows away).
Both also write the pair list file, line for line the one matches_from_flow.assemble writes (ALL directed pairs, the ones the
database drops included), straight from the tables.

The rules (tests/golden/database_*.npz pin them to the reference's own function):
  keypoints   blob of image i = float32(xy + 0.5), the add in f64 (:82-84, database.py:185), shape (n, 2)
  pairs       the reference walks the images in the iteration order of `image_ids` -- the order of get_image_ids' SELECT, neither
              name order nor id order --, an image's pairs in dict order, and skips a pair whose unordered id pair is already
              written (:88-99).  Equivalent: directed pair (s, t) is written unless the reverse pair (t, s) exists and
              pos[t] < pos[s], pos = position in that order.  A self pair is written.  For trajectories with more than 20 kept
              points the two directions hold different matches, so the reference drops data here; this reproduces it.
  rows        pair_id = min(id_s, id_t) * (2**31 - 1) + max(id_s, id_t); rows are uint32, the two columns swapped when
              id_s > id_t -- by COLMAP id (database.py:196-207)
  geometry    with skip_geometric_verification the same blob goes into two_view_geometries with config = 2 and three 3x3 f64
              identities (database.py:209-225)
Insertion order is unobservable: pair_id and image_id are INTEGER PRIMARY KEYs, i.e. the rowid.  Compare tables keyed by id.

Deviations from the reference, both on input it cannot handle:
  * an image without keypoints gets a (0, 2) row with an empty blob; the reference fails its own
    `assert len(keypoints.shape) == 2` there, because np.array([]) is 1-D;
  * `image_ids` must name exactly the images of `image_names`, otherwise ValueError before anything is written; the reference
    raises KeyError only when a missing image is actually touched (after writing part of the database).
"""
import collections
import os
import sqlite3

import numpy as np

from . import matches_from_flow as mff

MAX_IMAGE_ID = 2 ** 31 - 1       # database.py:41

DatabaseTables = collections.namedtuple("DatabaseTables", "kp_off kp_f32 pair_id pair_key pair_off rows")
DatabaseTables.__doc__ = """kp_off (n_img+1) i64, kp_f32 (n_kp,2) f32 -- blob of image i = kp_f32[kp_off[i]:kp_off[i+1]];
pair_id (n_kept) i64; pair_key (n_kept) i64 = src * n_img + tgt of the kept pairs, ascending; pair_off (n_kept+1) i64 into rows;
rows (n_rows_kept,2) u32 -- blob of kept pair g = rows[pair_off[g]:pair_off[g+1]]."""


def ids_and_positions(image_ids, image_names):
    """`image_ids` (ordered mapping name -> COLMAP image_id) against the images in frame order: db_id[i] = id of image i,
    db_pos[i] = position of image i in the mapping's iteration order.  ValueError unless the mapping names exactly the images."""
    names = list(image_names)
    index = {name: i for i, name in enumerate(names)}
    if len(index) != len(names):
        raise ValueError("image_names holds a name twice")
    if len(image_ids) != len(names) or any(name not in index for name in image_ids):
        missing = sorted(set(names) - set(image_ids))
        extra = sorted(set(image_ids) - set(names))
        raise ValueError("image_ids must name exactly the images: missing %r, unknown %r" % (missing[:5], extra[:5]))
    db_id = np.empty(len(names), np.int64)
    db_pos = np.empty(len(names), np.int32)
    for k, (name, image_id) in enumerate(image_ids.items()):
        db_id[index[name]] = int(image_id)
        db_pos[index[name]] = k
    check_ids(db_id, db_pos, len(names))
    return db_id.astype(np.int32), db_pos


def check_ids(db_id, db_pos, n_img):
    """What psfm_matches_to_database answers with PSFM_ERR_ARG: ids in [1, 2**31 - 2] and distinct, db_pos a permutation."""
    db_id, db_pos = np.asarray(db_id, np.int64), np.asarray(db_pos, np.int64)
    if db_id.shape != (n_img,) or db_pos.shape != (n_img,):
        raise ValueError("db_id / db_pos must have one entry per image (%d)" % n_img)
    if n_img and (db_id.min() < 1 or db_id.max() > MAX_IMAGE_ID - 1):
        raise ValueError("image ids must lie in [1, 2**31 - 2]")
    if len(np.unique(db_id)) != n_img:
        raise ValueError("an image id is given to two images")
    if not np.array_equal(np.sort(db_pos), np.arange(n_img)):
        raise ValueError("db_pos is not a permutation of 0..n_img-1")


def database_tables_host(tables, db_id, db_pos):
    """The match tables of matches_from_flow.match_tables_host (or a copy of the device's) -> DatabaseTables, in NumPy: the model of
    psfm_matches_to_database."""
    kp_off, kp_xy, pair_key, pair_off, _, rows = tables
    n_img = len(kp_off) - 1
    check_ids(db_id, db_pos, n_img)
    db_id, db_pos = np.asarray(db_id, np.int64), np.asarray(db_pos, np.int64)
    kp_f32 = (np.asarray(kp_xy, np.float64).reshape(-1, 2) + 0.5).astype(np.float32)
    pair_key = np.asarray(pair_key, np.int64)
    n_p = len(pair_key)
    s, t = pair_key // n_img, pair_key % n_img
    rev = t * n_img + s
    at = np.minimum(np.searchsorted(pair_key, rev), max(n_p - 1, 0))
    exists = pair_key[at] == rev if n_p else np.zeros(0, bool)
    keep = ~(exists & (db_pos[t] < db_pos[s]))
    cnt = np.diff(np.asarray(pair_off, np.int64))[keep] if n_p else np.zeros(0, np.int64)
    out_off = np.zeros(len(cnt) + 1, np.int64)
    np.cumsum(cnt, out=out_off[1:])
    start = np.asarray(pair_off, np.int64)[:-1][keep] if n_p else np.zeros(0, np.int64)
    take = np.repeat(start - out_off[:-1], cnt) + np.arange(out_off[-1])       # source row of every output row
    id_s, id_t = db_id[s[keep]], db_id[t[keep]]
    out = np.asarray(rows).reshape(-1, 2)[take].astype(np.uint32)
    swap = np.repeat(id_s > id_t, cnt)
    out[swap] = out[swap][:, ::-1]
    pair_id = np.minimum(id_s, id_t) * MAX_IMAGE_ID + np.maximum(id_s, id_t)
    return DatabaseTables(np.asarray(kp_off, np.int64), kp_f32, pair_id.astype(np.int64), pair_key[keep], out_off, np.ascontiguousarray(out))


def chunk_rows():
    """Output rows per block of the device's row compaction (psfm_database_chunk_rows)."""
    from point_trajectory import _hip
    return int(_hip.lib().psfm_database_chunk_rows())


def database_tables_device(ctx, n_img, db_id, db_pos):
    """psfm_matches_to_database over the match tables that the last psfm_traj_to_matches / psfm_labels_to_matches left in `ctx`,
    then one copy of the finished tables (psfm_database_copy) -> DatabaseTables of host arrays.  Bad ids / positions: PsfmError."""
    import ctypes
    from point_trajectory import _hip
    L = _hip.lib()
    sp = _hip.current_stream_ptr(ctx.device)
    db_id = np.ascontiguousarray(db_id, np.int32)
    db_pos = np.ascontiguousarray(db_pos, np.int32)
    if db_id.shape != (n_img,) or db_pos.shape != (n_img,):
        raise ValueError("db_id / db_pos must have one entry per image (%d)" % n_img)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    n_p, n_r = ctypes.c_int64(0), ctypes.c_int64(0)
    _hip.check(L.psfm_matches_to_database(ctx.handle, int(n_img), vp(db_id), vp(db_pos), ctypes.byref(n_p), ctypes.byref(n_r), sp))
    kp_off = np.zeros(n_img + 1, np.int64)
    _hip.check(L.psfm_matches_copy(ctx.handle, vp(kp_off), None, None, None, None, None, sp))
    n_p, n_r = int(n_p.value), int(n_r.value)
    kp_f32 = np.empty((int(kp_off[-1]), 2), np.float32)
    pair_id, pair_key = np.empty(n_p, np.int64), np.empty(n_p, np.int64)
    pair_off = np.zeros(n_p + 1, np.int64)
    rows = np.empty((n_r, 2), np.uint32)
    _hip.check(L.psfm_database_copy(ctx.handle, vp(kp_f32), vp(pair_id), vp(pair_key), vp(pair_off), vp(rows), sp))
    return DatabaseTables(kp_off, kp_f32, pair_id, pair_key, pair_off, rows)


def write_pair_file(match_list_file, image_names, pair_key, pair_first):
    """The pair list file of sfm/matches_from_flow.py:110-117 from the match tables: every directed pair, sources in image order,
    an image's pairs in order of first use."""
    n_img = len(image_names)
    pair_key = np.asarray(pair_key, np.int64)
    s, t = pair_key // n_img, pair_key % n_img
    order = np.lexsort((np.asarray(pair_first), s))
    with open(match_list_file, "w") as fp:
        fp.write("".join(image_names[a] + " " + image_names[b] + "\n" for a, b in zip(s[order].tolist(), t[order].tolist())))


_EYE = np.eye(3, dtype=np.float64).tobytes()


def write_database(database_path, image_ids, image_names, db_tables, skip_geometric_verification=False):
    """DatabaseTables -> rows of an existing COLMAP database (tables keypoints, matches, two_view_geometries), one executemany per
    table, every blob a slice of the table's buffer.  image_ids: ordered mapping name -> image_id naming exactly `image_names`
    (the images in frame order), else ValueError.  An image without keypoints gets a (0, 2) row with an empty blob."""
    db_id, _ = ids_and_positions(image_ids, image_names)
    t = db_tables
    if len(t.kp_off) != len(db_id) + 1:
        raise ValueError("the tables were built for %d images, image_names has %d" % (len(t.kp_off) - 1, len(db_id)))
    kp = memoryview(np.ascontiguousarray(t.kp_f32, np.float32).reshape(-1).view(np.uint8))
    rows = memoryview(np.ascontiguousarray(t.rows, np.uint32).reshape(-1).view(np.uint8))
    ko = (8 * np.asarray(t.kp_off, np.int64)).tolist()
    po = (8 * np.asarray(t.pair_off, np.int64)).tolist()
    pair_id = np.asarray(t.pair_id, np.int64).tolist()
    db = sqlite3.connect(str(database_path))
    try:
        db.executemany("INSERT INTO keypoints(image_id, rows, cols, data) VALUES (?, ?, ?, ?)",
                       ((image_id, (ko[i + 1] - ko[i]) // 8, 2, kp[ko[i]:ko[i + 1]]) for i, image_id in enumerate(db_id.tolist())))
        db.executemany("INSERT INTO matches(pair_id, rows, cols, data) VALUES (?, ?, ?, ?)",
                       ((pid, (po[g + 1] - po[g]) // 8, 2, rows[po[g]:po[g + 1]]) for g, pid in enumerate(pair_id)))
        if skip_geometric_verification:
            db.executemany("INSERT INTO two_view_geometries(pair_id, rows, cols, data, config, F, E, H) VALUES (?, ?, ?, ?, ?, ?, ?, ?)",
                           ((pid, (po[g + 1] - po[g]) // 8, 2, rows[po[g]:po[g + 1]], 2, _EYE, _EYE, _EYE) for g, pid in enumerate(pair_id)))
        db.commit()
    finally:
        db.close()


def import_keypoints_matches(image_ids, image_dir, database_path, match_list_file, traj_dir, skip_geometric_verification=False,
                             remove_dynamic=True, device=False):
    """sfm/import_feature_matches.py:76-104, same arguments, on the host: track.npy -> match tables -> database tables -> rows.
    device=True: the file goes into a context (point_trajectory.trajectory.load_track_npy_device) and the match tables and the
    database rows come from the device kernels (import_keypoints_matches_device); the same pair file and the same rows.  The file is
    loaded into the calling thread's context, whose result or labelled set is replaced; a TrajectorySet file that carries True labels
    (a result holds none) takes the host route below."""
    from point_trajectory.trajectory import load_track_npy
    image_names = sorted(os.listdir(image_dir))
    if device:
        from point_trajectory.trajectory import load_track_npy_device
        ctx, kind, sizes = load_track_npy_device(os.path.join(traj_dir, "track.npy"))
        if not (kind == "set" and sizes.get("true_labels")):
            import_keypoints_matches_device(ctx, image_ids, image_names, database_path, match_list_file, skip_geometric_verification,
                                            labelled=(kind == "labelled"), remove_dynamic=remove_dynamic, traj_min_len=1)
            return
    db_id, db_pos = ids_and_positions(image_ids, image_names)
    off, frames, xy, labels = mff._flatten(load_track_npy(os.path.join(traj_dir, "track.npy")))
    tables = mff.match_tables_host(off, frames, xy, labels, len(image_names), remove_dynamic)
    write_pair_file(match_list_file, image_names, tables[2], tables[4])
    write_database(database_path, image_ids, image_names, database_tables_host(tables, db_id, db_pos), skip_geometric_verification)


def import_keypoints_matches_device(ctx, image_ids, image_names, database_path, match_list_file, skip_geometric_verification=False,
                                    labelled=False, remove_dynamic=True, traj_min_len=3):
    """The same from HBM.  labelled=False: the saved set of the last psfm_track / psfm_connect of `ctx` (length >= traj_min_len,
    every point kept: --assume_static); labelled=True: the labelled set that LabelMerger.finish left in `ctx`, kept points =
    labels == 0 when remove_dynamic.  The match tables never leave the device: the pair list needs pair_key and pair_first (two
    small arrays), the database gets the finished blobs."""
    import ctypes
    from point_trajectory import _hip
    L = _hip.lib()
    sp = _hip.current_stream_ptr(ctx.device)
    image_names = list(image_names)
    n_img = len(image_names)
    db_id, db_pos = ids_and_positions(image_ids, image_names)
    n_kp, n_m, n_p = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    if labelled:
        _hip.check(L.psfm_labels_to_matches(ctx.handle, n_img, mff.SAMPLE_K, 1 if remove_dynamic else 0, ctypes.byref(n_kp),
                                            ctypes.byref(n_m), ctypes.byref(n_p), sp))
    else:
        k, npt = ctypes.c_int64(0), ctypes.c_int64(0)
        _hip.check(L.psfm_result_filter(ctx.handle, int(traj_min_len), ctypes.byref(k), ctypes.byref(npt), sp))
        _hip.check(L.psfm_traj_to_matches(ctx.handle, n_img, mff.SAMPLE_K, None, ctypes.byref(n_kp), ctypes.byref(n_m), ctypes.byref(n_p), sp))
    pair_key, pair_first = np.empty(int(n_p.value), np.int64), np.empty(int(n_p.value), np.int64)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    _hip.check(L.psfm_matches_copy(ctx.handle, None, None, vp(pair_key), None, vp(pair_first), None, sp))
    write_pair_file(match_list_file, image_names, pair_key, pair_first)
    tables = database_tables_device(ctx, n_img, db_id, db_pos)
    write_database(database_path, image_ids, image_names, tables, skip_geometric_verification)
    return tables
