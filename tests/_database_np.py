"""Shared by tests/test_database_host.py and tests/test_gpu_database.py: the fixtures of tests/golden/make_database_golden.py as
Python objects, a COLMAP database with the three tables the importer writes, and comparisons keyed by id (insertion order is
unobservable: image_id and pair_id are the rowid)."""
import sqlite3

import numpy as np

from _common import golden

CASES = ["database_a_permuted", "database_b_ascending", "database_c_descending", "database_d_hand"]
MAX_IMAGE_ID = 2 ** 31 - 1
EYE = np.eye(3).tobytes()


def fixture(name):
    """The .npz -> dict: trajectories (dict in the reference's dict order), names, image_ids (ordered), flat arrays, and the rows of
    the three tables as {id: tuple}."""
    g = golden(name)
    off = g["traj_off"]
    trajs = {int(k): {"locations": g["traj_xy"][off[i]:off[i + 1]], "labels": g["traj_labels"][off[i]:off[i + 1]].astype(np.int64),
                      "frame_ids": g["traj_frames"][off[i]:off[i + 1]]} for i, k in enumerate(g["traj_keys"])}
    cut = lambda data, o, i: bytes(data[o[i]:o[i + 1]])
    kp = {int(k): (int(g["kp_rows"][i]), int(g["kp_cols"][i]), cut(g["kp_data"], g["kp_off"], i)) for i, k in enumerate(g["kp_image_id"])}
    mt = {int(k): (int(g["m_rows"][i]), int(g["m_cols"][i]), cut(g["m_data"], g["m_off"], i)) for i, k in enumerate(g["m_pair_id"])}
    tv = {int(k): (int(g["g_rows"][i]), int(g["g_cols"][i]), cut(g["g_data"], g["g_off"], i), int(g["g_config"][i]),
                   bytes(g["g_F"][i]), bytes(g["g_E"][i]), bytes(g["g_H"][i])) for i, k in enumerate(g["g_pair_id"])}
    names = [str(n) for n in g["image_names"]]
    image_ids = {str(n): int(v) for n, v in zip(g["ids_names"], g["ids_values"])}
    return dict(trajs=trajs, names=names, image_ids=image_ids, off=off, frames=g["traj_frames"], xy=g["traj_xy"], labels=g["traj_labels"],
                keypoints=kp, matches=mt, geometries=tv, pair_file_hash=str(g["pair_file_hash"]), n_directed=int(g["n_directed_pairs"]))


def ids_pos(f):
    from psfm_sfm.database import ids_and_positions
    return ids_and_positions(f["image_ids"], f["names"])


def match_tables(f, remove_dynamic=True):
    from psfm_sfm import matches_from_flow as mff
    return mff.match_tables_host(f["off"], f["frames"], f["xy"], f["labels"].astype(bool), len(f["names"]), remove_dynamic)


def rows_by_id(t, db_id):
    """DatabaseTables -> ({image_id: (rows, cols, bytes)}, {pair_id: (rows, cols, bytes)})."""
    assert t.kp_f32.dtype == np.float32 and t.rows.dtype == np.uint32 and t.pair_id.dtype == np.int64
    kp = {int(db_id[i]): (int(t.kp_off[i + 1] - t.kp_off[i]), 2, t.kp_f32[t.kp_off[i]:t.kp_off[i + 1]].tobytes()) for i in range(len(db_id))}
    mt = {int(p): (int(t.pair_off[g + 1] - t.pair_off[g]), 2, t.rows[t.pair_off[g]:t.pair_off[g + 1]].tobytes()) for g, p in enumerate(t.pair_id)}
    assert len(mt) == len(t.pair_id)
    return kp, mt


def assert_tables_equal_fixture(t, f):
    db_id, _ = ids_pos(f)
    kp, mt = rows_by_id(t, db_id)
    assert kp == f["keypoints"]
    assert set(mt) == set(f["matches"])
    assert mt == f["matches"]
    assert len(t.pair_id) == len(f["matches"]) and len(t.rows) == sum(r[0] for r in f["matches"].values())
    assert f["n_directed"] >= len(t.pair_id)


def assert_tables_bit_equal(got, want):
    for key in got._fields:
        a, b = getattr(got, key), getattr(want, key)
        assert a.dtype == b.dtype and a.shape == b.shape, (key, a.dtype, b.dtype, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), key


def create_tables(path):
    """The three tables the importer writes, from COLMAP's public column lists."""
    db = sqlite3.connect(str(path))
    db.execute("CREATE TABLE keypoints (image_id INTEGER PRIMARY KEY NOT NULL, rows INTEGER NOT NULL, cols INTEGER NOT NULL, data BLOB)")
    db.execute("CREATE TABLE matches (pair_id INTEGER PRIMARY KEY NOT NULL, rows INTEGER NOT NULL, cols INTEGER NOT NULL, data BLOB)")
    db.execute("CREATE TABLE two_view_geometries (pair_id INTEGER PRIMARY KEY NOT NULL, rows INTEGER NOT NULL, cols INTEGER NOT NULL, "
               "data BLOB, config INTEGER NOT NULL, F BLOB, E BLOB, H BLOB)")
    db.commit()
    db.close()


def read_tables(path):
    db = sqlite3.connect(str(path))
    b = lambda x: b"" if x is None else bytes(x)
    kp = {r[0]: (r[1], r[2], b(r[3])) for r in db.execute("SELECT image_id, rows, cols, data FROM keypoints")}
    mt = {r[0]: (r[1], r[2], b(r[3])) for r in db.execute("SELECT pair_id, rows, cols, data FROM matches")}
    tv = {r[0]: (r[1], r[2], b(r[3]), r[4], b(r[5]), b(r[6]), b(r[7])) for r in
          db.execute("SELECT pair_id, rows, cols, data, config, F, E, H FROM two_view_geometries")}
    db.close()
    return kp, mt, tv


def assert_database_equals_fixture(path, f, geometries=True):
    kp, mt, tv = read_tables(path)
    assert kp == f["keypoints"]
    assert mt == f["matches"]
    assert tv == (f["geometries"] if geometries else {})
