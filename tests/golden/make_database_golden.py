#!/usr/bin/env python3
"""Golden vectors for the COLMAP database rows (sfm/import_feature_matches.py:76-104 writing through
sfm/colmap_utils/database.py:181-225), produced by the REFERENCE's own functions: import_feature_matches.py and
colmap_utils/database.py are imported UNMODIFIED from the reference checkout, the database is created by the reference's
create_empty_db, filled by its import_keypoints_matches(skip_geometric_verification=True) from a track.npy written here, and the
three tables are read back and dumped.  Only a `tqdm` stand-in is installed when the real one is missing (as oracle/ref_shim.py
does).  Fixtures hold data only: the trajectories, the image names, the image_ids mapping in iteration order, the rows of the three
tables, the hash of the pair list file.  Run in the build container, never on the GPU machine:
    python tests/golden/make_database_golden.py
"""
import hashlib
import importlib
import os
import sqlite3
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import ref_shim          # noqa: E402

MAX_BYTES = 600000
N_IMG, N_TRAJ = 27, 300


def load_reference():
    if "tqdm" not in sys.modules:
        try:
            importlib.import_module("tqdm")
        except ImportError:
            m = types.ModuleType("tqdm")
            m.tqdm = lambda it, *a, **k: it
            sys.modules["tqdm"] = m
    sfm = os.path.join(ref_shim.REFERENCE_ROOT, "sfm")
    if not os.path.isdir(sfm):
        raise RuntimeError("reference tree not present at %s" % ref_shim.REFERENCE_ROOT)
    sys.path.insert(0, sfm)
    return importlib.import_module("import_feature_matches")


def random_trajectories(seed):
    """About 300 trajectories over 27 images, lengths 3..27 (more than 20 kept points: the two directions of a pair differ), some
    with a frame gap, about 10 % of the points dynamic."""
    rng = np.random.default_rng(seed)
    trajs = {}
    for key in range(N_TRAJ):
        n = int(rng.integers(3, N_IMG + 1))
        gap = n < N_IMG and rng.random() < 0.3
        span = n + 1 if gap else n
        f0 = int(rng.integers(0, N_IMG - span + 1))
        frames = np.arange(f0, f0 + span)
        if gap:
            frames = np.delete(frames, int(rng.integers(1, span - 1)))
        trajs[3 * key + 1] = {"locations": rng.uniform(-2.0, 1900.0, size=(n, 2)), "labels": (rng.random(n) < 0.1).astype(np.int64),
                              "frame_ids": frames.astype(np.int64)}
    return trajs


def every_image_has_a_static_point(trajs, n_img):
    seen = np.zeros(n_img, bool)
    for t in trajs.values():
        seen[np.asarray(t["frame_ids"])[np.asarray(t["labels"]) == 0]] = True
    return bool(seen.all())


def hand_case():
    """4 images, 5 trajectories.  T0 has 21 kept points (frames repeat: a dict whose frame ids are not ascending), so its last point,
    the only one in image 3 besides T3's, is a source and never a target: pairs (3,0) and (3,1) exist in one direction only, and
    image 3 comes last in the iteration order.  Its repeated frames also give self pairs."""
    loc = lambda n, a: np.stack([a + 0.25 * np.arange(n), 100.0 - a - 0.5 * np.arange(n)], 1)
    trajs = {
        10: {"locations": loc(21, 1.0), "labels": np.zeros(21, np.int64), "frame_ids": np.array([0, 1, 2] * 6 + [0, 1, 3], np.int64)},
        4: {"locations": loc(2, 30.5), "labels": np.zeros(2, np.int64), "frame_ids": np.array([1, 0], np.int64)},
        7: {"locations": loc(3, 40.0), "labels": np.array([0, 1, 0], np.int64), "frame_ids": np.array([0, 2, 1], np.int64)},
        2: {"locations": loc(2, 55.5), "labels": np.zeros(2, np.int64), "frame_ids": np.array([2, 3], np.int64)},
        9: {"locations": loc(3, 60.0), "labels": np.array([0, 1, 0], np.int64), "frame_ids": np.array([1, 3, 2], np.int64)},
    }
    names = ["a0.png", "a1.png", "a2.png", "a3.png"]
    image_ids = {"a1.png": 7, "a0.png": 3, "a2.png": 9, "a3.png": 2}
    return trajs, names, image_ids


def read_table(db, sql):
    return sorted(db.execute(sql).fetchall())


def blobs(rows, col):
    off = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r[col]) for r in rows], out=off[1:])
    return off, np.frombuffer(b"".join(bytes(r[col]) for r in rows), np.uint8)


def run_case(ref, name, trajs, names, image_ids):
    with tempfile.TemporaryDirectory() as tmp:
        img_dir, traj_dir = os.path.join(tmp, "images"), os.path.join(tmp, "traj")
        os.makedirs(img_dir)
        os.makedirs(traj_dir)
        for n in names:
            open(os.path.join(img_dir, n), "w").close()
        assert sorted(os.listdir(img_dir)) == list(names)
        np.save(os.path.join(traj_dir, "track.npy"), trajs, allow_pickle=True)
        db_path, pair_file = os.path.join(tmp, "database.db"), os.path.join(tmp, "pairs.txt")
        ref.create_empty_db(db_path)
        ref.import_keypoints_matches(image_ids, img_dir, db_path, pair_file, traj_dir, skip_geometric_verification=True)
        db = sqlite3.connect(db_path)
        kp = read_table(db, "SELECT image_id, rows, cols, data FROM keypoints")
        mt = read_table(db, "SELECT pair_id, rows, cols, data FROM matches")
        tv = read_table(db, "SELECT pair_id, rows, cols, data, config, F, E, H FROM two_view_geometries")
        db.close()
        pair_hash = hashlib.sha256(open(pair_file).read().encode()).hexdigest()
        n_lines = len(open(pair_file).read().splitlines())
    cnt = [len(t["frame_ids"]) for t in trajs.values()]
    off = np.zeros(len(cnt) + 1, np.int64)
    np.cumsum(cnt, out=off[1:])
    kp_off, kp_data = blobs(kp, 3)
    m_off, m_data = blobs(mt, 3)
    g_off, g_data = blobs(tv, 3)
    col = lambda rows, c, dt=np.int64: np.array([r[c] for r in rows], dt)
    mat = lambda rows, c: np.stack([np.frombuffer(bytes(r[c]), np.uint8) for r in rows]) if rows else np.zeros((0, 72), np.uint8)
    out = dict(
        traj_keys=np.array(list(trajs), np.int64), traj_off=off,
        traj_frames=np.concatenate([np.asarray(t["frame_ids"], np.int64) for t in trajs.values()]),
        traj_xy=np.concatenate([np.asarray(t["locations"], np.float64) for t in trajs.values()]),
        traj_labels=np.concatenate([np.asarray(t["labels"]) for t in trajs.values()]).astype(np.uint8),
        image_names=np.array(list(names)), ids_names=np.array(list(image_ids)), ids_values=np.array(list(image_ids.values()), np.int64),
        kp_image_id=col(kp, 0), kp_rows=col(kp, 1), kp_cols=col(kp, 2), kp_off=kp_off, kp_data=kp_data,
        m_pair_id=col(mt, 0), m_rows=col(mt, 1), m_cols=col(mt, 2), m_off=m_off, m_data=m_data,
        g_pair_id=col(tv, 0), g_rows=col(tv, 1), g_cols=col(tv, 2), g_off=g_off, g_data=g_data, g_config=col(tv, 4),
        g_F=mat(tv, 5), g_E=mat(tv, 6), g_H=mat(tv, 7),
        pair_file_hash=np.array(pair_hash), n_directed_pairs=np.int64(n_lines))
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < MAX_BYTES, (name, size)
    print("%s: %d images, %d trajectories, %d of %d directed pairs kept, %d rows, %d bytes"
          % (name, len(names), len(trajs), len(mt), n_lines, int(col(mt, 1).sum()), size))
    return out


def main():
    ref = load_reference()
    seed = 4100
    while True:
        trajs = random_trajectories(seed)
        if every_image_has_a_static_point(trajs, N_IMG):
            break
        seed += 1
    names = ["%05d.png" % i for i in range(N_IMG)]
    rng = np.random.default_rng(seed + 1)
    ids = (rng.permutation(N_IMG) + 1 + 40).tolist()
    order = rng.permutation(N_IMG).tolist()
    a = run_case(ref, "database_a_permuted", trajs, names, {names[i]: ids[i] for i in order})
    assert int(a["n_directed_pairs"]) > len(a["m_pair_id"]) > 0
    run_case(ref, "database_b_ascending", trajs, names, {names[i]: i + 1 for i in range(N_IMG)})
    run_case(ref, "database_c_descending", trajs, names, {names[i]: N_IMG - i for i in range(N_IMG)})
    t, n, m = hand_case()
    d = run_case(ref, "database_d_hand", t, n, m)
    rows = d["m_rows"].tolist()
    assert 1 in rows and any(r > 1 and r % 2 == 1 for r in rows), rows
    pid = lambda x, y: min(x, y) * (2 ** 31 - 1) + max(x, y)
    assert pid(m["a3.png"], m["a0.png"]) in d["m_pair_id"].tolist() and pid(m["a3.png"], m["a1.png"]) in d["m_pair_id"].tolist()


if __name__ == "__main__":
    main()
