"""The COLMAP database rows without a GPU, against golden vectors that the REFERENCE's own sfm/import_feature_matches.py
(import_keypoints_matches through colmap_utils/database.py, on a database made by its create_empty_db) produced
(tests/golden/make_database_golden.py: both imported unmodified in the build container).

Two statements of the rules are pinned: psfm_sfm.database.database_tables_host (NumPy; the model the GPU tests compare with) to the
fixtures byte for byte, and particle-sfm_amd/csrc/psfm_database.h -- the per-element rules of the kernels -- compiled for the host
through tests/host/shim by tests/host/database_host.cpp with -ffp-contract=off, to the NumPy model on enumerated inputs.  The writer
and the reference-signature importer are pinned to the fixtures through a database whose tables the tests create themselves."""
import ctypes
import hashlib
import os
import subprocess

import numpy as np
import pytest

from _database_np import (CASES, EYE, MAX_IMAGE_ID, assert_database_equals_fixture, assert_tables_equal_fixture, create_tables, fixture,
                          ids_pos, match_tables, read_tables)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("database") / "libdatabase_host.so")
    cmd = ["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "tests", "host", "shim"),
           "-I", os.path.join(ROOT, "particle-sfm_amd", "csrc"), os.path.join(ROOT, "tests", "host", "database_host.cpp"), "-o", out]
    subprocess.run(cmd, check=True)
    L = ctypes.CDLL(out)
    vp = ctypes.c_void_p
    L.psfm_host_db_keypoints.argtypes = [vp, ctypes.c_long, vp]
    L.psfm_host_db_keypoints.restype = None
    L.psfm_host_db_keep.argtypes = [vp, ctypes.c_long, ctypes.c_long, vp, vp]
    L.psfm_host_db_keep.restype = None
    L.psfm_host_db_rows.argtypes = [vp, vp, vp, ctypes.c_long, vp, vp]
    L.psfm_host_db_rows.restype = None
    return L


@pytest.fixture(scope="module")
def fixtures():
    return {name: fixture(name) for name in CASES}


def model_tables(f, remove_dynamic=True):
    from psfm_sfm.database import database_tables_host
    db_id, db_pos = ids_pos(f)
    return database_tables_host(match_tables(f, remove_dynamic), db_id, db_pos)


# ---- the NumPy model against the reference ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CASES)
def test_numpy_model_equals_reference_fixture(fixtures, name):
    assert_tables_equal_fixture(model_tables(fixtures[name]), fixtures[name])


def test_fixtures_hold_the_edges_they_are_there_for(fixtures):
    a, b, c, d = (fixtures[n] for n in CASES)
    for f in (a, b, c):
        assert len(f["matches"]) < f["n_directed"]                       # the reference drops directed pairs
        assert max(len(t["frame_ids"]) for t in f["trajs"].values()) > 20   # ... whose two directions differ
        assert any(np.any(np.diff(t["frame_ids"]) > 1) for t in f["trajs"].values())
        assert 0 < np.mean(f["labels"]) < 0.2
    assert list(a["image_ids"]) != sorted(a["image_ids"]) and list(a["image_ids"].values()) != sorted(a["image_ids"].values())
    assert list(b["image_ids"]) == b["names"] and list(b["image_ids"].values()) == sorted(b["image_ids"].values())
    assert list(c["image_ids"].values()) == sorted(c["image_ids"].values(), reverse=True)
    # ascending and descending ids write the same pairs with the columns exchanged
    pid = lambda x, y: min(x, y) * MAX_IMAGE_ID + max(x, y)
    n = len(b["names"])
    for i in range(n):
        for j in range(i + 1, n):
            pb, pc = pid(i + 1, j + 1), pid(n - i, n - j)
            assert (pb in b["matches"]) == (pc in c["matches"])
            if pb in b["matches"]:
                rb = np.frombuffer(b["matches"][pb][2], np.uint32).reshape(-1, 2)
                rc = np.frombuffer(c["matches"][pc][2], np.uint32).reshape(-1, 2)
                assert np.array_equal(rb, rc[:, ::-1])
    rows = [r[0] for r in d["matches"].values()]
    assert 1 in rows and any(r > 1 and r % 2 for r in rows)
    assert any(np.any(np.diff(t["frame_ids"]) < 0) for t in d["trajs"].values())
    ids = d["image_ids"]
    assert list(ids)[-1] == "a3.png"                                     # the one-directional pairs' source comes last
    for other in ("a0.png", "a1.png"):
        assert pid(ids["a3.png"], ids[other]) in d["matches"]
    assert pid(ids["a0.png"], ids["a0.png"]) in d["matches"]             # a self pair
    for f in (a, b, c, d):
        for p, g in f["geometries"].items():
            assert g[:3] == f["matches"][p] and g[3:] == (2, EYE, EYE, EYE)
        assert set(f["geometries"]) == set(f["matches"])


def test_model_refuses_bad_ids_and_positions(fixtures):
    from psfm_sfm.database import database_tables_host
    f = fixtures[CASES[3]]
    t = match_tables(f)
    ok_id, ok_pos = np.array([3, 7, 9, 2]), np.array([1, 0, 2, 3])
    database_tables_host(t, ok_id, ok_pos)
    for ids, pos in (([3, 7, 7, 2], ok_pos), ([0, 7, 9, 2], ok_pos), ([3, 7, 9, 2 ** 31 - 1], ok_pos), (ok_id, [0, 0, 2, 3]),
                     (ok_id, [1, 2, 3, 4]), (ok_id[:3], ok_pos[:3])):
        with pytest.raises(ValueError):
            database_tables_host(t, np.array(ids), np.array(pos))
    database_tables_host(t, np.array([1, 2 ** 31 - 2, 9, 2]), ok_pos)


# ---- the header against the NumPy model ------------------------------------------------------------------------------------------

def test_header_keypoints_round_once_from_f64(host):
    f = np.array([1.0, 3.5, 1000.25, 1919.5, 0.5, 16777216.0, 123456.0, -7.75, -1000.5, 1e-3], np.float32)
    up = np.nextafter(f, np.float32(np.inf))
    half = (f.astype(np.float64) + up.astype(np.float64)) / 2          # exactly halfway between two floats
    x = half - 0.5
    assert np.array_equal(x + 0.5, half)                                # (representable: the tie really reaches the rounding)
    rng = np.random.default_rng(3)
    v = np.concatenate([x, np.nextafter(x, np.inf), np.nextafter(x, -np.inf), [-0.5, 0.0, -1e-300, 1e300, -1e300, 3e38, 3.4028235e38, 1e39],
                        rng.uniform(-4000, 4000, 5000), rng.uniform(-1e9, 1e9, 1000)])
    with np.errstate(over="ignore"):
        want = (v + 0.5).astype(np.float32)
        assert not np.array_equal(want, v.astype(np.float32) + np.float32(0.5))  # an f32 add of the rounded value differs
    got = np.full(len(v), np.nan, np.float32)
    host.psfm_host_db_keypoints(v.ctypes.data, len(v), got.ctypes.data)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    ties = (x + 0.5).astype(np.float32)
    assert np.all((ties == f) | (ties == up)) and np.all(ties.view(np.uint32) % 2 == 0)   # ties went to the even neighbour


def test_header_pair_id_and_swap(host):
    from psfm_sfm.database import database_tables_host
    big = 2 ** 31 - 2
    id_s = np.array([1, big, 1, big, big - 1, big, 5, 9, 7], np.int32)
    id_t = np.array([big, 1, 1, big, big, big - 1, 9, 5, 7], np.int32)
    rows = (np.arange(2 * len(id_s), dtype=np.int64) * 1000003 % (2 ** 31 - 1)).astype(np.int32).reshape(-1, 2)
    pid = np.zeros(len(id_s), np.int64)
    out = np.zeros((len(id_s), 2), np.uint32)
    host.psfm_host_db_rows(id_s.ctypes.data, id_t.ctypes.data, rows.ctypes.data, len(id_s), pid.ctypes.data, out.ctypes.data)
    want = [min(int(a), int(b)) * MAX_IMAGE_ID + max(int(a), int(b)) for a, b in zip(id_s, id_t)]       # Python integers: no overflow
    assert pid.tolist() == want and want[3] == big * MAX_IMAGE_ID + big > 2 ** 61
    for i in range(len(id_s)):
        assert out[i].tolist() == (rows[i, ::-1] if id_s[i] > id_t[i] else rows[i]).tolist()
    # the NumPy model on a two-image table with the same ids: pair (0,1) only
    for a, b in zip(id_s.tolist(), id_t.tolist()):
        if a == b:
            continue
        tables = (np.array([0, 1, 2]), np.zeros((2, 2)), np.array([1]), np.array([0, 1]), np.array([0]), np.array([[4, 6]], np.int32))
        t = database_tables_host(tables, np.array([a, b]), np.array([0, 1]))
        assert t.pair_id.tolist() == [min(a, b) * MAX_IMAGE_ID + max(a, b)] and t.rows.tolist() == ([[6, 4]] if a > b else [[4, 6]])


@pytest.mark.parametrize("pos", [[0, 1, 2, 3], [3, 2, 1, 0], [1, 0, 3, 2], [2, 3, 0, 1]])
def test_header_keep_predicate_equals_model(host, pos):
    """(0,1) and (1,0) both exist, (0,2) and (3,1) exist alone, (2,2) is a self pair, (2,3) and (3,2) both exist: over the four orders
    every combination of "reverse exists" x "reverse's source comes earlier" occurs."""
    from psfm_sfm.database import database_tables_host
    n_img = 4
    pairs = sorted([(0, 1), (1, 0), (0, 2), (3, 1), (2, 2), (2, 3), (3, 2)])
    key = np.array([s * n_img + t for s, t in pairs], np.int64)
    posa = np.array(pos, np.int32)
    keep = np.full(len(key), 9, np.uint8)
    host.psfm_host_db_keep(key.ctypes.data, len(key), n_img, posa.ctypes.data, keep.ctypes.data)
    want = [not ((t, s) in pairs and pos[t] < pos[s]) for s, t in pairs]
    assert keep.astype(bool).tolist() == want
    assert want[pairs.index((2, 2))] and want[pairs.index((0, 2))] and want[pairs.index((3, 1))]
    assert want[pairs.index((0, 1))] != want[pairs.index((1, 0))]
    tables = (np.zeros(n_img + 1, np.int64), np.zeros((0, 2)), key, np.arange(len(key) + 1), np.arange(len(key)),
              np.arange(2 * len(key), dtype=np.int32).reshape(-1, 2))
    t = database_tables_host(tables, np.array([5, 6, 7, 8]), posa)
    assert t.pair_key.tolist() == key[np.array(want)].tolist()


def test_header_keep_on_the_fixture_tables(host, fixtures):
    from psfm_sfm.database import database_tables_host
    for name in CASES:
        f = fixtures[name]
        db_id, db_pos = ids_pos(f)
        tables = match_tables(f)
        key = np.ascontiguousarray(tables[2], np.int64)
        keep = np.zeros(len(key), np.uint8)
        host.psfm_host_db_keep(key.ctypes.data, len(key), len(f["names"]), np.ascontiguousarray(db_pos, np.int32).ctypes.data, keep.ctypes.data)
        assert key[keep.astype(bool)].tolist() == database_tables_host(tables, db_id, db_pos).pair_key.tolist()
        assert len(key) == f["n_directed"]


# ---- the writer ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CASES)
def test_write_database_equals_reference_fixture(fixtures, name, tmp_path):
    from psfm_sfm.database import write_database
    f = fixtures[name]
    t = model_tables(f)
    path = tmp_path / "with_geometry.db"
    create_tables(path)
    write_database(path, f["image_ids"], f["names"], t, skip_geometric_verification=True)
    assert_database_equals_fixture(path, f)
    path = tmp_path / "without_geometry.db"
    create_tables(path)
    write_database(path, f["image_ids"], f["names"], t)
    assert_database_equals_fixture(path, f, geometries=False)


def test_an_image_without_keypoints_gets_an_empty_row(fixtures, tmp_path):
    """Deviation: the reference fails its own assert on np.array([]) here."""
    from psfm_sfm import matches_from_flow as mff
    from psfm_sfm.database import database_tables_host, write_database
    f = fixtures[CASES[3]]
    names = ["a0.png", "a1.png", "a1b.png", "a2.png", "a3.png"]           # frame index 2 is now an image nobody observes
    frames = np.where(f["frames"] >= 2, f["frames"] + 1, f["frames"])
    image_ids = {"a1.png": 7, "a1b.png": 11, "a0.png": 3, "a2.png": 9, "a3.png": 2}
    from psfm_sfm.database import ids_and_positions
    db_id, db_pos = ids_and_positions(image_ids, names)
    t = database_tables_host(mff.match_tables_host(f["off"], frames, f["xy"], f["labels"].astype(bool), 5), db_id, db_pos)
    path = tmp_path / "d.db"
    create_tables(path)
    write_database(path, image_ids, names, t, skip_geometric_verification=True)
    kp, mt, tv = read_tables(path)
    assert kp[11] == (0, 2, b"")
    del kp[11]
    assert kp == f["keypoints"] and mt == f["matches"] and tv == f["geometries"]     # the rest is the fixture's


def test_image_ids_must_name_exactly_the_images(fixtures, tmp_path):
    from psfm_sfm.database import write_database
    f = fixtures[CASES[3]]
    t = model_tables(f)
    path = tmp_path / "d.db"
    create_tables(path)
    ids = dict(f["image_ids"])
    for bad in ({k: v for k, v in ids.items() if k != "a0.png"}, dict(ids, extra=99), {("x" + k if k == "a2.png" else k): v for k, v in ids.items()}):
        with pytest.raises(ValueError):
            write_database(path, bad, f["names"], t)
    assert read_tables(path) == ({}, {}, {})                             # nothing was written
    write_database(path, ids, f["names"], t)


# ---- the reference's signature ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CASES)
def test_import_keypoints_matches_on_a_track_npy(fixtures, name, tmp_path):
    from psfm_sfm.database import import_keypoints_matches
    f = fixtures[name]
    img_dir, traj_dir = tmp_path / "images", tmp_path / "traj"
    img_dir.mkdir()
    traj_dir.mkdir()
    for n in f["names"]:
        (img_dir / n).touch()
    np.save(str(traj_dir / "track.npy"), f["trajs"], allow_pickle=True)
    path = tmp_path / "database.db"
    create_tables(path)
    import_keypoints_matches(f["image_ids"], str(img_dir), str(path), str(tmp_path / "pairs.txt"), str(traj_dir), skip_geometric_verification=True)
    assert_database_equals_fixture(path, f)
    assert hashlib.sha256(open(str(tmp_path / "pairs.txt")).read().encode()).hexdigest() == f["pair_file_hash"]


def test_pair_file_equals_assembles(fixtures, tmp_path):
    from psfm_sfm import matches_from_flow as mff
    from psfm_sfm.database import write_pair_file
    for name in CASES:
        f = fixtures[name]
        tables = match_tables(f)
        mff.assemble(f["names"], tables, str(tmp_path / "a.txt"), as_arrays=True)
        write_pair_file(str(tmp_path / "b.txt"), f["names"], tables[2], tables[4])
        assert open(str(tmp_path / "a.txt")).read() == open(str(tmp_path / "b.txt")).read()
        assert hashlib.sha256(open(str(tmp_path / "b.txt")).read().encode()).hexdigest() == f["pair_file_hash"]
