"""The sparse depth maps, poses and intrinsics of a COLMAP model without a GPU, against golden vectors that the REFERENCE's own
sfm/convert.py (write_depth_pose_from_colmap_format on models written by its write_model) produced
(tests/golden/make_sparse_depth_golden.py: both imported unmodified in the build container).

Three statements of the rules are pinned: psfm_sfm.convert.sparse_depth_host (NumPy; the model the GPU tests compare with) to the
fixtures within the derived bound (tests/_sparse_depth_np.py), particle-sfm_amd/csrc/psfm_sparse_depth.h -- the per-element rules of
the kernels -- compiled for the host through tests/host/shim by tests/host/sparse_depth_host.cpp with -ffp-contract=off, to the NumPy
model bit for bit, and the reader (read_model_arrays, with the library's bounds-checked walk over points3D.bin) to the arrays the
fixtures were written from.

Truncated points3D.bin: the file announces its record count, so a buffer cut at ANY byte offset -- record boundaries included -- is
refused; there is no count-less form that would accept a prefix of the records."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

from _sparse_depth_np import CASES, assert_map_accepts, case_dir, fixture, winners

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("sparse_depth") / "libsparse_depth_host.so")
    cmd = ["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "tests", "host", "shim"),
           "-I", os.path.join(ROOT, "particle-sfm_amd", "csrc"), os.path.join(ROOT, "tests", "host", "sparse_depth_host.cpp"), "-o", out]
    subprocess.run(cmd, check=True)
    L = ctypes.CDLL(out)
    vp = ctypes.c_void_p
    L.psfm_host_sd_pixels.argtypes = [vp, ctypes.c_long, ctypes.c_int, vp, vp]
    L.psfm_host_sd_pixels.restype = None
    L.psfm_host_sd_maps.argtypes = [vp, vp, vp, ctypes.c_int, vp, vp, vp, ctypes.c_int64, vp, vp, ctypes.POINTER(ctypes.c_int64)]
    L.psfm_host_sd_maps.restype = ctypes.c_int
    L.psfm_host_sd_points3d.argtypes = [vp, ctypes.c_ulong, ctypes.POINTER(ctypes.c_uint64), vp, vp, vp, vp]
    L.psfm_host_sd_points3d.restype = ctypes.c_long
    return L


@pytest.fixture(scope="module")
def models():
    from psfm_sfm.convert import read_model_arrays
    return {c: read_model_arrays(case_dir(c)) for c in CASES + ["f"]}


def header_maps(host, model):
    """The header's two passes over the whole model -> ([map per image], status, missing id)."""
    from psfm_sfm.convert import image_descriptors
    desc = image_descriptors(model)
    order = np.argsort(model.ids, kind="stable")
    srt, row = np.ascontiguousarray(model.ids[order]), order.astype(np.int32)
    n_pix = int((desc["w"].astype(np.int64) * desc["h"]).sum())
    winner, depth = np.full(n_pix, 7, np.uint32), np.full(n_pix, np.nan)
    missing = ctypes.c_int64(-1)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    st = host.psfm_host_sd_maps(p(model.xys), p(model.point3D_ids), p(desc), len(desc), p(srt), p(row), p(np.ascontiguousarray(model.xyz)),
                                len(srt), p(winner), p(depth), ctypes.byref(missing))
    maps = [depth[int(d["out_off"]):int(d["out_off"]) + int(d["w"]) * int(d["h"])].reshape(int(d["h"]), int(d["w"])) for d in desc]
    return maps, st, int(missing.value)


# ---- the reader ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES + ["f"])
def test_read_model_arrays_equals_what_the_fixture_was_written_from(models, case):
    m, f = models[case], fixture(case)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)
    assert m.ids.dtype == np.int64 and np.array_equal(m.ids.view(np.uint64), f["ids"])
    assert np.array_equal(bits(m.xyz), bits(f["xyz"])) and m.xyz.shape == (len(f["ids"]), 3)
    assert np.array_equal(bits(m.xys), bits(f["xys"])) and np.array_equal(m.point3D_ids, f["point3D_ids"])
    assert np.array_equal(m.obs_off, f["obs_off"])
    assert [im.id for im in m.images] == f["image_ids"].tolist() and [im.name for im in m.images] == f["names"].tolist()
    assert [im.camera_id for im in m.images] == f["camera_ids"].tolist()
    assert np.array_equal(bits(np.stack([im.qvec for im in m.images])), bits(f["qvecs"]))
    assert np.array_equal(bits(np.stack([im.tvec for im in m.images])), bits(f["tvecs"]))
    assert list(m.cameras) == f["cam_ids"].tolist()
    assert [c.model for c in m.cameras.values()] == f["cam_models"].tolist()
    assert [[c.width, c.height] for c in m.cameras.values()] == f["cam_wh"].tolist()
    assert np.array_equal(bits(np.concatenate([c.params for c in m.cameras.values()])), bits(f["cam_params"]))


def test_scan_returns_errors_and_track_lengths(host):
    f = fixture("a")
    buf = np.fromfile(os.path.join(case_dir("a"), "points3D.bin"), np.uint8)
    n = ctypes.c_uint64(0)
    ids, xyz, err, tl = np.zeros(500, np.uint64), np.zeros((500, 3)), np.zeros(500), np.zeros(500, np.uint64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert host.psfm_host_sd_points3d(p(buf), buf.size, ctypes.byref(n), p(ids), p(xyz), p(err), p(tl)) == -1 and n.value == 500
    assert np.array_equal(ids, f["ids"]) and np.array_equal(xyz, f["xyz"]) and np.array_equal(err, f["errors"])
    assert np.array_equal(tl, f["track_len"]) and len(set(tl.tolist())) > 3          # records of different lengths


def three_records():
    rec = lambda i, xyz, n: struct.pack("<QdddBBBdQ", i, *xyz, 1, 2, 3, 0.5, n) + b"".join(struct.pack("<ii", k, k + 1) for k in range(n))
    return struct.pack("<Q", 3) + rec(11, (1.0, 2.0, 3.0), 2) + rec(2 ** 40, (4.0, 5.0, 6.0), 0) + rec(7, (7.0, 8.0, 9.0), 3)


def test_scan_refuses_a_file_cut_at_every_byte(host):
    whole = three_records()
    assert len(whole) == 8 + 3 * 51 + 8 * 5
    n = ctypes.c_uint64(9)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    starts = [8, 8 + 51 + 16, 8 + 51 + 16 + 51, len(whole)]               # where records 0, 1, 2 begin, and the end
    for cut in range(len(whole)):
        buf = np.frombuffer(whole[:cut], np.uint8).copy() if cut else np.zeros(0, np.uint8)      # exactly `cut` bytes are owned
        ids, xyz = np.full(3, 99, np.uint64), np.full((3, 3), -1.0)
        bad = host.psfm_host_sd_points3d(p(buf) if cut else None, cut, ctypes.byref(n), p(ids), p(xyz), None, None)
        # the count announces three records, 153 bytes at least: shorter buffers are refused before record 0; longer ones at the
        # record whose bytes are cut
        want = 0 if cut < 8 + 3 * 51 else max(k for k in range(3) if starts[k] <= cut)
        assert bad == want and n.value == 0, (cut, bad, want)
        assert np.all(ids == 99) and np.all(xyz == -1.0)                  # nothing was written
    buf = np.frombuffer(whole, np.uint8).copy()
    ids, xyz = np.zeros(3, np.uint64), np.zeros((3, 3))
    assert host.psfm_host_sd_points3d(p(buf), buf.size, ctypes.byref(n), p(ids), p(xyz), None, None) == -1 and n.value == 3
    assert ids.tolist() == [11, 2 ** 40, 7] and xyz.reshape(-1).tolist() == [float(v) for v in range(1, 10)]
    # trailing bytes, a count that is too large, a track length that wraps 8 * L
    buf = np.frombuffer(whole + b"\x00", np.uint8).copy()
    assert host.psfm_host_sd_points3d(p(buf), buf.size, ctypes.byref(n), None, None, None, None) == 3
    for count in (4, 2 ** 61, 2 ** 64 - 1):
        buf = np.frombuffer(struct.pack("<Q", count) + whole[8:], np.uint8).copy()
        assert host.psfm_host_sd_points3d(p(buf), buf.size, ctypes.byref(n), None, None, None, None) >= 0
    for length in (2 ** 61, 2 ** 61 + 2, 2 ** 64 - 1, 6):
        b = bytearray(whole)
        b[8 + 43:8 + 51] = struct.pack("<Q", length)
        buf = np.frombuffer(bytes(b), np.uint8).copy()
        assert host.psfm_host_sd_points3d(p(buf), buf.size, ctypes.byref(n), None, None, None, None) >= 0
    # fewer records announced than the file holds: bytes trail
    buf = np.frombuffer(struct.pack("<Q", 2) + whole[8:], np.uint8).copy()
    assert host.psfm_host_sd_points3d(p(buf), buf.size, ctypes.byref(n), None, None, None, None) == 2


def test_library_entries_refuse_a_file_cut_at_every_byte():
    """psfm_colmap_points3d_count / _scan of the library itself (host code: no GPU is initialised): PSFM_ERR_ARG at every cut, the
    record index in psfm_last_error(), the outputs untouched."""
    from point_trajectory import _hip
    L = _hip.lib()
    whole = three_records()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    n = ctypes.c_uint64(9)
    for cut in range(len(whole)):
        buf = np.frombuffer(whole[:cut], np.uint8).copy() if cut else np.zeros(0, np.uint8)
        ids, xyz, err, tl = np.full(3, 99, np.uint64), np.full((3, 3), -1.0), np.full(3, -1.0), np.full(3, 99, np.uint64)
        assert L.psfm_colmap_points3d_count(p(buf) if cut else None, cut, ctypes.byref(n)) == _hip.PSFM_ERR_ARG and n.value == 0
        assert L.psfm_colmap_points3d_scan(p(buf) if cut else None, cut, p(ids), p(xyz), p(err), p(tl)) == _hip.PSFM_ERR_ARG
        want = 0 if cut < 8 + 3 * 51 else (1 if cut < 126 else 2)
        assert ("at record %d " % want).encode() in L.psfm_last_error()
        assert np.all(ids == 99) and np.all(xyz == -1.0) and np.all(err == -1.0) and np.all(tl == 99)
    buf = np.frombuffer(whole, np.uint8).copy()
    ids, xyz, err, tl = np.zeros(3, np.uint64), np.zeros((3, 3)), np.zeros(3), np.zeros(3, np.uint64)
    assert L.psfm_colmap_points3d_count(p(buf), buf.size, ctypes.byref(n)) == _hip.PSFM_OK and n.value == 3
    assert L.psfm_colmap_points3d_scan(p(buf), buf.size, p(ids), p(xyz), p(err), p(tl)) == _hip.PSFM_OK
    assert ids.tolist() == [11, 2 ** 40, 7] and tl.tolist() == [2, 0, 3] and err.tolist() == [0.5] * 3
    assert L.psfm_colmap_points3d_count(p(buf), buf.size, None) == _hip.PSFM_ERR_ARG


def test_reader_refuses_truncated_files(tmp_path):
    from psfm_sfm.convert import read_model_arrays
    src = case_dir("d")
    for name, cuts in (("points3D.bin", (0, 7, 100, -1)), ("images.bin", (0, 7, 30, 80, -1)), ("cameras.bin", (0, 20, 40))):
        for cut in cuts:
            d = tmp_path / ("%s_%d" % (name, cut))
            d.mkdir()
            for n in ("cameras.bin", "images.bin", "points3D.bin"):
                data = open(os.path.join(src, n), "rb").read()
                (d / n).write_bytes(data[:cut] if n == name else data)
            with pytest.raises(ValueError):
                read_model_arrays(str(d))
    with pytest.raises(FileNotFoundError):
        read_model_arrays(str(tmp_path))
    t = tmp_path / "text"
    t.mkdir()
    for n in ("cameras.txt", "images.txt", "points3D.txt"):
        (t / n).write_text("# empty\n")
    with pytest.raises(NotImplementedError):
        read_model_arrays(str(t))


# ---- the NumPy model against the reference ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES)
def test_numpy_model_accepts_reference_fixture(models, case):
    from psfm_sfm.convert import sparse_depth_host
    f = fixture(case)
    got = list(sparse_depth_host(models[case]))
    assert [n for n, _ in got] == f["names"].tolist()
    for i, (_, depth) in enumerate(got):
        assert_map_accepts(depth, f, i)


def test_fixtures_hold_the_edges_they_are_there_for():
    a, b, c, d, e = (fixture(x) for x in CASES)
    assert a["cam_models"].tolist() == ["SIMPLE_PINHOLE", "SIMPLE_RADIAL"] and a["cam_wh"].tolist() == [[37, 23], [5, 4]]
    assert a["depth_0"].shape == (23, 37) and a["depth_3"].shape == (4, 5) and a["camera_ids"].tolist() == [1, 1, 1, 2]
    assert 0.25 < np.mean(a["point3D_ids"] == -1) < 0.35 and int(a["ids"].max()) == 2 ** 20
    assert a["ids"].tolist() != sorted(a["ids"].tolist())
    # duplicates everywhere, and the observations of one pixel differ by far more than the bound: the bound pins the winner
    from psfm_sfm.convert import qvec2rotmat
    for f, i in ((a, 0), (b, 0)):
        win, mag = winners(f, i)
        o0 = int(f["obs_off"][i])
        valid = np.flatnonzero(f["point3D_ids"][o0:int(f["obs_off"][i + 1])] != -1)
        assert len(valid) > 2 * np.count_nonzero(win >= 0)
        per_point = f["xyz"] @ qvec2rotmat(f["qvecs"][i])[2] + f["tvecs"][i][2]     # the depth any observation of a point would store
        assert np.all(np.diff(np.sort(per_point)) > 1e-9) and 4 * 2.0 ** -53 * mag.max() < 1e-13
    assert np.count_nonzero(b["depth_0"]) == 3 and int(b["obs_off"][1]) == 3000 and not np.any(b["point3D_ids"] == -1)
    x = c["xys"][:, 0]
    frac = x - np.floor(x)
    on_half = x[(frac == 0.5) & (np.abs(x) < 100)]
    assert np.any(np.floor(on_half) % 2 == 0) and np.any(np.floor(on_half) % 2 == 1) and np.any(on_half < 0)
    assert 36.5 in x and np.any(x > 37) and 2147483647.0 in x and -2147483647.5 in x
    assert d["png_failed"].tolist() == ["d1.png", "d2.png"] and not d["depth_1"].any() and not d["depth_2"].any()
    assert int(d["obs_off"][3] - d["obs_off"][2]) == 0 and np.all(d["point3D_ids"][int(d["obs_off"][1]):int(d["obs_off"][2])] == -1)
    assert np.count_nonzero(e["ids"] >= 2 ** 32) > 40 and int(e["ids"].max()) == 2 ** 63 - 1 and np.count_nonzero(e["ids"] > 2 ** 61) > 40
    assert int(fixture("f")["missing_id"]) == 4242 and 4242 not in fixture("f")["ids"]


def test_model_raises_the_reference_key_error(models):
    from psfm_sfm.convert import sparse_depth_host
    with pytest.raises(KeyError) as e:
        list(sparse_depth_host(models["f"]))
    assert e.value.args == (4242,)


def test_model_refuses_coordinates_outside_the_domain(models):
    from psfm_sfm.convert import sparse_depth_host
    m = models["d"]
    for bad in (np.nan, np.inf, -np.inf, 2.0 ** 31, -2.0 ** 31, 2147483647.5, 1e300):
        xys = m.xys.copy()
        xys[3, 1] = bad
        with pytest.raises(ValueError):
            list(sparse_depth_host(m._replace(xys=xys)))
    xys = m.xys.copy()
    xys[int(m.obs_off[1]) + 2, 0] = np.nan                                 # an observation with id -1 is never rounded
    xys[3, 0], xys[4, 1] = 2147483647.0, -2147483647.5
    list(sparse_depth_host(m._replace(xys=xys)))


def test_other_camera_models_are_not_implemented(models):
    from psfm_sfm.convert import Camera, sparse_depth_host
    m = models["d"]
    cams = dict(m.cameras)
    cams[1] = Camera(1, "PINHOLE", 37, 23, np.array([30.0, 30.0, 18.5, 11.5]))
    with pytest.raises(NotImplementedError):
        list(sparse_depth_host(m._replace(cameras=cams)))


# ---- the header against the NumPy model ------------------------------------------------------------------------------------------

def test_header_pixels_round_half_to_even_and_clip(host):
    from psfm_sfm.convert import coord_ok, pixels
    rng = np.random.default_rng(5)
    v = np.concatenate([[0.5, 1.5, 2.5, 3.5, -0.5, -1.5, -0.0, 0.0, 35.5, 36.5, 37.0, 1e6, -1e6, 2147483647.0, 2147483647.49, 2147483647.5,
                         2147483648.0, -2147483647.5, -2147483648.0, -2147483649.0, np.nan, np.inf, -np.inf, 1e300, -1e300,
                         0.49999999999999994, 1.5000000000000002], rng.uniform(-5, 45, 4000), np.arange(-3, 41) + 0.5])
    pix, ok = np.full(len(v), -7, np.int32), np.full(len(v), 9, np.uint8)
    host.psfm_host_sd_pixels(v.ctypes.data, len(v), 37, pix.ctypes.data, ok.ctypes.data)
    want_ok = coord_ok(v)
    assert ok.astype(bool).tolist() == want_ok.tolist()
    assert want_ok[:15].tolist() == [True] * 15 and want_ok[15:27].tolist() == [False, False, True, False, False] + [False] * 5 + [True, True]
    assert np.array_equal(pix[want_ok], pixels(v[want_ok], 37))
    assert pix[:13].tolist() == [0, 2, 2, 4, 0, 0, 0, 0, 36, 36, 36, 36, 0]
    # inside the int32 range the rule is the reference's expression literally
    small = v[want_ok & (np.abs(v) < 2e9)]
    assert np.array_equal(pixels(small, 37), np.clip(np.round(small).astype(np.int32), 0, 36))


@pytest.mark.parametrize("case", CASES)
def test_header_equals_numpy_model_bit_for_bit(host, models, case):
    from psfm_sfm.convert import sparse_depth_host
    maps, st, _ = header_maps(host, models[case])
    assert st == 0
    for got, (_, want) in zip(maps, sparse_depth_host(models[case])):
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


def test_header_reports_the_smallest_missing_id(host, models):
    m = models["f"]
    _, st, missing = header_maps(host, m)
    assert (st, missing) == (1, 4242)
    p3d = m.point3D_ids.copy()
    p3d[7], p3d[60] = 9000, -5
    assert header_maps(host, m._replace(point3D_ids=p3d))[1:] == (1, -5)


def test_equal_ids_resolve_to_the_last_point_in_file_order(host, models):
    """What a dict built in file order holds for an id that occurs twice."""
    from psfm_sfm.convert import sparse_depth_host
    m = models["d"]
    ids = m.ids.copy()
    ids[20] = ids[3]                                                       # rows 3 and 20 share an id: row 20 is the one a dict keeps
    p3d = np.where(m.point3D_ids == m.ids[20], -1, m.point3D_ids)
    m2 = m._replace(ids=ids, point3D_ids=p3d)
    xyz = m.xyz.copy()
    xyz[3] = 1e6                                                           # never used
    m3 = m2._replace(xyz=xyz)
    for (_, x), (_, y) in zip(sparse_depth_host(m2), sparse_depth_host(m3)):
        assert np.array_equal(x, y)
    assert np.any(m2.point3D_ids == ids[3])
    for x, (_, y) in zip(header_maps(host, m3)[0], sparse_depth_host(m3)):
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64))


# ---- the files -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES)
def test_pose_and_intrinsics_files_equal_the_reference_text(case, tmp_path):
    from psfm_sfm.convert import write_depth_pose_from_colmap_format
    f = fixture(case)
    os.environ.setdefault("MPLBACKEND", "Agg")
    write_depth_pose_from_colmap_format(case_dir(case), str(tmp_path), device=False)
    for i, name in enumerate(f["names"].tolist()):
        stem = os.path.splitext(name)[0]
        assert open(str(tmp_path / "poses" / (stem + ".txt"))).read() == str(f["pose_%d" % i])
        assert open(str(tmp_path / "intrinsics" / (stem + ".txt"))).read() == str(f["intr_%d" % i])
        assert_map_accepts(np.load(str(tmp_path / "depths" / (stem + ".npy"))), f, i)
        assert os.path.exists(str(tmp_path / "depths" / (stem + ".png"))) == (name not in f["png_failed"].tolist())


def test_png_is_within_one_grey_level_of_the_reference(tmp_path):
    from matplotlib import pyplot as plt
    from psfm_sfm.convert import write_depth_pose_from_colmap_format
    os.environ.setdefault("MPLBACKEND", "Agg")
    write_depth_pose_from_colmap_format(case_dir("a"), str(tmp_path), device=False)
    got = plt.imread(str(tmp_path / "depths" / "00000.png"))
    want = plt.imread(os.path.join(case_dir("a"), "expected_00000.png"))
    assert got.shape == want.shape
    assert np.max(np.abs(np.round(got * 255) - np.round(want * 255))) <= 1


def test_save_depth_pose_takes_the_reference_dicts(models, tmp_path):
    """The reference's signature: dicts of objects with its attributes."""
    import collections
    from psfm_sfm.convert import save_depth_pose
    m, f = models["d"], fixture("d")
    Im = collections.namedtuple("Im", ["id", "qvec", "tvec", "camera_id", "name", "xys", "point3D_ids"])
    Pt = collections.namedtuple("Pt", ["id", "xyz"])
    images = {im.id: Im(im.id, im.qvec, im.tvec, im.camera_id, im.name, m.xys[a:b], m.point3D_ids[a:b])
              for im, a, b in zip(m.images, m.obs_off[:-1], m.obs_off[1:])}
    points = {int(i): Pt(int(i), x) for i, x in zip(m.ids, m.xyz)}
    os.environ.setdefault("MPLBACKEND", "Agg")
    save_depth_pose(str(tmp_path), m.cameras, images, points, device=False)
    for i, name in enumerate(f["names"].tolist()):
        stem = os.path.splitext(name)[0]
        assert_map_accepts(np.load(str(tmp_path / "depths" / (stem + ".npy"))), f, i)
        assert open(str(tmp_path / "poses" / (stem + ".txt"))).read() == str(f["pose_%d" % i])


@pytest.mark.parametrize("case", ["a", "c"])
def test_restated_reference_of_the_benchmark_equals_the_fixtures(case, tmp_path):
    """scripts/micro/sparse_depth_restated.py, the yardstick of scripts/micro/sparse_depth.py: the reference's operations on the
    reference's types, so its maps are the fixture's bit for bit and its texts byte for byte."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("sparse_depth_restated", os.path.join(ROOT, "scripts", "micro", "sparse_depth_restated.py"))
    restated = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(restated)
    os.environ.setdefault("MPLBACKEND", "Agg")
    f = fixture(case)
    restated.convert(case_dir(case), str(tmp_path))
    for i, name in enumerate(f["names"].tolist()):
        stem = os.path.splitext(name)[0]
        d = np.load(str(tmp_path / "depths" / (stem + ".npy")))
        assert np.array_equal(d.view(np.uint64), f["depth_%d" % i].view(np.uint64))
        assert open(str(tmp_path / "poses" / (stem + ".txt"))).read() == str(f["pose_%d" % i])
        assert open(str(tmp_path / "intrinsics" / (stem + ".txt"))).read() == str(f["intr_%d" % i])


def test_batches_respect_the_budget():
    from psfm_sfm.convert import IMAGE_DESC, batches
    d = np.zeros(5, IMAGE_DESC)
    d["w"], d["h"] = [10, 10, 20, 10, 10], [10, 10, 20, 10, 10]       # 1200, 1200, 4800, 1200, 1200 bytes
    assert batches(d, 0) == [(0, 5)]
    assert batches(d, 1) == [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)]
    assert batches(d, 2400) == [(0, 2), (2, 3), (3, 5)]
    assert batches(d, 6000) == [(0, 2), (2, 4), (4, 5)]
    assert batches(d[:0], 100) == []
