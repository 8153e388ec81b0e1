"""The display images of the sparse depth maps without a GPU, against golden vectors that the REFERENCE's own
normalize_depth_for_display and matplotlib's byte conversion produced (tests/golden/make_depth_display_golden.py).

Two statements of the rule are pinned to the fixture, bytes and both percentiles exact: psfm_sfm.convert.depth_display_host (NumPy;
the model the GPU tests compare with) and particle-sfm_amd/csrc/psfm_depth_display.h -- the per-element rules of the kernels,
selection included -- compiled for the host through tests/host/shim by tests/host/depth_display_host.cpp with -ffp-contract=off.
The interpolation is also compared with np.percentile directly; png / writers of save_model are checked on the NumPy route."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from _depth_display_np import case, case_names, fixture, same_bits, table_words
from _sparse_depth_np import case_dir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PCS = (98, 2, 50, 0, 100)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("depth_display") / "libdepth_display_host.so")
    cmd = ["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "tests", "host", "shim"),
           "-I", os.path.join(ROOT, "particle-sfm_amd", "csrc"), os.path.join(ROOT, "tests", "host", "depth_display_host.cpp"), "-o", out]
    subprocess.run(cmd, check=True)
    L = ctypes.CDLL(out)
    vp, u32, f64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_double
    L.psfm_host_dd_rank.argtypes = [u32, f64, ctypes.POINTER(u32), ctypes.POINTER(u32), ctypes.POINTER(f64)]
    L.psfm_host_dd_rank.restype = None
    L.psfm_host_dd_lerp.argtypes = [f64, f64, f64]
    L.psfm_host_dd_lerp.restype = f64
    L.psfm_host_dd_image.argtypes = [vp, ctypes.c_int64, f64, vp, vp, vp, vp]
    L.psfm_host_dd_image.restype = ctypes.c_int64
    return L


def test_fixture_holds_the_cases_it_is_there_for():
    f, names = fixture(), case_names()
    assert int(f["chunk"]) == 1024 and {"chunk_1023", "chunk_1024", "chunk_1025", "blocks", "no_positive"} <= set(names)
    for name, n in (("chunk_1023", 1023), ("chunk_1024", 1024), ("chunk_1025", 1025), ("blocks", 40000), ("n51_pc98", 51), ("n101_pc2", 101),
                    ("n_1_pc98", 1), ("n_2_pc50", 2)):
        assert int(np.count_nonzero(case(name)[0][0] > 0)) == n
    assert [m.shape for m in case("batch_misaligned")[0]] == [(3, 5), (4, 4), (2, 3)]
    assert [m.shape[1] for m in case("batch_widths")[0]] == list(range(1, 10))
    maps, want, _, _ = case("batch_with_empty")
    assert [w[0] is None for w in want] == [False, True, False, True, False]
    assert case("no_positive")[1][0][0] is None and np.any(case("no_positive")[0][0] == -1.0)
    d, (rgba, z) = case("all_equal_pc98")[0][0], case("all_equal_pc98")[1][0]
    assert z[0] == z[1] and np.all(rgba[d > 0] == f["bad_binary"])         # 0/0: the bad colour
    assert np.any(np.all(rgba == f["table_binary"][255], -1)) and np.any(np.all(rgba == f["table_binary"][0], -1))     # +inf, -inf
    lo = (1.0 / (case("low_byte")[0][0].reshape(-1) + 1.0)).view(np.uint64)
    assert len(set((lo >> np.uint64(8)).tolist())) == 1 and len(set(lo.tolist())) > 20
    ex = case("exponent")[0][0]
    inv = (1.0 / (ex[ex > 0] + 1.0)).view(np.uint64)
    assert np.all(inv & np.uint64(2 ** 52 - 1) == 0) and len(set(inv.tolist())) == 40
    t = case("ties")[0][0]
    s = np.sort(1.0 / (t[t > 0] + 1.0))
    assert s[1] == s[2] and s[-2] == s[-3]                                # ties at the ranks of pc 98 and 2 (n = 100: vi = 1.98, 97.02)
    neg = case("negative")[0][0]
    assert np.any(neg == -1.0) and np.any(np.isnan(neg)) and np.any(neg < -1.0) and np.any(np.isinf(neg))
    assert sorted(set(f["case_pc"].tolist())) == [0.0, 2.0, 50.0, 98.0, 100.0] and set(f["case_cmap"].tolist()) == {"binary", "gray"}
    assert case("exponent_pc2")[1][0][1][0] < case("exponent_pc2")[1][0][1][1]       # pc = 2: z1 < z2
    assert not np.array_equal(f["table_binary"][:, 0], 255 - np.arange(256)) and f["bad_binary"].tolist() == [0, 0, 0, 255]


def test_colour_table_equals_the_fixture():
    from psfm_sfm.convert import colour_table
    os.environ.setdefault("MPLBACKEND", "Agg")
    f = fixture()
    for cmap in ("binary", "gray"):
        table, bad = colour_table(cmap)
        assert table.dtype == np.uint8 and table.shape == (256, 4) and bad.shape == (4,)
        assert np.array_equal(table, f["table_" + cmap]) and np.array_equal(bad, f["bad_" + cmap])


@pytest.mark.parametrize("name", case_names())
def test_numpy_model_equals_the_reference(name):
    from psfm_sfm.convert import depth_display_host
    os.environ.setdefault("MPLBACKEND", "Agg")
    maps, want, pc, cmap = case(name)
    for d, (rgba, z) in zip(maps, want):
        got, z1, z2 = depth_display_host(d, pc, cmap)
        if rgba is None:
            assert got is None
        else:
            assert got.dtype == np.uint8 and np.array_equal(got, rgba) and same_bits([z1, z2], z)


@pytest.mark.parametrize("name", case_names())
def test_header_equals_the_reference(host, name):
    maps, want, pc, cmap = case(name)
    table = table_words(cmap)
    for d, (rgba, z) in zip(maps, want):
        d = np.ascontiguousarray(d)
        out, zz, sel = np.full(d.size, 0xA5A5A5A5, np.uint32), np.full(2, 7.0), np.full(4, 9, np.uint64)
        n = host.psfm_host_dd_image(d.ctypes.data, d.size, pc, table.ctypes.data, out.ctypes.data, zz.ctypes.data, sel.ctypes.data)
        assert n == int(np.count_nonzero(d > 0))
        if rgba is None:
            assert n == 0 and np.all(out == 0xA5A5A5A5) and np.all(zz == 7.0)
            continue
        assert np.array_equal(out.view(np.uint8).reshape(d.shape + (4,)), rgba) and same_bits(zz, z)
        # the selection against a sort
        with np.errstate(divide="ignore"):
            s = np.sort((1.0 / (d[d > 0] + 1.0)).view(np.uint64))
        j, j1, g = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_double()
        for k, q in enumerate((pc, 100.0 - pc)):
            host.psfm_host_dd_rank(n, q, ctypes.byref(j), ctypes.byref(j1), ctypes.byref(g))
            assert sel[2 * k] == s[j.value] and sel[2 * k + 1] == s[j1.value]


def test_interpolation_equals_np_percentile_for_every_n(host):
    from psfm_sfm.convert import percentile_lerp, percentile_rank
    rng = np.random.default_rng(3)
    j, j1, g = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_double()
    for n in range(1, 301):
        s = np.sort(rng.uniform(0, 1, n))
        if n > 4:
            s[n // 2] = s[n // 2 - 1]                                     # a tie
        for q in PCS:
            want = np.percentile(s, q)
            host.psfm_host_dd_rank(n, q, ctypes.byref(j), ctypes.byref(j1), ctypes.byref(g))
            mj, mj1, mg = percentile_rank(n, q)
            assert (j.value, j1.value) == (mj, mj1) and same_bits(g.value, mg)
            assert same_bits(host.psfm_host_dd_lerp(s[j.value], s[j1.value], g.value), want), (n, q)
            assert same_bits(percentile_lerp(s[mj], s[mj1], mg), want), (n, q)


# ---- the files ---------------------------------------------------------------------------------------------------------------------

def pngs(path):
    return sorted(n for n in os.listdir(os.path.join(path, "depths")) if n.endswith(".png"))


def test_png_false_writes_no_png(tmp_path):
    from psfm_sfm.convert import read_model_arrays, save_model
    os.environ.setdefault("MPLBACKEND", "Agg")
    m = read_model_arrays(case_dir("a"))
    save_model(str(tmp_path / "on"), m, device=False)
    save_model(str(tmp_path / "off"), m, device=False, png=False)
    assert len(pngs(str(tmp_path / "on"))) == 4 and pngs(str(tmp_path / "off")) == []
    npy = lambda p: sorted(n for n in os.listdir(os.path.join(p, "depths")) if n.endswith(".npy"))
    assert npy(str(tmp_path / "on")) == npy(str(tmp_path / "off")) and len(npy(str(tmp_path / "off"))) == 4
    for sub in ("poses", "intrinsics"):
        assert sorted(os.listdir(str(tmp_path / "on" / sub))) == sorted(os.listdir(str(tmp_path / "off" / sub)))


def test_three_writers_write_what_one_writes(tmp_path):
    from matplotlib import pyplot as plt
    from psfm_sfm.convert import read_model_arrays, save_model
    os.environ.setdefault("MPLBACKEND", "Agg")
    for c in ("a", "d"):
        m = read_model_arrays(case_dir(c))
        one, three = str(tmp_path / (c + "1")), str(tmp_path / (c + "3"))
        save_model(one, m, device=False, writers=1)
        save_model(three, m, device=False, writers=3)
        assert pngs(one) == pngs(three) and len(pngs(one)) == (4 if c == "a" else 2)
        for n in pngs(one):
            assert np.array_equal(plt.imread(os.path.join(one, "depths", n)), plt.imread(os.path.join(three, "depths", n)))
        for n in os.listdir(os.path.join(one, "depths")):
            if n.endswith(".npy"):
                assert np.array_equal(np.load(os.path.join(one, "depths", n)), np.load(os.path.join(three, "depths", n)))


def test_bad_arguments_of_save_model(tmp_path):
    from psfm_sfm.convert import read_model_arrays, save_model
    m = read_model_arrays(case_dir("d"))
    with pytest.raises(ValueError):
        save_model(str(tmp_path), m, device=False, display="device")
    with pytest.raises(ValueError):
        save_model(str(tmp_path), m, device=False, display="gpu")
    with pytest.raises(ValueError):
        save_model(str(tmp_path), m, device=False, writers=0)
