"""The motion-boundary option without a GPU, against golden vectors that the REFERENCE's own point_trajectory/trajectory.py produced
(tests/golden/make_motion_boundary_golden.py: motion_boundary as it stands; step_forward in both forms of its kill rule, the
motion-boundary form being the reference's function with its commented line switched on at run time).

Two statements are pinned to those vectors bit for bit: tests/_motion_boundary_np.py (NumPy) and the arithmetic of the kernels --
particle-sfm_amd/csrc/psfm_motion_boundary.h and psfm_step_finish<MB> of psfm_chain.h -- compiled for the host through tests/host/shim
by tests/host/motion_boundary_host.cpp, with -ffp-contract=off."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from _common import golden
from _motion_boundary_np import MASK_CASES, MASK_THRES, STEP_FIXTURE, mask_case, motion_boundary_np, step_np, taps_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("motion_boundary") / "libmotion_boundary_host.so")
    cmd = ["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "tests", "host", "shim"),
           "-I", os.path.join(ROOT, "particle-sfm_amd", "csrc"), os.path.join(ROOT, "tests", "host", "motion_boundary_host.cpp"), "-o", out]
    subprocess.run(cmd, check=True)
    L = ctypes.CDLL(out)
    vp = ctypes.c_void_p
    L.psfm_host_motion_boundary.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float, vp]
    L.psfm_host_motion_boundary.restype = None
    L.psfm_host_step.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_long, ctypes.c_int, vp, vp, vp]
    L.psfm_host_step.restype = None
    return L


def host_mask(L, stack, thres, occ=None):
    stack = np.ascontiguousarray(stack, np.float32)
    n, h, w = stack.shape[:3]
    out = np.full((n, h, w), 77, np.uint8)
    occ = None if occ is None else np.ascontiguousarray(occ, np.uint8)
    L.psfm_host_motion_boundary(stack.ctypes.data, None if occ is None else occ.ctypes.data, n, h, w, thres, out.ctypes.data)
    return out


def host_step(L, flow, mask, xy, mb):
    flow = np.ascontiguousarray(flow, np.float32)
    mask = np.ascontiguousarray(mask, np.uint8)
    xy = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
    n = len(xy)
    nxt, alive, fs = np.full((n, 2), np.nan), np.full(n, 77, np.uint8), np.full((n, 2), np.nan, np.float32)
    L.psfm_host_step(flow.ctypes.data, mask.ctypes.data, flow.shape[0], flow.shape[1], xy.ctypes.data, n, int(mb), nxt.ctypes.data,
                     alive.ctypes.data, fs.ctypes.data)
    return nxt, alive.astype(bool), fs


# ---- the mask ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", MASK_CASES)
def test_masks_of_both_statements_equal_reference_fixture(host, name):
    stack, want = mask_case(name)
    for key, thres in MASK_THRES.items():
        assert want[key].dtype == bool and want[key].shape == stack.shape[:3]
        assert np.array_equal(np.stack([motion_boundary_np(f, thres) for f in stack]), want[key]), key
        assert np.array_equal(host_mask(host, stack, thres), want[key].astype(np.uint8)), key


def test_mask_fixtures_hold_the_edges_they_are_there_for():
    nf, m = mask_case("nonfinite_12x13")
    assert np.isnan(nf).any() and np.isinf(nf).any() and m["mb002"].any() and not m["mb002"].all()
    with np.errstate(all="ignore"):
        assert np.isnan(nf[0, 5, 5, 0] - nf[0, 5, 6, 0]) and not m["mb002"][0, 5, 5]          # inf - inf: a NaN gradient is no boundary
    sub, m = mask_case("subnormal_6x7")
    sq = sub.astype(np.float64) ** 2
    assert ((sq > 0) & (sq < 1.1754944e-38)).any() and ((sub != 0) & (sub * sub == 0)).any() and np.signbit(sub[sub == 0]).any()
    assert m["mb002"].any()                                                                    # a flushed gradient would be no boundary
    z, m = mask_case("zeros_6x6")
    zero = (z[0] == 0).all(-1)
    assert zero.any() and (m["mb002"][0] & zero).any() and (~m["mb002"][0] & zero).any()
    s, m = mask_case("stack2_3x5")
    assert s.shape[0] == 2 and (s.shape[1] * s.shape[2]) % 4 != 0
    big, m = mask_case("m37x53")
    assert 0.01 < m["mb002"].mean() < 0.2
    assert any((mask_case(n)[1]["mb002"] != mask_case(n)[1]["mb03"]).any() for n in MASK_CASES)


def test_kill_map_keeps_the_occlusion_bit_apart(host):
    stack, want = mask_case("m37x53")
    rng = np.random.default_rng(2)
    occ = (rng.uniform(size=stack.shape[:3]) < 0.3).astype(np.uint8) * rng.integers(1, 256, size=stack.shape[:3]).astype(np.uint8)
    kill = host_mask(host, stack, 0.02, occ)
    assert np.array_equal(kill & 1, (occ != 0).astype(np.uint8)) and np.array_equal(kill >> 1, want["mb002"].astype(np.uint8))


# ---- the step ----------------------------------------------------------------------------------------------------------------------

def test_step_of_both_statements_equals_reference_fixture(host):
    g = golden(STEP_FIXTURE)
    flow, occ, mb, xy = g["flow"], g["occ"], g["mb"], g["xy"]
    kill = occ.astype(np.uint8) | (mb.astype(np.uint8) << 1)
    nxt, alive, fs = host_step(host, flow, kill, xy, True)
    assert np.array_equal(fs.view(np.uint32), g["flow_sample"].view(np.uint32))
    assert np.array_equal(nxt, g["next"]) and np.array_equal(alive, g["alive_mb"])
    nxt_np, alive_np = step_np(xy, flow, occ, mb, "mb")
    assert np.array_equal(nxt_np, g["next"]) and np.array_equal(alive_np, g["alive_mb"])


def test_step_without_the_option_gives_the_shipped_verdicts(host):
    g = golden(STEP_FIXTURE)
    nxt, alive, _ = host_step(host, g["flow"], g["occ"].astype(np.uint8), g["xy"], False)
    assert np.array_equal(nxt, g["next"]) and np.array_equal(alive, g["alive_shipped"])
    assert np.array_equal(step_np(g["xy"], g["flow"], g["occ"], g["mb"], "shipped")[1], g["alive_shipped"])
    # MB = false reads a mask byte as "non-zero": any byte value is an occluded pixel, as today
    _, alive255, _ = host_step(host, g["flow"], g["occ"].astype(np.uint8) * 255, g["xy"], False)
    assert np.array_equal(alive255, g["alive_shipped"])


def test_one_verdict_over_the_union_is_another_rule(host):
    """occ | mb through the single verdict does NOT reproduce the fixture: the discriminating positions discriminate."""
    g = golden(STEP_FIXTURE)
    union = (g["occ"] | g["mb"]).astype(np.uint8)
    _, alive_or, _ = host_step(host, g["flow"], union, g["xy"], False)
    assert np.array_equal(alive_or, step_np(g["xy"], g["flow"], g["occ"], g["mb"], "or")[1])
    differ = alive_or != g["alive_mb"]
    assert differ.any() and not (alive_or & ~g["alive_mb"]).any()          # the union only ever kills more
    n_pl = int(g["n_planted"])
    assert differ[-n_pl:][:4].all()                                         # the planted pairs of 0.075-weight taps


def test_step_fixture_holds_the_tap_patterns_it_is_there_for():
    g = golden(STEP_FIXTURE)
    occ, mb, xy = g["occ"], g["mb"], g["xy"]
    H, W = occ.shape
    x0, y0, wts = taps_np(xy, H, W)
    taps = [(x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1)]
    inside = [(xx >= 0) & (xx < W) & (yy >= 0) & (yy < H) for xx, yy in taps]

    def hit(m, k):
        xx, yy = taps[k]
        return inside[k] & m[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]
    lo, hi = np.float32(0.05), np.float32(0.1)
    # one occluded tap and one boundary tap, each of weight in (0.05, 0.1), nothing else set
    n_occ = sum(hit(occ, k).astype(int) for k in range(4))
    n_mb = sum(hit(mb, k).astype(int) for k in range(4))
    w_occ = sum(np.where(hit(occ, k), wts[k], 0) for k in range(4))
    w_mb = sum(np.where(hit(mb, k), wts[k], 0) for k in range(4))
    pair = (n_occ == 1) & (n_mb == 1) & (w_occ > lo) & (w_occ < hi) & (w_mb > lo) & (w_mb < hi)
    # (neither verdict fires there: the track lives unless its next position leaves the image, as under the shipped rule)
    assert np.array_equal(g["alive_mb"][pair], g["alive_shipped"][pair]) and g["alive_mb"][pair].sum() >= 4
    # a lone boundary tap just above / just below 0.1
    lone = (n_occ == 0) & (n_mb == 1)
    assert (lone & (w_mb > hi) & (w_mb < np.float32(0.102)) & ~g["alive_mb"] & g["alive_shipped"]).any()
    assert (lone & (w_mb < hi) & (w_mb > np.float32(0.098)) & g["alive_mb"]).any()
    # taps outside the map: one, two and all four
    n_out = sum((~i).astype(int) for i in inside)
    assert (n_out == 2).any() and (n_out == 3).any() and (n_out == 4).any()
    assert (g["alive_shipped"] & ~g["alive_mb"]).sum() >= 10


# ---- the Python surface that needs no device -----------------------------------------------------------------------------------------

def test_motion_boundary_of_the_package_on_host_arrays_equals_the_fixture():
    from point_trajectory.trajectory import motion_boundary
    for name in MASK_CASES:
        stack, want = mask_case(name)
        for key, thres in MASK_THRES.items():
            for f, m in zip(stack, want[key]):
                got = motion_boundary(f, thres)
                assert got.dtype == bool and np.array_equal(got, m)


def test_the_names_the_reference_imports_beside_it_resolve():
    from point_trajectory.trajectory import grid_sample, motion_boundary  # noqa: F401
