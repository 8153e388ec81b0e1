"""psfm_track_queries without a GPU, against golden vectors that the REFERENCE's own point_trajectory Python produced
(tests/golden/make_queries_golden.py: utils.flow_check, trajectory.grid_sample, trajectory.motion_boundary and trajectory.step_forward,
per frame on the positions still alive; the motion-boundary case with the reference's commented kill rule switched on at run time).

Two statements are pinned to those vectors bit for bit -- births, lengths, positions: tests/_queries_np.py (NumPy, one step_np per
frame) and the per-lane frame loop the kernel compiles, particle-sfm_amd/csrc/psfm_query.h, built for the host through tests/host/shim
by tests/host/queries_host.cpp with -ffp-contract=off.  No tolerance: the step is the arithmetic that is already pinned bit for bit,
and p + (double)flow has one rounding."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import _queries_np as qn
from _motion_boundary_np import motion_boundary_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("queries") / "libqueries_host.so")
    cmd = ["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "tests", "host", "shim"),
           "-I", os.path.join(ROOT, "particle-sfm_amd", "csrc"), os.path.join(ROOT, "tests", "host", "queries_host.cpp"), "-o", out]
    subprocess.run(cmd, check=True)
    L = ctypes.CDLL(out)
    vp = ctypes.c_void_p
    L.psfm_host_track_queries.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp, ctypes.c_long, ctypes.c_int, ctypes.c_int,
                                          vp, vp]
    L.psfm_host_track_queries.restype = None
    return L


@pytest.fixture(scope="module")
def cases():
    return {c: qn.load_case(c) for c in qn.CASES}


def host_track_queries(L, xy, t, flows_f=None, occ_f=None, flows_b=None, occ_b=None, mb=False):
    """(birth, length, xy) as psfm_track_queries builds them: both directions into ONE slab by absolute frame, then rows
    birth .. birth + len - 1 of every query."""
    xy = np.ascontiguousarray(xy, np.float64)
    t = np.ascontiguousarray(t, np.int32)
    Q = len(t)
    n = len(flows_f if flows_f is not None else flows_b)
    slab = np.full((n + 1, Q, 2), np.nan)
    lens = []
    for flows, occ, back in ((flows_f, occ_f, 0), (flows_b, occ_b, 1)):
        if flows is None:
            lens.append(np.ones(Q, np.int32))
            continue
        flows = np.ascontiguousarray(flows, np.float32)
        masks = (np.asarray(occ) != 0).astype(np.uint8)
        if mb:
            masks = masks | (np.stack([motion_boundary_np(f, qn.MB_THRES) for f in flows]).astype(np.uint8) << 1)
        masks = np.ascontiguousarray(masks)
        ln = np.full(Q, -7, np.int32)
        L.psfm_host_track_queries(flows.ctypes.data, masks.ctypes.data, n, flows.shape[1], flows.shape[2], xy.ctypes.data, t.ctypes.data, Q,
                                  int(mb), back, slab.ctypes.data, ln.ctypes.data)
        lens.append(ln)
    birth = (t - (lens[1] - 1)).astype(np.int32)
    length = (lens[1] + lens[0] - 1).astype(np.int32)
    rows = [slab[birth[q]:birth[q] + length[q], q] for q in range(Q)]
    return birth, length, np.concatenate(rows, 0)


def _stacks(case, direction):
    ff, fb, of, ob, xy, t, g = case
    kw = {}
    if direction in ("forward", "both"):
        kw.update(flows_f=ff, occ_f=of)
    if direction in ("backward", "both"):
        kw.update(flows_b=fb, occ_b=ob)
    return kw


@pytest.mark.parametrize("case,direction", qn.CASE_DIRS)
def test_both_statements_equal_the_reference_fixture(host, cases, case, direction):
    ff, fb, of, ob, xy, t, g = cases[case]
    want_birth, want_len, want_xy = qn.expected(g, case, direction)
    mb = qn.CASES[case]["mb"]
    for name, got in (("numpy", qn.track_queries_np(xy, t, mb=mb, **_stacks(cases[case], direction))),
                      ("header", host_track_queries(host, xy, t, mb=mb, **_stacks(cases[case], direction)))):
        assert np.array_equal(got[0], want_birth), name
        assert np.array_equal(got[1], want_len), name
        assert got[2].shape == want_xy.shape and np.array_equal(got[2], want_xy), name
        assert got[2].tobytes() == want_xy.tobytes(), name        # (-0.0 and 0.0 are different queries)


def test_fixture_holds_the_queries_it_is_there_for(cases):
    for case, c in qn.CASES.items():
        ff, fb, of, ob, xy, t, g = cases[case]
        H, W, n = c["H"], c["W"], c["T"] - 1
        assert len(ff) == n and len(t) == c["n_random"] + 21 and t.min() == 0 and t.max() == n
        assert np.array_equal(xy, qn.make_queries(case)[0]) and np.array_equal(t, qn.make_queries(case)[1])
        hand = xy[c["n_random"]:]
        assert np.signbit(hand[8, 0]) and hand[8, 0] == 0 and hand[9, 0] == 1e-38 and (np.abs(hand) == 1e6).any()
        assert np.array_equal(hand[6], hand[7]) and t[c["n_random"] + 6] == t[c["n_random"] + 7]
        outside = (xy[:, 0] < 0) | (xy[:, 0] > W - 1) | (xy[:, 1] < 0) | (xy[:, 1] > H - 1)
        assert outside[:c["n_random"]].sum() >= 10
        for d in c["dirs"]:
            birth, length, pts = qn.expected(g, case, d)
            assert (length >= 1).all() and (birth >= 0).all() and (birth + length - 1 <= n).all() and length.sum() == len(pts)
            k = c["n_random"]
            assert length[k + 6] == length[k + 7]                                   # the identical queries
            far = np.abs(hand).max(1) == 1e6                                         # absurd coordinates: the query alone
            assert (length[k:][far] == 1).all()
            if d == "forward":
                assert (length[t == n] == 1).all() and (birth == t).all() and length.max() == n + 1
            if d == "backward":
                assert (length[t == 0] == 1).all() and (birth + length - 1 == t).all() and length.max() == n + 1
            if d == "both":
                bf, lf, _ = qn.expected(g, case, "forward")
                bb, lb, _ = qn.expected(g, case, "backward")
                assert np.array_equal(birth, bb) and np.array_equal(length, lb + lf - 1)
