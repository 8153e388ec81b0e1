"""psfm_track_queries_optimize without a GPU, against golden vectors that the REFERENCE's own point_trajectory Python produced
(tests/golden/make_queries_pc_golden.py: IncrementalTrajectorySet(buffer_size=3) fed with caller-given points, the body of
track_optimize.py:37-50, optimize_location being the C oracle).

  1. tests/_queries_pc_np.py (NumPy: step_np + the refs / scale arithmetic restated + oracle.optimize_location, rows in query order)
     reproduces the fixture: births, lengths, rows per solve and the solver's decisions exactly, positions within 1e-4 px (the
     reference's rows are in the order of its active list -- survivors, then the frame's new queries -- so the f64 sums of the solve
     may differ in their last bits; observed: 0).
  2. The per-lane text the kernels compile, particle-sfm_amd/csrc/psfm_query_pc.h, built for the host by tests/host/queries_pc_host.cpp
     with -ffp-contract=off and driven over absolute frames as psfm_query_pc.hip drives it (backward: dir = -1): step verdicts, row
     membership and the rows (uv12, ref1, ref2, scale) bit for bit equal to the NumPy statement on every frame of every case.
  3. The resource census of psfm_query_pc.hip from the cross-compile's code-object metadata: no scratch, no spills, LDS only in the
     scan, the step kernel at 8 waves per SIMD (profiles/EXPERIMENTS.md section 23 quotes the figures)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import _queries_np as qn
import _queries_pc_np as qp
from _motion_boundary_np import motion_boundary_np
from test_persist_resources import _census

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("queries_pc") / "libqueries_pc_host.so")
    cmd = ["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "tests", "host", "shim"),
           "-I", os.path.join(ROOT, "particle-sfm_amd", "csrc"), os.path.join(ROOT, "tests", "host", "queries_pc_host.cpp"), "-o", out]
    subprocess.run(cmd, check=True)
    L = ctypes.CDLL(out)
    vp, i = ctypes.c_void_p, ctypes.c_int
    L.psfm_host_query_pc_frame.argtypes = [vp, vp, vp, vp, vp, i, i, vp, ctypes.c_long, i, i, i, vp, vp, vp, vp, vp, vp, vp, vp]
    L.psfm_host_query_pc_frame.restype = i
    L.psfm_host_query_pc_scatter.argtypes = [i, i, ctypes.c_long, i, i, vp, vp, vp, i]
    L.psfm_host_query_pc_scatter.restype = None
    return L


@pytest.fixture(scope="module")
def cases():
    return {c: qp.load_case(c) for c in qp.CASES}


@pytest.fixture(scope="module")
def numpy_runs(cases):
    """The NumPy statement of every case and direction, computed once."""
    return {(c, d): qp.track_queries_pc_np(cases[c]["xy"], cases[c]["t"], mb=qp.CASES[c]["mb"], **qp.stacks(cases[c], d)) for c, d in qp.CASE_DIRS}


@pytest.mark.parametrize("case,direction", qp.CASE_DIRS)
def test_numpy_statement_reproduces_the_reference_fixture(cases, numpy_runs, case, direction):
    want = qp.expected(cases[case]["g"], case, direction)
    got = numpy_runs[(case, direction)]
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert got[2].shape == want[2].shape
    err = float(np.abs(got[2] - want[2]).max())
    print(case, direction, "max |xy - reference| = %.3g px" % err)
    assert err <= qp.TOL
    for k in (3, 4, 5):                                   # rows, iterations, termination of every solve
        assert np.array_equal(got[k], want[k]), k
    assert len(want[3]) > 0 and want[4].max() > 1


def _ptr(a):
    return a.ctypes.data if a is not None else None


def header_direction(L, xy, t, flows, occ, flows2, occ2, mb, back):
    """One direction over ABSOLUTE frames as psfm_query_pc.hip runs it; the log of every frame in the format of qp.engine_np."""
    from oracle import oracle
    xy = np.ascontiguousarray(xy, np.float64)
    t = np.ascontiguousarray(t, np.int32)
    Q, n = len(t), len(flows)
    H, W = flows[0].shape[:2]
    flows = [np.ascontiguousarray(f, np.float32) for f in flows]
    flows2 = [np.ascontiguousarray(f, np.float32) for f in flows2]
    masks = [(np.asarray(o) != 0).astype(np.uint8) for o in occ]
    if mb:
        masks = [m | (motion_boundary_np(f, qp.MB_THRES).astype(np.uint8) << 1) for m, f in zip(masks, flows)]
    masks = [np.ascontiguousarray(m) for m in masks]
    occ2 = [np.ascontiguousarray((np.asarray(o) != 0).astype(np.uint8)) for o in occ2]
    slab = np.full((n + 1, Q, 2), np.nan)
    slab[t, np.arange(Q)] = xy
    ln = np.ones(Q, np.int32)
    took = np.zeros(Q, np.uint8)
    uv12, ref1, ref2, scale, owner = np.zeros((Q, 4)), np.zeros((Q, 2)), np.zeros((Q, 2)), np.zeros(Q), np.zeros(Q, np.int32)
    d = -1 if back else 1
    log = []
    for k in range(n):
        frm = n - k if back else k
        m = frm - 1 if back else frm
        f01 = f02 = o02 = None
        if k >= 1:
            f01, f02, o02 = flows[frm if back else frm - 1], flows2[frm - 1], occ2[frm - 1]
        nr = L.psfm_host_query_pc_frame(_ptr(flows[m]), _ptr(masks[m]), _ptr(f01), _ptr(f02), _ptr(o02), H, W, _ptr(t), Q, int(mb), frm, d,
                                        _ptr(slab), _ptr(ln), _ptr(took), _ptr(uv12), _ptr(ref1), _ptr(ref2), _ptr(scale), _ptr(owner))
        assert nr >= 0, "the step launch and the rows launch disagree on a lane's membership"
        idx = np.nonzero(took)[0]
        e = dict(f=k, idx=idx, alive=took[idx] == 2, owner=owner[:nr].astype(np.int64).copy())
        if nr:
            e.update(uv12=uv12[:nr].copy(), ref1=ref1[:nr].copy(), ref2=ref2[:nr].copy(), scale=scale[:nr].copy())
            out = np.ascontiguousarray(oracle.optimize_location(uv12[:nr], ref1[:nr], ref2[:nr], scale[:nr], flows[m]))
            L.psfm_host_query_pc_scatter(H, W, Q, frm, d, _ptr(slab), _ptr(out), _ptr(owner), nr)
        log.append(e)
    return slab, ln, log


@pytest.mark.parametrize("case,direction", [cd for cd in qp.CASE_DIRS if cd[1] != "both"])
def test_header_equals_the_numpy_statement_bit_for_bit_on_every_frame(host, cases, numpy_runs, case, direction):
    c = cases[case]
    mb = qp.CASES[case]["mb"]
    back = direction == "backward"
    xy, t = c["xy"], c["t"]
    if back:
        stk = (c["flows_b"], c["occ_b"], c["flows_b2"], c["occ_b2"])
        tr, fl, oc, fl2, oc2 = qp.reversed_direction(t, *stk)
    else:
        stk = (c["flows_f"], c["occ_f"], c["flows_f2"], c["occ_f2"])
        tr, fl, oc, fl2, oc2 = t, list(stk[0]), list(stk[1]), list(stk[2]), list(stk[3])
    want_log = []
    qp.engine_np(xy, tr, fl, oc, fl2, oc2, mb=mb, log=want_log)
    slab, ln, got_log = header_direction(host, xy, t, *stk, mb=mb, back=back)
    assert len(got_log) == len(want_log) == len(fl)
    n_rows = 0
    for g, w in zip(got_log, want_log):
        assert np.array_equal(g["idx"], w["idx"]) and np.array_equal(g["alive"], w["alive"]), g["f"]       # who stepped, the verdicts
        assert np.array_equal(g["owner"], w["owner"]), g["f"]                                              # row membership, in query order
        for k in ("uv12", "ref1", "ref2", "scale"):
            assert (k in g) == (k in w)
            if k in g:
                assert g[k].tobytes() == np.ascontiguousarray(w[k], np.float64).tobytes(), (g["f"], k)
        n_rows += len(g["owner"])
    assert n_rows > 100
    # ... and the result: the slab's rows against the statement's CSR
    birth, length, pts = numpy_runs[(case, direction)][:3]
    rows = np.concatenate([slab[birth[q]:birth[q] + length[q], q] for q in range(len(t))], 0)
    assert np.array_equal(length, ln) and rows.tobytes() == pts.tobytes()


def test_fixture_holds_the_queries_it_is_there_for(cases):
    for case, c in qp.CASES.items():
        d = cases[case]
        n = c["T"] - 1
        xy, t = qp.make_queries(case)
        assert np.array_equal(d["xy"], xy) and np.array_equal(d["t"], t) and len(d["flows_f2"]) == n - 1 and len(d["occ_b2"]) == n - 1
        for direction in c["dirs"]:
            birth, length, pts, rows, its, term = qp.expected(d["g"], case, direction)
            assert length.sum() == len(pts) and (length >= 1).all()
            assert len(rows) == (n - 1) * (2 if direction == "both" else 1) and rows.min() >= 20      # every frame from the second solves
            plain = qn.track_queries_np(xy, t, mb=c["mb"], **{k: v for k, v in qp.stacks(d, direction).items() if not k.endswith("2")})
            # the stride-2 stack matters: positions differ from the raw chained flow
            same = np.array_equal(plain[1], length)
            assert not same or float(np.abs(plain[2] - pts).max()) > 1e-3


# ---- 3. the resource census of the new translation unit ----
@pytest.fixture(scope="module")
def census(tmp_path_factory):
    return _census("psfm_query_pc.hip", tmp_path_factory.mktemp("query_pc"))


def test_census_of_the_new_kernels(census):
    names = sorted(census)
    print(*("%s%s %s" % (k[0], k[1], v) for k, v in sorted(census.items())), sep="\n")
    assert names == [("psfm_query_pc_init_kernel", ()), ("psfm_query_pc_rows_kernel", ()), ("psfm_query_pc_scan_kernel", ()),
                     ("psfm_query_pc_scatter_kernel", ()), ("psfm_query_pc_step_kernel", (0,)), ("psfm_query_pc_step_kernel", (1,))]
    for key, k in census.items():
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, key
        if key[0] == "psfm_query_pc_scan_kernel":
            assert k["group_segment_fixed_size"] == 16, "the scan's four wave totals"
        else:
            assert k["group_segment_fixed_size"] == 0, key
        assert k["vgpr_count"] <= 64, key                  # 8 waves per SIMD: the step is a chain of dependent gathers
