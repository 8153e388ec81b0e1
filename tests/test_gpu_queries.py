"""psfm_track_queries on the GPU (csrc/psfm_query.hip) through run_track_queries / run_connect_queries: every fixture of
tests/golden/queries.npz (the REFERENCE's own functions, tests/golden/make_queries_golden.py) bit for bit; subsets on wave and block
edges; the stride grid at t = 0 against the trajectories psfm_track gives birth 0; backward against forward on the time-flipped
stacks; the consumers of a result on a query result against the package's host statements; the refusals."""
import ctypes

import numpy as np
import pytest

import psfm_synth
import _queries_np as qn

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pt():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from point_trajectory import trajectory, utils, _hip
    _hip.context()
    class NS: pass
    ns = NS()
    ns.trajectory, ns.utils, ns.hip, ns.torch = trajectory, utils, _hip, torch
    return ns


@pytest.fixture(scope="module")
def cases():
    return {c: qn.load_case(c) for c in qn.CASES}


def csr(R):
    return np.array(R.birth), np.array(R.length), np.array(R.off), np.array(R.xy)


def rows_of(birth, length, xy, sel):
    """The CSR of the trajectories `sel` of a CSR."""
    off = np.concatenate([[0], np.cumsum(length)])
    pts = np.concatenate([xy[off[i]:off[i + 1]] for i in sel], 0) if len(sel) else np.zeros((0, 2))
    return birth[sel], length[sel], pts


def assert_same(got, want):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert got[2].shape == want[2].shape and got[2].tobytes() == want[2].tobytes()


def stacks(case, direction):
    ff, fb, of, ob, xy, t, g = case
    kw = {}
    if direction in ("forward", "both"):
        kw.update(flows=ff, occ=of)
    if direction in ("backward", "both"):
        kw.update(flows_b=fb, occ_b=ob)
    return kw


@pytest.mark.parametrize("case,direction", qn.CASE_DIRS)
def test_fixture_bit_equal_through_both_entry_points(pt, cases, case, direction):
    ff, fb, of, ob, xy, t, g = cases[case]
    want = qn.expected(g, case, direction)
    mb = dict(motion_boundary=qn.CASES[case]["mb"], mb_thres=qn.MB_THRES)
    R = pt.trajectory.run_track_queries(xy, t, **stacks(cases[case], direction), **mb)
    assert len(R) == len(t) and R.info["n_traj"] == len(t) and R.info["chain_mode"] == 4 and R.info["n_points"] == len(want[2])
    b, l, o, p = csr(R)
    assert_same((b, l, p), want)
    assert np.array_equal(o, np.concatenate([[0], np.cumsum(l)]))
    R2 = pt.trajectory.run_track_queries(xy, t, **stacks(cases[case], direction), **mb)      # identical calls, identical bytes
    assert all(x.tobytes() == y.tobytes() for x, y in zip(csr(R), csr(R2)))
    C = pt.trajectory.run_connect_queries(xy, t, ff, fb, thres=1.0, direction=direction, **mb)   # the maps from flow_check_device
    b, l, o, p = csr(C)
    assert_same((b, l, p), want)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257])
def test_subsets_on_wave_and_block_edges_give_their_rows(pt, cases, n):
    ff, fb, of, ob, xy, t, g = cases["q37x53"]
    want = qn.expected(g, "q37x53", "both")
    sel = np.arange(len(t))[::-1][:n][::-1] if n > 1 else np.array([len(t) - 14])    # the tail holds the hand-placed queries
    R = pt.trajectory.run_track_queries(xy[sel], t[sel], flows=ff, occ=of, flows_b=fb, occ_b=ob)
    b, l, o, p = csr(R)
    assert_same((b, l, p), rows_of(*want, sel))


def test_stride_grid_at_t0_equals_the_births_of_frame_0(pt):
    """131 x 259, 6 flows, r = 2: 8 580 queries (34 blocks); the trajectories psfm_track (one launch per frame) gives birth 0 are the
    tracks of the grid points, matched by their first point."""
    torch = pt.torch
    H, W, n, r = 131, 259, 6, 2
    d = psfm_synth.synth_sequence(n + 1, H, W, seed=23, sigma=0.2, n_occluders=2, stride2=False)
    ff, fb = torch.from_numpy(np.stack(d["flows_f"])).cuda(), torch.from_numpy(np.stack(d["flows_b"])).cuda()
    occ = pt.utils.flow_check_device(ff, fb, 1.0)[1]
    ctx = pt.hip.context()
    ctx.set_chain_mode(1)
    try:
        T = pt.trajectory.run_track(ff, occ, None, None, r)
    finally:
        ctx.set_chain_mode(0)
    assert T.info["chain_mode"] == 1
    yy, xx = np.mgrid[0:H:r, 0:W:r]
    grid = np.stack([xx.ravel(), yy.ravel()], 1).astype(np.float64)
    assert len(grid) == 8580
    Q = pt.trajectory.run_track_queries(grid, np.zeros(len(grid), np.int32), flows=ff, occ=occ)
    sel = np.nonzero(T.birth == 0)[0]
    first = T.xy[T.off[sel]]
    key = lambda p: (p[:, 1].astype(np.int64) * W + p[:, 0].astype(np.int64))
    assert len(sel) == len(grid) and np.array_equal(np.sort(key(first)), key(grid))
    order = sel[np.argsort(key(first))]                       # trajectory of grid point k (the grid is in key order)
    want = rows_of(np.array(T.birth), np.array(T.length), np.array(T.xy), order)
    b, l, o, p = csr(Q)
    assert_same((b, l, p), want)
    assert l.min() == 1 and l.max() == n + 1 and len(np.unique(l)) > 3


def test_backward_equals_forward_on_the_time_flipped_stacks(pt, cases):
    ff, fb, of, ob, xy, t, g = cases["q24x30"]
    n = len(fb)
    B = pt.trajectory.run_track_queries(xy, t, flows_b=fb, occ_b=ob)
    F = pt.trajectory.run_track_queries(xy, n - t, flows=fb[::-1].copy(), occ=ob[::-1].copy())
    bb, bl, bo, bp = csr(B)
    fb_, fl, fo, fp = csr(F)
    assert np.array_equal(bl, fl) and np.array_equal(bb + bl - 1, t) and np.array_equal(fb_, n - t)
    flipped = np.concatenate([fp[fo[i]:fo[i + 1]][::-1] for i in range(len(t))], 0)      # a backward track in ascending time
    assert flipped.tobytes() == bp.tobytes() and bl.max() == n + 1


def test_consumers_work_on_a_query_result(pt, cases):
    """psfm_result_filter(3), sample_window_device and match_tables_device on a query result against the package's host statements
    fed with the same CSR."""
    from point_trajectory.trajectory import result_to_trajectory_set
    from psfm_motion_seg.load_cut_seq import sample_window_device
    from psfm_sfm import matches_from_flow as mff
    ff, fb, of, ob, xy, t, g = cases["q37x53"]
    c = qn.CASES["q37x53"]
    T, H, W = c["T"], c["H"], c["W"]
    R = pt.trajectory.run_track_queries(xy, t, flows=ff, occ=of, flows_b=fb, occ_b=ob)
    ctx = pt.hip.context()
    info = pt.hip.TrackInfo(n_traj=len(R), n_points=R.n_points)
    host = R.to_trajectory_set(3)
    dev = result_to_trajectory_set(ctx, info, 3)
    for a, b in zip(host._csr[:5], dev._csr[:5]):
        assert np.array_equal(a, b)
    assert 0 < len(dev._csr[0]) < len(R)
    host.build_invert_indexes()
    want = host.sample_inside_window(list(range(2, 7)), min_length=3, max_num_tracks=10 ** 9)
    ids, raw, _, mask = sample_window_device(ctx, 2, 5, (H, W), (H, W), 10 ** 9)
    assert np.array_equal(ids.cpu().numpy(), np.asarray(want["traj_ids"], np.int32)) and len(want["traj_ids"]) > 50
    assert np.array_equal(raw.cpu().numpy(), np.stack(want["locations"], -1))
    assert np.array_equal(mask.cpu().numpy()[:, :, 0], 1.0 - want["masks"])
    ids_, birth, length, off, pts = host._csr[:5]
    frames = (np.repeat(birth, length) + np.arange(len(pts)) - np.repeat(off[:-1], length)).astype(np.int64)
    want_tables = mff.match_tables_host(off, frames, pts, np.zeros(len(pts), bool), T)
    got_tables = mff.match_tables_device(ctx, T)
    for a, b in zip(got_tables, want_tables):
        assert np.array_equal(a, b)
    assert len(want_tables[5]) > 100


def test_refusals_leave_the_previous_result_intact(pt, cases):
    torch = pt.torch
    ff, fb, of, ob, xy, t, g = cases["q24x30"]
    n = len(ff)
    ctx = pt.hip.context()
    L, sp = pt.hip.lib(), pt.hip.current_stream_ptr(ctx.device)
    info = pt.trajectory.run_track_queries(xy, t, flows=ff, occ=of, return_device=True)
    before = csr(pt.trajectory._result_to_host(ctx, info))

    def intact():
        return all(x.tobytes() == y.tobytes() for x, y in zip(before, csr(pt.trajectory._result_to_host(ctx, info))))

    def refused(xy_, t_, **kw):
        with pytest.raises(pt.hip.PsfmError) as e:
            pt.trajectory.run_track_queries(xy_, t_, **kw)
        assert e.value.status == pt.hip.PSFM_ERR_ARG and intact()
        return str(e.value)
    for bad in (np.nan, np.inf, -np.inf):
        q = xy.copy()
        q[7, 1] = bad
        q[200, 0] = bad
        assert "query 7 " in refused(q, t, flows=ff, occ=of)
    for bad_t, at in ((-1, 5), (n + 1, 0), (n + 1, len(t) - 1)):
        tt = t.copy()
        tt[at] = bad_t
        assert "query %d " % at in refused(xy, tt, flows=ff, occ=of)
    assert "stack" in refused(xy, t)                                          # no stack given
    assert "stack" in refused(xy, t, flows=ff)                                # a stack without its maps
    assert "stack" in refused(xy, t, flows=ff, occ=of, flows_b=fb)
    assert "stack" in refused(xy, t, occ=of)                                  # maps without their stack
    # n_q beyond a 4 GB slab row: refused on the arguments alone, nothing is allocated or read
    st = L.psfm_track_queries(ctx.handle, pt.hip.ptr(torch.from_numpy(ff).cuda()), pt.hip.ptr(torch.from_numpy(of.astype(np.uint8)).cuda()), None,
                              None, n, ff.shape[1], ff.shape[2], ctypes.c_void_p(16), ctypes.c_void_p(16), 1 << 28, None, sp)
    assert st == pt.hip.PSFM_ERR_ARG and intact()
    # psfm_result_keys needs a birth grid index, which a query does not have
    keys = torch.zeros(len(t), dtype=torch.int64, device="cuda")
    assert L.psfm_result_keys(ctx.handle, 2, ff.shape[2], pt.hip.ptr(keys), sp) == pt.hip.PSFM_ERR_ARG
    assert b"query" in L.psfm_last_error() and intact()
    # ... and works again on the result of psfm_track
    T = pt.trajectory.run_track(ff, of, None, None, 2)
    keys = torch.zeros(len(T), dtype=torch.int64, device="cuda")
    pt.hip.check(L.psfm_result_keys(ctx.handle, 2, ff.shape[2], pt.hip.ptr(keys), sp))
    torch.cuda.synchronize()
    assert (np.diff(keys.cpu().numpy()) > 0).all()


def test_no_queries_is_an_empty_result(pt, cases):
    ff, fb, of, ob, xy, t, g = cases["q24x30"]
    R = pt.trajectory.run_track_queries(np.zeros((0, 2)), np.zeros(0, np.int32), flows=ff, occ=of)
    assert len(R) == 0 and R.n_points == 0 and R.info["chain_mode"] == 4
