"""psfm_track_queries_optimize on the GPU (csrc/psfm_query_pc.hip) through run_track_queries / run_connect_queries with the stride-2
stacks given: every fixture of tests/golden/queries_pc.npz (the REFERENCE's own classes fed with caller-given points,
tests/golden/make_queries_pc_golden.py) -- births and lengths exactly, positions within 1e-4 px, rows, iterations and termination of
every solve equal to the oracle's; the composed form on the device (psfm_grid_sample + psfm_optimize_location per frame, same rows
in the same order) within 1e-9 px; the edges of the compaction and of the frame loop; refusals and consumers; and, with every
stride-2 argument omitted, the bytes of psfm_track_queries."""
import ctypes

import numpy as np
import pytest

import _queries_np as qn
import _queries_pc_np as qp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pt():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from point_trajectory import trajectory, utils, _hip
    from point_trajectory.optimize.build import particlesfm
    _hip.context()
    class NS: pass
    ns = NS()
    ns.trajectory, ns.utils, ns.hip, ns.torch, ns.particlesfm = trajectory, utils, _hip, torch, particlesfm
    return ns


@pytest.fixture(scope="module")
def cases():
    return {c: qp.load_case(c) for c in qp.CASES}


def csr(R):
    return np.array(R.birth), np.array(R.length), np.array(R.off), np.array(R.xy)


def kwargs(case, direction):
    """qp.stacks under the names run_track_queries uses."""
    names = {"flows_f": "flows", "occ_f": "occ"}
    return {names.get(k, k): v for k, v in qp.stacks(case, direction).items()}


def solves(R):
    return tuple(np.array([s[k] for s in R.solve_stats], np.int32) for k in ("iterations", "termination"))


def rows_from_lengths(t, birth, length, n, directions):
    """Rows of every solve that ran, from the result alone: behind the step from frame f (reversed time for the backward half) a row is
    a query born two frames or more before f + 1 and alive there."""
    t = np.asarray(t).astype(np.int64)
    out = []
    for back in directions:
        tt = n - t if back else t
        ln = (t - birth + 1) if back else (birth + length - t)
        for f in range(1, n):
            k = int(((tt <= f - 1) & (tt + ln - 1 >= f + 1)).sum())
            if k:
                out.append(k)
    return np.array(out, np.int32)


def assert_matches(R, want, tol, what):
    """births, lengths exactly, positions within tol, iterations and termination of every solve; want: (birth, length, xy, rows, its, term)."""
    b, l, o, p = csr(R)
    assert np.array_equal(b, want[0]) and np.array_equal(l, want[1]), what
    assert np.array_equal(o, np.concatenate([[0], np.cumsum(l)])) and p.shape == want[2].shape
    err = float(np.abs(p - want[2]).max()) if len(p) else 0.0
    print(what, "max |xy - expected| = %.3g px" % err)
    assert err <= tol, what
    its, term = solves(R)
    assert R.info["n_solves"] == len(want[3]) and np.array_equal(its, want[4]) and np.array_equal(term, want[5]), what
    assert R.info["solver_iterations"] == int(want[4].sum())
    return err


@pytest.mark.parametrize("case,direction", qp.CASE_DIRS)
def test_fixture_through_both_entry_points(pt, cases, case, direction):
    c = cases[case]
    want = qp.expected(c["g"], case, direction)
    mb = dict(motion_boundary=qp.CASES[case]["mb"], mb_thres=qp.MB_THRES)
    R = pt.trajectory.run_track_queries(c["xy"], c["t"], **kwargs(c, direction), **mb)
    assert len(R) == len(c["t"]) and R.info["n_traj"] == len(c["t"]) and R.info["chain_mode"] == 5 and R.info["n_points"] == len(want[2])
    assert_matches(R, want, qp.TOL, "%s %s fixture:" % (case, direction))
    # rows per solve (psfm_solve_stats carries none): from the lengths, which are exact
    b, l, o, p = csr(R)
    dirs = {"forward": (False,), "backward": (True,), "both": (False, True)}[direction]
    assert np.array_equal(rows_from_lengths(c["t"], b, l, len(c["flows_f"]), dirs), want[3])
    k = qp.CASES[case]["n_random"]
    i6, i7 = k + 6, k + 7                                   # the two identical queries: identical trajectories
    assert l[i6] == l[i7] and p[o[i6]:o[i6 + 1]].tobytes() == p[o[i7]:o[i7 + 1]].tobytes()
    # two identical calls
    R2 = pt.trajectory.run_track_queries(c["xy"], c["t"], **kwargs(c, direction), **mb)
    b2, l2, o2, p2 = csr(R2)
    assert np.array_equal(b, b2) and np.array_equal(l, l2) and float(np.abs(p - p2).max()) <= qp.ROUNDING
    print("%s %s identical calls bit-identical: %s" % (case, direction, p.tobytes() == p2.tobytes()))
    # the maps from flow_check_device, each direction's in its own orientation
    C = pt.trajectory.run_connect_queries(c["xy"], c["t"], c["flows_f"], c["flows_b"], thres=1.0, direction=direction,
                                          flows_f2=c["flows_f2"], flows_b2=c["flows_b2"], **mb)
    assert C.info["chain_mode"] == 5
    assert_matches(C, want, qp.TOL, "%s %s connect:" % (case, direction))


def composed_engine(pt):
    """qp.engine_np with every piece on the device: psfm_grid_sample for the step and the refs, psfm_optimize_location for the solve."""
    torch = pt.torch
    F = np.float32

    def sample(m, xy):                                        # (H,W) or (H,W,2) map -> (n,) / (n,2) f32
        m = torch.from_numpy(np.ascontiguousarray(m, F))
        m = m.unsqueeze(0) if m.dim() == 2 else m.permute(2, 0, 1)
        out = pt.trajectory.grid_sample(m, xy)
        return out[:, 0] if out.shape[1] == 1 else out

    def engine(xy, t, flows, occ, flows2, occ2, mb=False, mb_thres=None):
        assert not mb
        H, W = flows[0].shape[:2]

        def step(f, p, idx):
            nxt = p + sample(flows[f], p).astype(np.float64)
            oc = sample((np.asarray(occ[f]) != 0).astype(F), p) > F(0.1)
            return nxt, (nxt[:, 0] > 0) & (nxt[:, 0] < W - 1) & (nxt[:, 1] > 0) & (nxt[:, 1] < H - 1) & ~oc

        def refs(p0, flow01, flow02, occ02):
            f01, f02, o02 = sample(flow01, p0), sample(flow02, p0), sample((np.asarray(occ02) != 0).astype(F), p0)
            nrm = np.sqrt(f02[:, 0] * f02[:, 0] + f02[:, 1] * f02[:, 1])
            scale = (F(1.0) - o02) * (nrm < F(20.0)).astype(F)
            return p0 + f01.astype(np.float64), p0 + f02.astype(np.float64), scale.astype(np.float64)

        def solve(uv12, ref1, ref2, scale, flow12):
            out = pt.particlesfm.optimize_location(uv12, ref1, ref2, scale, flow12, len(uv12), W, H)
            return out, pt.particlesfm.optimize_location.last_stats
        return qp.engine_np(xy, t, flows, occ, flows2, occ2, step=step, refs=refs, solve=solve)
    return engine


@pytest.mark.parametrize("case,direction", [("q37x53", "both"), ("q24x30", "forward"), ("q24x30", "backward")])
def test_equals_the_composed_form_on_the_device_to_rounding(pt, cases, case, direction):
    c = cases[case]
    want = qp.track_queries_pc_np(c["xy"], c["t"], engine=composed_engine(pt), **qp.stacks(c, direction))
    R = pt.trajectory.run_track_queries(c["xy"], c["t"], **kwargs(c, direction))
    assert_matches(R, want, qp.ROUNDING, "%s %s composed:" % (case, direction))


@pytest.fixture(scope="module")
def prefix_statement(cases):
    c = cases["q37x53"]
    return lambda n: qp.track_queries_pc_np(c["xy"][:n], c["t"][:n], **qp.stacks(c, "both"))


@pytest.mark.parametrize("n", [1, 64, 65, 257])
def test_prefixes_on_wave_and_block_edges_of_the_compaction(pt, cases, prefix_statement, n):
    c = cases["q37x53"]
    R = pt.trajectory.run_track_queries(c["xy"][:n], c["t"][:n], **kwargs(c, "both"))
    assert_matches(R, prefix_statement(n), qp.TOL, "prefix %d:" % n)


def test_edges_of_the_frame_loop(pt, cases):
    c = cases["q24x30"]
    xy, t = c["xy"], c["t"]
    n = len(c["flows_f"])
    # every query at the last frame: nothing to do forward (length 1, no solve); backward they all start together
    R = pt.trajectory.run_track_queries(xy, np.full(len(t), n, np.int32), **kwargs(c, "forward"))
    assert (R.length == 1).all() and np.array_equal(R.birth, np.full(len(t), n)) and R.info["n_solves"] == 0 and R.xy.tobytes() == xy.tobytes()
    want = qp.track_queries_pc_np(xy, np.full(len(t), n, np.int32), **qp.stacks(c, "both"))
    R = pt.trajectory.run_track_queries(xy, np.full(len(t), n, np.int32), **kwargs(c, "both"))
    assert_matches(R, want, qp.TOL, "all at the last frame, both:")
    assert R.length.max() == n + 1
    # a call in which no frame has a row: queries that start one frame before the end reach two points at most -- no solve, no error
    tl = np.full(len(t), n - 1, np.int32)
    R = pt.trajectory.run_track_queries(xy, tl, **kwargs(c, "forward"))
    P = pt.trajectory.run_track_queries(xy, tl, flows=c["flows_f"], occ=c["occ_f"])
    assert R.info["n_solves"] == 0 and R.info["chain_mode"] == 5 and R.length.max() == 2
    assert all(x.tobytes() == y.tobytes() for x, y in zip(csr(R), csr(P)))
    # ... and one in which SOME frame has none: two queries, the second starting when the first (outside the image) has long ended
    xy2, t2 = np.array([[-5.0, -5.0], [xy[0, 0], xy[0, 1]]]), np.array([0, 2], np.int32)
    want = qp.track_queries_pc_np(xy2, t2, **qp.stacks(c, "forward"))
    R = pt.trajectory.run_track_queries(xy2, t2, **kwargs(c, "forward"))
    assert_matches(R, want, qp.TOL, "a frame with no row:")
    assert R.length[0] == 1
    # one flow: no solve can happen and the stride-2 stacks may be empty (NULL to the library)
    e2, eo = np.zeros((0,) + c["flows_f"].shape[1:], np.float32), np.zeros((0,) + c["occ_f"].shape[1:], bool)
    R = pt.trajectory.run_track_queries(xy, np.minimum(t, 1), flows=c["flows_f"][:1], occ=c["occ_f"][:1], flows_f2=e2, occ_f2=eo)
    P = pt.trajectory.run_track_queries(xy, np.minimum(t, 1), flows=c["flows_f"][:1], occ=c["occ_f"][:1])
    assert R.info["chain_mode"] == 5 and P.info["chain_mode"] == 4 and R.info["n_solves"] == 0
    assert all(x.tobytes() == y.tobytes() for x, y in zip(csr(R), csr(P)))
    # no queries
    R = pt.trajectory.run_track_queries(np.zeros((0, 2)), np.zeros(0, np.int32), **kwargs(c, "both"))
    assert len(R) == 0 and R.n_points == 0 and R.info["chain_mode"] == 5


def test_refusals_leave_the_previous_result_intact_and_consumers_run(pt, cases):
    from point_trajectory.trajectory import result_to_trajectory_set
    from psfm_motion_seg.load_cut_seq import sample_window_device
    from psfm_sfm import matches_from_flow as mff
    torch = pt.torch
    case = "q37x53"
    c = cases[case]
    xy, t = c["xy"], c["t"]
    T, H, W = qp.CASES[case]["T"], qp.CASES[case]["H"], qp.CASES[case]["W"]
    n = T - 1
    ctx = pt.hip.context()
    L, sp = pt.hip.lib(), pt.hip.current_stream_ptr(ctx.device)
    info = pt.trajectory.run_track_queries(xy, t, return_device=True, **kwargs(c, "both"))
    R = pt.trajectory._result_to_host(ctx, info)
    before = csr(R)

    def intact():
        return all(x.tobytes() == y.tobytes() for x, y in zip(before, csr(pt.trajectory._result_to_host(ctx, info))))

    def refused(xy_, t_, **kw):
        with pytest.raises(pt.hip.PsfmError) as e:
            pt.trajectory.run_track_queries(xy_, t_, **kw)
        assert e.value.status == pt.hip.PSFM_ERR_ARG and intact()
        return str(e.value)
    fwd = kwargs(c, "forward")
    for bad in (np.nan, np.inf):
        q = xy.copy()
        q[7, 1] = bad
        q[200, 0] = bad
        assert "query 7 " in refused(q, t, **fwd)
    for bad_t, at in ((-1, 5), (n + 1, len(t) - 1)):
        tt = t.copy()
        tt[at] = bad_t
        assert "query %d " % at in refused(xy, tt, **fwd)
    assert "stack" in refused(xy, t, flows_f2=c["flows_f2"], occ_f2=c["occ_f2"])                       # no stride-1 stack
    assert "stack" in refused(xy, t, flows=c["flows_f"], flows_f2=c["flows_f2"], occ_f2=c["occ_f2"])   # a stack without its maps
    assert "stride-2" in refused(xy, t, flows=c["flows_f"], occ=c["occ_f"], flows_f2=c["flows_f2"])    # a stride-2 stack without its maps
    assert "stride-2" in refused(xy, t, flows=c["flows_f"], occ=c["occ_f"], flows_b=c["flows_b"], occ_b=c["occ_b"],
                                 flows_f2=c["flows_f2"], occ_f2=c["occ_f2"])                          # a direction without its stride-2 stack
    dv = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(device="cuda", dtype=dt)
    ff, of = dv(c["flows_f"], torch.float32), dv(c["occ_f"], torch.uint8)
    f2, o2 = dv(c["flows_f2"], torch.float32), dv(c["occ_f2"], torch.uint8)
    st = L.psfm_track_queries_optimize(ctx.handle, pt.hip.ptr(ff), pt.hip.ptr(of), pt.hip.ptr(f2), pt.hip.ptr(o2), None, None, None, None,
                                       n, H, W, ctypes.c_void_p(16), ctypes.c_void_p(16), 1 << 28, None, sp)
    assert st == pt.hip.PSFM_ERR_ARG and intact()            # n_q beyond a 4 GB slab row: refused on the arguments alone
    keys = torch.zeros(len(t), dtype=torch.int64, device="cuda")
    assert L.psfm_result_keys(ctx.handle, 2, W, pt.hip.ptr(keys), sp) == pt.hip.PSFM_ERR_ARG
    assert b"query" in L.psfm_last_error() and intact()
    # the consumers of a result, unchanged, against the package's host statements fed with the same CSR
    host = R.to_trajectory_set(3)
    dev = result_to_trajectory_set(ctx, pt.hip.TrackInfo(n_traj=len(R), n_points=R.n_points), 3)
    for a, b in zip(host._csr[:5], dev._csr[:5]):
        assert np.array_equal(a, b)
    assert 0 < len(dev._csr[0]) < len(R)
    host.build_invert_indexes()
    want = host.sample_inside_window(list(range(2, 7)), min_length=3, max_num_tracks=10 ** 9)
    ids, raw, _, mask = sample_window_device(ctx, 2, 5, (H, W), (H, W), 10 ** 9)
    assert np.array_equal(ids.cpu().numpy(), np.asarray(want["traj_ids"], np.int32)) and len(want["traj_ids"]) > 50
    assert np.array_equal(raw.cpu().numpy(), np.stack(want["locations"], -1))
    ids_, birth, length, off, pts = host._csr[:5]
    frames = (np.repeat(birth, length) + np.arange(len(pts)) - np.repeat(off[:-1], length)).astype(np.int64)
    want_tables = mff.match_tables_host(off, frames, pts, np.zeros(len(pts), bool), T)
    got_tables = mff.match_tables_device(ctx, T)
    for a, b in zip(got_tables, want_tables):
        assert np.array_equal(a, b)
    assert len(want_tables[5]) > 100


@pytest.mark.parametrize("case,direction", [("q37x53", "both"), ("q24x30", "backward"), ("q48x64_mb", "forward")])
def test_without_stride2_arguments_the_call_is_psfm_track_queries(pt, case, direction):
    ff, fb, of, ob, xy, t, g = qn.load_case(case)
    want = qn.expected(g, case, direction)
    kw = {}
    if direction in ("forward", "both"):
        kw.update(flows=ff, occ=of)
    if direction in ("backward", "both"):
        kw.update(flows_b=fb, occ_b=ob)
    mb = dict(motion_boundary=qn.CASES[case]["mb"], mb_thres=qn.MB_THRES)
    R = pt.trajectory.run_track_queries(xy, t, **kw, **mb)
    assert R.info["chain_mode"] == 4 and R.info["n_solves"] == 0
    b, l, o, p = csr(R)
    assert np.array_equal(b, want[0]) and np.array_equal(l, want[1]) and p.tobytes() == want[2].tobytes()
    C = pt.trajectory.run_connect_queries(xy, t, ff, fb, thres=1.0, direction=direction, **mb)
    assert C.info["chain_mode"] == 4 and np.array(C.xy).tobytes() == want[2].tobytes()
