"""psfm_track_queries_optimize_batch on the GPU (csrc/psfm_query_pc_batch.hip + the multi-problem launch chain of
csrc/psfm_solver_multi.hip) through run_track_queries_pc_batch / run_connect_queries_pc_batch.

Against the REFERENCE (tests/golden/queries_pc.npz through tests/_queries_pc_np.py): births, lengths, the rows, iterations and
termination of every solve exactly, positions within qp.TOL.  Against the SINGLE call on each sequence alone: births, lengths,
offsets, solve statistics and positions byte for byte -- the batch runs the launch chain, the single call (alone on the device) its
resident form, and the two are the same solve bit for bit; should position bits ever differ, the comparison falls back to the single
call with PSFM_PC_PERSIST=0 (the variable is read per call) under the hard bar qp.ROUNDING with exact integers, and says so.
Then the edges of the tables (0, 1, 64, 65, 257 queries; sequences that end early, have no row in some or in every frame, or one
flow and no stride-2 stacks; 64 sequences; a block cap that binds on the device), independence of the companions, determinism, the
census, every refusal with every context untouched, and the consumers of a result on a context of the batch."""
import ctypes

import numpy as np
import pytest

import _queries_pc_np as qp

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
    return {c: qp.load_case(c) for c in qp.CASES}


NAMES = {"flows_f": "flows", "occ_f": "occ"}


def seq_of(case, direction, sel=slice(None), xy=None, t=None):
    """One sequence of a batch: the stacks of a direction under the names run_track_queries uses, and (a cut of) the queries."""
    d = {NAMES.get(k, k): v for k, v in qp.stacks(case, direction).items()}
    d["xy"] = case["xy"][sel] if xy is None else xy
    d["t"] = case["t"][sel] if t is None else t
    return d


def parts(R):
    """Everything the call leaves for a sequence, as bytes-comparable arrays: birth, length, off, xy, the solve statistics."""
    st = np.array([[s[k] for k in ("iterations", "successful_steps", "termination", "dogleg_nonGN")] for s in R.solve_stats], np.int64).reshape(-1, 4)
    cost = np.array([[s["initial_cost"], s["final_cost"]] for s in R.solve_stats], np.float64).reshape(-1, 2)
    return np.array(R.birth), np.array(R.length), np.array(R.off), np.array(R.xy), st, cost


def single(pt, sq, **mb):
    return pt.trajectory.run_track_queries(sq["xy"], sq["t"], **{k: v for k, v in sq.items() if k not in ("xy", "t")}, **mb)


def assert_same_as_single(pt, monkeypatch, R, sq, what, **mb):
    """Byte for byte what run_track_queries leaves on the sequence alone (see the module's docstring for the fallback)."""
    S = single(pt, sq, **mb)
    got, want = parts(R), parts(S)
    assert R.info["n_solves"] == S.info["n_solves"] and R.info["solver_iterations"] == S.info["solver_iterations"], what
    for k in (0, 1, 2, 4):
        assert got[k].tobytes() == want[k].tobytes(), (what, k)
    if got[3].tobytes() == want[3].tobytes() and got[5].tobytes() == want[5].tobytes():
        return
    monkeypatch.setenv("PSFM_PC_PERSIST", "0")
    S0 = single(pt, sq, **mb)
    monkeypatch.delenv("PSFM_PC_PERSIST")
    w0 = parts(S0)
    chain_equal = got[3].tobytes() == w0[3].tobytes() and got[5].tobytes() == w0[5].tobytes()
    err = float(np.abs(got[3] - want[3]).max())
    print("FINDING about the single call: %s differs from its resident form in position bits (max %.3g px); equal to its launch chain: %s"
          % (what, err, chain_equal))
    assert err <= qp.ROUNDING and chain_equal, what


def rows_from_lengths(t, birth, length, n, directions):
    """Rows of every solve that ran, from the result alone (tests/test_gpu_queries_pc.py)."""
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


DIRS = {"forward": (False,), "backward": (True,), "both": (False, True)}


def assert_matches_reference(R, want, t, n, direction, what):
    b, l, o, p = np.array(R.birth), np.array(R.length), np.array(R.off), np.array(R.xy)
    assert np.array_equal(b, want[0]) and np.array_equal(l, want[1]), what
    assert np.array_equal(o, np.concatenate([[0], np.cumsum(l)])) and p.shape == want[2].shape
    err = float(np.abs(p - want[2]).max()) if len(p) else 0.0
    print(what, "max |xy - expected| = %.3g px" % err)
    assert err <= qp.TOL, what
    its = np.array([s["iterations"] for s in R.solve_stats], np.int32)
    term = np.array([s["termination"] for s in R.solve_stats], np.int32)
    assert R.info["chain_mode"] == 7 and R.info["n_solves"] == len(want[3]), what
    assert np.array_equal(its, want[4]) and np.array_equal(term, want[5]), what
    assert R.info["solver_iterations"] == int(want[4].sum())
    assert np.array_equal(rows_from_lengths(t, b, l, n, DIRS[direction]), want[3]), what


@pytest.mark.parametrize("direction", ["forward", "backward", "both"])
def test_two_fixtures_of_two_sizes_and_lengths_in_one_batch(pt, cases, monkeypatch, direction):
    names = ["q37x53", "q24x30"]                       # 8 and 6 flows: one sequence ends while the other goes on
    seqs = [seq_of(cases[c], direction) for c in names]
    Rs = pt.trajectory.run_track_queries_pc_batch(seqs)
    Cs = pt.trajectory.run_connect_queries_pc_batch(
        [dict(xy=cases[c]["xy"], t=cases[c]["t"], **{k: cases[c][k] for k in ("flows_f", "flows_b", "flows_f2", "flows_b2")}) for c in names],
        thres=1.0, direction=direction)
    assert len(Rs) == 2 and len(Cs) == 2
    for c, sq, R, C in zip(names, seqs, Rs, Cs):
        want = qp.expected(cases[c]["g"], c, direction)
        n = len(cases[c]["flows_f"])
        assert len(R) == len(sq["t"]) and R.info["n_traj"] == len(sq["t"]) and R.info["n_points"] == len(want[2])
        assert_matches_reference(R, want, sq["t"], n, direction, "%s %s batch:" % (c, direction))
        assert_matches_reference(C, want, sq["t"], n, direction, "%s %s connect batch:" % (c, direction))
        assert_same_as_single(pt, monkeypatch, R, sq, "%s %s" % (c, direction))


def test_motion_boundary_with_per_sequence_thresholds(pt, cases, monkeypatch):
    c = cases["q48x64_mb"]
    seqs = [seq_of(c, "forward"), seq_of(c, "forward", slice(0, 300))]
    thr = [qp.MB_THRES, 0.1 * qp.MB_THRES]          # (the tenth: eleven of the 300 lengths differ in the NumPy statement)
    Rs = pt.trajectory.run_track_queries_pc_batch(seqs, motion_boundary=True, mb_thres=thr)
    want = qp.expected(c["g"], "q48x64_mb", "forward")
    assert_matches_reference(Rs[0], want, seqs[0]["t"], len(c["flows_f"]), "forward", "q48x64_mb forward batch:")
    for R, sq, v in zip(Rs, seqs, thr):
        assert_same_as_single(pt, monkeypatch, R, sq, "q48x64_mb thres %g" % v, motion_boundary=True, mb_thres=v)
    assert parts(Rs[1])[1].tobytes() != parts(Rs[0])[1][:300].tobytes()       # (the second threshold is the second sequence's own)
    C = pt.trajectory.run_connect_queries_pc_batch(
        [dict(xy=c["xy"], t=c["t"], **{k: c[k] for k in ("flows_f", "flows_b", "flows_f2", "flows_b2")})], direction="forward",
        motion_boundary=True, mb_thres=qp.MB_THRES)
    assert_matches_reference(C[0], want, c["t"], len(c["flows_f"]), "forward", "q48x64_mb forward connect batch:")


@pytest.mark.parametrize("direction", ["forward", "backward"])
def test_cuts_on_the_edges_of_the_tables(pt, cases, monkeypatch, direction):
    c = cases["q37x53"]
    cuts = [1, 64, 0, 65, 257]
    seqs = [seq_of(c, direction, slice(0, n)) for n in cuts]
    Rs = pt.trajectory.run_track_queries_pc_batch(seqs)
    for n, sq, R in zip(cuts, seqs, Rs):
        assert len(R) == n and R.info["chain_mode"] == 7
        assert_same_as_single(pt, monkeypatch, R, sq, "cut %d %s" % (n, direction))
    assert Rs[2].n_points == 0 and Rs[2].info["n_solves"] == 0 and Rs[4].info["n_solves"] > 0


def test_sequences_without_rows_and_with_one_flow(pt, cases, monkeypatch):
    c = cases["q24x30"]
    xy, t = c["xy"], c["t"]
    n = len(c["flows_f"])
    # no frame has a row; some frame has none (the two-query case of the single test); one flow and no stride-2 stacks; a full one
    s_none = seq_of(c, "forward", t=np.full(len(t), n - 1, np.int32))
    ref = qp.expected(c["g"], "q24x30", "forward")
    live = int(np.flatnonzero((t == 2) & (ref[1] >= 4))[0])          # a query of frame 2 that the reference carries over four frames
    s_some = seq_of(c, "forward", xy=np.array([[-5.0, -5.0], [xy[live, 0], xy[live, 1]]]), t=np.array([0, 2], np.int32))
    s_one = dict(xy=xy, t=np.minimum(t, 1).astype(np.int32), flows=c["flows_f"][:1], occ=c["occ_f"][:1])
    s_full = seq_of(c, "forward")
    seqs = [s_none, s_some, s_one, s_full]
    Rs = pt.trajectory.run_track_queries_pc_batch(seqs)
    assert Rs[0].info["n_solves"] == 0 and Rs[0].length.max() == 2
    assert Rs[2].info["n_solves"] == 0 and Rs[2].info["chain_mode"] == 7
    assert 0 < Rs[1].info["n_solves"] < n - 1 and Rs[1].length[0] == 1
    for k, (sq, R) in enumerate(zip(seqs, Rs)):
        if k == 2:   # (without stride-2 arguments the single entry point is psfm_track_queries: empty stacks make it the optimize call)
            e2, eo = np.zeros((0,) + c["flows_f"].shape[1:], np.float32), np.zeros((0,) + c["occ_f"].shape[1:], bool)
            sq = dict(sq, flows_f2=e2, occ_f2=eo)
        assert_same_as_single(pt, monkeypatch, R, sq, "sequence %d" % k)
    want = qp.expected(c["g"], "q24x30", "forward")
    assert_matches_reference(Rs[3], want, t, n, "forward", "q24x30 among sequences without rows:")


def test_sixty_four_sequences_of_small_cuts(pt, cases, monkeypatch):
    c = cases["q24x30"]
    seqs = [seq_of(c, "both", slice(4 * i, 4 * i + 1 + i % 7)) for i in range(64)]
    ctxs, infos = pt.trajectory.run_track_queries_pc_batch(seqs, return_device=True)
    assert len(ctxs) == 64
    Rs = [pt.trajectory._result_to_host(x, i) for x, i in zip(ctxs, infos)]
    for i, (sq, R) in enumerate(zip(seqs, Rs)):
        assert len(R) == 1 + i % 7
        assert_same_as_single(pt, monkeypatch, R, sq, "small cut %d" % i)
    assert sum(R.info["n_solves"] for R in Rs) > 64


def test_block_cap_of_the_contexts_binds_on_the_device(pt, cases, monkeypatch):
    """Contexts with a resident budget of 2 blocks and 700 queries that start together: solves of more than 512 rows, whose three
    chunks go to two blocks (pc_multi_blocks caps on the device what pc_blocks caps on the host)."""
    c = cases["q37x53"]
    H, W = qp.CASES["q37x53"]["H"], qp.CASES["q37x53"]["W"]
    rng = np.random.default_rng(77)
    xy = rng.uniform([W * 0.3, H * 0.3], [W * 0.7, H * 0.7], size=(700, 2))
    sq = seq_of(c, "forward", xy=xy, t=np.zeros(700, np.int32))
    ctxs = pt.hip.batch_contexts(2)
    try:
        for x in ctxs:
            x.set_resident_budget(2)
        Rs = pt.trajectory.run_track_queries_pc_batch([sq, seq_of(c, "forward", slice(0, 100))])
        rows = rows_from_lengths(sq["t"], Rs[0].birth, Rs[0].length, len(c["flows_f"]), (False,))
        print("rows per solve:", rows)
        assert rows.max() > 2 * 256, "the cap of 2 blocks does not bind on this input"
        assert_same_as_single(pt, monkeypatch, Rs[0], sq, "700 queries under a budget of 2 blocks")
    finally:
        for x in ctxs:
            x.set_resident_budget(0)
    want = qp.track_queries_pc_np(sq["xy"], sq["t"], **qp.stacks(c, "forward"))
    assert np.array_equal(Rs[0].birth, want[0]) and np.array_equal(Rs[0].length, want[1])
    assert float(np.abs(np.array(Rs[0].xy) - want[2]).max()) <= qp.TOL
    assert np.array_equal(rows, want[3]) and np.array_equal([s["iterations"] for s in Rs[0].solve_stats], want[4])


def test_a_sequence_does_not_depend_on_its_companions_and_calls_repeat(pt, cases):
    a, b = cases["q37x53"], cases["q24x30"]
    sq = seq_of(a, "both")
    alone = pt.trajectory.run_track_queries_pc_batch([sq])[0]
    among = pt.trajectory.run_track_queries_pc_batch([seq_of(b, "both"), seq_of(b, "both", slice(0, 70)), sq, seq_of(a, "both", slice(5, 200)),
                                                      seq_of(b, "both", slice(100, 101))])
    again = pt.trajectory.run_track_queries_pc_batch([seq_of(b, "both"), seq_of(b, "both", slice(0, 70)), sq, seq_of(a, "both", slice(5, 200)),
                                                      seq_of(b, "both", slice(100, 101))])
    assert alone.info["n_solves"] > 8
    for x, y in zip(parts(alone), parts(among[2])):
        assert x.tobytes() == y.tobytes()
    for R1, R2 in zip(among, again):
        for x, y in zip(parts(R1), parts(R2)):
            assert x.tobytes() == y.tobytes()


def test_census_does_not_grow_with_the_batch(pt, cases):
    """launches_fixed and host_syncs of 16 copies of a sequence are those of one copy.  host_syncs against the single call: the single
    call synchronises once for the refusals, twice in its finish, and per step k >= 1 of a direction once for the row count plus, with
    rows, at least once in the solve's poll and once behind its write-back: 3 + sum(1 + 2 [rows]) is a LOWER bound of its count.  The
    batch synchronises three times around the loop and once per poll."""
    c = cases["q24x30"]
    sq = seq_of(c, "both")
    n = len(c["flows_f"])
    own = pt.hip.context()
    R1 = pt.trajectory.run_track_queries_pc_batch([sq])[0]
    one = own.query_pc_batch_census()
    R16 = pt.trajectory.run_track_queries_pc_batch([sq] * 16)
    many = own.query_pc_batch_census()
    print("one copy:", one, " sixteen copies:", many)
    assert many["launches_fixed"] == one["launches_fixed"] and many["host_syncs"] == one["host_syncs"]
    assert many["launches_iter"] == one["launches_iter"] >= 4 * R1.info["n_solves"]
    for R in R16:
        for x, y in zip(parts(R), parts(R1)):
            assert x.tobytes() == y.tobytes()
    steps_with_solve = 2 * (n - 1)
    single_lower_bound = 3 + steps_with_solve + 2 * R1.info["n_solves"]
    print("host synchronisations: batch %d, single call at least %d" % (one["host_syncs"], single_lower_bound))
    assert one["host_syncs"] >= 3 + steps_with_solve and one["host_syncs"] <= single_lower_bound


def test_refusals_leave_every_context_untouched(pt, cases):
    a, b = cases["q37x53"], cases["q24x30"]
    good = [seq_of(a, "forward"), seq_of(b, "forward"), seq_of(a, "forward", slice(0, 50))]
    ctxs, infos = pt.trajectory.run_track_queries_pc_batch(good, return_device=True)
    before = [parts(pt.trajectory._result_to_host(x, i)) for x, i in zip(ctxs, infos)]
    assert all(len(p[4]) > 0 for p in before)

    def intact():
        now = [parts(pt.trajectory._result_to_host(x, i)) for x, i in zip(ctxs, infos)]
        return all(u.tobytes() == v.tobytes() for p, q in zip(before, now) for u, v in zip(p, q))

    def refused(seqs, **kw):
        with pytest.raises(pt.hip.PsfmError) as e:
            pt.trajectory.run_track_queries_pc_batch(seqs, **kw)
        assert e.value.status == pt.hip.PSFM_ERR_ARG and intact()
        assert "psfm_track_queries_optimize_batch" in str(e.value)
        return str(e.value)

    def edit(k, **kw):
        return [dict(s, **kw) if i == k else s for i, s in enumerate(good)]
    # the queries: the lowest bad sequence, its lowest bad query
    for bad in (np.nan, np.inf):
        q1, q2 = b["xy"].copy(), a["xy"][:50].copy()
        q1[7, 1] = bad
        q1[200, 0] = bad
        q2[3, 0] = bad
        msg = refused([good[0], dict(good[1], xy=q1), dict(good[2], xy=q2)])
        assert "sequence 1:" in msg and "query 7 " in msg
    for bad_t, at in ((-1, 5), (len(b["flows_f"]) + 1, len(b["t"]) - 1)):
        tt = b["t"].copy()
        tt[at] = bad_t
        msg = refused(edit(1, t=tt))
        assert "sequence 1:" in msg and "query %d " % at in msg
    # the stride-2 stacks: a direction whose stride-1 stack lacks them (the lowest such sequence), a stack without its maps, stacks of a
    # direction that is not tracked
    no2 = lambda s: {k: v for k, v in s.items() if k not in ("flows_f2", "occ_f2")}
    msg = refused([good[0], no2(good[1]), no2(good[2])])
    assert "sequence 1:" in msg and "stride-2" in msg
    msg = refused([{k: v for k, v in s.items() if k != "occ_f2"} for s in good])
    assert "stride-2" in msg
    msg = refused(edit(2, occ_f2=None))
    assert "sequence 2:" in msg and "stride-2" in msg
    msg = refused([dict(s, flows_b2=c["flows_b2"], occ_b2=c["occ_b2"]) for s, c in zip(good, (a, b, a))])
    assert "stride-2" in msg
    # the arguments of the batch itself, through the library: a context given twice, a bad frame size, contexts that disagree about the
    # motion-boundary option
    L, vp = pt.hip.lib(), ctypes.c_void_p
    dv = lambda x, dt: pt.torch.from_numpy(np.ascontiguousarray(x)).to(device="cuda", dtype=dt)
    f32, u8 = pt.torch.float32, pt.torch.uint8
    dev = [[dv(s[k], dt) for k, dt in (("flows", f32), ("occ", u8), ("flows_f2", f32), ("occ_f2", u8))] for s in good[:2]]
    qx = [dv(s["xy"], pt.torch.float64) for s in good[:2]]
    qt = [dv(s["t"], pt.torch.int32) for s in good[:2]]

    def call(handles, hs=None, mb=None):
        arr = lambda k: (vp * 2)(*[d[k].data_ptr() for d in dev])
        nf = (ctypes.c_int * 2)(*[len(s["flows"]) for s in good[:2]])
        hh = (ctypes.c_int * 2)(*(hs or [s["flows"].shape[1] for s in good[:2]]))
        ww = (ctypes.c_int * 2)(*[s["flows"].shape[2] for s in good[:2]])
        nq = (ctypes.c_int64 * 2)(*[len(s["t"]) for s in good[:2]])
        return L.psfm_track_queries_optimize_batch((vp * 2)(*handles), 2, arr(0), arr(1), arr(2), arr(3), None, None, None, None, nf, hh, ww,
                                                   (vp * 2)(*[x.data_ptr() for x in qx]), (vp * 2)(*[x.data_ptr() for x in qt]), nq, None,
                                                   pt.hip.current_stream_ptr(ctxs[0].device))
    assert call([ctxs[0].handle, ctxs[0].handle]) == pt.hip.PSFM_ERR_ARG and b"given twice" in L.psfm_last_error() and intact()
    assert call([ctxs[0].handle, ctxs[1].handle], hs=[37, 0]) == pt.hip.PSFM_ERR_ARG and b"sequence 1" in L.psfm_last_error() and intact()
    try:
        ctxs[1].set_motion_boundary(True, 0.02)
        assert call([ctxs[0].handle, ctxs[1].handle]) == pt.hip.PSFM_ERR_ARG and b"motion-boundary" in L.psfm_last_error() and intact()
    finally:
        ctxs[1].set_motion_boundary(False)
    assert call([ctxs[0].handle, ctxs[1].handle]) == pt.hip.PSFM_OK          # (and the same arguments, unedited, are accepted)
    # run_track_queries_batch keeps refusing stride-2 stacks
    with pytest.raises(ValueError):
        pt.trajectory.run_track_queries_batch(good)


def test_consumers_of_a_result_on_a_context_of_the_batch(pt, cases):
    from point_trajectory.trajectory import result_to_trajectory_set
    from psfm_motion_seg.load_cut_seq import sample_window_device
    from psfm_sfm import matches_from_flow as mff
    torch = pt.torch
    case = "q37x53"
    c = cases[case]
    T, H, W = qp.CASES[case]["T"], qp.CASES[case]["H"], qp.CASES[case]["W"]
    ctxs, infos = pt.trajectory.run_track_queries_pc_batch([seq_of(cases["q24x30"], "both"), seq_of(c, "both")], return_device=True)
    ctx, info = ctxs[1], infos[1]
    R = pt.trajectory._result_to_host(ctx, info)
    L, sp = pt.hip.lib(), pt.hip.current_stream_ptr(ctx.device)
    keys = torch.zeros(len(R), dtype=torch.int64, device="cuda")
    assert L.psfm_result_keys(ctx.handle, 2, W, pt.hip.ptr(keys), sp) == pt.hip.PSFM_ERR_ARG and b"query" in L.psfm_last_error()
    host = R.to_trajectory_set(3)
    dev = result_to_trajectory_set(ctx, pt.hip.TrackInfo(n_traj=len(R), n_points=R.n_points), 3)
    for x, y in zip(host._csr[:5], dev._csr[:5]):
        assert np.array_equal(x, y)
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
    for x, y in zip(got_tables, want_tables):
        assert np.array_equal(x, y)
    assert len(want_tables[5]) > 100
