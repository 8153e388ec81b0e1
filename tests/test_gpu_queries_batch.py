"""psfm_track_queries_batch on the GPU (csrc/psfm_query_batch.hip) through run_track_queries_batch / run_connect_queries_batch: the
fixtures of tests/golden/queries.npz (the REFERENCE's own functions) through a batch of two frame sizes, bit for bit; every context
byte-equal to psfm_track_queries on its sequence alone -- at the wave and block edges, with an empty sequence, with 64 sequences,
with per-sequence motion-boundary thresholds; the census; the consumers of a result on a batch result; the refusals."""
import ctypes

import numpy as np
import pytest

import _queries_np as qn

pytestmark = pytest.mark.gpu

BATCHED = 6         # info.chain_mode of psfm_track_queries_batch


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


def assert_rows(R, want):
    b, l, o, p = csr(R)
    assert np.array_equal(b, want[0]) and np.array_equal(l, want[1])
    assert p.shape == want[2].shape and p.tobytes() == want[2].tobytes()
    assert np.array_equal(o, np.concatenate([[0], np.cumsum(l)]))


def same_bytes(A, B):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(csr(A), csr(B)))


def seq_of(case, direction, sel=None):
    """A sequence of a batch: the stacks of a fixture in the directions asked for, all its queries or the subset `sel`."""
    ff, fb, of, ob, xy, t, g = case
    sel = np.arange(len(t)) if sel is None else np.asarray(sel, np.int64)
    sq = dict(xy=xy[sel], t=t[sel])
    if direction in ("forward", "both"):
        sq.update(flows=ff, occ=of)
    if direction in ("backward", "both"):
        sq.update(flows_b=fb, occ_b=ob)
    return sq


def single(pt, sq, **kw):
    return pt.trajectory.run_track_queries(sq["xy"], sq["t"], **{k: v for k, v in sq.items() if k not in ("xy", "t")}, **kw)


@pytest.mark.parametrize("direction", ["forward", "backward", "both"])
def test_reference_fixtures_through_the_batch(pt, cases, direction):
    """[q37x53, q24x30]: 8 and 6 flows, two frame sizes, 321 queries each."""
    names = ["q37x53", "q24x30"]
    R = pt.trajectory.run_track_queries_batch([seq_of(cases[c], direction) for c in names])
    assert len(R) == 2
    for r, c in zip(R, names):
        want = qn.expected(cases[c][6], c, direction)
        assert_rows(r, want)
        assert r.info["chain_mode"] == BATCHED and r.info["n_traj"] == len(want[0]) == 321 and r.info["n_points"] == len(want[2])


@pytest.mark.parametrize("direction", ["forward", "backward", "both"])
def test_reference_fixtures_through_connect_queries_batch(pt, cases, direction):
    """... with the maps of each direction from flow_check_device in that direction's orientation."""
    names = ["q37x53", "q24x30"]
    seqs = [dict(xy=cases[c][4], t=cases[c][5], flows_f=cases[c][0], flows_b=cases[c][1]) for c in names]
    R = pt.trajectory.run_connect_queries_batch(seqs, thres=1.0, direction=direction)
    for r, c in zip(R, names):
        want = qn.expected(cases[c][6], c, direction)
        assert_rows(r, want)
        assert r.info["chain_mode"] == BATCHED and r.info["n_points"] == len(want[2])


@pytest.mark.parametrize("direction", ["forward", "backward"])
def test_motion_boundary_with_one_threshold_per_sequence(pt, cases, direction):
    case = cases["q48x64_mb"]
    want = qn.expected(case[6], "q48x64_mb", direction)
    first = np.arange(65)
    seqs = [seq_of(case, direction), seq_of(case, direction, first)]
    R = pt.trajectory.run_track_queries_batch(seqs, motion_boundary=True, mb_thres=[qn.MB_THRES, qn.MB_THRES])
    assert_rows(R[0], want)
    assert_rows(R[1], rows_of(*want, first))
    alone = single(pt, seqs[1], motion_boundary=True, mb_thres=0.05)
    R = pt.trajectory.run_track_queries_batch(seqs, motion_boundary=True, mb_thres=[qn.MB_THRES, 0.05])
    assert_rows(R[0], want)
    assert same_bytes(R[1], alone)
    # 0.02 and 0.05 end the same steps on this sequence (tests/_queries_np.py says so); 0.001 ends more, forward and backward
    fine = single(pt, seqs[1], motion_boundary=True, mb_thres=0.001)
    R = pt.trajectory.run_track_queries_batch(seqs, motion_boundary=True, mb_thres=[qn.MB_THRES, 0.001])
    assert_rows(R[0], want)
    assert same_bytes(R[1], fine) and R[1].n_points < alone.n_points
    off = pt.trajectory.run_track_queries_batch(seqs)          # the option is off again in the batch contexts
    assert same_bytes(off[0], single(pt, seqs[0])) and same_bytes(off[1], single(pt, seqs[1]))


def test_byte_equal_to_the_single_call_at_the_edges(pt, cases):
    """5 sequences cut from q37x53 with 1, 63, 0, 256 and 257 queries, both directions; the tail holds the hand-placed queries."""
    case = cases["q37x53"]
    Q = len(case[5])
    sels = [np.array([Q - 14]), np.arange(Q - 63, Q), np.zeros(0, np.int64), np.arange(Q - 256, Q), np.arange(0, 257)]
    seqs = [seq_of(case, "both", s) for s in sels]
    want = [single(pt, sq) for sq in seqs]
    R = pt.trajectory.run_track_queries_batch(seqs)
    fixture = qn.expected(case[6], "q37x53", "both")
    for r, w, s in zip(R, want, sels):
        assert same_bytes(r, w) and len(r) == len(s) and r.info["chain_mode"] == BATCHED
        assert_rows(r, rows_of(*fixture, s))
    assert R[2].info["n_traj"] == 0 and R[2].info["n_points"] == 0 and np.array_equal(R[2].off, [0])


def test_a_batch_without_any_query_gives_empty_results(pt, cases):
    none = np.zeros(0, np.int64)
    R = pt.trajectory.run_track_queries_batch([seq_of(cases[c], "both", none) for c in ("q37x53", "q24x30", "q37x53")])
    for r in R:
        assert len(r) == 0 and r.n_points == 0 and np.array_equal(r.off, [0]) and r.info["chain_mode"] == BATCHED
    assert pt.hip.context().query_batch_census()["host_syncs"] == 2       # nothing to validate


def test_64_sequences_and_the_census(pt, cases):
    case = cases["q24x30"]
    Q = len(case[5])
    sizes = [(1, 64, 65, 321)[i % 4] for i in range(64)]
    sels = [(np.arange(n) + 5 * i) % Q if n < Q else np.arange(Q) for i, n in enumerate(sizes)]
    seqs = [seq_of(case, "both", s) for s in sels]
    fixture = qn.expected(case[6], "q24x30", "both")
    alone = [single(pt, sq) for sq in seqs]
    R = pt.trajectory.run_track_queries_batch(seqs)
    census64 = pt.hip.context().query_batch_census()
    R2 = pt.trajectory.run_track_queries_batch(seqs)
    for i in range(64):
        assert same_bytes(R[i], alone[i]) and same_bytes(R[i], R2[i]), i
        assert_rows(R[i], rows_of(*fixture, sels[i]))
    pt.trajectory.run_track_queries_batch(seqs[:2])
    census2 = pt.hip.context().query_batch_census()
    print(census64, census2)
    assert census64 == census2 and census64["host_syncs"] == 3 and census64["launches"] > 0


def test_more_than_64_sequences_are_cut_into_groups(pt, cases):
    case = cases["q24x30"]
    seqs = [seq_of(case, "forward", np.arange(3) + i) for i in range(66)]
    R = pt.trajectory.run_track_queries_batch(seqs)
    fixture = qn.expected(case[6], "q24x30", "forward")
    assert len(R) == 66
    for i in (0, 63, 64, 65):
        assert_rows(R[i], rows_of(*fixture, np.arange(3) + i))
    with pytest.raises(ValueError):
        pt.trajectory.run_track_queries_batch(seqs, return_device=True)


def test_consumers_work_on_a_batch_result(pt, cases):
    """psfm_result_filter_batch + psfm_traj_to_matches_batch over the contexts of a batch, and sample_window_device on each: the
    bytes they give after the single calls."""
    from psfm_motion_seg.load_cut_seq import sample_window_device
    from psfm_sfm import matches_from_flow as mff
    torch = pt.torch
    names = ["q37x53", "q24x30"]
    seqs = [seq_of(cases[c], "both") for c in names]
    ctx0 = pt.hip.context()
    want = []
    for c, sq in zip(names, seqs):
        T, H, W = qn.CASES[c]["T"], qn.CASES[c]["H"], qn.CASES[c]["W"]
        single(pt, sq, return_device=True)
        win = [x.cpu().numpy() for x in sample_window_device(ctx0, 2, 4, (H, W), (H, W), 10 ** 9) if x is not None]
        want.append((mff.match_tables_device(ctx0, T), win))
    ctxs, infos = pt.trajectory.run_track_queries_batch(seqs, return_device=True)
    assert ctxs[0] is ctx0 and all(i.chain_mode == BATCHED and i.n_traj == 321 for i in infos)
    tables = mff.match_tables_batch_device(ctxs, [qn.CASES[c]["T"] for c in names])
    L, sp = pt.hip.lib(), pt.hip.current_stream_ptr(ctx0.device)
    for c, ctx, got, (want_tables, want_win) in zip(names, ctxs, tables, want):
        H, W = qn.CASES[c]["H"], qn.CASES[c]["W"]
        assert len(want_tables[5]) > 100
        for a, b in zip(got, want_tables):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
        win = [x.cpu().numpy() for x in sample_window_device(ctx, 2, 4, (H, W), (H, W), 10 ** 9) if x is not None]
        assert len(win[0]) > 50 and all(a.tobytes() == b.tobytes() for a, b in zip(win, want_win))
        keys = torch.zeros(321, dtype=torch.int64, device="cuda")
        assert L.psfm_result_keys(ctx.handle, 2, W, pt.hip.ptr(keys), sp) == pt.hip.PSFM_ERR_ARG      # no birth grid index in a query result
        assert b"query" in L.psfm_last_error()


def test_refusals_leave_every_context_intact(pt, cases):
    torch = pt.torch
    ca, cb = cases["q37x53"], cases["q24x30"]
    ctxs = pt.hip.batch_contexts(2)
    L, sp = pt.hip.lib(), pt.hip.current_stream_ptr(ctxs[0].device)
    vp = ctypes.c_void_p
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(device="cuda", dtype=dt)
    # a known result in each context, from single calls
    before, infos = [], []
    for ctx, case in zip(ctxs, (cb, ca)):
        info = pt.hip.TrackInfo()
        keep = [dev(case[0], torch.float32), dev(case[2], torch.uint8), dev(case[4], torch.float64), dev(case[5], torch.int32)]
        pt.hip.check(L.psfm_track_queries(ctx.handle, pt.hip.ptr(keep[0]), pt.hip.ptr(keep[1]), None, None, len(case[0]), case[0].shape[1],
                                          case[0].shape[2], pt.hip.ptr(keep[2]), pt.hip.ptr(keep[3]), len(case[5]), ctypes.byref(info), sp))
        infos.append(info)
        before.append(csr(pt.trajectory._result_to_host(ctx, info)))
        assert info.chain_mode == 4 and info.n_points > 321

    def intact():
        return all(x.tobytes() == y.tobytes() for ctx, info, was in zip(ctxs, infos, before)
                   for x, y in zip(was, csr(pt.trajectory._result_to_host(ctx, info))))

    # the batch: sequence 0 = q37x53, sequence 1 = q24x30, forward
    stacks = [(dev(c[0], torch.float32), dev(c[2], torch.uint8)) for c in (ca, cb)]
    nfl, hs, ws = [len(c[0]) for c in (ca, cb)], [c[0].shape[1] for c in (ca, cb)], [c[0].shape[2] for c in (ca, cb)]

    def call(handles, n_seq, xys, ts, flows=True, occ=True):
        n = len(xys)
        q_xy, q_t = [dev(a, torch.float64) for a in xys], [dev(a, torch.int32) for a in ts]
        arr = lambda ptrs: (vp * max(n, 1))(*ptrs)
        st = L.psfm_track_queries_batch((vp * len(handles))(*handles), n_seq,
                                        arr([s[0].data_ptr() for s in stacks[:n]]) if flows else None,
                                        arr([s[1].data_ptr() for s in stacks[:n]]) if occ else None, None, None,
                                        (ctypes.c_int * 2)(*nfl), (ctypes.c_int * 2)(*hs), (ctypes.c_int * 2)(*ws),
                                        arr([a.data_ptr() for a in q_xy]), arr([a.data_ptr() for a in q_t]),
                                        (ctypes.c_int64 * max(n, 1))(*[len(a) for a in ts]), None, sp)
        torch.cuda.synchronize()
        return st, L.psfm_last_error().decode()
    h2 = [c.handle for c in ctxs]
    xys, ts = [ca[4].copy(), cb[4].copy()], [ca[5].copy(), cb[5].copy()]
    xys[1][7, 0] = np.nan
    ts[0][300] = nfl[0] + 1
    ts[0][310] = -1
    st, msg = call(h2, 2, xys, ts)
    assert st == pt.hip.PSFM_ERR_ARG and "sequence 0" in msg and "query 300 " in msg and intact()
    ts[0] = ca[5].copy()
    st, msg = call(h2, 2, xys, ts)                                              # ... and sequence 1 alone is found too
    assert st == pt.hip.PSFM_ERR_ARG and "sequence 1" in msg and "query 7 " in msg and intact()
    good_xy, good_t = [ca[4], cb[4]], [ca[5], cb[5]]
    st, msg = call([h2[0], h2[0]], 2, good_xy, good_t)                          # a repeated context
    assert st == pt.hip.PSFM_ERR_ARG and "twice" in msg and intact()
    ctxs[1].set_motion_boundary(True, 0.02)                                    # contexts that disagree about the motion boundary
    try:
        st, msg = call(h2, 2, good_xy, good_t)
    finally:
        ctxs[1].set_motion_boundary(False)
    assert st == pt.hip.PSFM_ERR_ARG and "motion-boundary" in msg and intact()
    st, msg = call(h2, 2, good_xy, good_t, occ=False)                           # a stack without its maps
    assert st == pt.hip.PSFM_ERR_ARG and "stack" in msg and intact()
    st, msg = call(h2, 2, good_xy, good_t, flows=False, occ=False)              # no direction
    assert st == pt.hip.PSFM_ERR_ARG and "stack" in msg and intact()
    st, msg = call(h2, 0, good_xy, good_t)
    assert st == pt.hip.PSFM_ERR_ARG and "n_seq=0" in msg and intact()
    st, msg = call(h2, 65, good_xy, good_t)
    assert st == pt.hip.PSFM_ERR_ARG and "n_seq=65" in msg and intact()
    with pytest.raises(ValueError):                                             # sequences that give different directions
        pt.trajectory.run_track_queries_batch([seq_of(ca, "forward"), seq_of(cb, "both")])
    with pytest.raises(ValueError, match="run_track_queries"):                  # the stride-2 form is out of scope
        pt.trajectory.run_track_queries_batch([dict(seq_of(ca, "forward"), flows_f2=ca[0][:-1], occ_f2=ca[2][:-1])])
    assert intact()
    st, msg = call(h2, 2, good_xy, good_t)                                      # ... and the same call, unbroken, goes through
    assert st == pt.hip.PSFM_OK
