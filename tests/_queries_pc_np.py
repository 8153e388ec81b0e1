"""NumPy statement of psfm_track_queries_optimize -- caller-given points carried through a flow stack by the body of
track_optimize.py:37-50: one step of tests/_motion_boundary_np.step_np per frame on the active queries, then, from the second frame
on, ONE joint stride-2 path-consistency solve (oracle.optimize_location, the C restatement of trajectory_optimize.cpp:30-96) over
the queries that hold three positions, rows in query order -- and the names of its fixtures
(tests/golden/make_queries_pc_golden.py -> tests/golden/queries_pc.npz).  Pinned to the reference's fixtures by
tests/test_queries_pc_host.py, beside the header the kernels compile (particle-sfm_amd/csrc/psfm_query_pc.h)."""
import numpy as np

import psfm_synth
from _common import golden, input_hash
from _motion_boundary_np import SEQ_SYNTH, motion_boundary_np, sample_np, step_np
import _queries_np as qn

F = np.float32
FIXTURE = "queries_pc"
MB_THRES = qn.MB_THRES
TOL = 1e-4            # px: the project's position tolerance against the oracle (TOL of tests/test_gpu_solver.py)
ROUNDING = 1e-9       # px: "to rounding" between two device forms of the same solve (tests/test_gpu_solver.py)
# case -> frames, size, seed of the flows, random queries, kill rule, directions.  The shapes, seeds and queries of tests/_queries_np.py,
# the flows with their stride-2 stacks.  qseed: the seed of the random queries when the default (1000 + seed) misses a condition of the
# generator
CASES = {
    "q37x53": dict(T=9, H=37, W=53, seed=5, n_random=300, mb=False, dirs=("forward", "backward", "both"), qseed=None),
    "q24x30": dict(T=7, H=24, W=30, seed=7, n_random=300, mb=False, dirs=("forward", "backward", "both"), qseed=None),
    "q48x64_mb": dict(T=9, H=48, W=64, seed=3, n_random=600, mb=True, dirs=("forward",), qseed=None),
}
CASE_DIRS = [(c, d) for c, v in CASES.items() for d in v["dirs"]]


def synth(case):
    c = CASES[case]
    return psfm_synth.synth_realistic(c["T"], c["H"], c["W"], seed=c["seed"], stride2=True, **dict(psfm_synth.REALISTIC, **SEQ_SYNTH))


def make_queries(case):
    """The queries of tests/_queries_np.make_queries (random ones, then the hand-placed list), the random ones from `qseed` if given."""
    c = CASES[case]
    xy, t = qn.make_queries(case)
    if c["qseed"] is not None:
        H, W, n = c["H"], c["W"], c["T"] - 1
        rng = np.random.default_rng(c["qseed"])
        xy[:c["n_random"]] = rng.uniform([-1.0, -1.0], [float(W), float(H)], size=(c["n_random"], 2))
        t[:c["n_random"]] = rng.integers(0, n + 1, size=c["n_random"])
    return xy, t


def load_case(case):
    """dict: the four flow stacks re-synthesised from the seed (checked against the fixture's hash), their occlusion maps, xy, t, g."""
    g = golden(FIXTURE)
    d = synth(case)
    assert input_hash(d) == str(g[case + "__input_hash"]), "psfm_synth.synth_realistic no longer reproduces this fixture's inputs"
    out = {k: np.stack(d[k]) for k in ("flows_f", "flows_b", "flows_f2", "flows_b2")}
    out.update({k: g[case + "__" + k] for k in ("occ_f", "occ_b", "occ_f2", "occ_b2", "xy", "t")})
    out["g"] = g
    return out


def expected(g, case, direction):
    """birth, length, xy, rows per solve, iterations per solve, termination per solve."""
    return tuple(g["%s__%s_%s" % (case, direction, k)] for k in ("birth", "length", "xy", "rows", "iterations", "termination"))


def stacks(case, direction):
    """The arguments of a direction as track_queries_pc_np (and, renamed, run_track_queries) takes them."""
    kw = {}
    if direction in ("forward", "both"):
        kw.update(flows_f=case["flows_f"], occ_f=case["occ_f"], flows_f2=case["flows_f2"], occ_f2=case["occ_f2"])
    if direction in ("backward", "both"):
        kw.update(flows_b=case["flows_b"], occ_b=case["occ_b"], flows_b2=case["flows_b2"], occ_b2=case["occ_b2"])
    return kw


def pc_refs_np(p0, flow01, flow02, occ02):
    """ref1, ref2 (n,2) f64 and scale (n,) f64 from p0: trajectory.py:173-183 -- the fp32 sampler on flow01, flow02 and occ02, the
    norm as sqrt(u*u + v*v) and the product in fp32 (pc_refs of psfm_pc_tracks.h, psfm_query_pc_refs of psfm_query_pc.h)."""
    p0 = np.asarray(p0, np.float64).reshape(-1, 2)
    f01 = np.stack([sample_np(flow01[..., 0], p0), sample_np(flow01[..., 1], p0)], 1)
    f02 = np.stack([sample_np(flow02[..., 0], p0), sample_np(flow02[..., 1], p0)], 1)
    o02 = sample_np((np.asarray(occ02) != 0).astype(F), p0)
    with np.errstate(all="ignore"):
        nrm = np.sqrt(f02[:, 0] * f02[:, 0] + f02[:, 1] * f02[:, 1])
        scale = (F(1.0) - o02) * (nrm < F(20.0)).astype(F)
    assert f01.dtype == F and f02.dtype == F and scale.dtype == F
    return p0 + f01.astype(np.float64), p0 + f02.astype(np.float64), scale.astype(np.float64)


def _solve(uv12, ref1, ref2, scale, flow12):
    from oracle import oracle
    out, st = oracle.optimize_location(uv12, ref1, ref2, scale, flow12, return_stats=True)
    return out, st


def engine_np(xy, t, flows, occ, flows2, occ2, mb=False, mb_thres=MB_THRES, solve=_solve, step=None, log=None, refs=None):
    """The forward engine on lists of maps (the backward direction runs it on the time-reversed lists).  Returns (pts, stats): per query
    the list of its points in the order they were reached (the query first); per solve that ran dict(frame, rows, iterations,
    termination).  step(f, positions, query indices) -> (next, alive) replaces step_np, refs(p0, flow01, flow02, occ02) pc_refs_np and
    solve optimize_location (the composed form on the device: tests/test_gpu_queries_pc.py); log: a list that receives per frame
    dict(f, idx, alive, owner, uv12, ref1, ref2, scale)."""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    t = np.asarray(t).astype(np.int64)
    n = len(flows)
    pts = [[p.copy()] for p in xy]
    stats = []
    if step is None:
        masks = [motion_boundary_np(f, mb_thres) if mb else np.zeros(f.shape[:2], bool) for f in flows]
        step = lambda f, p, idx: step_np(p, flows[f], occ[f], masks[f], "mb" if mb else "shipped")
    for f in range(n):
        # active: the tail is at frame f (t <= f and alive so far); in query order
        idx = np.array([q for q in range(len(t)) if t[q] + len(pts[q]) - 1 == f], np.int64)
        entry = dict(f=f, idx=idx, alive=np.zeros(0, bool), owner=np.zeros(0, np.int64))
        if log is not None:
            log.append(entry)
        if len(idx) == 0:
            continue
        nxt, alive = step(f, np.array([pts[q][-1] for q in idx]), idx)
        alive = np.asarray(alive) != 0
        entry["alive"] = alive
        for k, q in enumerate(idx):
            if alive[k]:
                pts[q].append(np.array(nxt[k], np.float64))
        if f < 1:
            continue
        owner = np.array([q for k, q in enumerate(idx) if alive[k] and len(pts[q]) >= 3], np.int64)
        entry["owner"] = owner
        if len(owner) == 0:
            continue                                     # no row: no solve
        p0 = np.array([pts[q][-3] for q in owner])
        uv12 = np.array([np.concatenate([pts[q][-2], pts[q][-1]]) for q in owner])
        ref1, ref2, scale = (refs or pc_refs_np)(p0, flows[f - 1], flows2[f - 1], occ2[f - 1])
        entry.update(uv12=uv12, ref1=ref1, ref2=ref2, scale=scale)
        out, st = solve(uv12, ref1, ref2, scale, flows[f])
        stats.append(dict(frame=f, rows=len(owner), iterations=int(st["iterations"]), termination=int(st["termination"])))
        for k, q in enumerate(owner):
            pts[q][-2] = np.array(out[k, :2], np.float64)
            pts[q][-1] = np.array(out[k, 2:], np.float64)
    return pts, stats


def reversed_direction(t, flows_b, occ_b, flows_b2, occ_b2):
    """The backward direction as a forward run: the time-reversed stacks (flows_b2[f]: frame f+2 -> f) and query frames."""
    n = len(flows_b)
    return n - np.asarray(t).astype(np.int64), list(flows_b)[::-1], list(occ_b)[::-1], list(flows_b2)[::-1], list(occ_b2)[::-1]


def stats_arrays(stats):
    return tuple(np.array([s[k] for s in stats], np.int32) for k in ("rows", "iterations", "termination"))


def track_queries_pc_np(xy, t, flows_f=None, occ_f=None, flows_f2=None, occ_f2=None, flows_b=None, occ_b=None, flows_b2=None, occ_b2=None,
                        mb=False, mb_thres=MB_THRES, engine=engine_np):
    """(birth, length, xy, rows, iterations, termination) of psfm_track_queries_optimize; the solves forward frames ascending, then
    backward frames in the order they ran."""
    fwd = bwd = None
    stats = []
    if flows_f is not None:
        fwd, st = engine(xy, t, list(flows_f), list(occ_f), list(flows_f2), list(occ_f2), mb=mb, mb_thres=mb_thres)
        stats += st
    if flows_b is not None:
        tr, fl, oc, fl2, oc2 = reversed_direction(t, flows_b, occ_b, flows_b2, occ_b2)
        bwd, st = engine(xy, tr, fl, oc, fl2, oc2, mb=mb, mb_thres=mb_thres)
        stats += st
    return qn.to_csr(t, fwd, bwd) + stats_arrays(stats)
