"""NumPy statement of psfm_track_queries -- caller-given points (x, y, t) carried through a flow stack by the body of track.py:37-47,
one step of tests/_motion_boundary_np.step_np per frame on the positions still alive -- and the names of its fixtures
(tests/golden/make_queries_golden.py -> tests/golden/queries.npz).  Pinned to the reference's fixtures by tests/test_queries_host.py,
beside the header the kernels compile (particle-sfm_amd/csrc/psfm_query.h)."""
import numpy as np

import psfm_synth
from _common import golden, input_hash
from _motion_boundary_np import SEQ_SYNTH, motion_boundary_np, step_np

FIXTURE = "queries"
# case -> frames, size, seed of the flows, random queries, kill rule, directions
CASES = {
    "q37x53": dict(T=9, H=37, W=53, seed=5, n_random=300, mb=False, dirs=("forward", "backward", "both")),
    "q24x30": dict(T=7, H=24, W=30, seed=7, n_random=300, mb=False, dirs=("forward", "backward", "both")),
    "q48x64_mb": dict(T=9, H=48, W=64, seed=3, n_random=600, mb=True, dirs=("forward", "backward")),
}
MB_THRES = 0.02
CASE_DIRS = [(c, d) for c, v in CASES.items() for d in v["dirs"]]


def synth(case):
    c = CASES[case]
    return psfm_synth.synth_realistic(c["T"], c["H"], c["W"], seed=c["seed"], stride2=False, **dict(psfm_synth.REALISTIC, **SEQ_SYNTH))


def make_queries(case):
    """The queries of a case: n_random uniform in [-1, W] x [-1, H] with t uniform in 0 .. n_flows, then the hand-placed ones."""
    c = CASES[case]
    H, W, n = c["H"], c["W"], c["T"] - 1
    rng = np.random.default_rng(1000 + c["seed"])
    xy = rng.uniform([-1.0, -1.0], [float(W), float(H)], size=(c["n_random"], 2))
    t = rng.integers(0, n + 1, size=c["n_random"])
    hand = [
        (0.0, 0.0, 0), (W - 1.0, H - 1.0, 0),                       # the corners that are pixels
        (0.0, 0.0, n), (W - 1.0, H - 1.0, n),
        (12.0, 8.0, 1), (12.0, 8.0, n - 1),                         # an exact grid point
        (10.25, 7.5, 2), (10.25, 7.5, 2),                           # two identical queries
        (-0.0, 3.5, 0), (1e-38, 2.0, 0), (-0.0, 3.5, n), (1e-38, 2.0, n),
        (-1e6, 5.0, 1), (1e6, 1e6, 1), (-1e6, 5.0, n - 1), (1e6, 1e6, n - 1),
        (W / 2.0 + 0.3, H / 2.0 + 0.2, n), (W / 2.0 + 0.3, H / 2.0 + 0.2, 0),    # nothing to do forward / backward
        (W / 3.0, H / 3.0, n), (W / 3.0, H / 3.0, 0), (W / 3.0, H / 3.0, n // 2),
    ]
    hand = np.array(hand, np.float64)
    return np.concatenate([xy, hand[:, :2]], 0), np.concatenate([t, hand[:, 2].astype(np.int64)]).astype(np.int32)


def load_case(case):
    """(flows_f, flows_b, occ_f, occ_b, xy, t, fixture): flows re-synthesised from the seed and checked against the fixture's hash."""
    g = golden(FIXTURE)
    d = synth(case)
    assert input_hash(d) == str(g[case + "__input_hash"]), "psfm_synth.synth_realistic no longer reproduces this fixture's inputs"
    return (np.stack(d["flows_f"]), np.stack(d["flows_b"]), g[case + "__occ_f"], g[case + "__occ_b"], g[case + "__xy"], g[case + "__t"], g)


def expected(g, case, direction):
    return g["%s__%s_birth" % (case, direction)], g["%s__%s_length" % (case, direction)], g["%s__%s_xy" % (case, direction)]


def walk(step, xy, t, n_flows, back):
    """One direction.  step(map index, positions (k,2), their query indices (k,)) -> (next (k,2), alive (k,) bool).  Returns per query
    the list of its points in the order they were reached (the query first)."""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    tt = np.asarray(t).astype(np.int64).copy()
    cur = xy.copy()
    pts = [[p.copy()] for p in xy]
    live = (tt > 0) if back else (tt < n_flows)
    for f in (range(n_flows, 0, -1) if back else range(n_flows)):
        idx = np.nonzero(live & (tt == f))[0]
        if len(idx) == 0:
            continue
        nxt, alive = step(f - 1 if back else f, cur[idx].copy(), idx)
        alive = np.asarray(alive) != 0
        for k, q in enumerate(idx):
            if alive[k]:
                cur[q] = nxt[k]
                tt[q] = f - 1 if back else f + 1
                pts[q].append(np.array(nxt[k], np.float64))
                live[q] = tt[q] > 0 if back else tt[q] < n_flows
            else:
                live[q] = False
    return pts


def to_csr(t, fwd, bwd):
    """The two halves as one trajectory: points in ascending time, the query once; birth = t - (len_b - 1)."""
    Q = len(t)
    fwd = fwd if fwd is not None else [[None]] * Q
    bwd = bwd if bwd is not None else [[None]] * Q
    birth = np.array([int(t[q]) - (len(bwd[q]) - 1) for q in range(Q)], np.int32)
    length = np.array([len(bwd[q]) + len(fwd[q]) - 1 for q in range(Q)], np.int32)
    rows = []
    for q in range(Q):
        first = bwd[q][0] if bwd[q][0] is not None else fwd[q][0]
        rows.extend(bwd[q][:0:-1] + [first] + fwd[q][1:])
    return birth, length, np.array(rows, np.float64).reshape(-1, 2)


def track_queries_np(xy, t, flows_f=None, occ_f=None, flows_b=None, occ_b=None, mb=False, mb_thres=MB_THRES):
    """(birth, length, xy) of psfm_track_queries, every step by step_np."""
    halves = []
    for flows, occ, back in ((flows_f, occ_f, False), (flows_b, occ_b, True)):
        if flows is None:
            halves.append(None)
            continue
        n = len(flows)
        masks = [motion_boundary_np(f, mb_thres) if mb else np.zeros(f.shape[:2], bool) for f in flows]
        halves.append(walk(lambda m, p, idx: step_np(p, flows[m], occ[m], masks[m], "mb" if mb else "shipped"), xy, t, n, back))
    return to_csr(t, halves[0], halves[1])
