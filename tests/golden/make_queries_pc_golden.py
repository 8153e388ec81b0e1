#!/usr/bin/env python3
"""Golden vectors for psfm_track_queries_optimize (tests/golden/queries_pc.npz), produced by the REFERENCE's own point_trajectory
Python (oracle/ref_shim.load()), unmodified: IncrementalTrajectorySet(n + 1, h, w, 2, buffer_size=3); per frame new_traj_all with the
queries of that frame in place of sample_candidates, then get_cur_pos, grid_sample, motion_boundary, step_forward, extend_all and
optimize_buffer exactly as track_optimize.py:37-50 calls them; then clear_active.  Backward: the same on the time-reversed lists.
optimize_location is the shim's -- the C oracle (oracle/psfm_oracle.c); the real Ceres module cannot be built where this runs
(oracle/_ref/BUILD.md), as for every other solver fixture.  The motion-boundary case uses the reference's step_forward with its
commented line switched on at run time (make_motion_boundary_golden.motion_boundary_step_forward).  Only arrays are stored; the flows
are re-synthesised from the seed by the tests and checked against `input_hash`.

Two inputs the reference's loop cannot take are handled outside it: a query at frame n_flows (never steps: length 1), and a frame
whose solve would have no row (np.stack([]) raises; no fixture has one -- asserted).

Asserted here, on the reference alone, per case and direction, over the random queries:
  1. at least 40 % take part in at least one solve;
  2. at least 10 die after having been in a solve;
  3. at least 10 die before their buffer is full (one or two points);
  4. at least 5 end more than 1e-3 px (ten times the position tolerance) away from the same walk with buffer_size=0 -- the last point
     of the two walks' common frames;
  5. every step taken from a position that a solve has touched decides with margin: `next` at least 1e-6 px from 0, W-1, H-1, the
     sampled occlusion / boundary value at least 1e-6 from 0.1 (this is what lets lengths be compared exactly).
Printed: the figures above and rows, iterations and termination of every solve.

Run where a reference checkout is present (PSFM_REFERENCE_ROOT), never on the GPU machine:
    python tests/golden/make_queries_pc_golden.py
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for p in (ROOT, os.path.join(ROOT, "particle-sfm_amd"), TESTS, HERE):
    sys.path.insert(0, p)
from oracle import oracle, ref_shim                                 # noqa: E402
from _common import input_hash                                      # noqa: E402
import _queries_np as qn                                            # noqa: E402
import _queries_pc_np as qp                                         # noqa: E402
from make_motion_boundary_golden import motion_boundary_step_forward   # noqa: E402

MAX_BYTES = 1 << 20
SOLVES = []          # (rows, iterations, termination) of every optimize_location the reference called, in call order


def recording_optimize_location(uv12, uv_ref1, uv_ref2, ref2_scale, flow12_map, total_num, width, height):
    out, st = oracle.optimize_location(uv12, uv_ref1, uv_ref2, ref2_scale, flow12_map, total_num, width, height, return_stats=True)
    SOLVES.append((int(total_num), int(st["iterations"]), int(st["termination"])))
    return out


def reference_engine(ref, step_fn, xy, t, flows, occ, flows2, occ2, buffer_size, thres):
    """The reference's classes over caller-given points, forward over the lists.  Returns (pts per query, stats, facts): facts holds
    per query in_solve, died, and the smallest margins of the steps taken from a solved position."""
    import torch
    n = len(flows)
    H, W = flows[0].shape[:2]
    Q = len(t)
    trajs = ref.IncrementalTrajectorySet(n + 1, H, W, 2, buffer_size=buffer_size)
    obj = [None] * Q
    active = []                                   # query index of every entry of trajs.active_trajs
    in_solve, died, touched = np.zeros(Q, bool), np.zeros(Q, bool), np.zeros(Q, bool)
    margin_next, margin_val = np.inf, np.inf
    first = len(SOLVES)
    rows_seen = []
    for f in range(n):
        sel = np.nonzero(t == f)[0]
        trajs.new_traj_all([int(x) for x in t[sel]], [xy[q].copy() for q in sel])
        for k, q in enumerate(sel):
            obj[q] = trajs.active_trajs[len(active) + k]
        active += [int(q) for q in sel]
        assert len(active) == len(trajs.active_trajs) and len(active) > 0, "a frame with no active query"
        cur = trajs.get_cur_pos()
        flow_t = torch.from_numpy(flows[f]).permute(2, 0, 1).float()
        fs = ref.grid_sample(flow_t, cur)
        mbm = ref.trajectory.motion_boundary(flows[f], thres)
        nxt, flags = step_fn(cur, fs, occ[f], mbm)
        alive = np.asarray(flags) != 0
        # condition 5: the margins of the steps taken from a position a solve has touched
        tq = touched[active]
        if tq.any():
            nx = np.asarray(nxt, np.float64)[tq]
            margin_next = min(margin_next, float(np.abs(np.stack([nx[:, 0], nx[:, 0] - (W - 1), nx[:, 1], nx[:, 1] - (H - 1)])).min()))
            vals = [ref.grid_sample(torch.from_numpy(np.asarray(occ[f])).unsqueeze(0).float(), cur[tq])]
            if step_fn is not ref.step_forward:
                vals.append(ref.grid_sample(torch.from_numpy(mbm).unsqueeze(0).float(), cur[tq]))
            margin_val = min(margin_val, float(np.abs(np.concatenate(vals).astype(np.float64) - np.float64(np.float32(0.1))).min()))
        trajs.extend_all(nxt, f + 1, flags)
        died[[q for q, a in zip(active, alive) if not a]] = True
        active = [q for q, a in zip(active, alive) if a]
        touched[:] = False
        if buffer_size == 3 and f + 1 >= 2:
            rows = [q for q, tr in zip(active, trajs.active_trajs) if len(tr.buffer_xys) == 3]
            assert len(rows) > 0, "a frame whose solve has no row: the reference raises"
            trajs.optimize_buffer(flows[f - 1], flows[f], flows2[f - 1], occ2[f - 1], f + 1)
            in_solve[rows] = True
            touched[rows] = True
            rows_seen.append(len(rows))
    trajs.clear_active()
    pts = []
    for q in range(Q):
        if t[q] == n:
            pts.append([xy[q].copy()])                       # never steps
            continue
        tr = obj[q]
        assert tr.times == list(range(int(t[q]), int(t[q]) + tr.length())) and not tr.buffer_xys
        pts.append([np.asarray(p, np.float64) for p in tr.xys])
    stats = [dict(rows=r, iterations=i, termination=k) for (r, i, k) in SOLVES[first:]]
    assert [s["rows"] for s in stats] == rows_seen
    return pts, stats, dict(in_solve=in_solve, died=died, margin_next=margin_next, margin_val=margin_val)


def main():
    ref = ref_shim.load(optimize_location=recording_optimize_location)
    mb_step = motion_boundary_step_forward(ref)
    arrays = {}
    any_hard_solve = False
    for case, c in qp.CASES.items():
        d = qp.synth(case)
        n = len(d["flows_f"])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            occ = {"occ_f": ref.flow_check(d["flows_f"], d["flows_b"], 1.0)[1], "occ_b": ref.flow_check(d["flows_b"], d["flows_f"], 1.0)[1],
                   "occ_f2": ref.flow_check(d["flows_f2"], d["flows_b2"], 1.0)[1], "occ_b2": ref.flow_check(d["flows_b2"], d["flows_f2"], 1.0)[1]}
        occ = {k: [np.asarray(o) != 0 for o in v] for k, v in occ.items()}
        xy, t = qp.make_queries(case)
        nr = c["n_random"]
        arrays.update({case + "__input_hash": input_hash(d), case + "__xy": xy, case + "__t": t})
        arrays.update({case + "__" + k: np.stack(v) for k, v in occ.items()})
        step_fn = mb_step if c["mb"] else ref.step_forward
        halves = {}
        for direction in ("forward", "backward"):
            if direction not in c["dirs"] and "both" not in c["dirs"]:
                continue
            if direction == "forward":
                tt, fl, oc, fl2, oc2 = t.astype(np.int64), d["flows_f"], occ["occ_f"], d["flows_f2"], occ["occ_f2"]
            else:
                tt, fl, oc, fl2, oc2 = qp.reversed_direction(t, d["flows_b"], occ["occ_b"], d["flows_b2"], occ["occ_b2"])
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                pts, stats, facts = reference_engine(ref, step_fn, xy, tt, fl, oc, fl2, oc2, 3, qp.MB_THRES)
                plain, _, _ = reference_engine(ref, step_fn, xy, tt, fl, oc, fl2, oc2, 0, qp.MB_THRES)
            halves[direction] = (pts, stats)
            r = slice(0, nr)
            length = np.array([len(p) for p in pts])
            moved = np.array([np.abs(a[min(len(a), len(b)) - 1] - b[min(len(a), len(b)) - 1]).max() for a, b in zip(pts, plain)])
            n_solved = int(facts["in_solve"][r].sum())
            n_die_after = int((facts["died"] & facts["in_solve"])[r].sum())
            n_die_early = int((facts["died"] & (length <= 2))[r].sum())
            n_moved = int((moved[r] > 1e-3).sum())
            print("  %-10s %-8s rows per frame %d .. %d, in a solve %d, die after a solve %d, die before a full buffer %d, moved > 1e-3 px %d"
                  " (max %.3g), margins next %.3g value %.3g" % (case, direction, min(s["rows"] for s in stats), max(s["rows"] for s in stats),
                                                                 n_solved, n_die_after, n_die_early, n_moved, moved[r].max(),
                                                                 facts["margin_next"], facts["margin_val"]))
            print("             solves (rows, iterations, termination):", [(s["rows"], s["iterations"], s["termination"]) for s in stats])
            any_hard_solve |= any(s["iterations"] > 1 for s in stats)
            assert n_solved >= 0.4 * nr, (case, direction, "condition 1")
            assert n_die_after >= 10, (case, direction, "condition 2")
            assert n_die_early >= 10, (case, direction, "condition 3")
            assert n_moved >= 5, (case, direction, "condition 4")
            assert facts["margin_next"] >= 1e-6 and facts["margin_val"] >= 1e-6, (case, direction, "condition 5")
        for direction in c["dirs"]:
            fwd = halves["forward"] if direction in ("forward", "both") else None
            bwd = halves["backward"] if direction in ("backward", "both") else None
            birth, length, pts = qn.to_csr(t, fwd[0] if fwd else None, bwd[0] if bwd else None)
            assert (length >= 1).all() and (birth >= 0).all() and (birth + length - 1 <= n).all() and len(pts) == length.sum()
            rows, its, term = qp.stats_arrays((fwd[1] if fwd else []) + (bwd[1] if bwd else []))
            arrays.update({"%s__%s_birth" % (case, direction): birth, "%s__%s_length" % (case, direction): length,
                           "%s__%s_xy" % (case, direction): pts, "%s__%s_rows" % (case, direction): rows,
                           "%s__%s_iterations" % (case, direction): its, "%s__%s_termination" % (case, direction): term})
    assert any_hard_solve, "no solve of the fixture takes more than one iteration: add the noisy case"
    path = os.path.join(HERE, qp.FIXTURE + ".npz")
    np.savez_compressed(path, **arrays)
    assert os.path.getsize(path) <= MAX_BYTES, os.path.getsize(path)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
