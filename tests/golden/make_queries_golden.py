#!/usr/bin/env python3
"""Golden vectors for psfm_track_queries (tests/golden/queries.npz), produced by the REFERENCE's own point_trajectory Python
(oracle/ref_shim.load()): utils.flow_check for the occlusion maps of each stack, and per frame, on the positions still alive,
trajectory.grid_sample, trajectory.motion_boundary and trajectory.step_forward -- the body of track.py:37-47 for caller-given points.
The motion-boundary case uses the reference's step_forward with its commented line switched on at run time
(make_motion_boundary_golden.motion_boundary_step_forward).  Only arrays are stored; the flows are re-synthesised from the seed by the
tests and checked against `input_hash`.

Asserted here, on the reference alone, per case and direction, over the random queries: at least 10 die by occlusion, at least 10 die
by leaving the frame, between 25 % and 85 % reach the end of the stack; for the motion-boundary case, at least 10 queries per
direction get a length different from the shipped rule's on the same input.

Run where a reference checkout is present (PSFM_REFERENCE_ROOT), never on the GPU machine:
    python tests/golden/make_queries_golden.py
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
from oracle import ref_shim                                        # noqa: E402
from _common import input_hash                                      # noqa: E402
import _queries_np as qn                                            # noqa: E402
from make_motion_boundary_golden import motion_boundary_step_forward   # noqa: E402

MAX_BYTES = 1 << 20


def reference_walk(ref, step_fn, flows, occ, xy, t, back, thres):
    """qn.walk with the reference's functions as the step; also says how every query ended: 0 reached the end of the stack,
    1 occlusion (or motion boundary), 2 left the frame."""
    import torch
    H, W = flows[0].shape[:2]
    end = np.zeros(len(xy), np.int64)

    def step(m, p, idx):
        flow_t = torch.from_numpy(flows[m]).permute(2, 0, 1).float()
        fs = ref.grid_sample(flow_t, p.copy())
        mb = ref.trajectory.motion_boundary(flows[m], thres)
        nxt, flags = step_fn(p.copy(), fs, occ[m], mb)
        nxt, alive = np.asarray(nxt, np.float64), np.asarray(flags) != 0
        valid = (nxt[:, 0] > 0) & (nxt[:, 0] < W - 1) & (nxt[:, 1] > 0) & (nxt[:, 1] < H - 1)
        end[idx[~alive]] = np.where(valid, 1, 2)[~alive]
        return nxt, alive
    return qn.walk(step, xy, t, len(flows), back), end


def main():
    ref = ref_shim.load()
    mb_step = motion_boundary_step_forward(ref)
    arrays = {}
    for case, c in qn.CASES.items():
        d = qn.synth(case)
        flows_f, flows_b = d["flows_f"], d["flows_b"]
        n = len(flows_f)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _, occ_f = ref.flow_check(flows_f, flows_b, 1.0)
            _, occ_b = ref.flow_check(flows_b, flows_f, 1.0)       # the backward stack's OWN maps
        occ_f, occ_b = [np.asarray(o) != 0 for o in occ_f], [np.asarray(o) != 0 for o in occ_b]
        xy, t = qn.make_queries(case)
        nr = c["n_random"]
        arrays.update({case + "__input_hash": input_hash(d), case + "__occ_f": np.stack(occ_f), case + "__occ_b": np.stack(occ_b),
                       case + "__xy": xy, case + "__t": t})
        step_fn = mb_step if c["mb"] else ref.step_forward
        halves = {}
        for direction, flows, occ, back in (("forward", flows_f, occ_f, False), ("backward", flows_b, occ_b, True)):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                pts, end = reference_walk(ref, step_fn, flows, occ, xy, t, back, qn.MB_THRES)
            halves[direction] = pts
            n_end, n_occ, n_out = int((end[:nr] == 0).sum()), int((end[:nr] == 1).sum()), int((end[:nr] == 2).sum())
            print("  %-10s %-8s reach the end %4d, die by occlusion %4d, die leaving the frame %4d" % (case, direction, n_end, n_occ, n_out))
            assert n_occ >= 10 and n_out >= 10 and 0.25 * nr <= n_end <= 0.85 * nr, (case, direction)
            if c["mb"]:
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    shipped, _ = reference_walk(ref, ref.step_forward, flows, occ, xy, t, back, qn.MB_THRES)
                differ = sum(len(a) != len(b) for a, b in zip(pts, shipped))
                print("  %-10s %-8s lengths that differ from the shipped rule's: %d" % (case, direction, differ))
                assert differ >= 10, (case, direction, differ)
        for direction in c["dirs"]:
            fwd = halves["forward"] if direction in ("forward", "both") else None
            bwd = halves["backward"] if direction in ("backward", "both") else None
            birth, length, pts = qn.to_csr(t, fwd, bwd)
            assert (length >= 1).all() and (birth >= 0).all() and (birth + length - 1 <= n).all() and len(pts) == length.sum()
            arrays.update({"%s__%s_birth" % (case, direction): birth, "%s__%s_length" % (case, direction): length,
                           "%s__%s_xy" % (case, direction): pts})
    path = os.path.join(HERE, qn.FIXTURE + ".npz")
    np.savez_compressed(path, **arrays)
    assert os.path.getsize(path) <= MAX_BYTES, os.path.getsize(path)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
