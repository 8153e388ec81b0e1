"""psfm_connect_batch with psfm_ctx_set_batch_redo(ctxs[0], 1) (run_connect_batch(..., redo="together")): the sequences that leave
the fused batch -- their solves reject trust-region steps, or their context is pinned to the launch chain -- are run again from frame 0
through ONE set of launches: the batched chain step of every frame and the frame's solves of all of them as the frame-mode
multi-problem launch chain (psfm_pc_multi_frame_*_kernel), one poll and one synchronisation per chunk of iterations for the whole
table, one segmented finalize.  info.chain_mode is 8 for such a sequence.

What is held (include/psfm.h states the weaker, always-true form): against what psfm_connect leaves for the sequence alone on a context
pinned to the launch chain (set_solver(1, 0)) with no resident budget, the same lane capacity and the same motion-boundary setting,
ids, births, lengths, offsets, positions and every solve's decisions byte for byte -- positions in ONE case and the two costs
everywhere only as far as psfm_connect reproduces its own bytes (measured: it does not, see COST_BITS and the capacity case); and the
oracle's ids, lengths and solve decisions (the helpers of tests/test_gpu_batch.py).
Every "hard" sequence rejects a step in the ORACLE's run (asserted).

Shapes: the smallest at which each mechanism can go wrong -- sequences of 1, 2 and 8 flows (no solve, exactly one, several);
12 k lanes at sample_ratio 1 (96 chain blocks: the tree of the block sums and the ticket over many blocks) and the same under a
resident budget of 8 blocks (every block walks 12 list chunks, the banded plan); a table of one; the only rejecting sequence in the
last row; lane tables sized 1 x the grid (they run full inside the joint redo); a non-default stream behind a gate."""
import contextlib

import numpy as np
import pytest

import psfm_synth
from test_gpu_batch import _check, _dev, _oracle
from test_gpu_stream_order import Gated, assert_same_pc_tree, env, run_sync_gated, sequence, traj_tree  # noqa: F401 (env: fixture)

pytestmark = pytest.mark.gpu
STATS = ("iterations", "successful_steps", "termination", "dogleg_nonGN", "initial_cost", "final_cost")
# The two costs.  MEASURED on an MI355X (96 x 128, sample_ratio 1, seeds 132 / 133, four runs of each route): psfm_connect alone on the
# reference context does not reproduce its OWN cost bytes -- run 0 against run 2: initial_cost of solve 2 93.4677194874552 /
# 93.46771948745521, final_cost of solve 3 16.925001969547914 / ...917, and a lane high-water mark of 12 545 against 12 548 -- and
# neither does the joint redo (budget 8: final_cost of solve 1 28.806751128601785 / ...782); one bit in the last place of one or two
# of ten costs in about four of ten runs, every other byte identical in all of them.  This is what tests/test_gpu_stream_order.py
# (assert_same_pc_tree) found for two identical psfm_connect calls: a track's lane is handed out by blocks that race inside a chain
# step, and a solve's f64 sums run in lane order.  A cost is therefore held to the bytes where they agree (every disagreement is
# collected in COST_BITS and printed) and, where they do not, to what another order of the same terms can do: a sum of n <= lane
# capacity non-negative f64 terms differs between two orders by at most n * 2^-52 relative (each order is within n * 2^-53 of the
# exact sum) -- that suite's bound.  Everything else -- ids, births, lengths, offsets, positions, iterations, accepted steps,
# terminations, non-Gauss-Newton counts -- is compared byte for byte, always (positions with the one exception stated in
# test_tables_that_run_full_inside_the_joint_redo).
COST_BITS = []


@pytest.fixture(scope="module")
def pt():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from point_trajectory import trajectory, _hip
    first = _hip.context()

    class NS:
        pass
    ns = NS()
    ns.trajectory, ns.hip, ns.torch = trajectory, _hip, torch
    # the reference of every comparison: psfm_connect for the sequence ALONE on a context of its own, pinned to the launch chain
    ns.ref = _hip.Context(first.device)
    ns.ref.set_solver(1, 0)
    yield ns
    ns.ref.close()


@contextlib.contextmanager
def solver_modes(pt, modes, budget=0):
    """The thread's batch contexts with psfm_ctx_set_solver(mode, k) each and a resident budget; left adaptive, without budget and with
    the redo option off, whatever happens."""
    ctxs = pt.hip.batch_contexts(len(modes))
    for c, (mode, k) in zip(ctxs, modes):
        c.set_solver(mode, k)
        c.set_resident_budget(budget)
    try:
        yield ctxs
    finally:
        for c in ctxs:
            c.set_solver(0, 0)
            c.set_resident_budget(0)
        assert ctxs[0].batch_redo == 0, "run_connect_batch left the redo option on"


def rejects(O):
    """At least one solve of the oracle's run rejects a step (or leaves the Gauss-Newton path)."""
    return any(s["iterations"] - s["successful_steps"] > 1 or s["dogleg_nonGN"] > 0 for s in O.solves)


def hard(T, H, W, seed, **kw):
    return psfm_synth.synth_sequence(T, H, W, seed=seed, stride2=True, **(kw or psfm_synth.HARD))


def reference(pt, d, r, mb_thres=None, budget=0, capacity=None):
    """psfm_connect for the sequence alone on the reference context: pinned to the launch chain, `budget` resident blocks (0: none),
    the table factors the batch ran with (call it BEHIND the batch)."""
    a, b, a2, b2 = _dev(pt, d, True)
    n, H, W = int(a.shape[0]), int(a.shape[1]), int(a.shape[2])
    pt.ref.set_resident_budget(budget)
    # (the batch contexts remember the table factors a shape once needed: the reference gets the ones the batch ran with)
    capacity = capacity or pt.hip.batch_contexts(1)[0]._capacity.get(("batch", H, W, int(r), True), (2.0, 8.0))
    pt.ref._capacity = {("connect", n, H, W, int(r), True): capacity}
    try:
        return pt.trajectory.run_connect(a, b, a2, b2, 1.0, r, motion_boundary=mb_thres is not None, mb_thres=mb_thres or 0.02, ctx=pt.ref)
    finally:
        pt.ref.set_resident_budget(0)


def diff(R, S, xy_bytes=True):
    """What differs between two results, byte for byte: [] when nothing does.  xy_bytes=False (ONE case, see
    test_tables_that_run_full_inside_the_joint_redo): positions that are not byte-equal are held to ROUNDING = 1e-9 px, the bar
    include/psfm.h states and the suite uses between two device runs of one solve (tests/_queries_pc_np.py)."""
    from _queries_pc_np import ROUNDING
    out = []
    for k in ("birth", "length", "off", "xy"):
        a, b = np.asarray(getattr(R, k)), np.asarray(getattr(S, k))
        if a.shape != b.shape or a.dtype != b.dtype:
            out.append("%s: shape %s / %s" % (k, a.shape, b.shape))
        elif a.tobytes() != b.tobytes():
            err = float(np.abs(a.astype(np.float64) - b).max())
            if k == "xy" and not xy_bytes and err <= ROUNDING:
                COST_BITS.append("xy: %d of %d elements, max |d| %.3g px" % (int((a != b).sum()), a.size, err))
                continue
            out.append("%s: %d of %d elements, max |d| %.3g" % (k, int((a != b).sum()), a.size, float(np.abs(a.astype(np.float64) - b).max())))
    sa, sb = [dict(s) for s in R.solve_stats], [dict(s) for s in S.solve_stats]
    if len(sa) != len(sb):
        out.append("solves: %d / %d" % (len(sa), len(sb)))
    rel = float(max(int(dict(S.info)["lane_capacity"]), 1)) * 2.0 ** -52
    for i, (x, y) in enumerate(zip(sa, sb)):
        for k in STATS[:4]:
            if x[k] != y[k]:
                out.append("solve %d %s: %r / %r" % (i, k, x[k], y[k]))
        for k in STATS[4:]:
            if x[k] != y[k]:
                COST_BITS.append("solve %d %s: %r / %r" % (i, k, x[k], y[k]))
                if abs(x[k] - y[k]) > rel * abs(y[k]):
                    out.append("solve %d %s: %r / %r (beyond the lane-order bound %.3g relative)" % (i, k, x[k], y[k], rel))
    return out


def together(pt, data, r, **kw):
    ctxs, infos = pt.trajectory.run_connect_batch([_dev(pt, d, True) for d in data], 1.0, r, redo="together", **kw)
    return ctxs, infos, [pt.trajectory._result_to_host(c, i) for c, i in zip(ctxs, infos)], ctxs[0].connect_batch_census()


def assert_equal_to_references(got, refs, which=None, xy_bytes=True):
    for k, (R, S) in enumerate(zip(got, refs)):
        if which is not None and k not in which:
            continue
        del COST_BITS[:]
        d = diff(R, S, xy_bytes)
        if COST_BITS:
            print("sequence %d: costs that differ in their last bits (within the lane-order bound unless listed below): %s" % (k, COST_BITS))
        print("sequence %d: %d trajectories, %d solves, differs from psfm_connect alone in: %s" % (k, len(R), len(R.solve_stats), d or "nothing"))
        assert not d, (k, d)


def test_all_sequences_through_the_joint_redo(pt):
    """Sequences of 1, 2 and 8 flows, contexts pinned to the launch chain: all three go straight into the joint redo.  The 1-flow
    sequence runs no solve, the 2-flow sequence exactly one.  Launches and synchronisations equal those of the same call with the
    8-flow sequence alone; two identical calls give identical bytes."""
    H, W, r = 120, 200, 2
    # (the one solve of the 2-flow sequence takes 25 iterations, the first of the 8-flow sequence 32: no frame of the batch needs a
    # chunk of iteration launches that the 8-flow sequence alone does not need)
    data = [hard(2, H, W, 94), hard(3, H, W, 96), hard(9, H, W, 92)]
    oracles = [_oracle(d, 1.0, r, True) for d in data]
    assert rejects(oracles[1]) and rejects(oracles[2]) and len(oracles[0].solves) == 0 and len(oracles[1].solves) == 1
    with solver_modes(pt, [(1, 0)] * 3):
        ctxs, infos, got, census = together(pt, data, r)
        modes = [int(i.chain_mode) for i in infos]
        _check(pt, ctxs, infos, oracles, True)
        _, _, again, census2 = together(pt, data, r)
        _, infos1, got1, census1 = together(pt, data[2:], r)
    refs = [reference(pt, d, r) for d in data]
    print("modes", modes, "census", census, "census of the 8-flow sequence alone", census1)
    assert modes == [8, 8, 8] and census["n_left"] == 3 and census["n_together"] == 3
    assert len(got[0].solve_stats) == 0 and len(got[1].solve_stats) == 1 and len(got[2].solve_stats) == 7
    assert [int(i.n_solves) for i in infos] == [0, 1, 7]
    assert int(infos[2].solver_iterations) == sum(s["iterations"] for s in oracles[2].solves)
    assert_equal_to_references(got, refs)
    # seven frames with a solve in both calls: the launches and synchronisations of a frame do not depend on the number of sequences
    assert int(infos1[0].chain_mode) == 8 and census1["n_together"] == 1 and not diff(got1[0], refs[2])
    assert census["host_syncs"] == census1["host_syncs"] and census["launches_fixed"] == census1["launches_fixed"]
    assert census["launches_iter"] == census1["launches_iter"]
    # one poll per synchronisation but the last; per frame: chain step, init launch, write-back launch
    assert census["launches_fixed"] == 2 + 8 + 2 * 7 + (census["host_syncs"] - 1)
    assert census2 == census
    for k, (a, b) in enumerate(zip(again, got)):
        assert not diff(a, b), ("two identical calls", k, diff(a, b))


def test_a_mixed_batch_keeps_its_rejecting_sequences_together(pt):
    """The five sequences of tests/test_gpu_batch.py's mixed batch under the adaptive policy: the two HARD ones leave the fused batch at
    a checkpoint and are redone together (mode 8, equal to psfm_connect alone), the smooth ones stay (mode 3, untouched)."""
    H, W, r = 120, 200, 2
    spec = [(9, 91, dict(sigma=0.05, n_occluders=1)), (8, 92, psfm_synth.HARD), (24, 93, dict(sigma=0.04, n_occluders=0)),
            (7, 94, psfm_synth.HARD), (20, 95, dict(sigma=0.05, n_occluders=0))]
    data = [psfm_synth.synth_sequence(T, H, W, seed=seed, stride2=True, **kw) for (T, seed, kw) in spec]
    oracles = [_oracle(d, 1.0, r, True) for d in data]
    assert rejects(oracles[1]) and rejects(oracles[3])
    with solver_modes(pt, [(0, 0)] * 5):
        # (the adaptive policy carries the iterations per fused launch from a context's last call into this one: a K too small for a
        # smooth sequence makes its first solve stall and the sequence leave -- the first call settles every context's K, the joint
        # redo folding its solves into the policy as psfm_connect's checkpoints do; the second call is the one under test)
        ctxs, first, got0, census0 = together(pt, data, r)
        modes0 = [int(i.chain_mode) for i in first]
        _check(pt, ctxs, first, oracles, True)
        ctxs, infos, got, census = together(pt, data, r)
        modes = [int(i.chain_mode) for i in infos]
        _check(pt, ctxs, infos, oracles, True)
    print("modes of the settling call", modes0, "census", census0, "\nmodes", modes, "census", census)
    # every sequence that ended in mode 8, in either call, against psfm_connect for it alone; every other one stayed (mode 3)
    refs = [reference(pt, d, r) if 8 in (modes0[k], modes[k]) else None for k, d in enumerate(data)]
    for m, c, g in ((modes0, census0, got0), (modes, census, got)):
        assert m[1] == 8 and m[3] == 8 and all(x in (3, 8) for x in m), m
        assert c["n_together"] == sum(x == 8 for x in m) == c["n_left"]
        assert_equal_to_references(g, refs, which=[k for k in range(5) if m[k] == 8])
    assert modes[2] == 3 and modes[4] == 3 and modes[0] in (3, 8), modes


@pytest.mark.parametrize("budget", [0, 8])
def test_many_blocks_and_a_block_limit(pt, budget):
    """96 x 128 at sample_ratio 1: 12 288 grid points, a lane table of 24 576 -- 96 chain blocks, so the tree of the block sums and the
    ticket run over many blocks.  With a resident budget of 8 blocks on the batch contexts AND on the reference a block walks 12 list
    chunks (the banded plan)."""
    H, W, r = 96, 128, 1
    data = [hard(7, H, W, seed, sigma=0.08, n_occluders=2) for seed in (132, 133)]
    oracles = [_oracle(d, 1.0, r, True) for d in data]
    assert all(rejects(O) for O in oracles)
    with solver_modes(pt, [(1, 0)] * 2, budget=budget):
        ctxs, infos, got, census = together(pt, data, r)
        _check(pt, ctxs, infos, oracles, True)
    refs = [reference(pt, d, r, budget=budget) for d in data]
    print("census", census, "lane capacity", int(infos[0].lane_capacity))
    assert [int(i.chain_mode) for i in infos] == [8, 8] and census["n_together"] == 2
    assert int(infos[0].lane_capacity) >= 2 * H * W
    assert_equal_to_references(got, refs)


def test_motion_boundary_in_every_context(pt):
    """The option on in both contexts, each with its own threshold: the joint redo runs the motion-boundary forms of the chain step on
    the batch's kill maps and equals psfm_connect with the option on."""
    H, W, r = 90, 140, 2
    thres = [0.02, 0.05]
    data = [hard(7, H, W, seed) for seed in (141, 142)]
    assert all(rejects(_oracle(d, 1.0, r, True)) for d in data)
    with solver_modes(pt, [(1, 0)] * 2):
        ctxs, infos, got, census = together(pt, data, r, motion_boundary=True, mb_thres=thres, mb_engine="batch")
    refs = [reference(pt, d, r, mb_thres=t) for d, t in zip(data, thres)]
    plain = [reference(pt, d, r) for d in data]
    assert all(diff(a, b) for a, b in zip(refs, plain)), "the option changes nothing on these flows"
    print("census", census, "solves", [len(R.solve_stats) for R in got])
    assert [int(i.chain_mode) for i in infos] == [8, 8] and census["n_together"] == 2
    assert_equal_to_references(got, refs)


def test_a_table_of_one_and_the_only_rejecting_sequence_last(pt):
    H, W, r = 120, 200, 2
    smooth = [psfm_synth.synth_sequence(T, H, W, seed=seed, stride2=True, sigma=0.04, n_occluders=0) for T, seed in ((8, 93), (6, 95))]
    last = hard(6, H, W, 92)
    data = smooth + [last]
    oracles = [_oracle(d, 1.0, r, True) for d in data]
    assert rejects(oracles[2]) and not rejects(oracles[0]) and not rejects(oracles[1])
    with solver_modes(pt, [(1, 0)]):
        ctxs, infos, got, census = together(pt, [last], r)
        _check(pt, ctxs, infos, oracles[2:], True)
    ref = reference(pt, last, r)
    assert int(infos[0].chain_mode) == 8 and census["n_together"] == 1 and census["n_left"] == 1
    assert_equal_to_references(got, [ref])
    # the fused solve forced on the smooth ones keeps them in; the last row goes straight into the joint redo
    with solver_modes(pt, [(2, 4), (2, 4), (1, 0)]):
        ctxs, infos, got, census = together(pt, data, r)
        _check(pt, ctxs, infos, oracles, True)
    assert [int(i.chain_mode) for i in infos] == [3, 3, 8] and census["n_together"] == 1 and census["n_left"] == 1
    assert_equal_to_references(got, [None, None, ref], which=(2,))


def test_tables_that_run_full_inside_the_joint_redo(pt):
    """Lane and record tables sized 1 x the grid, on the sequences of tests/test_gpu_batch.py's capacity case (they kill and respawn
    half of their tracks every frame): the record tables run full inside the joint redo (PSFM_ERR_CAPACITY from the poll), the
    mirror grows the tables of all contexts and runs the batch again; the results equal psfm_connect alone with the tables the
    batch ended up with, and so does another call on the grown tables."""
    H, W, r = 150, 210, 1
    data = [psfm_synth.synth_sequence(13, H, W, seed=seed, sigma=0.9, n_occluders=3, stride2=True) for seed in (121, 122)]
    oracles = [_oracle(d, 1.0, r, True) for d in data]
    assert all(rejects(O) for O in oracles)
    assert oracles[0].n_traj > 2.5 * H * W + 70000        # (more records than tables of 1 x + 1 x the grid + their head-room hold)
    key = ("batch", H, W, r, True)
    with solver_modes(pt, [(1, 0)] * 2) as ctxs0:
        saved = dict(getattr(ctxs0[0], "_capacity", None) or {})
        ctxs0[0]._capacity = {key: (1.0, 1.0)}
        try:
            ctxs, infos, got, census = together(pt, data, r)
            _check(pt, ctxs, infos, oracles, True)
            grown = ctxs[0]._capacity[key]
            _, _, again, _ = together(pt, data, r)
        finally:
            ctxs0[0]._capacity = saved
    print("table factors the batch ended up with:", grown, "census", census)
    assert grown[1] > 1.0, "the tables never ran full: the case shows nothing"
    assert [int(i.chain_mode) for i in infos] == [8, 8] and census["n_together"] == 2
    refs = [reference(pt, d, r, capacity=grown) for d in data]
    # These sequences lose and respawn half of their 31 500 tracks in every frame: lanes are handed out by blocks that race inside a
    # chain step, the solves' sums run in lane order, and here -- unlike at the other shapes of this file -- that reaches the dogleg
    # coefficients.  MEASURED on an MI355X: 3 of 514 080 coordinates of sequence 0 differ from psfm_connect alone, by 8.9e-16 px,
    # and six of its 22 costs in their last bits.  psfm_connect ALONE AGAINST ITSELF, four runs (profiles/EXPERIMENTS.md 33.2): 8, 0
    # and 0 of sequence 0's coordinates and 11, 15 and 8 of sequence 1's differ from run 0, by up to 2.8e-14 px, with 6-10 of 22
    # costs and lane high-water marks from 33 107 to 33 317 -- the same kind and size; this run's figures are printed below.  Positions are held to the
    # bytes where they agree and to the suite's bar between two device runs of a solve (1e-9 px) where they do not; ids, births,
    # lengths, offsets and every solve's decisions byte for byte, as everywhere.
    once_more = [reference(pt, d, r, capacity=grown) for d in data]
    print("psfm_connect alone against itself:", [diff(a, b) or "nothing" for a, b in zip(once_more, refs)])
    assert_equal_to_references(got, refs, xy_bytes=False)
    assert_equal_to_references(again, refs, xy_bytes=False)


def test_stream_contract_of_the_joint_redo(pt, env):
    """The call on a non-default stream behind a gated kernel (tests/_stream_gate.py), as the batch case of
    tests/test_gpu_stream_order.py: all eight flow stacks come through the gate.  A violation -- a chunk of flow_check, a chain step
    or a solve launch that reads the flows before the gate's copies land -- gives other ids, lengths and positions than the
    default-stream run and the oracle; the result is complete when the call returns."""
    H, W, r = 120, 200, 2
    spec = [(5, 92), (4, 94)]
    data = [sequence(T, H, W, seed, True, **psfm_synth.HARD) for T, seed in spec]
    decoys = [sequence(T, H, W, seed + 100, True, **psfm_synth.HARD) for T, seed in spec]
    keys = ("flows_f", "flows_b", "flows_f2", "flows_b2")
    ins = [[Gated(env, d[k], e[k]) for k in keys] for d, e in zip(data, decoys)]
    oracles = [_oracle({k: list(d[k]) for k in keys}, 1.0, r, True) for d in data]
    assert all(rejects(O) for O in oracles)

    def batch():
        ctxs, infos = env.trajectory.run_connect_batch([tuple(x.t for x in s) for s in ins], 1.0, r, redo="together")
        return [traj_tree(env.trajectory._result_to_host(c, i)) for c, i in zip(ctxs, infos)]

    def check(ts):
        for t, O in zip(ts, oracles):
            assert t["info"]["chain_mode"] == 8
            assert np.array_equal(t["birth"], O.birth) and np.array_equal(t["length"], O.length)
            assert float(np.abs(t["xy"] - O.xy).max()) <= 1e-4
            assert [s["iterations"] for s in t["solve_stats"]] == [s["iterations"] for s in O.solves]
    with solver_modes(pt, [(1, 0)] * 2):
        run_sync_gated(env, "psfm_connect_batch, joint redo", [x for s in ins for x in s], batch, check, compare=assert_same_pc_tree)


def test_default_is_unchanged(pt):
    """Without the option the batch runs as before: the sequence that leaves runs alone through psfm_connect (mode 1), the census says
    nothing went through the joint redo; redo="alone" is that path."""
    H, W, r = 120, 200, 2
    data = [psfm_synth.synth_sequence(8, H, W, seed=93, stride2=True, sigma=0.04, n_occluders=0), hard(6, H, W, 92)]
    oracles = [_oracle(d, 1.0, r, True) for d in data]
    out = []
    with solver_modes(pt, [(2, 4), (1, 0)]):
        for redo in (None, "alone"):
            ctxs, infos = pt.trajectory.run_connect_batch([_dev(pt, d, True) for d in data], 1.0, r, redo=redo)
            _check(pt, ctxs, infos, oracles, True)
            out.append(([int(i.chain_mode) for i in infos], ctxs[0].connect_batch_census(), pt.trajectory._result_to_host(ctxs[1], infos[1])))
    ref = reference(pt, data[1], r)
    for modes, census, R in out:
        print("modes", modes, "census", census, "differs from psfm_connect alone in:", diff(R, ref) or "nothing")
        assert modes == [3, 1]
        assert census == {"n_left": 1, "n_together": 0, "launches_fixed": 0, "launches_iter": 0, "host_syncs": 0}
        assert not diff(R, ref)
    with pytest.raises(ValueError):
        pt.trajectory.run_connect_batch([_dev(pt, d, True) for d in data], 1.0, r, redo="both")
    with pytest.raises(pt.hip.PsfmError):
        pt.hip.context().set_batch_redo(2)
    assert pt.hip.context().batch_redo == 0
