"""The id assignment of long sequences: the library's own record sort on 64-bit keys (csrc/psfm_sort64.hip) and the boundary between
the one-block group plan and decode + scan (csrc/psfm_finalize.hip).  Every case against the CPU oracle (flow_check + track: ids,
lengths and positions equal) and, because every form gives the same bytes, with the form that ran asserted through
psfm_ctx_get_finalize_forms (sort: 1 own 32-bit, 2 own 64-bit, 3 rocPRIM; offsets: 1 one-block plan, 3 decode + scan; 2 is the chunked
plan, which was measured slower than decode + scan at both long benchmark shapes and is not part of the library:
profiles/EXPERIMENTS.md 20 -- sequences of more than 178 flows therefore report 3).

PSFM_FIN_SORT=0 PSFM_FIN_PLAN=0 (read once per process) must send every shape down rocPRIM and decode + scan: the last test runs
the plan-boundary cases of this file that way in a process of its own, where they expect forms 3 and 3 and the same oracle bytes."""
import os
import subprocess
import sys

import numpy as np
import pytest

import psfm_synth

pytestmark = pytest.mark.gpu

OLD_FORMS = os.environ.get("PSFM_FIN_SORT") == "0" and os.environ.get("PSFM_FIN_PLAN") == "0"


def groups(n_flows):
    lmax = n_flows + 1
    return lmax * (lmax + 1) // 2 + lmax + 1


def expect(sort, offsets):
    return {"sort": 3, "offsets": 3} if OLD_FORMS else {"sort": sort, "offsets": offsets}


@pytest.fixture(scope="module")
def pt():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from point_trajectory import trajectory, track, _hip
    class NS: pass
    ns = NS()
    ns.trajectory, ns.track, ns.hip, ns.torch = trajectory, track.track, _hip, torch
    ns.ctx = _hip.context()
    return ns


def run_against_oracle(pt, T, H, W, r, seed, sigma, nocc, kill_frame=None):
    from oracle import oracle as orc
    d = psfm_synth.synth_sequence(T, H, W, seed=seed, sigma=sigma, n_occluders=nocc, stride2=False)
    _, occ = orc.flow_check(d["flows_f"], d["flows_b"], 1.0)
    if kill_frame is not None:
        occ = [o.copy() for o in occ]
        occ[kill_frame][:] = True
    O = orc.track(d["flows_f"], occ, r)
    R = pt.track(d["flows_f"], occ, r)
    forms = pt.ctx.finalize_forms()
    assert R.birth.shape[0] == O.n_traj
    assert np.array_equal(R.birth, O.birth) and np.array_equal(R.length, O.length)
    assert np.array_equal(R.off, np.concatenate([[0], np.cumsum(O.length)]))
    assert np.array_equal(R.xy, O.xy)
    return forms, O


def test_group_counts_of_the_boundary_cases():
    """What the cases below rely on: 178 flows are the last sequence length whose groups fit one plan block."""
    assert groups(178) == 16290 <= 16384 < groups(179) == 16471
    assert groups(400) > 4 * 16384


@pytest.mark.parametrize("n_flows,offsets", [(178, 1), (179, 3), (400, 3)])
def test_plan_boundary(pt, n_flows, offsets):
    forms, _ = run_against_oracle(pt, n_flows + 1, 24, 30, 2, seed=300 + n_flows, sigma=0.3, nocc=1)
    assert forms == expect(1, offsets)


def test_long_stretches_of_empty_groups(pt):
    """Every track dies at one frame (its occlusion map all true): thousands of consecutive (death, birth) groups without a record."""
    forms, O = run_against_oracle(pt, 401, 24, 30, 2, seed=77, sigma=0.1, nocc=0, kill_frame=150)
    assert forms == expect(1, 3)
    last = O.birth + O.length - 1
    assert any(not ((O.birth <= t) & (last > t)).any() for t in (149, 150, 151))      # no track lives across that frame


def test_64_bit_keys(pt):
    """64 x 90 at r = 1 (13 bits of grid index): from 1 022 flows on the triangular (death, birth) number needs 20 bits and the key no
    longer fits 32."""
    forms, O = run_against_oracle(pt, 1023, 64, 90, 1, seed=45, sigma=0.1, nocc=1)
    assert forms == expect(2, 3)
    assert (O.length < 3).any() and (O.length > 5).any()


def test_batch_whose_sequence_bits_need_64_bit_keys(pt):
    """33 sequences of 48 x 64 at r = 1, 181 frames: 12 bits of grid index + 15 of the (death, birth) number + 6 of the sequence do not
    fit 32 bits, the key of a sequence alone does -- the smallest such batch (32 sequences need 5 bits, 179 flows 14), and with fewer
    records than the count from which the finalize hands 64-bit keys to rocPRIM.  Eight distinct sequences in turn: every member of
    the batch must equal the psfm_connect of its own sequence."""
    H, W, T, r, B = 48, 64, 181, 1, 33
    data = [psfm_synth.synth_sequence_torch(T, H, W, seed=500 + k, sigma=0.05 + 0.05 * (k % 4), n_occluders=k % 3, stride2=False) for k in range(8)]
    alone = []
    for d in data:
        alone.append(pt.trajectory.run_connect(d["flows_f"], d["flows_b"], None, None, 1.0, r))
        assert pt.ctx.finalize_forms()["sort"] == expect(1, 3)["sort"]              # alone the key fits 32 bits
    order = [(3 * k) % 8 for k in range(B)]
    ctxs, infos = pt.trajectory.run_connect_batch([(data[k]["flows_f"], data[k]["flows_b"], None, None) for k in order], 1.0, r)
    forms = ctxs[0].finalize_forms()
    assert sum(int(i.n_traj) for i in infos) <= 5_000_000
    assert forms == expect(2, 3)                     # (the batch finalize keeps decode + scan)
    for q, k in enumerate(order):
        R = pt.trajectory._result_to_host(ctxs[q], infos[q])
        A = alone[k]
        assert len(R) == len(A) and len(R) > 48 * 64
        assert np.array_equal(R.birth, A.birth) and np.array_equal(R.length, A.length) and np.array_equal(R.off, A.off), q
        assert np.array_equal(R.xy, A.xy), q


def test_switches_keep_the_old_forms():
    if OLD_FORMS:
        return                                       # (this IS the process with the switches off)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PSFM_FIN_PLAN="0", PSFM_FIN_SORT="0")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x", "-k", "plan_boundary",
                        "-p", "no:cacheprovider"], capture_output=True, text=True, env=env, timeout=600, cwd=root)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "3 passed" in r.stdout
