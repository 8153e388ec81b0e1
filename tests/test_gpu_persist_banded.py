"""The persistent frame loop with its XCD-banded index arithmetic switched on, against the CPU oracle.

The parity shapes of test_gpu_parity.py (48x64 ... 120x160) all run with `xcd_per == 0` and `fc_xcd_per == 0`: block b owns
lanes [256 b, 256 b + 256) and flow_check chunk b.  From G >= 64 * 256 grid points on, block b owns the lanes of virtual block
(b % 8) * per + b / 8 (psfm_vblock), and from P >= 64 * 1024 pixels on the fused flow_check takes its chunks in the same banded
order -- the form the 1080p headline runs in, otherwise only covered by the whole-sequence tests.  Every shape here has
G = 128 * 128 = 64 * 256 grid points (the smallest that bands the lanes); all but 128x128 also band the flow_check chunks.  One
shape per instantiation of the kernel: sample_ratio 2, 1, 4 and the generic one (3).

Each case runs psfm_connect (flow_check fused into the loop) and flow_check + psfm_track (the loop on ready maps); ids, births
and lengths must equal the oracle's, positions bit for bit, and both must report chain_mode 2 (the loop ran, nothing was
handed over to per-frame launches).
"""
import numpy as np
import pytest

import psfm_synth

pytestmark = pytest.mark.gpu

T_FLOWS = 6
# name -> (H, W, sample_ratio, seed, frame pair in which every track dies or None)
CASES = {
    "256x256_r2": (256, 256, 2, 71, None),
    "128x128_r1": (128, 128, 1, 72, None),
    "512x512_r4": (512, 512, 4, 73, None),
    "384x384_r3": (384, 384, 3, 74, None),
    # mass respawn: every track dies in step 2, every grid point respawns in frame 3 -- phase 2 in several passes of 256 entries,
    # guest lanes, lanes popped from the global stacks and handed to their owners
    "256x256_r2_all_die": (256, 256, 2, 75, 2),
}
_REF = {}


def _case(name):
    """Inputs and the oracle's result of a case, computed once per session and never modified."""
    if name not in _REF:
        from oracle import oracle as orc
        H, W, r, seed, die = CASES[name]
        d = psfm_synth.synth_sequence(T_FLOWS + 1, H, W, seed=seed, sigma=0.8, n_occluders=3, stride2=False)
        ff = [np.ascontiguousarray(f) for f in d["flows_f"]]
        fb = [np.ascontiguousarray(f) for f in d["flows_b"]]
        if die is not None:
            # a backward flow that contradicts the forward one by 50 px everywhere: flow_check (the oracle's, the stand-alone
            # kernel and the one fused into the loop) marks every pixel of that pair occluded
            fb[die] = (fb[die] + np.float32(50.0)).astype(np.float32)
        _, occ = orc.flow_check(ff, fb, 1.0)
        O = orc.track(ff, occ, r)
        _REF[name] = (ff, fb, [np.asarray(o) for o in occ], O)
    return _REF[name]


@pytest.fixture(scope="module")
def pt():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from point_trajectory import utils, trajectory, _hip
    ctx = _hip.context()
    ctx.set_chain_mode(2)    # the persistent loop is required: a launch that cannot run it is an error, not a fall-back
    class NS: pass
    ns = NS()
    ns.utils, ns.trajectory, ns.hip = utils, trajectory, _hip
    yield ns
    ctx.set_chain_mode(0)


def _same(R, O):
    assert R.birth.shape[0] == O.n_traj
    assert np.array_equal(R.birth, O.birth) and np.array_equal(R.length, O.length)
    assert np.array_equal(R.xy, O.xy)


@pytest.mark.parametrize("name", list(CASES))
def test_banded_loop_vs_oracle(pt, name):
    import torch
    H, W, r, _, die = CASES[name]
    ff, fb, occ_o, O = _case(name)
    G = ((H + r - 1) // r) * ((W + r - 1) // r)
    assert G >= 64 * 256, "the shape must band the lanes (xcd_per > 0)"
    # the inputs do what the case is for: tracks die in every step and are born in every frame
    birth, last = np.asarray(O.birth), np.asarray(O.birth) + np.asarray(O.length) - 1
    assert set(range(T_FLOWS)) <= set(birth.tolist())
    assert set(range(T_FLOWS)) <= set(last.tolist())
    if die is not None:
        assert np.stack(occ_o)[die].all()
        assert not ((birth <= die) & (last > die)).any(), "no track survives the all-occluded step"
        # (all but grid point 0: with nothing marked, the reference's distance transform measures to a phantom feature beside it)
        assert (birth == die + 1).sum() == G - 1, "every grid point respawns behind it"
    tf = torch.from_numpy(np.stack(ff)).cuda()
    tb = torch.from_numpy(np.stack(fb)).cuda()
    # fused: psfm_connect computes the occlusion maps inside the loop
    Rc = pt.trajectory.run_connect(tf, tb, None, None, 1.0, r)
    assert Rc.info["chain_mode"] == 2
    _same(Rc, O)
    # ready maps: flow_check, then psfm_track
    _, occ = pt.utils.flow_check_device(tf, tb, 1.0)
    assert np.array_equal(occ.cpu().numpy().astype(bool), np.stack(occ_o).astype(bool))
    Rt = pt.trajectory.run_track(tf, occ, None, None, r)
    assert Rt.info["chain_mode"] == 2
    _same(Rt, O)
