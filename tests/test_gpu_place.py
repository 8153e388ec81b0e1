"""The placed finalize of the persistent frame loop (csrc/psfm_place.h, psfm_place.hip): records laid out by birth order -- from the
birth masks the loop leaves behind -- and sorted in ONE pass on the last valid time, instead of compaction + four passes.

Every case runs with the loop required (chain mode 2) and is checked twice: against the CPU oracle (trajectory ids = order, births,
lengths, offsets, positions bit for bit), and bit for bit against the same call in a process started with PSFM_FIN_PLACE=0, which runs
the compaction and the four passes (one such process computes all cases; this file is its program when run as a script).  Which form
ran is asserted through psfm_ctx_get_finalize_placed: nothing in the bytes tells them apart."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    for p in (ROOT, os.path.join(ROOT, "particle-sfm_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)

import psfm_synth

pytestmark = pytest.mark.gpu

# name -> frames, H, W, sample_ratio, seed, sigma, occluders, frame pair whose occlusion map is all true (or None), placed form expected
CASES = {
    "46x62_r2": (7, 46, 62, 2, 5, 0.3, 2, None, 1),                 # 713 grid points: 3 blocks, the last one ragged; banding off
    "260x260_r2": (7, 260, 260, 2, 3, 0.3, 2, None, 1),             # 16 900 grid points: 67 blocks, XCD-banded ownership on
    "30x40_r1": (6, 30, 40, 1, 8, 0.3, 2, None, 1),
    "70x90_r3": (6, 70, 90, 3, 9, 0.3, 2, None, 1),                 # the generic-ratio instantiation
    "46x62_r2_all_occluded": (7, 46, 62, 2, 6, 0.3, 2, 2, 1),       # mass respawn: every block's grid points are all born in frame 3
    "260x260_r2_all_occluded": (6, 260, 260, 2, 4, 0.3, 2, 1, 1),   # ... with banded ownership
    "200x200_r1_noisy": (6, 200, 200, 1, 5, 0.3, 2, None, 1),       # births beyond a block's free lanes: guest, popped and fresh lanes
    "46x62_r2_2_frames": (2, 46, 62, 2, 5, 0.3, 2, None, 1),        # n_flows 1: frame 0 only, no stored row of counts
    "46x62_r2_3_frames": (3, 46, 62, 2, 5, 0.3, 2, None, 1),
    "64x90_r1_1023_frames": (1023, 64, 90, 1, 45, 0.1, 1, None, 0), # 13 + 20 key bits: 64-bit keys (and more than 255 flows)
}
_IN, _REF = {}, {}


def grid(name):
    _, H, W, r = CASES[name][:4]
    return ((H + r - 1) // r) * ((W + r - 1) // r)


def inputs(name):
    """Forward / backward flows and the occlusion maps (the oracle's flow_check, one map overwritten where the case says so)."""
    if name not in _IN:
        from oracle import oracle as orc
        T, H, W, r, seed, sigma, nocc, kill, _ = CASES[name]
        d = psfm_synth.synth_sequence(T, H, W, seed=seed, sigma=sigma, n_occluders=nocc, stride2=False)
        _, occ = orc.flow_check(d["flows_f"], d["flows_b"], 1.0)
        occ = [np.asarray(o).copy() for o in occ]
        if kill is not None:
            occ[kill][:] = True
        _IN[name] = (d["flows_f"], d["flows_b"], occ)
    return _IN[name]


def reference(name):
    """The oracle's result of a case: computed once, shared, never modified."""
    if name not in _REF:
        from oracle import oracle as orc
        ff, _, occ = inputs(name)
        _REF[name] = orc.track(ff, occ, CASES[name][3])
    return _REF[name]


def gpu_track(name):
    """(result, placed, info) of psfm_track on the case with the persistent loop required."""
    from point_trajectory import trajectory, _hip
    ctx = _hip.context()
    ctx.set_chain_mode(2)
    try:
        ff, _, occ = inputs(name)
        R = trajectory.run_track(ff, occ, None, None, CASES[name][3])
        return R, ctx.finalize_placed(), ctx.finalize_forms()
    finally:
        ctx.set_chain_mode(0)


def _arrays(R):
    return {"birth": np.asarray(R.birth), "length": np.asarray(R.length), "off": np.asarray(R.off), "xy": np.asarray(R.xy)}


@pytest.fixture(scope="module")
def four_passes(tmp_path_factory):
    """Every case computed by a process with PSFM_FIN_PLACE=0 (read once per process): {case: arrays}."""
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    out = str(tmp_path_factory.mktemp("place") / "four_passes.npz")
    env = dict(os.environ, PSFM_FIN_PLACE="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    z = np.load(out)
    return {name: {k: z["%s/%s" % (name, k)] for k in ("birth", "length", "off", "xy", "placed")} for name in CASES}


def _check(name, R, placed, forms, four_passes):
    O = reference(name)
    want = CASES[name][8]
    assert R.info["chain_mode"] == 2, "the persistent loop did not run"
    assert placed == want and forms["sort"] == (1 if want else 2)
    a = _arrays(R)
    assert a["birth"].shape[0] == O.n_traj
    assert np.array_equal(a["birth"], O.birth) and np.array_equal(a["length"], O.length)
    assert np.array_equal(a["off"], np.concatenate([[0], np.cumsum(O.length)]))
    assert np.array_equal(a["xy"], O.xy)
    old = four_passes[name]
    assert int(old["placed"]) == 0
    for k in ("birth", "length", "off", "xy"):
        assert a[k].dtype == old[k].dtype and np.array_equal(a[k], old[k]), k


@pytest.mark.parametrize("name", list(CASES))
def test_placed_finalize_vs_oracle_and_four_passes(four_passes, name):
    T, H, W, r, _, _, _, kill, _ = CASES[name]
    O = reference(name)
    birth, length = np.asarray(O.birth), np.asarray(O.length)
    n_flows = T - 1
    # the inputs do what the case is for
    if n_flows >= 2:
        assert (birth == n_flows - 1).any(), "the last frame has births"
        assert set(range(n_flows)) <= set(birth.tolist())
    if kill is not None:
        assert (birth == kill + 1).sum() == grid(name) - 1, "every grid point (but the reference's phantom at 0) respawns behind the all-occluded pair"
    if name == "260x260_r2":
        assert (grid(name) + 255) // 256 >= 64, "the shape must band the lanes"
    R, placed, forms = gpu_track(name)
    if name == "200x200_r1_noisy":
        assert (length == 1).any(), "newborns lost in their first step"
        assert R.info["n_lanes_peak"] > grid(name), "the lane counter did not grow: no birth went beyond its block's free and guest lanes"
    _check(name, R, placed, forms, four_passes)


@pytest.mark.parametrize("name", ["46x62_r2", "260x260_r2", "70x90_r3"])
def test_placed_finalize_behind_the_fused_flow_check(name):
    """psfm_connect: the loop computes the occlusion maps itself (another code path around the same frame loop)."""
    import torch
    from oracle import oracle as orc
    from point_trajectory import trajectory, _hip
    ff, fb, _ = inputs(name)
    _, occ = orc.flow_check(ff, fb, 1.0)
    assert all(np.array_equal(a, b) for a, b in zip(occ, inputs(name)[2]))
    O = reference(name)
    ctx = _hip.context()
    ctx.set_chain_mode(2)
    try:
        R = trajectory.run_connect(torch.from_numpy(np.stack(ff)).cuda(), torch.from_numpy(np.stack(fb)).cuda(), None, None, 1.0, CASES[name][3])
        assert R.info["chain_mode"] == 2 and ctx.finalize_placed() == 1
    finally:
        ctx.set_chain_mode(0)
    assert np.array_equal(R.birth, O.birth) and np.array_equal(R.length, O.length) and np.array_equal(R.xy, O.xy)


def test_nothing_of_a_call_leaks_into_the_next(four_passes):
    """Different sequences back to back on one context, and the first ones again: the birth masks a call reads are all written by
    that call (longer sequences and other shapes in between, so that a call finds the others' masks where its own belong)."""
    for name in ("46x62_r2_all_occluded", "46x62_r2_3_frames", "46x62_r2", "46x62_r2_all_occluded", "30x40_r1", "46x62_r2"):
        R, placed, forms = gpu_track(name)
        _check(name, R, placed, forms, four_passes)


if __name__ == "__main__":
    # the program of the PSFM_FIN_PLACE=0 process: every case through psfm_track, arrays to argv[1]
    assert os.environ.get("PSFM_FIN_PLACE") == "0"
    res = {}
    for case in CASES:
        R_, placed_, _ = gpu_track(case)
        for k_, v_ in _arrays(R_).items():
            res["%s/%s" % (case, k_)] = v_
        res["%s/placed" % case] = np.int32(placed_)
    np.savez(sys.argv[1], **res)
