"""The finalize gather that sums in the write layout (psfm_gather_delta2_kernel; the rule: csrc/psfm_gather_exact.h): a half-wave forms
the prefix sum of a trajectory's 32 logged flows, and redoes in the loop's order every chunk in which an addition could have rounded.

Every case runs with the persistent loop required (chain mode 2) through run_track and is checked twice: against the CPU oracle
(births, lengths, offsets, positions bit for bit), and bit for bit against the same call in a process started with PSFM_FIN_GATHER=0,
which runs the serial kernel (one such process computes all cases; this file is its program when run as a script).  Which form ran is
asserted through psfm_ctx_get_finalize_gather: nothing in the bytes tells them apart."""
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

TINY = (1e-8, -3e-9)
STEP = (0.37, -0.21)
RATIO = 2
_IN, _REF = {}, {}


def _const(n_flows, H, W, uv):
    f = np.empty((n_flows, H, W, 2), np.float32)
    f[..., 0], f[..., 1] = uv
    return f


def _free(f):
    return [np.ascontiguousarray(x) for x in f], [np.zeros(f.shape[1:3], bool) for _ in range(len(f))]


def _edge(n_flows):
    return lambda: _free(_const(n_flows, 24, 30, (0.01, 0.02)))


def _mixed():
    f = _const(39, 30, 64, STEP)
    f[:, :, :32, 0], f[:, :, :32, 1] = TINY
    return _free(f)


def _sticky():
    f = _const(69, 30, 64, STEP)
    f[0, ..., 0], f[0, ..., 1] = TINY
    return _free(f)


def _big():
    f = _const(5, 6, 900, (0.25, 0.0))
    f[:2, ..., 0] = 300.0
    return _free(f)


def _synthetic(amp):
    def make():
        from oracle import oracle as orc
        d = psfm_synth.synth_sequence(70, 46, 62, seed=5, amp=amp, sigma=0.05, n_occluders=1, stride2=False)
        _, occ = orc.flow_check(d["flows_f"], d["flows_b"], 1.0)
        return d["flows_f"], [np.asarray(o).copy() for o in occ]
    return make


# name -> (flows, occlusion maps); all at sample ratio 2
CASES = {
    "points_32": _edge(31), "points_33": _edge(32), "points_34": _edge(33),     # a trajectory that ends on, one past, two past a chunk
    "zero": lambda: _free(_const(39, 30, 40, (0.0, 0.0))),                      # the zero class: positions stay integers
    "tiny": lambda: _free(_const(39, 30, 40, TINY)),                            # every chunk serial, every addition inexact
    "mixed": _mixed,                                                            # both classes inside one wave and one tile
    "sticky": _sticky,                                                          # three chunks, flagged in the first, x crossing 32
    "big": _big,                                                                # flows >= 2^8
    "synthetic": _synthetic(3.0),                                               # births, deaths and recycled lanes (the generator's own motion:
                                                                                #  no trajectory outlives 50 points, two chunks)
    "synthetic_calm": _synthetic(1.0),                                          # ... with a third of the motion: 185 trajectories of three chunks
}


def inputs(name):
    if name not in _IN:
        _IN[name] = CASES[name]()
    return _IN[name]


def reference(name):
    """The oracle's result of a case: computed once, shared, never modified."""
    if name not in _REF:
        from oracle import oracle as orc
        ff, occ = inputs(name)
        _REF[name] = orc.track(ff, occ, RATIO)
    return _REF[name]


def gpu_track(name):
    """(result, gather form) of psfm_track on the case with the persistent loop required."""
    from point_trajectory import trajectory, _hip
    ctx = _hip.context()
    ctx.set_chain_mode(2)
    try:
        ff, occ = inputs(name)
        R = trajectory.run_track(ff, occ, None, None, RATIO)
        return R, ctx.finalize_gather()
    finally:
        ctx.set_chain_mode(0)


def _bits(xy):
    return np.ascontiguousarray(xy, np.float64).view(np.uint64)


def _arrays(R):
    return {"birth": np.asarray(R.birth), "length": np.asarray(R.length), "off": np.asarray(R.off), "xy": np.asarray(R.xy)}


@pytest.fixture(scope="module")
def serial_kernel(tmp_path_factory):
    """Every case computed by a process with PSFM_FIN_GATHER=0 (read once per process): {case: arrays}."""
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    out = str(tmp_path_factory.mktemp("gather") / "serial_kernel.npz")
    env = dict(os.environ, PSFM_FIN_GATHER="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    z = np.load(out)
    return {name: {k: z["%s/%s" % (name, k)] for k in ("birth", "length", "off", "xy", "gather")} for name in CASES}


def _is_input_for(name, O):
    """The inputs do what the case is for."""
    length, xy = np.asarray(O.length), np.asarray(O.xy)
    n_flows = len(inputs(name)[0])
    if name.startswith("points_"):
        assert (length == n_flows + 1).all() and n_flows + 1 == int(name[7:])
    if name == "zero":
        assert (length == 40).sum() >= 200 and np.array_equal(xy, np.round(xy))          # (the frame's first row and column die at once)
    if name == "tiny":
        assert (length == 40).sum() >= 200 and not np.array_equal(xy, np.round(xy))
    if name == "mixed":
        x_last = xy[np.cumsum(length) - 1, 0]
        assert (length == 40).any() and (x_last < 31.0).any() and (x_last > 40.0).any()
    if name == "sticky":
        assert length.max() == 70 and (length < 70).any()
        first, last = np.cumsum(length) - length, np.cumsum(length) - 1
        assert ((xy[first, 0] < 32.0) & (xy[last, 0] > 32.0) & (length > 64)).any(), "no trajectory crosses x = 32 over three chunks"
    if name == "big":
        assert (length >= 3).any() and (np.abs(np.diff(xy[:, 0])) >= 256.0).any()
    if name.startswith("synthetic"):
        birth = np.asarray(O.birth)
        assert ((birth > 0) & (birth + length < 70)).sum() > 64 and (length > 32).any(), "born late, dead early; more than one chunk"
        assert name == "synthetic" or (length.max() == 70 and (length > 64).sum() > 64)


@pytest.mark.parametrize("name", list(CASES))
def test_blocked_gather_vs_oracle_and_serial_kernel(serial_kernel, name):
    O = reference(name)
    _is_input_for(name, O)
    R, gather = gpu_track(name)
    assert R.info["chain_mode"] == 2, "the persistent loop did not run"
    assert gather == 2, "the blocked gather did not run"
    a = _arrays(R)
    assert a["birth"].shape[0] == O.n_traj
    assert np.array_equal(a["birth"], O.birth) and np.array_equal(a["length"], O.length)
    assert np.array_equal(a["off"], np.concatenate([[0], np.cumsum(O.length)]))
    assert a["xy"].dtype == np.float64 and np.array_equal(_bits(a["xy"]), _bits(O.xy))
    old = serial_kernel[name]
    assert int(old["gather"]) == 1, "the other process did not run the serial kernel"
    for k in ("birth", "length", "off"):
        assert a[k].dtype == old[k].dtype and np.array_equal(a[k], old[k]), k
    assert np.array_equal(_bits(a["xy"]), _bits(old["xy"]))


if __name__ == "__main__":
    # the program of the PSFM_FIN_GATHER=0 process: every case through psfm_track, arrays to argv[1]
    assert os.environ.get("PSFM_FIN_GATHER") == "0"
    res = {}
    for case in CASES:
        R_, gather_ = gpu_track(case)
        for k_, v_ in _arrays(R_).items():
            res["%s/%s" % (case, k_)] = v_
        res["%s/gather" % case] = np.int32(gather_)
    np.savez(sys.argv[1], **res)
