#!/usr/bin/env python3
"""Golden vectors for the motion-boundary option, produced by the REFERENCE's own point_trajectory Python (oracle/ref_shim.load()):

  motion_boundary_masks.npz   trajectory.py:39-43 (motion_boundary, with utils.py:107-113) on flow maps, at thres 0.02 and 0.3
  motion_boundary_steps.npz   trajectory.py:45-62 (step_forward) on hand-placed positions, in both forms of its kill rule
  mb_track_*.npz, mb_opt_*.npz   track / track_optimize over whole sequences, in both forms

The motion-boundary form of step_forward is the reference's OWN function with its commented line switched on: the source comes
from inspect.getsource at run time, the `#flags = ... (1.0 - np.squeeze(mb_cond))` line is un-commented, the live `flags =` line is
deleted (each pattern must occur exactly once), the text is exec'd in the module's namespace and bound to the `step_forward` name
of the loaded track and track_optimize modules.  No reference text is stored: only arrays.

The whole-sequence inputs are psfm_synth.synth_realistic WITHOUT its error terms (tests/_motion_boundary_np.SEQ_SYNTH): the other
synthetic families make nearly every pixel a boundary.  Asserted here, on the reference alone, for every whole-sequence case: the
mean mask density lies between 1 % and 20 %, and the result differs from the shipped-rule run of the same input.
The solver of the track_optimize case is ref_shim's default optimize_location (the oracle's), wrapped to record its statistics.

Run where a reference checkout is present (PSFM_REFERENCE_ROOT), never on the GPU machine:
    python tests/golden/make_motion_boundary_golden.py
"""
import inspect
import os
import re
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for p in (ROOT, os.path.join(ROOT, "particle-sfm_amd"), TESTS):
    sys.path.insert(0, p)
import psfm_synth                                   # noqa: E402
from oracle import oracle as orc                   # noqa: E402
from oracle import ref_shim                        # noqa: E402
from _common import input_hash                      # noqa: E402
import _motion_boundary_np as mbn                   # noqa: E402

MAX_BYTES = 1 << 20


def motion_boundary_step_forward(ref):
    """The reference's step_forward with the motion-boundary line live."""
    src = inspect.getsource(ref.trajectory.step_forward)
    commented = re.compile(r"^(\s*)#(flags = .*\(1\.0 - np\.squeeze\(mb_cond\)\)\s*)$", re.M)
    live = re.compile(r"^\s*flags = valid_cond \* \(1\.0 - np\.squeeze\(occ_cond\)\)\s*\n", re.M)
    assert len(commented.findall(src)) == 1 and len(live.findall(src)) == 1
    src = live.sub("", src)
    src = commented.sub(lambda m: m.group(1) + m.group(2), src)
    ns = {}
    exec(compile(src, "<step_forward with motion boundary>", "exec"), vars(ref.trajectory), ns)
    return ns["step_forward"]


class Rule:
    """Binds one form of step_forward to the names the reference's frame loops call."""

    def __init__(self, ref, fn):
        self.mods = [sys.modules[ref.track.__module__], sys.modules[ref.track_optimize.__module__]]
        self.fn = fn

    def __enter__(self):
        self.saved = [m.step_forward for m in self.mods]
        for m in self.mods:
            m.step_forward = self.fn

    def __exit__(self, *exc):
        for m, f in zip(self.mods, self.saved):
            m.step_forward = f
        return False


def save(name, **arrays):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **arrays)
    assert os.path.getsize(path) <= MAX_BYTES, (name, os.path.getsize(path))
    return os.path.getsize(path)


# ---- masks -----------------------------------------------------------------------------------------------------------------------

def mask_inputs():
    rng = np.random.default_rng(20)
    out = {}
    for name, (h, w) in (("m2x2", (2, 2)), ("m2x5", (2, 5)), ("m5x2", (5, 2)), ("m3x7", (3, 7))):
        f = rng.normal(0, 2.0, size=(1, h, w, 2)).astype(np.float32)
        f[0, 0, 0] = f[0, 0, 1]                     # an exact zero gradient
        out[name] = f
    for name, (h, w), seed in (("m37x53", (37, 53), 5), ("m48x64", (48, 64), 3)):
        d = psfm_synth.synth_realistic(3, h, w, seed=seed, stride2=False, **dict(psfm_synth.REALISTIC, **mbn.SEQ_SYNTH))
        out[name] = np.stack(d["flows_f"][:1])
    out["stack2_3x5"] = rng.normal(0, 1.5, size=(2, 3, 5, 2)).astype(np.float32)
    f = rng.normal(0, 3.0, size=(1, 12, 13, 2)).astype(np.float32)
    vals = np.array(psfm_synth.NONFINITE_VALUES, np.float32)
    for k in range(40):
        f[0, rng.integers(0, 12), rng.integers(0, 13), rng.integers(0, 2)] = vals[k % len(vals)]
    f[0, 5, 5:7, 0] = np.inf                        # inf - inf across a column pair, and down a row pair
    f[0, 8:10, 3, 1] = -np.inf
    f[0, 11, 12] = (np.nan, 1.0)                    # the corner pixel
    out["nonfinite_12x13"] = f
    tiny = np.array([1e-20, 1e-21, 1e-22, 1e-23, -1e-20, -1e-22, 3e-23, -0.0, 0.0, 2e-19], np.float32)
    out["subnormal_6x7"] = tiny[rng.integers(0, len(tiny), size=(1, 6, 7, 2))]
    f = rng.normal(0, 1.0, size=(1, 6, 6, 2)).astype(np.float32)
    f[0, 1:3, 1:4] = 0.0
    f[0, 4, :, :] = 0.0
    f[0, 0, 5] = (0.0, -0.0)
    out["zeros_6x6"] = f
    assert sorted(out) == sorted(mbn.MASK_CASES)
    return out


def make_masks(ref):
    arrays = {}
    for name, stack in mask_inputs().items():
        arrays[name + "__flow"] = stack
        for key, thres in mbn.MASK_THRES.items():
            with np.errstate(all="ignore"), warnings.catch_warnings():
                warnings.simplefilter("ignore")
                m = np.stack([ref.trajectory.motion_boundary(f, thres) for f in stack])
            assert m.dtype == bool and m.shape == stack.shape[:3]
            arrays[name + "__" + key] = m
        print("  %-18s %-14s density %.3f / %.3f" % (name, stack.shape, arrays[name + "__mb002"].mean(), arrays[name + "__mb03"].mean()))
    sub = arrays["subnormal_6x7__flow"].astype(np.float64)
    assert ((sub * sub > 0) & (sub * sub < 1.1754944e-38)).any() and (np.float32(1e-23) * np.float32(1e-23) == 0)
    assert np.isnan(arrays["nonfinite_12x13__flow"]).any() and arrays["nonfinite_12x13__mb002"].any()
    return save(mbn.MASK_FIXTURE, **arrays)


# ---- steps -----------------------------------------------------------------------------------------------------------------------

def make_steps(ref, mb_step):
    rng = np.random.default_rng(21)
    H, W = 9, 11
    yy, xx = np.mgrid[0:H, 0:W]
    flow = np.stack([0.8 * np.sin(xx / 3.0) + 0.3, 0.6 * np.cos(yy / 2.5) - 0.2], -1).astype(np.float32)
    flow += rng.normal(0, 0.05, size=flow.shape).astype(np.float32)
    occ = rng.uniform(size=(H, W)) < 0.12
    mb = rng.uniform(size=(H, W)) < 0.12
    # a clean neighbourhood with one occluded and one boundary pixel side by side, and a lone boundary pixel
    occ[2:6, 2:8] = False
    mb[2:6, 2:8] = False
    occ[3, 3] = True
    mb[3, 4] = True
    mb[5, 6] = True
    pts = [rng.uniform([-1.2, -1.2], [W + 0.2, H + 0.2], size=(500, 2))]
    pts.append(np.stack([xx.ravel(), yy.ravel()], 1).astype(np.float64))                       # on the pixels
    pts.append(np.stack([xx.ravel() + 0.5, yy.ravel() + 0.25], 1)[::3])                        # between them
    planted = [
        # taps (3,3) occluded and (4,3) boundary, rows 3 / 4: north weights 0.15 x 0.5 = 0.075 each (0.05 < w < 0.1): each verdict
        # stays below 0.1, their OR does not
        (3.5, 3.85), (3.45, 3.86), (3.55, 3.84),
        # the same pair seen from the row above: south weights 0.075 each
        (3.5, 2.15),
        # the lone boundary pixel (6,5) as the east tap of row 5: weight just above / just below 0.1
        (5.101, 5.0), (5.099, 5.0), (5.11, 5.0), (5.09, 5.0),
        # ... and as the south tap of column 6
        (6.0, 4.101), (6.0, 4.099),
        # taps that leave the map
        (-0.5, 3.0), (-0.999, 0.5), (W - 0.5, 4.0), (W - 1.0, H - 1.0), (3.0, -0.5), (4.5, H - 0.5), (-0.5, -0.5), (W - 0.25, H - 0.25),
        (-1.5, 3.0), (W + 0.1, 2.0), (0.0, 0.0), (5.0, H + 0.15),
    ]
    pts.append(np.array(planted, np.float64))
    xy = np.concatenate(pts, 0)
    import torch
    flow_t = torch.from_numpy(flow).permute(2, 0, 1).float()
    fs = ref.grid_sample(flow_t, xy.copy())
    nxt_s, flags_s = ref.step_forward(xy.copy(), fs, occ, mb)
    nxt_m, flags_m = mb_step(xy.copy(), fs, occ, mb)
    assert np.array_equal(nxt_s, nxt_m)
    alive_s, alive_m = np.asarray(flags_s) != 0, np.asarray(flags_m) != 0
    assert not (alive_m & ~alive_s).any() and (alive_s & ~alive_m).any()
    n_pl = len(planted)
    # the planted cases do what they are there for, by the reference's own verdicts
    assert alive_m[-n_pl:][:4].all() and alive_m[-n_pl:][[4, 6, 8]].sum() == 0 and alive_m[-n_pl:][[5, 7, 9]].all()
    return save(mbn.STEP_FIXTURE, flow=flow, occ=occ, mb=mb, xy=xy, flow_sample=np.asarray(fs, np.float32), next=np.asarray(nxt_m, np.float64),
                alive_mb=alive_m, alive_shipped=alive_s, n_planted=np.int64(n_pl))


# ---- whole sequences -------------------------------------------------------------------------------------------------------------

def run_sequence(ref, mb_step, name, T, H, W, ratio, seed, optimize):
    d = psfm_synth.synth_realistic(T, H, W, seed=seed, stride2=optimize, **dict(psfm_synth.REALISTIC, **mbn.SEQ_SYNTH))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, occ = ref.flow_check(d["flows_f"], d["flows_b"], 1.0)
        occ2 = ref.flow_check(d["flows_f2"], d["flows_b2"], 1.0)[1] if optimize else None
    density = float(np.mean([ref.trajectory.motion_boundary(f).mean() for f in d["flows_f"]]))
    assert 0.01 <= density <= 0.20, (name, density)
    out = dict(T=T, H=H, W=W, ratio=ratio, seed=seed, input_hash=input_hash(d), mb_density=density,
               occ_density=float(np.mean([o.mean() for o in occ])))
    solver = ref.particlesfm.optimize_location
    for key, fn in (("shipped", ref.trajectory.step_forward), ("mb", mb_step)):
        stats = []

        def recording(uv12, r1, r2, sc, fm, n, w, h):
            res, st = orc.optimize_location(uv12, r1, r2, sc, fm, n, w, h, return_stats=True)
            stats.append(st)
            return res
        ref.particlesfm.optimize_location = recording
        try:
            with Rule(ref, fn), warnings.catch_warnings():
                warnings.simplefilter("ignore")
                full = ref.track_optimize(d["flows_f"], d["flows_f2"], occ, occ2, ratio) if optimize else ref.track(d["flows_f"], occ, ratio)
        finally:
            ref.particlesfm.optimize_location = solver
        birth, length, off, xy = ref_shim.trajs_to_csr(full)
        out.update({key + "_birth": birth, key + "_length": length, key + "_xy": xy})
        if optimize:
            for k in ("iterations", "successful_steps", "termination", "dogleg_nonGN"):
                out["%s_solve_%s" % (key, k)] = np.array([s[k] for s in stats], np.int32)
        print("  %-22s %-8s %6d trajectories %7d points" % (name, key, len(birth), len(xy)))
    same = (len(out["mb_birth"]) == len(out["shipped_birth"]) and np.array_equal(out["mb_length"], out["shipped_length"])
            and np.array_equal(out["mb_xy"], out["shipped_xy"]))
    assert not same, name
    print("  %-22s mask density %.3f, occluded %.3f" % (name, density, out["occ_density"]))
    return save(name, **out)


def main():
    orc.build()
    ref = ref_shim.load()
    mb_step = motion_boundary_step_forward(ref)
    print("masks", make_masks(ref), "bytes")
    print("steps", make_steps(ref, mb_step), "bytes")
    print(run_sequence(ref, mb_step, mbn.SEQ_TRACK[0], 9, 48, 64, 2, 3, False), "bytes")
    print(run_sequence(ref, mb_step, mbn.SEQ_TRACK[1], 7, 37, 53, 1, 4, False), "bytes")
    print(run_sequence(ref, mb_step, mbn.SEQ_OPT[0], 9, 48, 64, 2, 3, True), "bytes")


if __name__ == "__main__":
    main()
