#!/usr/bin/env python3
"""Recorded results of the REFERENCE's own functions for the tests that compare against them, so that those tests run without a
reference checkout:

  ref_traj_to_matches.npz      sfm/matches_from_flow.py::traj_to_matches on the inputs of tests/test_reference_consumers.py
                               (the committed track_gpu_60x80*.npy files, the long-track dict, the streamed track.npy layout):
                               per case the images in dict order, their keypoints, match lists in dict order, the pair file,
                               and a hash of the input the reference read
  refpy_opt_ct_60x84_r2.npz    the reference's track_optimize (Python, unmodified) with oracle/ceres_tr_numpy.py as the solver, on
                               the sequence of tests/test_oracle_golden.py::test_reference_python_with_the_second_restatement_as_solver

Only results are stored; the reference is imported unmodified through oracle/ref_shim.py.  Run where a reference checkout is
present (PSFM_REFERENCE_ROOT):
    python tests/golden/make_reference_runs_golden.py
"""
import os
import sys
import tempfile
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for p in (ROOT, os.path.join(ROOT, "particle-sfm_amd"), TESTS):
    sys.path.insert(0, p)
import psfm_synth                         # noqa: E402
from oracle import oracle as orc         # noqa: E402
from oracle import ref_shim              # noqa: E402
import test_reference_consumers as trc   # noqa: E402  (the tests' own input builders and record format)
from _common import input_hash           # noqa: E402


def encode(case, data, pairs_txt, in_hash):
    """One traj_to_matches result as flat arrays under `case__` (decoded by test_reference_consumers._recorded)."""
    names = list(data)
    kp_off, kp_xy, p_img, p_key, p_off, rows = [0], [], [], [], [0], []
    for i, n in enumerate(names):
        kp = np.asarray(data[n].keypoints, np.float64).reshape(-1, 2)
        kp_off.append(kp_off[-1] + len(kp))
        kp_xy.append(kp)
        for key, m in data[n].match_pairs.items():
            p_img.append(i)
            p_key.append(key)
            rows.append(np.asarray(m, np.int64).reshape(-1, 2))
            p_off.append(p_off[-1] + len(m))
    p = case + "__"
    return {p + "names": np.asarray(names), p + "kp_off": np.asarray(kp_off, np.int64),
            p + "kp_xy": np.concatenate(kp_xy, 0) if kp_xy else np.zeros((0, 2)),
            p + "pair_img": np.asarray(p_img, np.int32), p + "pair_key": np.asarray(p_key),
            p + "pair_off": np.asarray(p_off, np.int64), p + "rows": np.concatenate(rows, 0) if rows else np.zeros((0, 2), np.int64),
            p + "pairs_txt": np.asarray(pairs_txt), p + "input_hash": np.asarray(in_hash)}


def run_reference(ref, traj_file_writer, n_img, remove_dynamic):
    with tempfile.TemporaryDirectory() as tmp:
        img_dir, traj_dir = os.path.join(tmp, "images"), os.path.join(tmp, "trajectories")
        os.makedirs(img_dir)
        os.makedirs(traj_dir)
        for i in range(n_img):
            open(os.path.join(img_dir, "%05d.png" % i), "w").close()
        traj_file_writer(os.path.join(traj_dir, "track.npy"))
        data = ref.traj_to_matches(img_dir, traj_dir, os.path.join(tmp, "pairs.txt"), remove_dynamic=remove_dynamic)
        return data, open(os.path.join(tmp, "pairs.txt")).read()


def main():
    ref = ref_shim.load_consumers()
    ref.tqdm = lambda it, *a, **k: it
    out = {}
    for fname, rd in (("track_gpu_60x80.npy", True), ("track_gpu_60x80_legacy.npy", True), ("track_gpu_60x80_legacy.npy", False)):
        src = os.path.join(HERE, fname)
        data, txt = run_reference(ref, lambda dst: open(dst, "wb").write(open(src, "rb").read()), 7, rd)
        out.update(encode(trc.case_name(fname, rd), data, txt, trc.file_hash(src)))
    trajs = trc.long_tracks()
    for rd in (True, False):
        data, txt = run_reference(ref, lambda dst: np.save(dst, trajs), trc.LONG_N_IMG, rd)
        out.update(encode(trc.case_name("long", rd), data, txt, trc.trajs_hash(trajs)))
    with tempfile.TemporaryDirectory() as tmp:
        ts, T, _ = trc.streamed_layout_set()
        streamed, generic = os.path.join(tmp, "streamed.npy"), os.path.join(tmp, "generic.npy")
        trc.write_streamed(streamed, ts)
        trc.write_generic(generic, ts)
        data, txt = run_reference(ref, lambda dst: open(dst, "wb").write(open(streamed, "rb").read()), T, True)
        data_g, txt_g = run_reference(ref, lambda dst: open(dst, "wb").write(open(generic, "rb").read()), T, True)
        assert txt == txt_g and list(data) == list(data_g)
        for n in data:
            assert data[n].keypoints == data_g[n].keypoints and data[n].match_pairs == data_g[n].match_pairs
        out.update(encode(trc.case_name("streamed", True), data, txt, trc.file_hash(streamed)))
    np.savez_compressed(os.path.join(HERE, trc.RECORD + ".npz"), **out)
    print(trc.RECORD, sorted({k.split("__")[0] for k in out}))

    # the reference's track_optimize with the second (NumPy) restatement in the solver's seat
    from oracle import ceres_tr_numpy as ct
    refpt = ref_shim.load_reference(optimize_location=lambda *a: ct.optimize_location(*a)[0])
    T, H, W, r, seed = 7, 60, 84, 2, 91
    d = psfm_synth.synth_sequence(T, H, W, seed=seed, sigma=0.25, n_occluders=2, stride2=True)
    _, occ = orc.flow_check(d["flows_f"], d["flows_b"], 1.0)
    _, occ2 = orc.flow_check(d["flows_f2"], d["flows_b2"], 1.0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        full = refpt.track_optimize(d["flows_f"], d["flows_f2"], occ, occ2, r)
    birth, length, off, xy = ref_shim.trajs_to_csr(full)
    np.savez_compressed(os.path.join(HERE, "refpy_opt_ct_60x84_r2.npz"), T=T, H=H, W=W, ratio=r, seed=seed, sigma=0.25, n_occluders=2,
                        input_hash=input_hash(d), birth=birth, length=length, off=off, xy=xy)
    print("refpy_opt_ct_60x84_r2", len(birth), "trajectories,", int(off[-1]), "points")


if __name__ == "__main__":
    main()
