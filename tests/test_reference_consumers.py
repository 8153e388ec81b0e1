"""Drop-in proof on the consumer side: track.npy files written by this implementation ON THE GPU
(scripts/make_track_fixture.py -> tests/golden/track_gpu_60x80*.npy) are read by the REFERENCE's own, unmodified
sfm/matches_from_flow.py::traj_to_matches.  The reference is not part of this repository: what it returned on exactly these
inputs is recorded in tests/golden/ref_traj_to_matches.npz (tests/golden/make_reference_runs_golden.py, run where a reference
checkout is present), and every test first checks that its input is the one the record was made from.  The oracle provides the
expected trajectories."""
import hashlib
import os
import pickle
import sys

import numpy as np
import pytest

from _common import GOLDEN
import psfm_synth

RECORD = "ref_traj_to_matches"
LONG_N_IMG = 60


def case_name(what, remove_dynamic):
    return "%s_rd%d" % (what[:-4] if what.endswith(".npy") else what, int(remove_dynamic))


def file_hash(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def trajs_hash(trajs):
    h = hashlib.sha256()
    for tid in sorted(trajs):
        t = trajs[tid]
        h.update(np.asarray([tid] + list(t["frame_ids"]), np.int64).tobytes())
        h.update(np.asarray(t["locations"], np.float64).tobytes())
        h.update(np.asarray(t["labels"], bool).tobytes())
    return h.hexdigest()


class _Image:
    """One image of traj_to_matches' result as the reference returns it: keypoints [[x, y], ...], match_pairs {key: [[i, j], ...]}."""

    def __init__(self, keypoints):
        self.keypoints, self.match_pairs = keypoints, {}


def _recorded(case):
    """The reference's recorded traj_to_matches result of one case: (dict in its order, pair-file text, hash of its input)."""
    g = np.load(os.path.join(GOLDEN, RECORD + ".npz"))
    p = case + "__"
    names = [str(n) for n in g[p + "names"]]
    kp_off, kp_xy = g[p + "kp_off"], g[p + "kp_xy"]
    out = {n: _Image([[float(x), float(y)] for x, y in kp_xy[kp_off[i]:kp_off[i + 1]]]) for i, n in enumerate(names)}
    pair_off, rows = g[p + "pair_off"], g[p + "rows"]
    for j, (i, key) in enumerate(zip(g[p + "pair_img"], g[p + "pair_key"])):
        out[names[int(i)]].match_pairs[str(key)] = [[int(a), int(b)] for a, b in rows[pair_off[j]:pair_off[j + 1]]]
    return out, str(g[p + "pairs_txt"]), str(g[p + "input_hash"])


def long_tracks():
    """Trajectories longer than sample_k = 20 (strided sampling) and dynamic labels (motion-seg output is a plain dict)."""
    rng = np.random.default_rng(0)
    trajs = {}
    for tid in range(40):
        n = int(rng.integers(1, 58))
        b = int(rng.integers(0, LONG_N_IMG - n + 1))
        trajs[tid * 3] = {"frame_ids": list(range(b, b + n)), "locations": [rng.uniform(0, 100, 2) for _ in range(n)],
                          "labels": (rng.uniform(size=n) < 0.2).tolist()}
    return trajs


def streamed_layout_set():
    """The CSR-backed TrajectorySet the stage entry produces, on a seeded sequence: (set, number of frames, oracle result)."""
    from oracle import oracle as orc
    from point_trajectory.trajectory import TrajectoryList
    T, H, W, r = 9, 48, 64, 2
    d = psfm_synth.synth_sequence(T, H, W, seed=78, sigma=0.2, n_occluders=2, stride2=False)
    _, occ = orc.flow_check(d["flows_f"], d["flows_b"], 1.0)
    O = orc.track(d["flows_f"], occ, r)
    return TrajectoryList(O.birth, O.length, O.off, O.xy).to_trajectory_set(3), T, O


def write_streamed(path, ts):
    """The DEFAULT writer (point_trajectory/reference_pickle.py: the reference's pickle state as opcodes straight from the CSR)."""
    from point_trajectory.trajectory import save_track_npy
    save_track_npy(path, ts)


def write_generic(path, ts):
    """The file the generic pickler writes from the same set."""
    arr = np.empty((), dtype=object)
    arr[()] = ts
    with open(path, "wb") as fp:
        np.lib.format.write_array_header_1_0(fp, np.lib.format.header_data_from_array_1_0(arr))
        pickle.dump(arr, fp, protocol=3)


def _dirs(tmp_path, n_img, tag=""):
    traj_dir, img_dir = tmp_path / tag / "trajectories", tmp_path / tag / "images"
    traj_dir.mkdir(parents=True)
    img_dir.mkdir(parents=True)
    for i in range(n_img):
        (img_dir / ("%05d.png" % i)).write_bytes(b"")
    return traj_dir, img_dir


def _assert_same_result(A, B):
    assert list(A) == list(B)
    for name in A:
        assert A[name].keypoints == B[name].keypoints
        assert list(A[name].match_pairs) == list(B[name].match_pairs)
        for k in A[name].match_pairs:
            assert A[name].match_pairs[k] == B[name].match_pairs[k], k


@pytest.mark.parametrize("fname", ["track_gpu_60x80.npy", "track_gpu_60x80_legacy.npy"])
def test_reference_traj_to_matches_consumes_our_track_npy(fname):
    from oracle import oracle as orc
    import point_trajectory  # noqa: F401  (makes point_trajectory.optimize.build.particlesfm resolvable for the unpickler)
    T, H, W, r = 7, 60, 80, 2
    d = psfm_synth.synth_sequence(T, H, W, seed=77, sigma=0.1, n_occluders=1, stride2=True)
    _, occ = orc.flow_check(d["flows_f"], d["flows_b"], 1.0)
    _, occ2 = orc.flow_check(d["flows_f2"], d["flows_b2"], 1.0)
    O = orc.track_optimize(d["flows_f"], d["flows_f2"], occ, occ2, r)
    keep = [i for i in range(O.n_traj) if O.length[i] >= 3]

    data, pairs_txt, read = _recorded(case_name(fname, True))
    assert file_hash(os.path.join(GOLDEN, fname)) == read, "the record was made from another %s" % fname
    # every kept trajectory point became one keypoint of its frame (sfm/matches_from_flow.py:67-86)
    n_kp = sum(len(v.keypoints) for v in data.values())
    assert n_kp == int(sum(O.length[i] for i in keep))
    # keypoints of frame 0 are the time-0 points of the kept trajectories born at 0, in id order
    exp0 = [O.xy[O.off[i]] for i in keep if O.birth[i] == 0]
    kp0 = np.array(data["00000.png"].keypoints)
    assert kp0.shape == (len(exp0), 2) and np.abs(kp0 - np.array(exp0)).max() <= 1e-4
    assert len(pairs_txt) > 0
    # and the object the consumers unpickle is this package's class at the reference's dotted path
    ts = np.load(os.path.join(GOLDEN, fname), allow_pickle=True).item()
    assert type(ts).__module__ == "point_trajectory.optimize.build.particlesfm"
    assert sorted(ts.as_dict()) == keep


@pytest.mark.parametrize("fname,remove_dynamic", [("track_gpu_60x80.npy", True), ("track_gpu_60x80_legacy.npy", False)])
def test_vectorised_traj_to_matches_equals_reference(tmp_path, fname, remove_dynamic):
    """particle-sfm_amd/psfm_sfm/matches_from_flow.py (NumPy index arithmetic on the CSR) against the
    reference's loops, element for element -- keypoints, match lists, dict ordering, pair file."""
    from psfm_sfm import matches_from_flow as ours   # particle-sfm_amd/psfm_sfm (conftest puts it on sys.path)
    traj_dir, img_dir = _dirs(tmp_path, 7)
    (traj_dir / "track.npy").write_bytes(open(os.path.join(GOLDEN, fname), "rb").read())
    A, a_txt, read = _recorded(case_name(fname, remove_dynamic))
    assert file_hash(str(traj_dir / "track.npy")) == read, "the record was made from another %s" % fname
    B = ours.traj_to_matches(str(img_dir), str(traj_dir), str(tmp_path / "b.txt"), remove_dynamic=remove_dynamic)
    _assert_same_result(A, B)
    assert a_txt == open(str(tmp_path / "b.txt")).read()
    # array form (what sfm/import_feature_matches.py:82,96 turns the lists into anyway)
    C = ours.traj_to_matches(str(img_dir), str(traj_dir), str(tmp_path / "c.txt"), remove_dynamic=remove_dynamic, as_arrays=True)
    for name in A:
        assert np.array_equal(np.array(A[name].keypoints).reshape(-1, 2), C[name].keypoints)
        for k in A[name].match_pairs:
            assert np.array_equal(np.array(A[name].match_pairs[k]), C[name].match_pairs[k])


def test_vectorised_traj_to_matches_long_tracks_and_dynamic_labels(tmp_path):
    """Trajectories longer than sample_k = 20 (strided sampling) and dynamic labels (motion-seg output is a plain dict)."""
    from psfm_sfm import matches_from_flow as ours
    trajs = long_tracks()
    traj_dir, img_dir = _dirs(tmp_path, LONG_N_IMG)
    np.save(str(traj_dir / "track.npy"), trajs)
    for rd in (True, False):
        A, a_txt, read = _recorded(case_name("long", rd))
        assert trajs_hash(trajs) == read, "the record was made from other trajectories"
        B = ours.traj_to_matches(str(img_dir), str(traj_dir), str(tmp_path / "b.txt"), remove_dynamic=rd)
        assert list(A) == list(B)
        for name in A:
            assert np.allclose(np.array(A[name].keypoints).reshape(-1, 2), np.array(B[name].keypoints).reshape(-1, 2), atol=0)
            assert list(A[name].match_pairs) == list(B[name].match_pairs)
            for k in A[name].match_pairs:
                assert A[name].match_pairs[k] == B[name].match_pairs[k]
        assert a_txt == open(str(tmp_path / "b.txt")).read()


def test_launcher_resolves_point_trajectory_here_and_the_other_stages_in_the_checkout(tmp_path):
    """`python run_particlesfm.py` puts the checkout at sys.path[0] ahead of PYTHONPATH; particle-sfm_amd/run_with_psfm.py
    fixes the order explicitly.  The driver's three package imports (run_particlesfm.py:21,61,78) must then resolve:
    point_trajectory -> this package; motion_seg, sfm -> the checkout (this package ships no package of those names).
    The checkout is a stand-in with the reference's three top-level packages (empty), its own point_trajectory included."""
    import subprocess
    import textwrap
    ref = tmp_path / "checkout"
    for name in ("point_trajectory", "motion_seg", "sfm"):
        (ref / name).mkdir(parents=True)
        (ref / name / "__init__.py").write_text("")
    pkg = os.path.join(os.path.dirname(GOLDEN), "..", "particle-sfm_amd")
    launcher = os.path.abspath(os.path.join(pkg, "run_with_psfm.py"))
    probe = tmp_path / "probe.py"
    probe.write_text(textwrap.dedent("""
        import importlib.util, json, sys
        out = {n: importlib.util.find_spec(n).origin for n in ("point_trajectory", "motion_seg", "sfm")}
        from point_trajectory import main_connect_point_trajectories
        out["entry"] = main_connect_point_trajectories.__module__
        out["argv"] = sys.argv[1:]
        print(json.dumps(out))
    """))
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    r = subprocess.run([sys.executable, launcher, "--ref", str(ref), str(probe), "--flag", "x"], capture_output=True, text=True,
                       env=env, cwd=str(ref), timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    import json
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert os.path.abspath(out["point_trajectory"]).startswith(os.path.abspath(pkg))
    assert os.path.abspath(out["motion_seg"]).startswith(os.path.abspath(str(ref)))
    assert os.path.abspath(out["sfm"]).startswith(os.path.abspath(str(ref)))
    assert out["entry"] == "point_trajectory.main_connect_point_trajectories" and out["argv"] == ["--flag", "x"]


def test_reference_traj_to_matches_consumes_the_streamed_reference_layout(tmp_path):
    """The DEFAULT writer (point_trajectory/reference_pickle.py: the reference's pickle state as opcodes straight from the CSR
    arrays) read by the reference's own, unmodified traj_to_matches: same keypoints, matches and pair file as from the file the
    generic pickler writes from the same trajectories (both checked when the record was made), and as this package's vectorised
    consumer returns from either file."""
    from point_trajectory import reference_pickle
    from psfm_sfm import matches_from_flow as ours
    ts, T, O = streamed_layout_set()
    assert reference_pickle.can_stream(ts)
    A, a_txt, read = _recorded(case_name("streamed", True))
    out, txt = {}, {}
    for tag, write in (("streamed", write_streamed), ("generic", write_generic)):
        traj_dir, img_dir = _dirs(tmp_path, T, tag)
        write(str(traj_dir / "track.npy"), ts)
        if tag == "streamed":
            assert file_hash(str(traj_dir / "track.npy")) == read, "the streamed file is not the one the reference was recorded reading"
        out[tag] = ours.traj_to_matches(str(img_dir), str(traj_dir), str(tmp_path / (tag + ".txt")), remove_dynamic=True)
        txt[tag] = open(str(tmp_path / (tag + ".txt"))).read()
    assert sum(len(v.keypoints) for v in A.values()) == int(O.length[O.length >= 3].sum())
    _assert_same_result(A, out["streamed"])
    _assert_same_result(A, out["generic"])
    assert a_txt == txt["streamed"] == txt["generic"]
