"""Shared by tests/test_sparse_depth_host.py and tests/test_gpu_sparse_depth.py: the fixtures of tests/golden/sparse_depth_*/ (written by
the reference's own functions, tests/golden/make_sparse_depth_golden.py), a plain-loop statement of which observation wins a pixel,
and the acceptance check of the issue: support and winners exact, depth within 4 * 2^-53 * (|r20 X| + |r21 Y| + |r22 Z| + |t2|) of
the reference's -- the worst case of a three-term dot product plus one add in any order, with or without FMA (each of the at most
four roundings is relative to a partial sum bounded by that magnitude)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["a", "b", "c", "d", "e"]          # "f" fails in the reference (KeyError) and holds no maps


def case_dir(case):
    return os.path.join(GOLDEN, "sparse_depth_" + case)


_cache = {}


def fixture(case):
    """expected.npz of the case, loaded once and shared (read-only arrays)."""
    if case not in _cache:
        with np.load(os.path.join(case_dir(case), "expected.npz")) as z:
            f = {k: z[k] for k in z.files}
        for v in f.values():
            v.setflags(write=False)
        _cache[case] = f
    return _cache[case]


def winners(f, i):
    """Plain loop over image i of the fixture: (winner observation index per pixel or -1, magnitude of the bound per pixel)."""
    from psfm_sfm.convert import qvec2rotmat
    cam = list(f["cam_ids"]).index(f["camera_ids"][i])
    w, h = (int(v) for v in f["cam_wh"][cam])
    R, t = qvec2rotmat(f["qvecs"][i]), f["tvecs"][i]
    row = {int(k): n for n, k in enumerate(f["ids"].tolist())}
    win = np.full((h, w), -1, np.int64)
    mag = np.zeros((h, w))
    a, b = int(f["obs_off"][i]), int(f["obs_off"][i + 1])
    for p in range(a, b):
        pid = int(f["point3D_ids"][p])
        if pid == -1:
            continue
        x, y = (float(v) for v in f["xys"][p])
        px = min(max(int(round(x)), 0), w - 1)                  # Python's round: half to even, exact integers
        py = min(max(int(round(y)), 0), h - 1)
        X = f["xyz"][row[pid]]
        win[py, px] = p - a
        mag[py, px] = abs(R[2, 0] * X[0]) + abs(R[2, 1] * X[1]) + abs(R[2, 2] * X[2]) + abs(t[2])
    return win, mag


def assert_map_accepts(got, f, i):
    """got (h, w) f64 against the reference's map of image i."""
    ref = f["depth_%d" % i]
    assert got.shape == ref.shape and got.dtype == np.float64
    win, mag = winners(f, i)
    assert np.array_equal(ref != 0, win >= 0)                   # (the fixtures hold no exact-zero depth)
    assert np.array_equal(got != 0, ref != 0)
    err = np.abs(got - ref)
    bound = 4 * 2.0 ** -53 * mag
    assert np.all(err <= bound), (float(err.max()), float(bound[err > bound].min()))
    # the winner is the reference's: another observation of the pixel would miss the bound by orders of magnitude -- checked on the
    # fixture itself in test_sparse_depth_host.py (test_fixtures_hold_the_edges_they_are_there_for)
    return float(err.max())
