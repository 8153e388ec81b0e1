"""traj_to_matches and the window sampler on LONG trajectories, against plain-loop restatements written in this file.

The golden fixtures of test_consumers_golden.py hold trajectories of at most 27 points, so `n // sample_k` is 1 there and the
sampling branch of sfm/matches_from_flow.py:83-101 (n > K: the targets k * (n // K), the point itself skipped) runs only with
stride 1.  Here two sequences (r = 2, stride-1 flows) whose trajectories reach the whole sequence:

    48 x 64 x 101   sigma 0.02, 1 occluder, amp 1.0, seed 5     2 370 saved trajectories, 711 of >= 40 points, longest 101
    24 x 32 x 300   sigma 0.02, no occluder, amp 0.5, seed 5    1 093 saved trajectories, 394 of >= 40 points, longest 300
                                                                (300 images: frame sort of 9 bits, pair keys of 17+ bits)

with sample_k in {20, 7, 2, 1} and three labellings: none, 10 % random dynamic points, and designed labels that mark the tail of
each long trajectory dynamic so that the kept counts land on K-1, K, K+1, 2K-1, 2K, 2K+1 and 3K+1 -- the edges of `n <= K`, of
`n // K` and of the device's `j / stride < K` skip (csrc/psfm_matches.hip).

CPU part: psfm_sfm.matches_from_flow.match_tables_host + assemble from the oracle's trajectories.
GPU part (-m gpu): the device result of psfm_track (first checked bit-equal to the oracle's), then psfm_traj_to_matches on it; and
psfm_window_sample at the window edges of the 300-frame result, against a NumPy restatement of sample_inside_window + normalisation.
"""
import numpy as np
import pytest

import psfm_synth
from _common import check_match_tables, reference_sample_window

SEQS = {
    "48x64x101": dict(T=101, H=48, W=64, synth=dict(sigma=0.02, n_occluders=1, amp=1.0, seed=5)),
    "24x32x300": dict(T=300, H=24, W=32, synth=dict(sigma=0.02, n_occluders=0, amp=0.5, seed=5)),
}
KS = [20, 7, 2, 1]
LABELS = ["none", "random10", "designed"]
RATIO = 2


def loop_matches(off, frames, xy, labels, n_img, sample_k):
    """sfm/matches_from_flow.py:63-101 as plain loops, trajectory by trajectory in id order:
      :71-81  a point labelled dynamic is dropped; every kept point is appended to its image's keypoints, its keypoint index is the
              length of that list after the append;
      :83-101 kept point j of a trajectory with n kept points matches every other kept point when n <= K, otherwise the K points at
              k * (n // K), k = 0..K-1, skipping the one that is j itself; a match is the row (own keypoint index, target's keypoint
              index) filed under the image of j in a dict keyed by the target's image (insertion order = first use).
    Returns (keypoints per image, [{target image: [rows]} per image])."""
    kps = [[] for _ in range(n_img)]
    pairs = [{} for _ in range(n_img)]
    for t in range(len(off) - 1):
        imgs, kpi = [], []
        for p in range(int(off[t]), int(off[t + 1])):
            if labels[p]:
                continue
            f = int(frames[p])
            kps[f].append((float(xy[p, 0]), float(xy[p, 1])))
            kpi.append(len(kps[f]) - 1)
            imgs.append(f)
        n = len(imgs)
        targets = list(range(n)) if n <= sample_k else [k * (n // sample_k) for k in range(sample_k)]
        for j in range(n):
            for tj in targets:
                if tj == j:
                    continue
                pairs[imgs[j]].setdefault(imgs[tj], []).append((kpi[j], kpi[tj]))
    return kps, pairs


def _loop_as_fixture(kps, pairs):
    """The loop's tables in the layout of tests/golden/matches_*.npz."""
    kp_off = np.cumsum([0] + [len(k) for k in kps])
    kp_xy = np.array([p for k in kps for p in k], np.float64).reshape(-1, 2)
    src, tgt, blocks = [], [], []
    for i, d in enumerate(pairs):
        for j, rows in d.items():
            src.append(i)
            tgt.append(j)
            blocks.append(np.array(rows, np.int32).reshape(-1, 2))
    pair_off = np.cumsum([0] + [len(b) for b in blocks])
    rows = np.concatenate(blocks, 0) if blocks else np.zeros((0, 2), np.int32)
    return dict(kp_off=kp_off, kp_xy=kp_xy, pair_src=np.array(src, np.int64), pair_tgt=np.array(tgt, np.int64), pair_off=pair_off,
                rows=rows)


def _flows(seq):
    s = SEQS[seq]
    return psfm_synth.synth_sequence(s["T"], s["H"], s["W"], stride2=False, **s["synth"])


def _saved_csr(R, min_len=3):
    keep = R.length >= min_len
    length = R.length[keep].astype(np.int64)
    off = np.zeros(int(keep.sum()) + 1, np.int64)
    np.cumsum(length, out=off[1:])
    frames = np.concatenate([np.arange(b, b + n) for b, n in zip(R.birth[keep], length)]).astype(np.int64)
    xy = R.xy[np.repeat(keep, R.length)]
    return off, frames, xy


def _labels(kind, off, sample_k, seed):
    n_pts = int(off[-1])
    if kind == "none":
        return np.zeros(n_pts, bool)
    if kind == "random10":
        return np.random.default_rng(seed).uniform(size=n_pts) < 0.1
    # designed: trajectory t keeps its first targets[t % 7] points (when it has that many), the tail is dynamic
    K = sample_k
    targets = [K - 1, K, K + 1, 2 * K - 1, 2 * K, 2 * K + 1, 3 * K + 1]
    lab = np.zeros(n_pts, bool)
    for t in range(len(off) - 1):
        n, want = int(off[t + 1] - off[t]), targets[t % len(targets)]
        if want <= n:
            lab[off[t] + want:off[t + 1]] = True
    return lab


@pytest.fixture(scope="module")
def long_cases():
    """Per sequence: the oracle's maps and result, the saved set as CSR, and -- filled lazily, shared by the CPU and GPU parts -- the
    loop's tables per (sample_k, labels)."""
    import os
    from oracle import oracle as orc
    orc.set_num_threads(min(16, os.cpu_count() or 1))
    out = {}
    for seq in SEQS:
        d = _flows(seq)
        _, occ = orc.flow_check(d["flows_f"], d["flows_b"], 1.0)
        R = orc.track(d["flows_f"], occ, RATIO)
        off, frames, xy = _saved_csr(R)
        out[seq] = dict(flows=d["flows_f"], occ=occ, R=R, off=off, frames=frames, xy=xy, loop={})
    return out


def _case(c, seq, K, kind):
    """(labels, loop tables) of one case; the loop runs once per case per session."""
    key = (K, kind)
    if key not in c["loop"]:
        lab = _labels(kind, c["off"], K, seed=1000 + K)
        c["loop"][key] = (lab, _loop_as_fixture(*loop_matches(c["off"], c["frames"], c["xy"], lab, SEQS[seq]["T"], K)))
    return c["loop"][key]


def test_sequences_cover_long_trajectories(long_cases):
    """The two sequences are what the module docstring says: trajectories far longer than 2K for every K, a 300-image list."""
    for seq, (n_saved, n40, longest) in {"48x64x101": (2370, 711, 101), "24x32x300": (1093, 394, 300)}.items():
        length = np.diff(long_cases[seq]["off"])
        assert (len(length), int((length >= 40).sum()), int(length.max())) == (n_saved, n40, longest)


def test_designed_labels_hit_the_sampling_edges(long_cases):
    """Every kept count the designed labels aim at occurs for every K (on trajectories long enough for 3K+1)."""
    for seq, c in long_cases.items():
        for K in KS:
            lab = _labels("designed", c["off"], K, 0)
            kept = np.add.reduceat(~lab, c["off"][:-1]) if len(lab) else np.zeros(0)
            for want in {K - 1, K, K + 1, 2 * K - 1, 2 * K, 2 * K + 1, 3 * K + 1} - {0}:
                assert (kept == want).sum() >= 5, (seq, K, want)


@pytest.mark.parametrize("kind", LABELS)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("seq", list(SEQS))
def test_host_match_tables_equal_loop(long_cases, seq, K, kind, tmp_path):
    from psfm_sfm import matches_from_flow as mff
    c = long_cases[seq]
    lab, want = _case(c, seq, K, kind)
    T = SEQS[seq]["T"]
    names = ["%05d.png" % i for i in range(T)]
    tables = mff.match_tables_host(c["off"], c["frames"], c["xy"], lab, T, remove_dynamic=True, sample_k=K)
    check_match_tables(mff.assemble(names, tables, str(tmp_path / "pairs.txt"), as_arrays=True), names, want)


# ---------------------------------------------------------------------------------------------------------------------------- GPU


def _device_result(c):
    """psfm_track on the oracle's maps; the device result must be the oracle's before anything reads it."""
    import torch
    from point_trajectory import _hip
    from point_trajectory.trajectory import run_track, _result_to_host
    ctx = _hip.context()
    fl = torch.from_numpy(np.stack(c["flows"])).cuda()
    oc = torch.from_numpy(np.stack(c["occ"]).astype(np.uint8)).cuda()
    info = run_track(fl, oc, None, None, RATIO, return_device=True)
    D, R = _result_to_host(ctx, info), c["R"]
    assert len(D) == R.n_traj and D.n_points == R.n_points
    assert np.array_equal(D.birth, R.birth) and np.array_equal(D.length, R.length) and np.array_equal(D.xy, R.xy)
    return ctx


@pytest.mark.gpu
@pytest.mark.parametrize("seq", list(SEQS))
def test_device_match_tables_equal_loop(long_cases, seq, tmp_path):
    """psfm_result_filter -> psfm_traj_to_matches for every K and labelling, element for element the loop's tables; and once more
    with an image list 5 longer than the sequence (empty trailing images)."""
    import torch
    from psfm_sfm import matches_from_flow as mff
    c = long_cases[seq]
    ctx = _device_result(c)
    T = SEQS[seq]["T"]
    names = ["%05d.png" % i for i in range(T)]
    for K in KS:
        for kind in LABELS:
            lab, want = _case(c, seq, K, kind)
            lab_d = torch.from_numpy(lab.astype(np.uint8)).cuda() if kind != "none" else None
            tables = mff.match_tables_device(ctx, T, 3, K, lab_d)
            check_match_tables(mff.assemble(names, tables, str(tmp_path / "pairs.txt"), as_arrays=True), names, want)
    lab, want = _case(c, seq, 20, "random10")
    names5 = ["%05d.png" % i for i in range(T + 5)]
    tables = mff.match_tables_device(ctx, T + 5, 3, 20, torch.from_numpy(lab.astype(np.uint8)).cuda())
    assert np.array_equal(tables[0][T:], np.full(6, want["kp_off"][-1]))        # kp_off flat over the empty images
    want5 = dict(want, kp_off=np.concatenate([want["kp_off"], np.full(5, want["kp_off"][-1])]))
    check_match_tables(mff.assemble(names5, tables, str(tmp_path / "pairs.txt"), as_arrays=True), names5, want5)


# (frame0, n_frames, min_length, traj_min_len): first frame, across frame 255, ending at the last frame, one-frame windows,
# min_length = n_frames, and the saved set's filter at 1 and 3
WINDOWS = [(0, 16, 3, 3), (0, 16, 3, 1), (248, 16, 3, 3), (250, 12, 12, 1), (284, 16, 3, 3), (284, 16, 16, 3),
           (0, 1, 1, 3), (255, 1, 1, 1), (299, 1, 1, 3), (299, 1, 0, 1), (240, 60, 60, 3), (0, 300, 3, 1)]


@pytest.mark.gpu
def test_device_windows_at_the_edges_of_the_300_frame_result(long_cases):
    """psfm_window_sample (ids, raw and normalised coordinates, absence masks) at the edges of a 300-frame result, against
    sample_inside_window + data_utils.py:74-89 restated in NumPy on the oracle's trajectories."""
    from psfm_motion_seg.load_cut_seq import sample_window_device
    c = long_cases["24x32x300"]
    R = c["R"]
    ctx = _device_result(c)
    H, W, in_hw = SEQS["24x32x300"]["H"], SEQS["24x32x300"]["W"], (10, 14)
    for f0, n, min_length, tml in WINDOWS:
        ids, raw, nor, mask = sample_window_device(ctx, f0, n, (H, W), in_hw, traj_max_num=10 ** 9, min_length=min_length,
                                                   traj_min_len=tml)
        w_ids, w_raw, w_nor, w_mask = reference_sample_window(R.birth, R.length, R.off, R.xy, f0, n, min_length, tml, (H, W), in_hw)
        assert len(w_ids) > 0, (f0, n, min_length, tml)
        assert np.array_equal(ids.cpu().numpy().astype(np.int64), w_ids), (f0, n, min_length, tml)
        assert np.array_equal(raw.cpu().numpy(), w_raw), (f0, n, min_length, tml)
        assert np.array_equal(nor.cpu().numpy(), w_nor), (f0, n, min_length, tml)
        assert np.array_equal(mask.cpu().numpy(), w_mask), (f0, n, min_length, tml)
