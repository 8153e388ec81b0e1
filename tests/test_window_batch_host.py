"""The rules of psfm_window_sample_batch without a GPU: particle-sfm_amd/csrc/psfm_window_batch.h -- eligibility, the splitmix64 key,
the cap rule, the block -> (window, local row) lookup of the flattened grids and the offsets of a plan -- compiled for the host by
tests/host/window_batch_host.cpp and compared with the NumPy statement tests/_window_batch_np.py; then the NumPy statement against the
host TrajectorySet.sample_inside_window on the sequence of tests/test_window_sample_cap.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import _window_batch_np as wb
from test_window_sample_cap import _sequence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX, BLOCK, INT32_MAX = 64, 256, 2 ** 31 - 1


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("window_batch") / "libwindow_batch_host.so")
    cmd = ["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "tests", "host", "shim"),
           "-I", os.path.join(ROOT, "tests", "host"), "-I", os.path.join(ROOT, "particle-sfm_amd", "csrc"),
           os.path.join(ROOT, "tests", "host", "window_batch_host.cpp"), "-o", out]
    subprocess.run(cmd, check=True)
    L = ctypes.CDLL(out)
    vp = ctypes.c_void_p
    L.psfm_host_winb_eligible.argtypes = [ctypes.c_long] + [vp] * 8
    L.psfm_host_winb_eligible.restype = None
    L.psfm_host_winb_hash.argtypes = [ctypes.c_long, vp, vp, vp]
    L.psfm_host_winb_hash.restype = None
    L.psfm_host_winb_rows.argtypes = [ctypes.c_long, ctypes.c_long]
    L.psfm_host_winb_rows.restype = ctypes.c_long
    L.psfm_host_winb_normalise.argtypes = [ctypes.c_double] * 3
    L.psfm_host_winb_normalise.restype = ctypes.c_double
    L.psfm_host_winb_offsets.argtypes = [vp, ctypes.c_int, ctypes.c_long, ctypes.c_long, vp, vp]
    L.psfm_host_winb_offsets.restype = ctypes.c_long
    L.psfm_host_winb_find.argtypes = [vp, ctypes.c_int]
    return L


def test_the_bounds_are_the_decoder_batch_s(host):
    assert host.psfm_host_winb_max() == MAX == wb.MAX_WINDOWS and host.psfm_host_winb_block() == BLOCK == wb.BLOCK


def test_eligibility_and_hash_against_numpy(host):
    rng = np.random.default_rng(41)
    n = 20000
    i32 = lambda lo, hi: np.ascontiguousarray(rng.integers(lo, hi, n), dtype=np.int32)
    birth, length, f0, L = i32(0, 60), i32(1, 40), i32(-12, 80), i32(1, 65)
    tml, ml = i32(0, 8), i32(0, 8)
    ov, flag = np.zeros(n, np.int32), np.zeros(n, np.uint8)
    host.psfm_host_winb_eligible(n, *[a.ctypes.data for a in (birth, length, f0, L, tml, ml, ov, flag)])
    assert np.array_equal(ov, wb.overlap_np(birth, length, f0, L))
    want = wb.eligible_np(birth, length, f0, L, tml, ml)
    assert np.array_equal(flag.astype(bool), want) and 0.05 < want.mean() < 0.95
    # brute force on a few: count the frames
    for i in range(200):
        frames = set(range(int(birth[i]), int(birth[i] + length[i]))) & set(range(int(f0[i]), int(f0[i] + L[i])))
        assert ov[i] == len(frames)
        assert bool(flag[i]) == (length[i] >= tml[i] and len(frames) > 0 and len(frames) >= ml[i])
    seed = np.ascontiguousarray(rng.integers(0, 2 ** 63, n, dtype=np.int64).astype(np.uint64) * np.uint64(2) + rng.integers(0, 2, n).astype(np.uint64))
    seed[:4] = [0, 1, 2 ** 64 - 1, 2 ** 63]
    ids = np.ascontiguousarray(rng.integers(0, 2 ** 31 - 1, n), dtype=np.int32)
    ids[:3] = [0, 1, 2 ** 31 - 2]
    key = np.zeros(n, np.uint64)
    host.psfm_host_winb_hash(n, seed.ctypes.data, ids.ctypes.data, key.ctypes.data)
    assert np.array_equal(key, wb.hash_np(seed, ids))
    assert all(int(key[i]) == wb.hash_int(int(seed[i]), int(ids[i])) for i in range(300))
    assert len(np.unique(key)) == n
    # the cap rule and the normalisation
    for count, cap in ((0, 0), (5, 0), (5, 5), (5, 6), (6, 5), (10 ** 9, 1), (1, 10 ** 9)):
        assert host.psfm_host_winb_rows(count, cap) == min(count, cap)
    for v, raw, tgt in ((13.7, 56, 48), (55.999, 56, 48), (-0.5, 40, 32), (1e9, 40, 32), (0.0, 84, 48), (83.0, 84, 84)):
        assert host.psfm_host_winb_normalise(v, raw / tgt, float(tgt)) == float(np.clip(np.float64(v) / np.float64(raw / tgt) / np.float64(tgt), 0, 1))


def k_lists():
    """k hitting 0, 1, a block boundary +-1 -- in rows of 10 frames (25, 26 rows: 250, 260 elements), of 1 unit (255 .. 257) and in
    trajectories of an encoder block (24 at L = 10) -- in padded tables (fewer than 64 windows) and a full one."""
    rng = np.random.default_rng(12)
    sizes = [0, 1, 23, 24, 25, 26, 255, 256, 257, 700]
    out = [[k] for k in sizes] + [[0, 0, 0], [0, 1, 0, 26, 0], [1] * 7, [25, 26, 0, 0, 257], [700, 0, 1], [0] * 63 + [1], [1] + [0] * 63]
    out += [[int(k) for k in rng.choice(sizes, n)] for n in (2, 5, 17, 63, 64, 64)]
    return out


@pytest.mark.parametrize("ks", k_lists(), ids=lambda ks: "n%d_%s" % (len(ks), "_".join(str(k) for k in ks[:5])))
@pytest.mark.parametrize("units,per_block", [(10, BLOCK), (1, 24), (23, BLOCK), (1, 8), (64, BLOCK)])
def test_offsets_and_lookup_against_enumeration(host, ks, units, per_block):
    """units = n_frames and 256 elements per block (the gather, the augment); 1 and the trajectories of a block (the encoder: 24 at
    L = 10, 8 at L = 23 .. 32)."""
    k = (ctypes.c_long * MAX)(*ks)
    row0, blk0 = (ctypes.c_long * (MAX + 1))(), (ctypes.c_long * MAX)()
    blocks = host.psfm_host_winb_offsets(k, len(ks), units, per_block, row0, blk0)
    w_row0, w_blk0, w_blocks = wb.offsets_np(ks, units, per_block)
    assert list(row0) == w_row0 and list(blk0) == w_blk0 and blocks == w_blocks
    assert all(v == INT32_MAX for v in list(blk0)[len(ks):])
    # brute force: every (window, block in the window) once, window-major; a block's rows lie inside its window
    want = [(b, j) for b, kb in enumerate(ks) for j in range(-(-(kb * units) // per_block))]
    got = []
    for blk in range(blocks):
        b = host.psfm_host_winb_find(blk0, blk)
        assert b == wb.find_np(list(blk0), blk)
        got.append((b, blk - blk0[b]))
        first_unit = (blk - blk0[b]) * per_block
        assert 0 <= first_unit < ks[b] * units                                 # the block's first (window, local row) exists
        assert row0[b] + first_unit // units < row0[b + 1]
    assert got == want
    assert row0[len(ks)] == sum(ks) == row0[MAX]


def _oracle_tracks():
    from oracle import oracle as orc
    d = _sequence()
    _, occ = orc.flow_check(d["flows_f"], d["flows_b"], 1.0)
    return orc.track(d["flows_f"], occ, 2)


WINDOWS = [(0, 8), (3, 8), (6, 8), (30, 8)]          # the last lies outside the sequence (T = 14)


@pytest.fixture(scope="module")
def tracked():
    from point_trajectory.optimize.build.particlesfm import Trajectory, TrajectorySet
    R = _oracle_tracks()
    ts = TrajectorySet()
    length = np.diff(np.asarray(R.off, np.int64))
    for i in range(R.n_traj):
        xy = R.xy[R.off[i]:R.off[i + 1]]
        if len(xy) >= 3:                                                       # the saved set: traj_min_len = 3
            ts.insert(i, Trajectory(times=list(range(int(R.birth[i]), int(R.birth[i]) + len(xy))), xys=[tuple(p) for p in xy]))
    ts.build_invert_indexes()
    return R, length, ts


def test_numpy_statement_equals_the_host_class_without_a_cap(tracked):
    R, length, ts = tracked
    k, row0, ids, raw, mask, _ = wb.sample_windows_np(R.birth, length, R.off, R.xy, WINDOWS, [0, 1, 2, 3], 10 ** 9)
    assert k[3] == 0 and all(k[:3] > 100) and row0[-1] == len(ids) == k.sum()
    for b, (f0, L) in enumerate(WINDOWS[:3]):
        full = ts.sample_inside_window(list(range(f0, f0 + L)), 3, 10 ** 9)
        lo, hi = row0[b], row0[b + 1]
        assert ids[lo:hi].tolist() == list(full["traj_ids"]) == sorted(full["traj_ids"])
        assert np.array_equal(raw[lo:hi, :, 0], full["locations"][0]) and np.array_equal(raw[lo:hi, :, 1], full["locations"][1])
        assert np.array_equal(1.0 - mask[lo:hi], np.asarray(full["masks"], np.float64))
    assert len({tuple(ids[row0[b]:row0[b + 1]].tolist()) for b in range(3)}) == 3


def test_numpy_statement_above_the_cap(tracked):
    R, length, ts = tracked
    k_all, row_all, ids_all, raw_all, mask_all, _ = wb.sample_windows_np(R.birth, length, R.off, R.xy, WINDOWS, [0] * 4, 10 ** 9)
    cap = int(k_all[:3].min()) // 3
    assert cap > 30
    picks = {}
    for seeds in ([0, 0, 0, 0], [1, 2, 3, 4]):
        k, row0, ids, raw, mask, _ = wb.sample_windows_np(R.birth, length, R.off, R.xy, WINDOWS, seeds, cap)
        assert k.tolist() == [cap, cap, cap, 0]
        for b in range(3):
            mine = ids[row0[b]:row0[b + 1]]
            elig = ids_all[row_all[b]:row_all[b + 1]]
            assert len(set(mine.tolist())) == cap and set(mine.tolist()) <= set(elig.tolist())
            rows = row_all[b] + np.searchsorted(elig, mine)
            assert np.array_equal(raw[row0[b]:row0[b + 1]], raw_all[rows]) and np.array_equal(mask[row0[b]:row0[b + 1]], mask_all[rows])
            assert mine.tolist() != sorted(mine.tolist())
            keys = [wb.hash_int(seeds[b], int(i)) for i in mine]
            assert keys == sorted(keys) and max(keys) <= min(wb.hash_int(seeds[b], int(i)) for i in set(elig.tolist()) - set(mine.tolist()))
            picks[(tuple(seeds), b)] = set(mine.tolist())
    assert all(picks[((0, 0, 0, 0), b)] != picks[((1, 2, 3, 4), b)] for b in range(3))
    # at the cap, not above it: untouched, ascending
    k, row0, ids, _, _, _ = wb.sample_windows_np(R.birth, length, R.off, R.xy, WINDOWS[:1], [9], int(k_all[0]))
    assert np.array_equal(ids, ids_all[:k_all[0]])


def test_no_cpu_fallback(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    from psfm_motion_seg.augment import augment_windows_device
    from psfm_motion_seg.encoder import WEIGHT_COUNT, encode_windows_device
    from psfm_motion_seg.merge_labels import label_sequences_batched, label_trajectories_batched
    packed = np.zeros(WEIGHT_COUNT, np.float32)
    with pytest.raises(RuntimeError):
        augment_windows_device([np.zeros((4, 10, 2))], [np.zeros((4, 10, 1))], [np.zeros((10, 30, 50), np.float32)], (30, 50))
    with pytest.raises(RuntimeError):
        encode_windows_device([np.zeros((10, 4, 10), np.float32)], [np.zeros((4, 10))], packed)
    with pytest.raises(RuntimeError):
        label_trajectories_batched(23, 10, (48, 64), (30, 50), 1000, packed, packed, lambda t: None, front="batch")
    assert label_sequences_batched([], [], 10, (48, 64), (30, 50), 1000, packed, packed, lambda s, t: None, front="batch") == []
    with pytest.raises(ValueError):
        label_sequences_batched([], [], 10, (48, 64), (30, 50), 1000, packed, packed, lambda s, t: None, front="rows")
