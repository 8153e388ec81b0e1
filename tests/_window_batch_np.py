"""The NumPy statement of psfm_window_sample_batch (csrc/psfm_window_batch.h, psfm_window_batch.hip): per (trajectory, window)
eligibility, the splitmix64 keys in uint64, the cap rule, the order of the rows and the concatenated layout of a call's outputs; and
of the flattened grids of the three batched front-end calls: per window its first row and first block, and the lookup of a block.
Test infrastructure: tests/test_window_batch_host.py pins it to the header (compiled for the host) and to the host
TrajectorySet.sample_inside_window; tests/test_gpu_front_batch.py pins the device to it."""
import numpy as np

MAX_WINDOWS = 64
BLOCK = 256
INT32_MAX = 2 ** 31 - 1
M64 = (1 << 64) - 1


def overlap_np(birth, length, f0, L):
    """Observations of trajectories (birth, length) on frames [f0, f0 + L)."""
    birth, length = np.asarray(birth, np.int64), np.asarray(length, np.int64)
    lo = np.maximum(birth, f0)
    hi = np.minimum(birth + length, np.asarray(f0, np.int64) + L)
    return np.maximum(hi - lo, 0)


def eligible_np(birth, length, f0, L, traj_min_len, min_length):
    ov = overlap_np(birth, length, f0, L)
    return (np.asarray(length, np.int64) >= traj_min_len) & (ov > 0) & (ov >= min_length)


def hash_np(seed, ids):
    """splitmix64 of (seed, id), as psfm_window_hash_kernel: uint64 arithmetic modulo 2^64."""
    with np.errstate(over="ignore"):
        z = np.asarray(seed, np.uint64) + np.uint64(0x9E3779B97F4A7C15) * (np.asarray(ids, np.int64) + 1).astype(np.uint64)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def hash_int(seed, i):
    """The same key in Python integers (no NumPy wrap-around involved)."""
    z = (seed + 0x9E3779B97F4A7C15 * (i + 1)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def select_np(birth, length, f0, L, traj_min_len, min_length, max_num, seed):
    """The ids of one window: eligible ones ascending; above the cap the max_num smallest keys in key order, equal keys by id."""
    ids = np.flatnonzero(eligible_np(birth, length, f0, L, traj_min_len, min_length)).astype(np.int32)
    if len(ids) > max_num:
        ids = ids[np.argsort(hash_np(seed, ids), kind="stable")][:max_num]
    return ids


def rows_np(ids, birth, off, length, xy, f0, L, raw_hw=None, input_size=None):
    """(raw (K,L,2) zero-padded, mask_absent (K,L), normalised (K,L,2) or None) of the rows `ids` of window [f0, f0 + L)."""
    ids = np.asarray(ids, np.int64)
    t = f0 + np.arange(L)[None, :]
    b, n = np.asarray(birth, np.int64)[ids][:, None], np.asarray(length, np.int64)[ids][:, None]
    present = (t >= b) & (t < b + n)
    src = np.where(present, np.asarray(off, np.int64)[ids][:, None] + (t - b), 0)
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    raw = np.where(present[:, :, None], xy[src] if len(xy) else np.zeros(src.shape + (2,)), 0.0)
    nor = None
    if raw_hw is not None:
        # data_utils.py:74-89: pt /= (raw / target); pt /= target; clip -- two f64 divisions, in order
        ratio = np.array([raw_hw[1] / input_size[1], raw_hw[0] / input_size[0]], np.float64)
        target = np.array([input_size[1], input_size[0]], np.float64)
        nor = np.clip(raw / ratio / target, 0.0, 1.0)
    return raw, (~present).astype(np.float64), nor


def sample_windows_np(birth, length, off, xy, windows, seeds, max_num, traj_min_len=3, min_length=3, raw_hw=None, input_size=None):
    """A whole call: windows [(f0, L), ...] of one L.  Returns (k (n_win,), row0 (n_win + 1,), ids, raw, mask_absent, normalised):
    window b occupies rows [row0[b], row0[b + 1]) of each concatenated output."""
    L = windows[0][1] if windows else 1
    assert all(n == L for _, n in windows) and len(windows) <= MAX_WINDOWS
    per = [select_np(birth, length, f0, L, traj_min_len, min_length, max_num, s) for (f0, _), s in zip(windows, seeds)]
    k = np.array([len(p) for p in per], np.int64)
    row0 = np.concatenate([[0], np.cumsum(k)]).astype(np.int64)
    parts = [rows_np(p, birth, off, length, xy, f0, L, raw_hw, input_size) for p, (f0, _) in zip(per, windows)]
    cat = lambda i, shape: np.concatenate([p[i] for p in parts]) if parts else np.zeros(shape)
    ids = np.concatenate(per).astype(np.int32) if per else np.zeros(0, np.int32)
    return k, row0, ids, cat(0, (0, L, 2)), cat(1, (0, L)), (cat(2, (0, L, 2)) if raw_hw is not None else None)


def offsets_np(ks, units_per_row, per_block):
    """(row0 (65,), blk0 (64,), blocks): window b owns ceil(k * units_per_row / per_block) blocks from blk0[b]; rows and blocks of the
    windows before it; INT32_MAX in blk0 at and above n_win; row0 repeats the total there."""
    row0, blk0, rows, blocks = [], [], 0, 0
    for b in range(MAX_WINDOWS):
        row0.append(rows)
        blk0.append(blocks if b < len(ks) else INT32_MAX)
        if b < len(ks):
            rows += ks[b]
            blocks += -(-(ks[b] * units_per_row) // per_block)
    return row0 + [rows], blk0, blocks


def find_np(first, blk):
    """The window of block blk: the last entry of `first` that is <= blk."""
    return int(np.sum(np.asarray(first, np.int64) <= blk)) - 1
