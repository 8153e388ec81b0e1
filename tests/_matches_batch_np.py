"""The batched match-table pipeline (particle-sfm_amd/csrc/psfm_matches_batch.hip) as a NumPy statement: concatenate the sequences,
sort ONCE with the sequence above the key -- (b, frame) and (b, src * n_img[b] + tgt), both stable --, count with global
cumulative sums read at the sequence bases, then split and make everything sequence-local.  tests/test_matches_batch_host.py holds
it against psfm_sfm.matches_from_flow.match_tables_host per sequence (which tests/test_consumers_golden.py pins to the reference)
and against the host build of psfm_matches_batch.h; tests/test_gpu_matches_batch.py holds the device against both.  Also: the
lookup of a block on the flattened grid, the bases, the key codec, the grouping rule, the hand-shaped batch of the tests, and the
sets that take the single entry points to the edges of a block and of the key widths."""
import numpy as np

MAX_SEQ, BLOCK, INT32_MAX = 64, 256, 2 ** 31 - 1


def bits_np(v):
    """bits needed for values < v (psfm_mtb_bits)"""
    b = 1
    while b < 64 and (1 << b) < v:
        b += 1
    return b


def key_bits_np(n_seq, local_range):
    """(bits of the composed key or 0 when it does not fit 64, bits of the local key); one sequence spends no bit on the sequence"""
    lb, sb = bits_np(local_range), (bits_np(n_seq) if n_seq > 1 else 0)
    if lb >= 64 or (1 << lb) < local_range:
        return 0, lb
    return (lb + sb if lb + sb <= 64 else 0), lb


def key_np(b, local, local_bits):
    return (int(b) << local_bits) | int(local)


def grid_np(n):
    """blk0[64] (INT32_MAX at and above len(n)) and the blocks of the flattened grid"""
    blk0, blocks = [], 0
    for b in range(MAX_SEQ):
        blk0.append(min(blocks, INT32_MAX) if b < len(n) else INT32_MAX)
        if b < len(n):
            blocks += -(-int(n[b]) // BLOCK)
    return blk0, blocks


def bases_np(n):
    base, total = [], 0
    for b in range(MAX_SEQ + 1):
        base.append(total)
        if b < len(n):
            total += int(n[b])
    return base


def find_np(blk0, blk):
    return sum(1 for v in blk0 if v <= blk) - 1


def group_np(n_points, max_points, max_seq=MAX_SEQ):
    """[(start, end, alone)]: consecutive groups of at most max_seq sequences and max_points points; above the cap: alone"""
    out, i = [], 0
    while i < len(n_points):
        if n_points[i] > max_points:
            out.append((i, i + 1, True))
            i += 1
            continue
        e, total = i, 0
        while e < len(n_points) and e - i < max_seq and n_points[e] <= max_points and total + n_points[e] <= max_points:
            total += n_points[e]
            e += 1
        out.append((i, e, False))
        i = e
    return out


def match_tables_batch_np(seqs, remove_dynamic=True, sample_k=20):
    """seqs: [(off, frames, xy, labels(bool), n_img)] -> one table tuple per sequence (kp_off, kp_xy, pair_key, pair_off, pair_first,
    rows), computed over the concatenation."""
    B = len(seqs)
    assert 1 <= B <= MAX_SEQ
    n_img = np.array([s[4] for s in seqs], np.int64)
    fkey_bits, fbits = key_bits_np(B, int(n_img.max()))
    pkey_bits, pbits = key_bits_np(B, int(n_img.max()) ** 2)
    assert fkey_bits and pkey_bits
    npts = [len(s[1]) for s in seqs]
    pts0 = bases_np(npts)
    # ---- concatenate: per point its sequence, its trajectory (numbered over all sequences), frame, keep flag ----
    seq = np.repeat(np.arange(B), npts)
    frames = np.concatenate([np.asarray(s[1], np.int64) for s in seqs]) if sum(npts) else np.zeros(0, np.int64)
    xy = np.concatenate([np.asarray(s[2], np.float64).reshape(-1, 2) for s in seqs])
    labels = np.concatenate([np.asarray(s[3]).astype(bool) for s in seqs]) if sum(npts) else np.zeros(0, bool)
    ntraj = [len(s[0]) - 1 for s in seqs]
    traj0 = bases_np(ntraj)
    owner = np.concatenate([traj0[b] + np.repeat(np.arange(ntraj[b]), np.diff(np.asarray(s[0], np.int64))) for b, s in enumerate(seqs)]).astype(np.int64)
    bad = [bool(npts[b]) and bool(((frames[pts0[b]:pts0[b + 1]] < 0) | (frames[pts0[b]:pts0[b + 1]] >= n_img[b])).any()) for b in range(B)]
    if any(bad):
        raise IndexError("sequence %d: a frame outside its image list" % bad.index(True))
    keep = ~labels if remove_dynamic else np.ones(len(frames), bool)
    q_of = np.concatenate([[0], np.cumsum(keep)])                        # the global scan
    n_kept = [int(q_of[pts0[b + 1]] - q_of[pts0[b]]) for b in range(B)]  # read at the bases
    kept0 = bases_np(n_kept)
    seq, frames, xy, owner = seq[keep], frames[keep], xy[keep], owner[keep]
    K = len(frames)
    # ---- keypoints: ONE stable sort by (sequence, frame) ----
    kfr = (seq << fbits) | frames
    order = np.argsort(kfr, kind="stable")
    fsorted = kfr[order]
    kp_ind = np.empty(K, np.int64)
    kp_off = []
    for b in range(B):
        local = fsorted[kept0[b]:kept0[b + 1]] & ((1 << fbits) - 1)
        kp_off.append(np.searchsorted(local, np.arange(n_img[b] + 1)).astype(np.int64))
    s_local = np.arange(K) - np.asarray(kept0)[seq[order]]
    kp_ind[order] = s_local - np.concatenate([kp_off[b][fsorted[kept0[b]:kept0[b + 1]] & ((1 << fbits) - 1)] for b in range(B)])
    kp_xy = xy[order]
    # ---- matches: counts, global scan, emit in loop order ----
    cnt = np.bincount(owner, minlength=traj0[B]).astype(np.int64)
    toff = np.concatenate([[0], np.cumsum(cnt)])
    n_of, j_loc = cnt[owner], np.arange(K) - toff[owner]
    reps = np.where(n_of <= sample_k, n_of, sample_k)
    src = np.repeat(np.arange(K), reps)
    r = np.arange(len(src)) - np.repeat(np.cumsum(reps) - reps, reps)
    stride = np.where(n_of[src] <= sample_k, 1, n_of[src] // sample_k)
    tgt_loc = r * stride
    ok = tgt_loc != j_loc[src]
    src, tgt = src[ok], (toff[owner[src]] + tgt_loc)[ok]
    m_cnt = np.bincount(src, minlength=K)
    m_off = np.concatenate([[0], np.cumsum(m_cnt)])
    n_m = [int(m_off[kept0[b + 1]] - m_off[kept0[b]]) for b in range(B)]
    m0 = bases_np(n_m)
    key = (seq[src] << pbits) | (frames[src] * n_img[seq[src]] + frames[tgt])
    po = np.argsort(key, kind="stable")                                 # ONE stable sort by (sequence, pair)
    pk = key[po]
    rows = np.stack([kp_ind[src[po]], kp_ind[tgt[po]]], 1).astype(np.int32) if len(po) else np.zeros((0, 2), np.int32)
    out = []
    for b in range(B):
        lo, hi = m0[b], m0[b + 1]
        k_b = pk[lo:hi]
        bounds = np.flatnonzero(np.r_[True, k_b[1:] != k_b[:-1], True]) if hi > lo else np.zeros(1, np.int64)
        pair_key = (k_b[bounds[:-1]] & ((1 << pbits) - 1)) if hi > lo else np.zeros(0, np.int64)
        pair_first = (po[lo:hi][bounds[:-1]] - lo) if hi > lo else np.zeros(0, np.int64)
        out.append((kp_off[b], kp_xy[kept0[b]:kept0[b + 1]], pair_key.astype(np.int64), bounds.astype(np.int64), pair_first.astype(np.int64),
                    rows[lo:hi]))
    return out


# ---- the hand-shaped batch ---------------------------------------------------------------------------------------------------------

def _set(lengths, n_img, seed, dynamic=0.0, gaps=False, one_image=False):
    """A labelled set: trajectories of the given lengths on `n_img` images, in time order (with frame gaps when asked)."""
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    frames = []
    for n in lengths:
        if one_image:
            frames.append(np.zeros(n, np.int64))
        elif gaps:
            frames.append(np.sort(rng.choice(n_img, n, replace=False)))
        else:
            f0 = int(rng.integers(0, n_img - n + 1))
            frames.append(np.arange(f0, f0 + n))
    frames = np.concatenate(frames).astype(np.int64) if len(lengths) else np.zeros(0, np.int64)
    xy = rng.uniform(0, 500, size=(len(frames), 2))
    labels = rng.random(len(frames)) < dynamic
    return off, frames, xy, labels, n_img


def hand_shaped_batch():
    """The eight labelled sets of the tests, in order (tests/test_matches_batch_host.py lists what each one is for)."""
    first = _set([3, 20, 21, 41, 1, 2, 40], 45, 1, dynamic=0.3)
    empty = (np.zeros(1, np.int64), np.zeros(0, np.int64), np.zeros((0, 2)), np.zeros(0, bool), 7)
    all_dyn = _set([5, 3, 8], 12, 3, dynamic=2.0)
    one_img = _set([1, 1, 1, 1], 1, 4, one_image=True)
    s256 = _set([4] * 64, 11, 5, gaps=True)
    s255 = _set([4] * 63 + [3], 11, 6, gaps=True)
    s257 = _set([4] * 64 + [1], 11, 7, gaps=True)
    again = tuple(np.copy(a) if isinstance(a, np.ndarray) else a for a in first)
    return [first, empty, all_dyn, one_img, s256, s255, s257, again]


def orders():
    """The list as it is, with the empty set moved to the front, and to the back."""
    base = hand_shaped_batch()
    return {"as_listed": base, "empty_first": [base[1]] + base[:1] + base[2:], "empty_last": base[:1] + base[2:] + [base[1]]}


# ---- the sets for the single entry points at their edges --------------------------------------------------------------------------

EDGE_LENGTHS = (1, 2, 20, 21, 40, 41)          # no match; a pair; both sides of sample_k = 20; stride 2 with and without j // 2 >= 20
EDGE_POINTS = (1, 255, 256, 257, 513)          # the edges of a 256-thread block, and a third block
EDGE_N_IMG = (1, 2, 255, 256, 257)             # frame key 8 -> 9 bits, pair key 16 -> 17 bits


def edge_lengths(n_points):
    """Trajectory lengths that add up to n_points: each of EDGE_LENGTHS once where it fits, then again, largest first."""
    out, left = [], n_points
    for n in EDGE_LENGTHS:
        if n <= left:
            out.append(n)
            left -= n
    while left:
        for n in reversed(EDGE_LENGTHS):
            if n <= left:
                out.append(n)
                left -= n
    return out


def edge_set(n_points, seed, n_img=64, dynamic=0.3):
    """A labelled set of n_points points in edge_lengths trajectories; a trajectory's frames are distinct images drawn from all
    n_img in random order: not ascending, with gaps."""
    rng = np.random.default_rng(seed)
    lengths = edge_lengths(n_points)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    frames = np.concatenate([rng.permutation(n_img)[:n] for n in lengths]).astype(np.int64)
    xy = rng.uniform(0, 500, size=(n_points, 2))
    return off, frames, xy, rng.random(n_points) < dynamic, n_img


def n_img_set(n_img, seed):
    """A set without dynamic points on n_img images: trajectories of 2, 20, 21, 41, 1 and 2 points where n_img has room for their
    distinct frames (five one-point trajectories on one image); the first one is (last image, image 0)."""
    rng = np.random.default_rng(seed)
    lengths = [n for n in (2, 20, 21, 41, 1, 2) if n <= n_img] if n_img > 1 else [1] * 5
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    frames = [rng.permutation(n_img)[:n] for n in lengths]
    if n_img > 1:
        frames[0] = np.array([n_img - 1, 0])
    frames = np.concatenate(frames).astype(np.int64)
    return off, frames, rng.uniform(0, 500, size=(len(frames), 2)), np.zeros(len(frames), bool), n_img


def n_matches_np(kept_lengths, sample_k=20):
    """matches of trajectories with these numbers of kept points (matches_from_flow.py:83-101), counted point by point"""
    total = 0
    for n in kept_lengths:
        stride = max(n // sample_k, 1)
        total += n * (n - 1) if n <= sample_k else sum(sample_k - (1 if j % stride == 0 and j // stride < sample_k else 0) for j in range(n))
    return total


EDGE_SETS = {n: edge_set(n, 40 + i) for i, n in enumerate(EDGE_POINTS)}
ALL_DYNAMIC_SET = edge_set(257, 50, dynamic=2.0)
N_IMG_SETS = {n: n_img_set(n, 60 + i) for i, n in enumerate(EDGE_N_IMG)}


def random_sets(n, seed, max_points=300):
    """n labelled sets of 0 .. max_points points from a seeded generator (lengths 1 .. 45 on 45 images, ~25 % dynamic)."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        target = int(rng.integers(0, max_points + 1))
        lengths = []
        while sum(lengths) < target:
            lengths.append(int(min(rng.integers(1, 46), target - sum(lengths))))
        out.append(_set(lengths, 45, 1000 * seed + i, dynamic=0.25, gaps=bool(i % 2)))
    return out
