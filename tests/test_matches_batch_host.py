"""The batched match tables without a GPU.

1. The NumPy statement of the batched pipeline (tests/_matches_batch_np.py: concatenate, composed keys, stable argsorts, split and
   localise) equals psfm_sfm.matches_from_flow.match_tables_host per sequence -- the function tests/test_consumers_golden.py pins to
   the reference -- on the hand-shaped batch, with remove_dynamic True and False, and with the empty set first and last.
2. particle-sfm_amd/csrc/psfm_matches_batch.h -- the block -> (sequence, local index) lookup of the flattened grid, the bases, the
   composed key's encode / decode and width check, the grouping rule, and the per-element rules the single and the batched kernels
   share -- compiled for the host by tests/host/matches_batch_host.cpp and compared with that statement.
3. The Python grouping function of psfm_sfm.matches_from_flow.

The hand-shaped batch, eight labelled sets in this order: (1) trajectories of 3, 20, 21, 41, 1, 2 and 40 points over 45 images, on
both sides of sample_k = 20 (both sampling rules, the n // K stride), ~30 % of the points dynamic; (2) an empty set, 7 images; (3)
three trajectories, all points dynamic; (4) four one-point trajectories on one image (n_img = 1, no match); (5) 64 trajectories of 4
points with frame gaps: 256 points; (6) 63 x 4 + 3 = 255 points; (7) 64 x 4 + 1 = 257 points; (8) the first set again: equal pair
keys in two sequences, identical tables."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import _matches_batch_np as mb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX, BLOCK, INT32_MAX = 64, 256, 2 ** 31 - 1


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("matches_batch") / "libmatches_batch_host.so")
    cmd = ["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "tests", "host", "shim"),
           "-I", os.path.join(ROOT, "tests", "host"), "-I", os.path.join(ROOT, "particle-sfm_amd", "csrc"),
           os.path.join(ROOT, "tests", "host", "matches_batch_host.cpp"), "-o", out]
    subprocess.run(cmd, check=True)
    L = ctypes.CDLL(out)
    vp, u64, lg, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_long, ctypes.c_int
    L.psfm_host_mtb_grid.argtypes = [vp, i32, vp, vp]
    L.psfm_host_mtb_grid.restype = lg
    L.psfm_host_mtb_find.argtypes = [vp, i32]
    L.psfm_host_mtb_bits.argtypes = [u64]
    L.psfm_host_mtb_key_bits.argtypes = [i32, u64, vp]
    L.psfm_host_mtb_key.argtypes = [i32, u64, i32]
    L.psfm_host_mtb_key.restype = u64
    L.psfm_host_mtb_key_seq.argtypes = [u64, i32]
    L.psfm_host_mtb_key_local.argtypes = [u64, i32]
    L.psfm_host_mtb_key_local.restype = u64
    L.psfm_host_mtb_group_end.argtypes = [vp, i32, i32, lg, vp]
    L.psfm_host_mt_match_count.argtypes = [lg, lg, i32]
    L.psfm_host_mt_match_count.restype = lg
    L.psfm_host_mt_targets.argtypes = [lg, lg, i32, vp]
    L.psfm_host_mt_owner.argtypes = [vp, lg, lg, vp]
    L.psfm_host_mt_owner.restype = None
    L.psfm_host_mt_frame_index.argtypes = [i32, i32, vp]
    L.psfm_host_mt_frame_index.restype = ctypes.c_uint
    L.psfm_host_mt_lower_bound.argtypes = [vp, lg, lg, u64, u64]
    L.psfm_host_mt_lower_bound.restype = lg
    return L


# ---- 1. the statement against the per-sequence model ---------------------------------------------------------------------------------

def assert_tables_equal(got, want):
    names = ("kp_off", "kp_xy", "pair_key", "pair_off", "pair_first", "rows")
    for name, g, w in zip(names, got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, (name, g.shape, w.shape, g.dtype, w.dtype)
        assert g.tobytes() == w.tobytes(), name


def single_tables(seq, remove_dynamic):
    from psfm_sfm import matches_from_flow as mff
    off, frames, xy, labels, n_img = seq
    return mff.match_tables_host(off, frames, xy, labels, n_img, remove_dynamic)


def test_the_hand_shaped_batch_is_what_it_says():
    s = mb.hand_shaped_batch()
    assert len(s) == 8
    assert np.diff(s[0][0]).tolist() == [3, 20, 21, 41, 1, 2, 40] and s[0][4] == 45 and 0.15 < s[0][3].mean() < 0.45
    assert len(s[1][1]) == 0 and s[1][4] == 7
    assert len(s[2][0]) == 4 and s[2][3].all()
    assert np.diff(s[3][0]).tolist() == [1] * 4 and s[3][4] == 1 and not s[3][1].any()
    assert [len(x[1]) for x in s[4:7]] == [256, 255, 257]
    assert any((np.diff(s[4][1][a:b]) > 1).any() for a, b in zip(s[4][0][:-1], s[4][0][1:]))          # frame gaps
    assert all(np.array_equal(a, b) for a, b in zip(s[0][:4], s[7][:4])) and s[0][4] == s[7][4]


@pytest.mark.parametrize("order", ["as_listed", "empty_first", "empty_last"])
@pytest.mark.parametrize("remove_dynamic", [True, False])
def test_numpy_statement_equals_the_model_per_sequence(order, remove_dynamic):
    seqs = mb.orders()[order]
    got = mb.match_tables_batch_np(seqs, remove_dynamic)
    assert len(got) == len(seqs) == 8
    n_matches = []
    for b, seq in enumerate(seqs):                      # no sequence skipped
        assert_tables_equal(got[b], single_tables(seq, remove_dynamic))
        n_matches.append(len(got[b][5]))
    first, again = [b for b, s in enumerate(seqs) if s[4] == 45]
    assert_tables_equal(got[first], got[again])         # equal pair keys in two sequences: identical tables
    assert n_matches[first] > 1000 and sum(1 for n in n_matches if n == 0) == (3 if remove_dynamic else 2)


def test_numpy_statement_on_sixty_four_random_sets():
    seqs = mb.random_sets(64, 5)
    got = mb.match_tables_batch_np(seqs, True)
    for b, seq in enumerate(seqs):
        assert_tables_equal(got[b], single_tables(seq, True))
    assert min(len(s[1]) for s in seqs) < 20 and max(len(s[1]) for s in seqs) > 250


def test_numpy_statement_names_the_sequence_with_a_frame_outside():
    seqs = mb.hand_shaped_batch()
    seqs[4] = seqs[4][:4] + (int(seqs[4][1].max()),)    # n_img = its last frame
    with pytest.raises(IndexError, match="sequence 4"):
        mb.match_tables_batch_np(seqs)


def test_the_edge_sets_are_what_they_say():
    """the sets tests/test_gpu_matches_batch.py gives the single entry points: every claimed property, by the model"""
    K = 20
    for n_points, seq in mb.EDGE_SETS.items():
        off, frames, xy, labels, n_img = seq
        lengths = np.diff(off).tolist()
        assert sum(lengths) == len(frames) == n_points and (n_points == 1 or set(mb.EDGE_LENGTHS) <= set(lengths))
        runs = [frames[a:b] for a, b in zip(off[:-1], off[1:])]
        assert all(len(set(r.tolist())) == len(r) for r in runs)
        if n_points > 1:
            assert any((np.diff(r) < 0).any() for r in runs) and any((np.abs(np.diff(np.sort(r))) > 1).any() for r in runs)
            assert 0.15 < labels.mean() < 0.45
        # all points kept: the lengths are the kept lengths -- 41 emits 20 matches at j = 40 (40 % 2 == 0, 40 // 2 >= 20) and 19 at j = 0
        assert len(single_tables(seq, False)[5]) == mb.n_matches_np(lengths, K)
        kept = [int((~labels[a:b]).sum()) for a, b in zip(off[:-1], off[1:])]
        assert len(single_tables(seq, True)[5]) == mb.n_matches_np(kept, K)
        assert (mb.n_matches_np(lengths, K) > 0) == (mb.n_matches_np(kept, K) > 0) == (n_points > 1)
    assert mb.n_matches_np([41], K) == 41 * K - 20 and mb.n_matches_np([40], K) == 40 * K - 20 and mb.n_matches_np([21], K) == 21 * K - 20
    assert mb.n_matches_np([20], K) == 380 and mb.n_matches_np([2], K) == 2 and mb.n_matches_np([1], K) == 0
    off, frames, xy, labels, n_img = mb.ALL_DYNAMIC_SET
    assert len(frames) == 257 and labels.all()
    got = single_tables(mb.ALL_DYNAMIC_SET, True)
    assert len(got[1]) == 0 and len(got[5]) == 0 and not got[0].any() and len(got[0]) == n_img + 1
    assert len(single_tables(mb.ALL_DYNAMIC_SET, False)[5]) == mb.n_matches_np(np.diff(off).tolist(), K) > 1000
    for n_img, seq in mb.N_IMG_SETS.items():
        off, frames, xy, labels, _ = seq
        assert seq[4] == n_img and frames.min() == 0 and frames.max() == n_img - 1 and not labels.any()
        kp_off, kp_xy, pair_key, pair_off, pair_first, rows = single_tables(seq, True)
        assert len(kp_off) == n_img + 1 and len(kp_xy) == len(frames)
        assert (len(rows) > 0) == (n_img > 1) and len(rows) == mb.n_matches_np(np.diff(off).tolist(), K)
        if n_img > 1:
            assert (n_img - 1) * n_img in pair_key.tolist()                       # (last image, image 0)
            assert mb.bits_np(n_img) == {2: 1, 255: 8, 256: 8, 257: 9}[n_img]
            assert (int(pair_key.max()) >= 2 ** 16) == (n_img == 257) and mb.bits_np(n_img * n_img) == {2: 2, 255: 16, 256: 16, 257: 17}[n_img]


# ---- 2. the header against the statement ------------------------------------------------------------------------------------------

def test_the_bounds(host):
    assert host.psfm_host_mtb_max() == MAX == mb.MAX_SEQ and host.psfm_host_mtb_block() == BLOCK == mb.BLOCK


def n_lists():
    """sizes 0, 1, 255, 256, 257 alone and mixed, in padded tables (fewer than 64 sequences) and full ones"""
    rng = np.random.default_rng(27)
    sizes = [0, 1, 255, 256, 257]
    out = [[n] for n in sizes] + [[0, 0, 0], [0, 1, 0, 257, 0], [1] * 7, [255, 256, 0, 0, 257], [257, 0, 1], [0] * 63 + [1], [1] + [0] * 63,
                                  sizes * 12 + [700, 0, 1, 256]]
    out += [[int(n) for n in rng.choice(sizes + [1000], k)] for k in (2, 5, 17, 63, 64, 64)]
    return out


@pytest.mark.parametrize("ns", n_lists(), ids=lambda ns: "n%d_%s" % (len(ns), "_".join(str(n) for n in ns[:5])))
def test_grid_bases_and_lookup_against_enumeration(host, ns):
    n = (ctypes.c_long * MAX)(*ns)
    blk0, base = (ctypes.c_long * MAX)(), (ctypes.c_long * (MAX + 1))()
    blocks = host.psfm_host_mtb_grid(n, len(ns), blk0, base)
    w_blk0, w_blocks = mb.grid_np(ns)
    assert list(blk0) == w_blk0 and blocks == w_blocks and list(base) == mb.bases_np(ns)
    assert all(v == INT32_MAX for v in list(blk0)[len(ns):]) and base[len(ns)] == sum(ns) == base[MAX]
    # brute force: every (sequence, block in the sequence) once, sequence-major; the block's first element exists
    want = [(b, j) for b, nb in enumerate(ns) for j in range(-(-nb // BLOCK))]
    got = []
    for blk in range(blocks):
        b = host.psfm_host_mtb_find(blk0, blk)
        assert b == mb.find_np(list(blk0), blk)
        got.append((b, blk - blk0[b]))
        assert 0 <= (blk - blk0[b]) * BLOCK < ns[b]
    assert got == want
    # every element of the concatenation is owned by exactly one (block, thread)
    owned = sum(min(BLOCK, ns[b] - j * BLOCK) for b, j in got)
    assert owned == sum(ns)


def test_key_codec_and_width_check(host):
    rng = np.random.default_rng(3)
    lb = ctypes.c_int(0)
    for n_seq, rng_local in ((1, 1), (1, 2), (2, 45), (64, 45 * 45), (64, 2 ** 31 - 1), (4, (2 ** 31 - 1) ** 2), (33, 2 ** 57), (64, 2 ** 58)):
        bits = host.psfm_host_mtb_key_bits(n_seq, rng_local, ctypes.byref(lb))
        w_bits, w_lb = mb.key_bits_np(n_seq, rng_local)
        assert (bits, lb.value) == (w_bits, w_lb) and bits > 0 and (1 << lb.value) >= rng_local
        assert bits == mb.bits_np(rng_local) + (mb.bits_np(n_seq) if n_seq > 1 else 0) <= 64
        for _ in range(200):
            b, local = int(rng.integers(0, n_seq)), int(rng.integers(0, rng_local))
            key = host.psfm_host_mtb_key(b, local, lb.value)
            assert key == mb.key_np(b, local, lb.value) < (1 << bits)
            assert host.psfm_host_mtb_key_seq(key, lb.value) == b and host.psfm_host_mtb_key_local(key, lb.value) == local
        # the order of the composed key is (sequence, local key)
        assert host.psfm_host_mtb_key(0, rng_local - 1, lb.value) < host.psfm_host_mtb_key(1, 0, lb.value)
    # what does not fit: 64 sequences above 59 bits, any local key of 64 bits
    for n_seq, rng_local in ((64, (2 ** 31 - 1) ** 2), (5, (2 ** 31 - 1) ** 2), (64, 2 ** 58 + 1), (2, 2 ** 63 + 1), (1, 2 ** 64 - 1), (64, 2 ** 62), (3, 2 ** 63)):
        assert host.psfm_host_mtb_key_bits(n_seq, rng_local, ctypes.byref(lb)) == 0 == mb.key_bits_np(n_seq, rng_local)[0], (n_seq, rng_local)
    for v in (0, 1, 2, 3, 4, 5, 255, 256, 257, 2 ** 32, 2 ** 63, 2 ** 64 - 1):
        assert host.psfm_host_mtb_bits(v) == mb.bits_np(v)


def test_one_sequence_spends_no_key_bit_on_the_sequence(host):
    """psfm_mtb_key_bits(1, r): the composed key of a single call is the local key, psfm_mtb_bits(r) bits wide"""
    lb = ctypes.c_int(0)
    for p in range(0, 64):
        for r in (2 ** p - 1, 2 ** p, 2 ** p + 1):
            if r < 1 or (p == 63 and r > 2 ** 63):
                continue
            bits = host.psfm_host_mtb_key_bits(1, r, ctypes.byref(lb))
            assert bits == lb.value == host.psfm_host_mtb_bits(r) == mb.bits_np(r) < 64, r
            assert (bits, lb.value) == mb.key_bits_np(1, r)
            assert host.psfm_host_mtb_key(0, r - 1, lb.value) == r - 1                  # sequence 0 leaves the local key as it is
            # two sequences still pay their bit
            assert host.psfm_host_mtb_key_bits(2, r, ctypes.byref(lb)) == (bits + 1 if bits < 64 else 0)
    # a local key that needs all 64 bits is refused even for one sequence (the shift of psfm_mtb_key)
    for r in (2 ** 63 + 1, 2 ** 64 - 1):
        assert host.psfm_host_mtb_key_bits(1, r, ctypes.byref(lb)) == 0 == mb.key_bits_np(1, r)[0]


GROUP_CASES = {
    "sixty_five": ([10] * 65, 10 ** 6),
    "above_the_cap": ([5, 2000, 7, 8], 1000),
    "cap_hit_exactly": ([400, 600, 1, 999, 1, 1], 1000),
    "above_first_and_last": ([1001, 1, 1001], 1000),
    "zeros": ([0] * 130, 0),
    "one": ([3], 1 << 25),
}


@pytest.mark.parametrize("case", list(GROUP_CASES))
def test_grouping_rule_header_python_and_statement(host, case):
    from psfm_sfm import matches_from_flow as mff
    n_points, cap = GROUP_CASES[case]
    want = mb.group_np(n_points, cap)
    assert mff.group_sequences(n_points, cap) == want
    arr = (ctypes.c_long * len(n_points))(*n_points)
    got, start, alone = [], 0, ctypes.c_int(0)
    while start < len(n_points):
        end = host.psfm_host_mtb_group_end(arr, len(n_points), start, cap, ctypes.byref(alone))
        got.append((start, end, bool(alone.value)))
        start = end
    assert got == want
    # the rule itself: consecutive, complete, within both bounds; alone exactly when above the cap
    assert [g[0] for g in want] == [0] + [g[1] for g in want[:-1]] and want[-1][1] == len(n_points)
    for lo, hi, single in want:
        assert 1 <= hi - lo <= MAX
        assert single == (n_points[lo] > cap) and (not single or hi == lo + 1)
        assert single or sum(n_points[lo:hi]) <= cap
        # greedy: the next sequence would not have fitted
        if not single and hi < len(n_points) and hi - lo < MAX:
            assert n_points[hi] > cap or sum(n_points[lo:hi + 1]) > cap
    if case == "sixty_five":
        assert want == [(0, 64, False), (64, 65, False)]
    if case == "above_the_cap":
        assert want == [(0, 1, False), (1, 2, True), (2, 4, False)]
    if case == "cap_hit_exactly":
        assert want == [(0, 2, False), (2, 4, False), (4, 6, False)]


def test_python_grouping_defaults():
    from psfm_sfm import matches_from_flow as mff
    assert mff.MAX_POINTS == 1 << 25 and mff.BATCH_MAX == 64
    # the worst case of the default cap stays under BATCH_BYTES of point_trajectory/batch.py: 20 matches of 40 bytes per point
    assert mff.MAX_POINTS * mff.SAMPLE_K * 40 < 48 * 2 ** 30


def test_shared_rules_against_the_model(host):
    """psfm_mt_match_count / psfm_mt_targets against the loops of matches_from_flow.py:83-101; owner, frame index, lower bound"""
    K = 20
    out = (ctypes.c_long * 64)()
    for n in list(range(1, 90)) + [399, 400, 401, 1000]:
        for j in range(n):
            if n <= K:
                want = [k for k in range(n) if k != j]
            else:
                want = [k * (n // K) for k in range(K) if k * (n // K) != j]
            m = host.psfm_host_mt_targets(n, j, K, out)
            assert list(out)[:m] == want and host.psfm_host_mt_match_count(n, j, K) == len(want)
    off = np.array([0, 3, 3, 4, 260, 261], np.int64)      # (an empty trajectory in the middle is never an owner)
    owner = np.zeros(261, np.int32)
    host.psfm_host_mt_owner(off.ctypes.data, len(off) - 1, 261, owner.ctypes.data)
    assert np.array_equal(owner, np.repeat(np.arange(5), np.diff(off)))
    o = ctypes.c_int(0)
    for f, n_img, want in ((0, 1, (0, 0)), (44, 45, (44, 0)), (45, 45, (0, 1)), (-1, 45, (0, 1)), (2 ** 31 - 1, 7, (0, 1))):
        assert (host.psfm_host_mt_frame_index(f, n_img, ctypes.byref(o)), o.value) == want
    keys = np.array([mb.key_np(1, f, 6) for f in (0, 0, 3, 3, 3, 9)] + [mb.key_np(2, f, 6) for f in (1, 2)], np.uint64)
    for v in range(12):
        assert host.psfm_host_mt_lower_bound(keys.ctypes.data, 0, 6, 63, v) == int(np.searchsorted([0, 0, 3, 3, 3, 9], v))
        assert host.psfm_host_mt_lower_bound(keys.ctypes.data, 6, 8, 63, v) == 6 + int(np.searchsorted([1, 2], v))


def test_no_cpu_fallback(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    from point_trajectory import _hip
    with pytest.raises(RuntimeError):
        _hip.batch_contexts(2)
