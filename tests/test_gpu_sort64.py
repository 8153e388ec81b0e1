"""psfm_sort_records64 -- the record sort of the id assignment on keys of up to 64 bits (the 8-byte instances of the kernels of
csrc/psfm_sort.hip) on its own: equal to numpy's stable sort, keys and lanes, on sizes around the tile and group boundaries, on every
pass count with whole and partial last digits, on the digit distributions that stress its pieces (one digit only; the word boundary;
the padding value itself as a key), with more group rows than the scatter kernel has in flight at once, and on a long-sequence key
layout.  The tile is the 32-bit sort's: 4 096 keys, groups of 8 tiles."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE = 4096
GROUP = 8 * TILE
FULL = (1 << 64) - 1


def _sort64(keys, vals, end_bit):
    import torch
    from point_trajectory import _hip
    ctx = _hip.context(0)
    k = torch.from_numpy(keys.view(np.int64).copy()).cuda()
    v = torch.from_numpy(vals.copy()).cuda()
    _hip.check(_hip.lib().psfm_sort_records64(ctx.handle, _hip.ptr(k), _hip.ptr(v), int(keys.size), int(end_bit), _hip.current_stream_ptr()))
    torch.cuda.synchronize()
    return k.cpu().numpy().view(np.uint64), v.cpu().numpy()


def _check(keys, end_bit=64):
    assert keys.dtype == np.uint64
    vals = np.arange(keys.size, dtype=np.int32)
    k, v = _sort64(keys, vals, end_bit)
    masked = keys if end_bit == 64 else keys & np.uint64((1 << end_bit) - 1)
    order = np.argsort(masked, kind="stable")
    assert np.array_equal(k, keys[order])          # the keys leave whole, bits at and above end_bit included
    assert np.array_equal(v, vals[order])          # equal keys keep their order: the sort is stable


def _random64(rng, n):
    return rng.integers(0, 1 << 64, n, dtype=np.uint64)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, GROUP - 1, GROUP, GROUP + 1, 3 * GROUP + 17, 300_001])
def test_sizes_around_tiles_and_groups(n):
    _check(_random64(np.random.default_rng(n), n))


END_BITS = [1, 7, 8, 9, 31, 32, 33, 36, 39, 40, 41, 48, 56, 57, 63, 64]


@pytest.mark.parametrize("end_bit", END_BITS)
def test_every_pass_count_and_partial_last_digit(end_bit):
    rng = np.random.default_rng(end_bit)
    keys = _random64(rng, 70_001)
    if end_bit < 64:
        keys &= np.uint64((1 << end_bit) - 1)
    _check(keys, end_bit)


@pytest.mark.parametrize("end_bit", END_BITS)
def test_bits_above_end_bit_are_ignored(end_bit):
    """Keys random over all 64 bits: the bits at and above end_bit must order nothing (a partial last digit is masked, later passes do
    not run), and the keys leave whole, in the order of their low bits, lanes with them."""
    _check(_random64(np.random.default_rng(100 + end_bit), 70_001), end_bit)


@pytest.mark.parametrize("kind", ["all-equal", "sorted", "reversed", "three-values", "low-word-only", "high-word-only", "bit-32-only",
                                  "top-byte-only", "all-ones"])
def test_digit_distributions(kind):
    n = 2 * GROUP + 1234
    rng = np.random.default_rng(7)
    if kind == "all-equal":
        keys = np.full(n, 0xDEADBEEF01234567, np.uint64)
    elif kind == "sorted":
        keys = np.sort(_random64(rng, n))
    elif kind == "reversed":
        keys = np.sort(_random64(rng, n))[::-1].copy()
    elif kind == "three-values":
        keys = rng.choice(np.array([5, 0x00FF00FF00FF00FF, FULL], np.uint64), n)
    elif kind == "low-word-only":
        keys = rng.integers(0, 1 << 32, n, dtype=np.uint64) | np.uint64(0xABCD123400000000)
    elif kind == "high-word-only":
        keys = (rng.integers(0, 1 << 32, n, dtype=np.uint64) << np.uint64(32)) | np.uint64(0x89ABCDEF)
    elif kind == "bit-32-only":
        keys = (rng.integers(0, 2, n, dtype=np.uint64) << np.uint64(32)) | np.uint64(0x7654321000FEDCBA & ~(1 << 32))
    elif kind == "top-byte-only":
        keys = rng.integers(0, 256, n, dtype=np.uint64) << np.uint64(56)
    else:
        keys = np.full(n, FULL, np.uint64)          # the tile padding value itself: real keys must still come out in lane order
    _check(keys)


def test_more_group_rows_than_one_chunk():
    """The scatter kernel takes the group rows 64 at a time: 2 200 001 keys are 68 rows."""
    _check(_random64(np.random.default_rng(21), 2_200_001))


def test_more_group_rows_than_one_chunk_32_bit():
    """The same size through psfm_sort_records (the 32-bit kernels: their own test file stops at 64 rows)."""
    import torch
    from point_trajectory import _hip
    rng = np.random.default_rng(22)
    keys = rng.integers(0, 1 << 32, 2_200_001, dtype=np.uint64).astype(np.uint32)
    vals = np.arange(keys.size, dtype=np.int32)
    k = torch.from_numpy(keys.view(np.int32).copy()).cuda()
    v = torch.from_numpy(vals.copy()).cuda()
    _hip.check(_hip.lib().psfm_sort_records(_hip.context(0).handle, _hip.ptr(k), _hip.ptr(v), int(keys.size), 32, _hip.current_stream_ptr()))
    torch.cuda.synchronize()
    order = np.argsort(keys, kind="stable")
    assert np.array_equal(k.cpu().numpy().view(np.uint32), keys[order]) and np.array_equal(v.cpu().numpy(), vals[order])


@pytest.mark.parametrize("layout", ["36-bit-triangular", "37-bit-fields"])
def test_long_sequence_key_layout(layout):
    """2 M records with the key layouts of 1080p x 401 frames at r = 2 -- death over birth over a 19-bit grid index, birth <= death:
    36 bits with the pair as its triangular number (17 bits; one too many for the 32-bit sort), 37 bits as the fields the 64-bit
    format really packs (9 + 9 + 19) -- in the order the frame loop leaves them: segments of ~2 000 records ordered by death."""
    rng = np.random.default_rng(11)
    n, seg = 2_000_003, 2023
    death = rng.integers(0, 402, n).astype(np.uint64)
    whole = (n // seg) * seg
    death[:whole] = np.sort(death[:whole].reshape(-1, seg), axis=1).reshape(-1)
    birth = np.minimum((rng.random(n) * (death + 1.0)).astype(np.uint64), death)
    idx = rng.integers(0, 518_400, n).astype(np.uint64)
    if layout == "36-bit-triangular":
        keys, bits = ((death * (death + np.uint64(1)) // np.uint64(2) + birth) << np.uint64(19)) | idx, 36
    else:
        keys, bits = (death << np.uint64(28)) | (birth << np.uint64(19)) | idx, 37
    assert int(keys.max()).bit_length() == bits
    _check(keys, bits)


def test_bad_arguments_are_refused():
    import torch
    from point_trajectory import _hip
    ctx = _hip.context(0)
    k = torch.zeros(8, dtype=torch.int64, device="cuda")
    v = torch.zeros(8, dtype=torch.int32, device="cuda")
    for n, end_bit, kp, vp in [(-1, 64, k, v), (8, 0, k, v), (8, 65, k, v), (8, 64, None, v), (8, 64, k, None)]:
        st = _hip.lib().psfm_sort_records64(ctx.handle, _hip.ptr(kp) if kp is not None else None, _hip.ptr(vp) if vp is not None else None,
                                            n, end_bit, _hip.current_stream_ptr())
        assert st == _hip.PSFM_ERR_ARG
    assert _hip.lib().psfm_sort_records64(ctx.handle, None, None, 0, 64, _hip.current_stream_ptr()) == 0      # nothing to sort
