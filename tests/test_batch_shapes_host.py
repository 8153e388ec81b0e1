"""The index rules of psfm_connect_batch over sequences of different frame sizes (particle-sfm_amd/csrc/psfm_batch_shapes.h: the rows of
the flow_check and kill-map tables, the rule that maps a block of their flattened grid to a sequence and a chunk of its frame, the
batch's common key format) compiled for the HOST.

tests/host/batch_shapes_host.cpp builds the tables and walks every block of the grid as the kernels do: every (sequence, pair, pixel
pair) of flow_check and every (sequence, frame, four-pixel lane) of the kill maps must be owned exactly once, nothing outside a
sequence, every sequence must start on a block whose number is a multiple of 8 and a block of a banded frame must sit on the XCD of its
band.  Tables of 1, 2, 7 and 64 sequences; frames of fewer than 8 chunks, of 63, 64 and 65 chunks (the banding limit), of odd pixel
counts and widths; sequences of different lengths, and ones without maps to make.  And the keys of a small grid in the batch's widened
format against its own: the same order, in the 32-bit and in the 64-bit form.  No GPU involved."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IP, LP = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_long)
BLOCKS, NOT_ONCE, OUTSIDE, OFF_BAND, UNALIGNED, IDLE, DISPATCHED = range(7)
FC_PIXELS, KM_PIXELS = 1024, 1024


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("batch_shapes") / "libbatch_shapes_host.so")
    subprocess.run(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "tests", "host", "shim"),
                    "-I", os.path.join(ROOT, "particle-sfm_amd", "csrc"), os.path.join(ROOT, "tests", "host", "batch_shapes_host.cpp"),
                    "-o", out], check=True)
    L = ctypes.CDLL(out)
    L.psfm_host_bs_fc_walk.argtypes = [ctypes.c_int, IP, IP, IP, ctypes.c_int, IP, IP, IP, IP, LP]
    L.psfm_host_bs_km_walk.argtypes = [ctypes.c_int, IP, IP, IP, IP, ctypes.c_int, IP, IP, IP, IP, LP]
    L.psfm_host_bs_km_form.argtypes = [ctypes.c_long, ctypes.c_int, ctypes.c_int]
    L.psfm_host_bs_common_key.argtypes = [ctypes.c_int, LP, IP, ctypes.c_long, IP]
    L.psfm_host_bs_key_order.argtypes = [ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    L.psfm_host_bs_key_order.restype = ctypes.c_long
    return L


def ints(v):
    return (ctypes.c_int * len(v))(*v)


def walk(L, shapes, frames, forms=None):
    """shapes [(H, W)], frames [n] -> (blk0, blk_end, chunks, xcd_per, census) of the flow_check grid (forms None) or the kill-map grid."""
    n = len(shapes)
    cols = [(ctypes.c_int * n)() for _ in range(4)]
    out = (ctypes.c_long * 7)()
    H, W = ints([s[0] for s in shapes]), ints([s[1] for s in shapes])
    n_y = max(frames)
    if forms is None:
        L.psfm_host_bs_fc_walk(n, H, W, ints(frames), n_y, *cols, out)
    else:
        L.psfm_host_bs_km_walk(n, H, W, ints(frames), ints(forms), n_y, *cols, out)
    return [list(c) for c in cols] + [list(out)]


def ceil_div(a, b):
    return (a + b - 1) // b


# frames by their number of 1024-pixel chunks: 2 and 7 (fewer than 8), 8, 9, 63 / 64 / 65 (the banding limit), 401 (480 x 854)
SMALL = [(32, 40), (75, 102), (64, 97), (81, 100), (96, 96)]
AT_THE_LIMIT = [(252, 256), (256, 256), (257, 256), (255, 257), (259, 257)]
TABLES = {
    "one": ([(75, 102)], [5]),
    "one-banded": ([(480, 854)], [3]),
    "two": ([(64, 97), (256, 256)], [4, 7]),
    "seven": (SMALL[:4] + AT_THE_LIMIT[:3], [9, 1, 4, 0, 6, 2, 9]),
    "sixty-four": ((SMALL + AT_THE_LIMIT + [(480, 854)]) * 6, [(3 * k) % 11 for k in range(66)]),
}
TABLES["sixty-four"] = (TABLES["sixty-four"][0][:64], TABLES["sixty-four"][1][:64])


def check_table(shapes, frames, blk0, blk_end, chunks, xcd_per, census, pixels_per_chunk):
    assert census[NOT_ONCE] == 0 and census[OUTSIDE] == 0 and census[OFF_BAND] == 0 and census[UNALIGNED] == 0, census
    start = 0
    for (H, W), n, b0, b1, c, x in zip(shapes, frames, blk0, blk_end, chunks, xcd_per):
        assert c == ceil_div(H * W, pixels_per_chunk) and x == (ceil_div(c, 8) if c >= 64 else 0), ((H, W), c, x)
        want = 0 if n == 0 else ceil_div(8 * x if x else c, 8) * 8
        assert b0 == start and b1 - b0 == want and b0 % 8 == 0, ((H, W), b0, b1, want)
        start = b1
    assert census[BLOCKS] == start and census[DISPATCHED] == start * max(frames)
    print("blocks %d x %d frames; %d of %d dispatched blocks return at once" % (start, max(frames), census[IDLE], census[DISPATCHED]))


@pytest.mark.parametrize("name", sorted(TABLES))
def test_every_pixel_pair_of_flow_check_is_owned_once(lib, name):
    shapes, frames = TABLES[name]
    shapes = [s for s in shapes if s[0] * s[1] % 2 == 0]       # (an odd pixel count sends the batch through the per-stack launches)
    frames = frames[:len(shapes)]
    check_table(shapes, frames, *walk(lib, shapes, frames), FC_PIXELS)


@pytest.mark.parametrize("name", sorted(TABLES))
def test_every_lane_of_the_kill_maps_is_owned_once(lib, name):
    shapes, frames = TABLES[name]
    forms = [lib.psfm_host_bs_km_form(H * W, W, 1) for H, W in shapes]
    assert all(f == (2 if H * W % 2 else W % 2) for f, (H, W) in zip(forms, shapes))
    res = walk(lib, shapes, frames, forms)
    assert res[4][NOT_ONCE] == 0 and res[4][OUTSIDE] == 0 and res[4][OFF_BAND] == 0 and res[4][UNALIGNED] == 0, res[4]
    for (H, W), f, c, x in zip(shapes, forms, res[2], res[3]):
        assert c == ceil_div(H * W if f == 2 else ceil_div(H * W, 4), 256) and x == (ceil_div(c, 8) if c >= 64 and f != 2 else 0), ((H, W), f, c, x)
    assert all(b % 8 == 0 for b in res[0]) and res[4][BLOCKS] == res[1][-1]


def test_one_pixel_per_thread_for_a_stack_that_is_not_aligned(lib):
    """The form of the kill maps for an even frame whose flows are off their 16-byte alignment: every pixel once, no banding."""
    shapes, frames = [(64, 96), (300, 300), (37, 53)], [3, 2, 4]
    forms = [lib.psfm_host_bs_km_form(H * W, W, 0) for H, W in shapes]
    assert forms == [2, 2, 2]
    res = walk(lib, shapes, frames, forms)
    assert res[4][NOT_ONCE] == 0 and res[4][OUTSIDE] == 0 and res[3] == [0, 0, 0] and res[2] == [24, 352, 8], res


def test_the_banding_limit(lib):
    """63 chunks: walked in order, 64 blocks with one spare; 64: banded, 8 per XCD; 65: banded, 9 per XCD and 7 spare blocks."""
    shapes, frames = AT_THE_LIMIT[:3], [1, 1, 1]
    blk0, blk_end, chunks, xcd_per, census = walk(lib, shapes, frames)
    assert chunks == [63, 64, 65] and xcd_per == [0, 8, 9]
    assert [b - a for a, b in zip(blk0, blk_end)] == [64, 64, 72] and census[IDLE] == 1 + 0 + 7 and census[NOT_ONCE] == 0


def grid_points(H, W, r):
    return ceil_div(H, r) * ceil_div(W, r)


def common(lib, G, n_flows, n_records=1000):
    out = (ctypes.c_int * 4)()
    lib.psfm_host_bs_common_key(len(G), (ctypes.c_long * len(G))(*G), ints(n_flows), n_records, out)
    return list(out)


def test_widened_keys_sort_like_a_sequences_own_32_bit(lib):
    """A grid of 1 200 points (11 index bits) and 4 flows beside one of 7 875 points (13 bits) and 11 flows: the batch takes 13 index
    bits and 4 time bits and still sorts 32-bit keys; the small grid's records keep their order and their fields."""
    G, n_flows = [grid_points(64, 97, 2) - 368, grid_points(150, 210, 2)], [4, 11]
    assert G == [1200, 7875]
    shift_b, tbits, shift_d, use32 = common(lib, G, n_flows)
    assert (shift_b, tbits, shift_d, use32) == (13, 4, 17, 1)
    for g, n in zip(G, n_flows):
        assert lib.psfm_host_bs_key_order(g, n, shift_b, shift_d, 1) == 0
        assert lib.psfm_host_bs_key_order(g, n, shift_b, shift_d, 0) == 0


def test_widened_keys_sort_like_a_sequences_own_64_bit(lib):
    """The same small grid beside a dense 2160 x 3840 frame (23 index bits) of 100 flows: 64-bit keys for the batch -- the format is
    chosen from the widest grid and the longest sequence -- and the small grid's records keep their order and their fields."""
    G, n_flows = [1200, 2160 * 3840], [4, 100]
    shift_b, tbits, shift_d, use32 = common(lib, G, n_flows, n_records=10 ** 7)
    assert (shift_b, tbits, shift_d, use32) == (23, 7, 30, 0)
    assert lib.psfm_host_bs_key_order(1200, 4, shift_b, shift_d, 0) == 0
    # (the small grid alone would have sorted 32-bit keys; widened, they no longer fit the word)
    assert common(lib, G[:1], n_flows[:1])[3] == 1 and lib.psfm_host_bs_key_order(1200, 12, 27, 31, 1) == -1
