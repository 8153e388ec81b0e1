"""The placed finalize without a GPU: particle-sfm_amd/csrc/psfm_place.h -- when the form runs, and the index arithmetic of its scan and
its placement -- compiled for the host through tests/host/shim and driven by tests/host/place_host.cpp.

The claim under test: lay the records out by (birth frame, births of that frame in the virtual blocks below + ordinal in the block),
sort them STABLY on `last` alone, and the result is np.lexsort((idx, birth, last)) -- the order of the trajectory ids.  The inputs are
what the persistent loop leaves: per frame >= 1 a mask of births, one 64-bit word per 64 consecutive grid points (a wave's ballot).
The rows nobody stores are poisoned, so an index that strays shows."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 0xA5A5A5A5A5A5A5A5


@pytest.fixture(scope="module")
def place(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("place") / "libplace_host.so")
    cmd = ["g++", "-O2", "-mfma", "-shared", "-fPIC", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "tests", "host", "shim"),
           "-I", os.path.join(ROOT, "particle-sfm_amd", "csrc"), os.path.join(ROOT, "tests", "host", "place_host.cpp"), "-o", out]
    subprocess.run(cmd, check=True)
    L = ctypes.CDLL(out)
    i32, i64, vp = ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p
    L.psfm_host_place_form.argtypes = [i32, i32, i32, i32, i64, i64, i32, i32]
    L.psfm_host_place_blocks.argtypes = [i64]
    L.psfm_host_place_table_words.argtypes = [i32, i64]
    L.psfm_host_place_table_words.restype = i64
    L.psfm_host_place_count.argtypes = [vp, i64, i32, i32, i32]
    L.psfm_host_place_run.argtypes = [vp, vp, vp, vp, i64, vp, i64, i32, i32, i32, vp, vp, vp, vp]
    return L


def bits_for(count):
    b = 1
    while (1 << b) < count:
        b += 1
    return b


def shifts(G, n_flows):
    """psfm_track_dims: the grid index takes shift_b bits, birth and last bits_for(n_flows + 2) each."""
    sb = bits_for(G)
    return sb, sb + bits_for(n_flows + 2)


def fits32(G, n_flows):
    lmax = n_flows + 1
    return bits_for(lmax * (lmax + 1) // 2 + lmax + 1) + bits_for(G) <= 32


def make_records(rng, G, n_flows, born, cap):
    """born(b) -> sorted grid indices born in frame b >= 1.  Frame 0: every grid point.  Returns the records in a shuffled order (the
    loop writes them in death order, block by block) and the mask table as the loop leaves it."""
    gw = 4 * ((G + 255) // 256)
    bmask = np.full((n_flows + 1, gw), POISON, np.uint64)
    rec = []
    for b in range(n_flows):
        idx = np.arange(G) if b == 0 else np.asarray(born(b), np.int64)
        assert len(np.unique(idx)) == len(idx) and (len(idx) == 0 or (idx.min() >= 0 and idx.max() < G))
        lanes = rng.permutation(cap)[:len(idx)]                  # tracks born in one frame sit on different columns
        last = rng.integers(b, n_flows + 1, len(idx))
        if b > 0:
            bits = np.zeros(gw * 64, np.uint8)
            bits[idx] = 1
            bmask[b] = np.packbits(bits.reshape(gw, 64), axis=1, bitorder="little").view("<u8").reshape(gw)   # every word stored, zeros too
        rec.append(np.stack([last, np.full(len(idx), b), idx, lanes], 1))
    rec = np.concatenate(rec).astype(np.int32)
    return rec[rng.permutation(len(rec))], bmask


def run(place, rec, bmask, G, n_flows):
    sb, sd = shifts(G, n_flows)
    n = len(rec)
    cols = [np.ascontiguousarray(rec[:, j]) for j in range(4)]
    outs = [np.full(n, -7, np.int32) for _ in range(4)]
    bmask = np.ascontiguousarray(bmask)
    rc = place.psfm_host_place_run(*[c.ctypes.data for c in cols], n, bmask.ctypes.data, G, n_flows, sb, sd, *[o.ctypes.data for o in outs])
    assert rc == 0, "the placement is no permutation of [0, n): code %d" % rc
    return outs


def check(place, rng, G, n_flows, born, cap=None):
    cap = cap or 2 * G + 64
    rec, bmask = make_records(rng, G, n_flows, born, cap)
    got = run(place, rec, bmask, G, n_flows)
    order = np.lexsort((rec[:, 2], rec[:, 1], rec[:, 0]))        # (last, birth, idx): the trajectory ids
    for j in range(4):
        assert np.array_equal(got[j], rec[order, j]), ("last", "birth", "idx", "lane")[j]


def random_born(rng, G, p):
    return lambda b: np.flatnonzero(rng.random(G) < p)


@pytest.mark.parametrize("G,n_flows,p", [(713, 5, 0.3), (256, 3, 0.5), (1000, 12, 0.05), (4225, 7, 0.2), (1, 4, 0.5), (257, 100, 0.02)])
def test_placed_layout_plus_one_stable_pass_is_the_id_order(place, G, n_flows, p):
    rng = np.random.default_rng(G * 1000 + n_flows)
    check(place, rng, G, n_flows, random_born(rng, G, p))


@pytest.mark.parametrize("n_flows", [1, 2])
def test_shortest_sequences(place, n_flows):
    """n_flows 1: frame 0 only, no stored row at all; n_flows 2: one stored row."""
    rng = np.random.default_rng(n_flows)
    check(place, rng, 700, n_flows, random_born(rng, 700, 0.4))


def test_empty_frames_full_blocks_and_a_ragged_last_block(place):
    """Frames without a birth between frames with births; a block whose 256 grid points are all born in one frame (mass respawn)
    beside empty blocks; G no multiple of 256, births on its last grid point."""
    G = 3 * 256 + 41
    rng = np.random.default_rng(11)

    def born(b):
        if b in (1, 4, 5):
            return []
        if b == 2:
            return np.arange(256, 512)                           # block 1 full, blocks 0, 2, 3 empty
        if b == 3:
            return np.arange(G)                                  # every block full, the last one with its 41
        if b == 6:
            return [0, 255, 256, G - 1]
        return np.flatnonzero(rng.random(G) < 0.3)
    check(place, rng, G, 9, born)


@pytest.mark.parametrize("n_flows", [254, 255])
def test_the_longest_sequences_the_form_takes(place, n_flows):
    G = 300
    assert fits32(G, n_flows)
    assert place.psfm_host_place_form(1, *shifts(G, n_flows), n_flows, 10_000, 1000, 1, 1) == 1
    rng = np.random.default_rng(n_flows)
    check(place, rng, G, n_flows, random_born(rng, G, 0.03))


def test_counts_from_the_masks(place):
    G, n_flows = 600, 4
    gb = place.psfm_host_place_blocks(G)
    assert gb == 3 and place.psfm_host_place_table_words(n_flows, G) == 5 * 12
    bmask = np.full((n_flows + 1, 4 * gb), POISON, np.uint64)
    bmask[1:4] = 0
    bmask[1, [0, 5, 6, 11]] = [1, 3, 1 << 63, 7]                 # 1 birth in block 0, 2 + 1 in block 1, 3 in block 2
    bmask[3, :9] = 0xFFFFFFFFFFFFFFFF
    bmask[3, 9] = (1 << 24) - 1                                  # grid points 576 .. 599
    cnt = lambda b, vb: place.psfm_host_place_count(bmask.ctypes.data, G, n_flows, b, vb)
    assert [cnt(0, v) for v in range(gb)] == [256, 256, 88]      # implied: every grid point is born in frame 0
    assert [cnt(3, v) for v in range(gb)] == [256, 256, 88]
    assert [cnt(1, v) for v in range(gb)] == [1, 3, 3]
    assert [cnt(2, v) for v in range(gb)] == [0, 0, 0]
    assert [cnt(4, v) for v in range(gb)] == [0, 0, 0]           # the loop's last frame is n_flows - 1: row n_flows is never read
    assert place.psfm_host_place_blocks(512) == 2 and place.psfm_host_place_blocks(513) == 3 and place.psfm_host_place_blocks(1) == 1


def test_when_the_form_runs(place):
    G = 540 * 960
    sb, sd = shifts(G, 100)
    cap = 2048 * 288
    form = lambda ran, sb, sd, nf, n, sort=1, switch=1, cap=cap: place.psfm_host_place_form(ran, sb, sd, nf, n, cap, sort, switch)
    assert fits32(G, 100)
    assert form(1, sb, sd, 100, 2_000_000) == 1                  # the headline shape
    assert form(0, sb, sd, 100, 2_000_000) == 0                  # per-frame launches: no birth masks
    assert form(1, sb, sd, 100, 2_000_000, switch=0) == 0        # PSFM_FIN_PLACE=0
    assert form(1, sb, sd, 100, 2_000_000, sort=0) == 0          # PSFM_FIN_SORT=0: rocPRIM's sort was asked for
    assert form(1, sb, sd, 100, 2_000_000, sort=2) == 1
    assert [form(1, sb, sd, 100, n) for n in (2**31 - 1, 2**31)] == [1, 0]
    assert [form(1, sb, sd, 100, 2_000_000, cap=c) for c in (2**24, 2**24 + 1)] == [1, 0]      # the lane beside `last` in 32 bits
    # key width: 5760 grid points (13 bits) take 32-bit keys up to 1021 flows -- far beyond 255 -- so the width switches with the grid:
    # 255 flows have 33153 groups (16 bits): 2^16 grid points fit, one more does not
    assert fits32(2**16, 255) and not fits32(2**16 + 1, 255)
    assert form(1, *shifts(2**16, 255), 255, 100_000) == 1
    assert form(1, *shifts(2**16 + 1, 255), 255, 100_000) == 0
    # 1080p at ratio 2 on 64-bit keys: 400 flows
    assert form(1, *shifts(G, 400), 400, 3_000_000) == 0
    # n_flows + 1 <= 256
    small = 300
    assert [form(1, *shifts(small, nf), nf, 50_000) for nf in (1, 2, 254, 255, 256, 257)] == [1, 1, 1, 1, 0, 0]
    assert fits32(small, 256)                                    # (it is the time range that ends the form there, not the key)
