"""The index rules of psfm_track_queries_batch without a GPU: particle-sfm_amd/csrc/psfm_query_batch.h -- the flattened grid, the
block -> (sequence, block inside the sequence) search in the inclusive block prefix, and the plan + scan + offsets over the
concatenation of all sequences -- compiled for the host by tests/host/queries_batch_host.cpp and compared with NumPy."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX, BLOCK, INT32_MAX = 64, 256, 2 ** 31 - 1
EDGES = (0, 1, 255, 256, 257)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("queries_batch") / "libqueries_batch_host.so")
    cmd = ["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "tests", "host", "shim"),
           "-I", os.path.join(ROOT, "tests", "host"), "-I", os.path.join(ROOT, "particle-sfm_amd", "csrc"),
           os.path.join(ROOT, "tests", "host", "queries_batch_host.cpp"), "-o", out]
    subprocess.run(cmd, check=True)
    L = ctypes.CDLL(out)
    vp = ctypes.c_void_p
    L.psfm_host_qb_grid.argtypes = [vp, ctypes.c_int, vp, vp, vp]
    L.psfm_host_qb_grid.restype = ctypes.c_long
    L.psfm_host_qb_locate.argtypes = [vp, vp, ctypes.c_int, vp, vp]
    L.psfm_host_qb_locate.restype = None
    L.psfm_host_qb_finish.argtypes = [vp, ctypes.c_int] + [vp] * 7
    L.psfm_host_qb_finish.restype = None
    return L


def tables():
    """Query counts per sequence: one sequence; 64 sequences; 0, 1, 255, 256 and 257 queries first, in the middle and last; several
    empty sequences in a row; all sequences empty."""
    out = [[n] for n in EDGES + (321, 5000)]
    rng = np.random.default_rng(7)
    out.append([int(v) for v in rng.integers(0, 700, MAX)])
    out.append([(1, 64, 65, 321)[i % 4] for i in range(MAX)])
    for e in EDGES:
        out.append([e, 300, 17])
        out.append([300, e, 17])
        out.append([300, 17, e])
        out.append([e] * 3)
    for a, b in itertools.product(EDGES, EDGES):
        out.append([a, b])
    out.append([5, 0, 0, 0, 257, 0, 0, 1])
    out.append([0, 0, 256, 0, 0])
    out.append([0] * 4)
    out.append([0] * MAX)
    return out


def grid(host, n_q):
    n = np.ascontiguousarray(n_q, dtype=np.int64)
    blk_end, blk0, q0 = np.zeros(MAX, np.int32), np.zeros(MAX, np.int32), np.zeros(MAX + 1, np.int64)
    blocks = host.psfm_host_qb_grid(n.ctypes.data, len(n), blk_end.ctypes.data, blk0.ctypes.data, q0.ctypes.data)
    return blocks, blk_end, blk0, q0


def test_the_bounds_are_the_batch_s(host):
    assert host.psfm_host_qb_max() == MAX and host.psfm_host_qb_block() == BLOCK


@pytest.mark.parametrize("n_q", tables(), ids=lambda v: "-".join(map(str, v[:8])) + ("..." if len(v) > 8 else ""))
def test_grid_and_block_search_against_numpy(host, n_q):
    n = np.asarray(n_q, np.int64)
    B = len(n)
    nblk = (n + BLOCK - 1) // BLOCK
    blocks, blk_end, blk0, q0 = grid(host, n)
    assert blocks == nblk.sum()
    assert np.array_equal(blk_end[:B], np.cumsum(nblk)) and (blk_end[B:] == INT32_MAX).all()
    assert np.array_equal(blk0[:B], np.cumsum(nblk) - nblk)
    assert np.array_equal(q0[:B], np.cumsum(n) - n) and (q0[B:] == n.sum()).all()
    seq, first = np.zeros(blocks, np.int32), np.zeros(blocks, np.int64)
    host.psfm_host_qb_locate(blk_end.ctypes.data, blk0.ctypes.data, blocks, seq.ctypes.data, first.ctypes.data)
    want_seq = np.repeat(np.arange(B), nblk)                       # block k belongs to the sequence whose blocks contain it
    want_first = np.concatenate([np.arange(k) * BLOCK for k in nblk]) if blocks else np.zeros(0, np.int64)
    assert np.array_equal(seq, want_seq) and np.array_equal(first, want_first)
    assert (first < n[seq]).all()                                  # no block without a query, none of an empty sequence


@pytest.mark.parametrize("dirs", ["forward", "backward", "both"])
@pytest.mark.parametrize("n_q", tables(), ids=lambda v: "-".join(map(str, v[:8])) + ("..." if len(v) > 8 else ""))
def test_flattened_plan_and_scan_equal_cumsum_per_sequence(host, n_q, dirs):
    n = np.asarray(n_q, np.int64)
    B, N = len(n), int(np.sum(n_q))
    rng = np.random.default_rng(100 + N + B)
    t = np.ascontiguousarray(rng.integers(0, 50, N), dtype=np.int32)
    lf = np.ascontiguousarray(rng.integers(1, 60, N), dtype=np.int32) if dirs != "backward" else None
    lb = np.ascontiguousarray(rng.integers(1, 60, N), dtype=np.int32) if dirs != "forward" else None
    birth, length = np.full(N, -99, np.int32), np.full(N, -99, np.int32)
    off, points = np.full(N + B, -99, np.int64), np.full(B, -99, np.int64)
    host.psfm_host_qb_finish(n.ctypes.data, B, t.ctypes.data, lf.ctypes.data if lf is not None else None,
                             lb.ctypes.data if lb is not None else None, birth.ctypes.data, length.ctypes.data, off.ctypes.data,
                             points.ctypes.data)
    nf = lf if lf is not None else np.ones(N, np.int32)
    nb = lb if lb is not None else np.ones(N, np.int32)
    assert np.array_equal(length, nb + nf - 1) and np.array_equal(birth, t - (nb - 1))
    q0 = np.cumsum(n) - n
    for b in range(B):
        ln = length[q0[b]:q0[b] + n[b]].astype(np.int64)
        want = np.concatenate([[0], np.cumsum(ln)])
        assert np.array_equal(off[q0[b] + b:q0[b] + b + n[b] + 1], want), b
        assert points[b] == want[-1]
