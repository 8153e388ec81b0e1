"""The index rules of the multi-problem launch chain (particle-sfm_amd/csrc/psfm_solver_multi.h: which blocks of the grid (blocks,
problems) work for a problem, with which block count, on which rows) compiled for the HOST beside psfm_pc_resident.h (list plan, tree
of the block sums), the per-track arithmetic and the control step, and the chain's host mirror of tests/host/pc_chain_host.cpp.

tests/host/solver_multi_host.cpp runs a table of problems under one grid and each problem alone with the single chain's block count,
and compares the lists, every launch's rows of block sums, every control block and the final iterates byte for byte; here the tables:
row counts 0, 1, 255, 256, 257, one past limit x 256 for limits 2 and 8 (the cap), 64 chunks under limit 8 (the banded plan), tables
of 1, 3 and 64 problems with an empty problem first, in the middle and last, problems that end iterations before their neighbours,
and problems that take no part in the step.  No GPU involved."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from _common import solver_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DP, FP, IP, LP = (ctypes.POINTER(t) for t in (ctypes.c_double, ctypes.c_float, ctypes.c_int, ctypes.c_long))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("solver_multi") / "libsolver_multi_host.so")
    subprocess.run(["g++", "-O2", "-mfma", "-shared", "-fPIC", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "particle-sfm_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "solver_multi_host.cpp"), os.path.join(ROOT, "tests", "host", "pc_chain_host.cpp"),
                    "-o", out], check=True)
    L = ctypes.CDLL(out)
    L.pc_host_multi_compare.argtypes = [ctypes.c_int, LP, IP, IP, IP, ctypes.c_int, ctypes.c_int] + [ctypes.POINTER(ctypes.c_void_p)] * 5 + [
        IP, IP, ctypes.c_int, DP, IP]
    L.pc_host_chain_solve.argtypes = [ctypes.c_long, DP, DP, DP, DP, FP, ctypes.c_int, ctypes.c_int, ctypes.c_int, DP, IP, DP]
    return L


@pytest.fixture(scope="module")
def pool():
    """Two batches to cut problems from (computed once): a quiet flow and a noisy one whose solves reject steps and run long."""
    return {"quiet": solver_batch(60, 80, 16400, 1, 0.02), "noisy": solver_batch(60, 80, 3000, 2, 0.5), "kink": solver_batch(45, 70, 600, 3, 0.3, True)}


def problem(pool, name, n, start=0):
    uv, r1, r2, sc, fl = pool[name]
    c = lambda a, w: np.ascontiguousarray(a[start:start + n], np.float64).reshape(-1, w)
    return dict(n=n, x0=c(uv, 4), ref1=c(r1, 2), ref2=c(r2, 2), scale=c(sc, 1).reshape(-1), flow=np.ascontiguousarray(fl, np.float32))


def run_table(L, probs, limits, n_flows=None, k=1, cap=None, banded=1, counted=None):
    B = len(probs)
    n_flows = n_flows or [3] * B
    cap = cap or [max(p["n"], 1) for p in probs]
    vp = ctypes.c_void_p
    ptrs = lambda key: (vp * B)(*[p[key].ctypes.data for p in probs])
    counted = (ctypes.c_long * B)(*(counted or [p["n"] for p in probs]))
    H = (ctypes.c_int * B)(*[p["flow"].shape[0] for p in probs])
    W = (ctypes.c_int * B)(*[p["flow"].shape[1] for p in probs])
    x_out = np.full(4 * sum(p["n"] for p in probs) + 4, np.nan)
    stats = np.zeros(4 * B, np.int32)
    rc = L.pc_host_multi_compare(B, counted, (ctypes.c_int * B)(*cap), (ctypes.c_int * B)(*limits), (ctypes.c_int * B)(*n_flows), banded, k,
                                 ptrs("x0"), ptrs("ref1"), ptrs("ref2"), ptrs("scale"), ptrs("flow"), H, W, 2 * 200 + 64,
                                 x_out.ctypes.data_as(DP), stats.ctypes.data_as(IP))
    return rc, x_out, stats.reshape(B, 4)


def chain_alone(L, p):
    """The chain's host mirror (terms added in track order): the same decisions, positions to rounding."""
    n = p["n"]
    out, stats, costs = np.empty((n, 4)), np.zeros(7, np.int32), np.zeros(2)
    H, W = p["flow"].shape[:2]
    rc = L.pc_host_chain_solve(n, p["x0"].ctypes.data_as(DP), p["ref1"].ctypes.data_as(DP), p["ref2"].ctypes.data_as(DP), p["scale"].ctypes.data_as(DP),
                               p["flow"].ctypes.data_as(FP), H, W, 1, out.ctypes.data_as(DP), stats.ctypes.data_as(IP), costs.ctypes.data_as(DP))
    assert rc == 0
    return out, stats


def test_index_rules_at_their_switching_points(lib):
    for limit in (1, 2, 8, 512):
        for n, want in ((1, 1), (255, 1), (256, 1), (257, 2), (limit * 256, limit), (limit * 256 + 1, limit), (10 ** 6, min(limit, 3907))):
            want = min(want, limit)
            assert lib.pc_host_multi_blocks(n, limit) == want, (n, limit)
            assert [lib.pc_host_multi_works(b, n, limit) for b in (0, want - 1, want, want + 7)] == [1, 1, 0, 0]
        assert lib.pc_host_multi_blocks(0, limit) == 1 and lib.pc_host_multi_works(0, 0, limit) == 0      # no rows: no block works
    # a problem takes part in steps 1 .. n_flows - 1; forward the solve samples map k, backward map n_flows - k - 1
    assert [lib.pc_host_multi_active(k, 5) for k in (-1, 0, 1, 4, 5)] == [0, 0, 1, 1, 0] and lib.pc_host_multi_active(1, 1) == 0
    assert [lib.pc_host_multi_map(k, 5, 0) for k in (1, 4)] == [1, 4] and [lib.pc_host_multi_map(k, 5, 1) for k in (1, 4)] == [3, 0]


@pytest.mark.parametrize("cap,limit", [(1, 512), (257, 512), (700, 2), (2049, 8), (16400, 8), (16400, 512), (40000, 16)])
def test_list_pitch_holds_every_row_count_up_to_the_capacity(lib, cap, limit):
    pitch = lib.pc_host_multi_pitch(cap, limit)
    counts = sorted(set([1, 255, 256, 257, cap] + [c for c in (511, 512, 513, 2048, 2049, 16128, 16129, 16385) if c <= cap]))
    for n in counts:
        for banded in (0, 1):
            assert lib.pc_host_longest_list(n, limit, banded) <= pitch, (n, banded)


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_a_table_of_one_problem(lib, pool, n):
    p = problem(pool, "noisy", n)
    rc, x, st = run_table(lib, [p], [512])
    assert rc == 0
    if n == 0:
        assert st[0, 2] == 0                      # no launch worked: no solve
        return
    want, ws = chain_alone(lib, p)
    assert st[0, 0] == ws[0] and st[0, 1] == ws[2] and float(np.abs(x[:4 * n].reshape(-1, 4) - want).max()) <= 1e-9


@pytest.mark.parametrize("empty_at", [0, 1, 2])
def test_three_problems_with_an_empty_one(lib, pool, empty_at):
    probs = [problem(pool, "noisy", 257), problem(pool, "quiet", 255, 100), problem(pool, "kink", 256)]
    probs[empty_at] = problem(pool, "quiet", 0)
    rc, x, st = run_table(lib, probs, [512, 512, 512])
    assert rc == 0 and st[empty_at, 2] == 0 and all(st[b, 2] > 0 for b in range(3) if b != empty_at)
    # one neighbour ends several launches before the other, and everybody was offered every launch (three behind the last end)
    worked = [st[b, 2] for b in range(3) if b != empty_at]
    assert len(set(st[:, 3])) == 1 and st[0, 3] >= max(worked) + 3 and min(worked) + 3 <= max(worked)
    off = 0
    for b, p in enumerate(probs):
        if p["n"]:
            want, ws = chain_alone(lib, p)
            assert st[b, 0] == ws[0] and st[b, 1] == ws[2]
            assert float(np.abs(x[off:off + 4 * p["n"]].reshape(-1, 4) - want).max()) <= 1e-9
        off += 4 * p["n"]


@pytest.mark.parametrize("limit,n", [(2, 2 * 256 + 1), (8, 8 * 256 + 1), (8, 64 * 256 + 3)])
def test_the_cap_binds_and_the_banded_plan(lib, pool, limit, n):
    """One row past limit x 256: the block count is the limit and some block takes two chunks.  64 chunks under limit 8: the XCD-banded
    plan (pc_list_plan bands a grid that is a multiple of 8 with 64 chunks or more)."""
    assert lib.pc_host_multi_blocks(n, limit) == limit
    probs = [problem(pool, "quiet", 100, 7), problem(pool, "quiet", n), problem(pool, "noisy", 300)]
    rc, x, st = run_table(lib, probs, [512, limit, 512])
    assert rc == 0 and all(st[:, 2] > 0)
    rc0, x0, st0 = run_table(lib, probs, [512, limit, 512], banded=0)
    assert rc0 == 0 and np.array_equal(st0[:, :2], st[:, :2])
    # the plan of the large problem is the banded one only at 64 chunks: block 1 then starts at the second band, not at chunk 1
    assert lib.pc_host_first_chunk(1, limit, n, 1) == ((n + 255) // 256 + 7) // 8 if n >= 64 * 256 else lib.pc_host_first_chunk(1, limit, n, 1) == 1
    assert lib.pc_host_first_chunk(1, limit, n, 0) == 1
    want, ws = chain_alone(lib, probs[1])
    assert st[1, 0] == ws[0] and st[1, 1] == ws[2] and float(np.abs(x[400:400 + 4 * n].reshape(-1, 4) - want).max()) <= 1e-9


def test_sixty_four_problems_some_empty_some_out_of_the_step(lib, pool):
    rng = np.random.default_rng(5)
    sizes = [0] + [int(v) for v in rng.choice([1, 3, 64, 65, 255, 256, 257, 300], size=62)] + [0]
    sizes[31] = 0
    names = ["noisy", "quiet", "kink"]
    probs = [problem(pool, names[b % 3], n, (7 * b) % 200) for b, n in enumerate(sizes)]
    n_flows = [3] * 64
    n_flows[5], n_flows[40] = 1, 2                # k = 2: a sequence of one flow and one that has ended take no part
    limits = [512 if b % 2 else 1 for b in range(64)]
    rc, x, st = run_table(lib, probs, limits, n_flows=n_flows, k=2)
    assert rc == 0
    worked = st[:, 2] > 0
    for b in range(64):
        assert worked[b] == (sizes[b] > 0 and n_flows[b] > 2), b
    assert len(set(st[worked, 0])) > 3            # they end at different iterations


def test_rows_beyond_the_capacity_are_not_touched(lib, pool):
    """The scan's count is bounded by the rows the buffers hold (pc_multi_rows): a count above the capacity solves the capacity's rows."""
    p = problem(pool, "noisy", 300)
    rc, x, st = run_table(lib, [p], [512])
    rc2, x2, st2 = run_table(lib, [p], [512], cap=[300], counted=[500])
    assert rc == 0 and rc2 == 0 and x.tobytes() == x2.tobytes() and np.array_equal(st, st2) and st[0, 2] > 0
