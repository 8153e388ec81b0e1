"""The index rules of the FRAME-MODE multi-problem launch chain (particle-sfm_amd/csrc/psfm_batch_chain.h: which sequences of a table
take part in frame f, gridDim.x, which blocks work for a sequence and with which count, the lanes a solve looks at, the list pitch for a
block count known on the host, the rebase of a row to a frame) compiled for the HOST with g++ beside the single chain's list plan
(psfm_pc_resident.h).

tests/host/batch_chain_host.cpp runs a table of sequences under one grid and each sequence alone with the single chain's block count
(pc_blocks of psfm_solver.hip restated, resident budget applied) and compares the set of working blocks, every block's list and the
count the ticket waits for; here the tables: lane counts 1, 255, 256, 257 and more lanes than the tables hold, capacities on both
sides of limit x 256, budgets 1, 2, 8, 16, the banded plan at 64 chunks, lengths n_flows = 1 and 2, frames below 1 and beyond a
sequence's end.  The same file with its own main is built with -fsanitize=address,undefined and run.  No GPU involved."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "batch_chain_host.cpp")
INC = os.path.join(ROOT, "particle-sfm_amd", "csrc")
IP = ctypes.POINTER(ctypes.c_int)
CHAIN_BLOCKS = 512          # PC_CHAIN_BLOCKS of psfm_pc_params.h


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("batch_chain") / "libbatch_chain_host.so")
    subprocess.run(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-I", INC, SRC, "-o", out], check=True)
    L = ctypes.CDLL(out)
    L.bc_blocks.argtypes = [ctypes.c_longlong, ctypes.c_int]
    L.bc_single_blocks.argtypes = [ctypes.c_longlong, ctypes.c_int, ctypes.c_int]
    L.bc_pitch.argtypes = [ctypes.c_longlong, ctypes.c_int]
    L.bc_rebase_check.argtypes = [ctypes.c_int, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int]
    L.bc_grid_x.argtypes = [IP, ctypes.c_int]
    L.bc_table_compare.argtypes = [ctypes.c_int, IP, IP, ctypes.c_int, IP, IP, ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_int, IP]
    return L


def limit_of(budget):
    return budget if 0 < budget < CHAIN_BLOCKS else CHAIN_BLOCKS


# (lanes in use, capacity, resident budget, n_flows)
TABLE = [(1, 1, 0, 1), (200, 255, 0, 2), (256, 256, 0, 3), (300, 257, 1, 3), (700, 700, 2, 5), (2100, 2049, 8, 9), (9000, 16400, 0, 4),
         (16385, 16400, 8, 6), (40000, 40000, 16, 2), (131072, 140000, 0, 7)]


def births(table, seed=3):
    rng = np.random.default_rng(seed)
    return [np.ascontiguousarray(rng.integers(-2, 9, size=cap), np.int32) for _, cap, _, _ in table]


def run_table(L, table, f, banded, birth):
    B = len(table)
    arr = lambda k: (ctypes.c_int * B)(*[row[k] for row in table])
    worked = (ctypes.c_int * B)()
    ptrs = (ctypes.c_void_p * B)(*[b.ctypes.data for b in birth])
    rc = L.bc_table_compare(B, arr(0), arr(1), CHAIN_BLOCKS, arr(2), arr(3), ptrs, f, banded, worked)
    return rc, list(worked)


def test_block_count_is_pc_blocks_with_the_resident_budget_applied(lib):
    for budget in (0, 1, 2, 8, 16, 511, 512, 600):
        limit = limit_of(budget)
        for cap in (1, 255, 256, 257, limit * 256 - 1, limit * 256, limit * 256 + 1, 10 ** 6):
            want = max(1, min((cap + 255) // 256, limit))
            assert lib.bc_blocks(cap, limit) == want == lib.bc_single_blocks(cap, CHAIN_BLOCKS, budget), (cap, budget)
            # the block set of a sequence: blocks 0 .. count - 1 of the grid, no other
            assert [lib.bc_works(b, want) for b in (-1, 0, want - 1, want, want + 7)] == [0, 1, 1, 0, 0]
    nb = (ctypes.c_int * 4)(3, 160, 1, 8)
    assert lib.bc_grid_x(nb, 4) == 160 and lib.bc_grid_x(nb, 1) == 3 and lib.bc_grid_x((ctypes.c_int * 1)(1), 1) == 1


def test_which_sequences_take_part_in_a_frame(lib):
    # a solve happens from frame 1 on; a sequence of one flow never solves, one of two solves exactly once
    assert [lib.bc_active(f, 1) for f in (-1, 0, 1, 2)] == [0, 0, 0, 0]
    assert [lib.bc_active(f, 2) for f in (-1, 0, 1, 2)] == [0, 0, 1, 0]
    assert [lib.bc_active(f, 9) for f in (0, 1, 8, 9, 10)] == [0, 1, 1, 0, 0]
    # the lanes of a solve: the device's count bounded by the tables
    assert [lib.bc_rows(n, 300) for n in (-5, 0, 1, 299, 300, 301, 10 ** 6)] == [0, 0, 1, 299, 300, 300, 300]


@pytest.mark.parametrize("banded", [0, 1])
def test_a_table_of_sequences_against_each_alone(lib, banded):
    birth = births(TABLE)
    f_top = max(n for _, _, _, n in TABLE)
    for f in range(-1, f_top + 2):
        rc, worked = run_table(lib, TABLE, f, banded, birth)
        assert rc == 0, (f, rc)
        for (lanes, cap, budget, n_flows), w in zip(TABLE, worked):
            # sequences beyond their last frame (and everybody in frames below 1) take no part; the others work with pc_blocks' count
            want = lib.bc_single_blocks(cap, CHAIN_BLOCKS, budget) if 1 <= f < n_flows else 0
            assert w == want, (f, lanes, cap, budget, n_flows)
    # the 1-flow sequence never worked, the 2-flow sequences exactly in frame 1
    assert [run_table(lib, TABLE, f, banded, birth)[1][0] for f in (0, 1, 2)] == [0, 0, 0]
    assert [run_table(lib, TABLE, f, banded, birth)[1][1] > 0 for f in (0, 1, 2)] == [False, True, False]


def test_one_sequence_and_the_only_long_one_last(lib):
    one = [(300, 600, 0, 4)]
    assert run_table(lib, one, 2, 1, births(one))[0] == 0
    tab = [(100, 256, 0, 2), (50, 256, 0, 1), (5000, 6000, 4, 9)]
    b = births(tab)
    for f in (1, 2, 8, 9):
        rc, worked = run_table(lib, tab, f, 1, b)
        assert rc == 0 and worked == [1 if f == 1 else 0, 0, 4 if f <= 8 else 0]


@pytest.mark.parametrize("cap,budget", [(1, 0), (257, 0), (700, 2), (2049, 8), (16400, 8), (16400, 0), (40000, 16), (140000, 0)])
def test_list_pitch_covers_every_lane_count_up_to_the_capacity(lib, cap, budget):
    nb = lib.bc_single_blocks(cap, CHAIN_BLOCKS, budget)
    pitch = lib.bc_pitch(cap, nb)
    # what pc_setup sizes for this context
    assert pitch == (((cap + 255) // 256 + nb - 1) // nb + 1) * 256
    counts = range(1, cap + 1) if cap <= 2049 else sorted(set(
        [1, 255, 256, 257, cap - 1, cap] + [c for c in (511, 512, 513, 2048, 2049, 16128, 16129, 16384, 16385, 131072, 131073) if c <= cap] +
        list(range(1, cap, 997))))
    for n in counts:
        for banded in (0, 1):
            assert lib.bc_longest_list(n, nb, banded) <= pitch, (n, banded)


@pytest.mark.parametrize("n_flows,cap,pix", [(2, 300, 35), (3, 257, 64), (9, 2049, 35), (50, 16400, 9)])
def test_rebase_of_a_row_is_pc_params_rebase(lib, n_flows, cap, pix):
    for f in sorted({1, 2, n_flows - 1}):
        if 1 <= f < n_flows:
            assert lib.bc_rebase_check(n_flows, cap, pix, f) == 0, f


def test_stand_alone_program_under_address_and_undefined_sanitizers(tmp_path):
    """The same file with its own main, every rule over a table, built with the sanitizers and run on the CPU (nothing loaded into
    python is run under a sanitizer)."""
    exe = str(tmp_path / "batch_chain_host_asan")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DBATCH_CHAIN_MAIN",
                    "-I", INC, SRC, "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "batch_chain_host: ok" in r.stdout, r.stdout
