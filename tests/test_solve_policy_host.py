"""The solve-pacing rules without a GPU: particle-sfm_amd/csrc/psfm_solve_policy.h -- the clean-solve predicate, the window tally
and what the next window does about it (fused solves or the launch chain, K device-paced and host-paced, the unroll), the launches
and the reach of a device-paced window, the K a stalled fused solve is retried with, when a sequence leaves its batch -- compiled
for the host with g++ and driven by tests/host/solve_policy_host.cpp.  Every function is checked against a restatement of its rule
written here, at its switching points, and the tally over random windows against a transcription of the two loops it replaced."""
import ctypes
import itertools
import os
import random
import subprocess
from collections import namedtuple

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRADIENT_TOL, FAILURE = 2, 5          # PSFM_TERM_* (include/psfm.h)
Q = namedtuple("Q", "iterations successful_steps termination dogleg_nonGN")
FIELDS = ("n_solved", "n_unclean", "k_need", "max_it", "mode_next", "k_device_paced", "k_host_paced", "unroll_next")


@pytest.fixture(scope="module")
def pol(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("solve_policy") / "libsolve_policy_host.so")
    cmd = ["g++", "-O2", "-mfma", "-shared", "-fPIC", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "tests", "host", "shim"), "-I", os.path.join(ROOT, "particle-sfm_amd", "csrc"),
           os.path.join(ROOT, "tests", "host", "solve_policy_host.cpp"), "-o", out]
    subprocess.run(cmd, check=True)
    L = ctypes.CDLL(out)
    i32, vp = ctypes.c_int, ctypes.c_void_p
    L.psfm_host_solve_clean.argtypes = [i32] * 5
    L.psfm_host_tally.argtypes = [vp, i32, i32, i32, i32, vp]
    L.psfm_host_tally.restype = None
    L.psfm_host_k_now.argtypes = [i32] * 2
    L.psfm_host_window_launches.argtypes = [i32] * 2
    L.psfm_host_window_reach.argtypes = [i32] * 3
    L.psfm_host_resume_fused_k.argtypes = [i32] * 5
    L.psfm_host_batch_leaves_on_stall.argtypes = [i32] * 3
    return L


def tally(L, window, kmax, k_prev=4, unroll_prev=6):
    flat = (ctypes.c_int * (4 * max(len(window), 1)))(*[v for q in window for v in q])
    out = (ctypes.c_longlong * 24)()
    L.psfm_host_tally(ctypes.addressof(flat), len(window), kmax, k_prev, unroll_prev, ctypes.addressof(out))
    d = dict(zip(FIELDS, [int(v) for v in out[:8]]))
    d["hist"] = [int(v) for v in out[8:]]
    return d


def clean_restated(q, kmax):
    """Every iteration but the terminating one took the Gauss-Newton step and was accepted (a solve that ends on the gradient
    tolerance may end ON an accepted step), the solve did not fail, and a fused launch of kmax iterations can hold it."""
    accepted_all = q.iterations == q.successful_steps + 1 or (q.termination == GRADIENT_TOL and q.iterations == q.successful_steps)
    return q.dogleg_nonGN == 0 and q.termination != FAILURE and accepted_all and q.successful_steps + 1 <= kmax


def solve(successful_steps, extra=1, termination=0, dogleg=0):
    return Q(successful_steps + extra, successful_steps, termination, dogleg)


@pytest.mark.parametrize("kmax", [8, 4])
def test_clean_predicate_over_the_full_product(pol, kmax):
    n = 0
    for term, nongn, diff, ss in itertools.product((-1, 0, 1, GRADIENT_TOL, 3, 4, FAILURE), (0, 1), (-1, 0, 1, 2),
                                                   (0, 1, kmax - 2, kmax - 1, kmax)):
        q = Q(ss + diff, ss, term, nongn)
        assert bool(pol.psfm_host_solve_clean(*q, kmax)) == clean_restated(q, kmax), (q, kmax)
        n += 1
    assert n == 7 * 2 * 4 * 5
    # by hand: iterations == successful_steps is clean on GRADIENT_TOL only
    assert pol.psfm_host_solve_clean(3, 3, GRADIENT_TOL, 0, kmax) == 1
    for term in (-1, 0, 1, 3, 4, FAILURE):
        assert pol.psfm_host_solve_clean(3, 3, term, 0, kmax) == 0
    # successful_steps + 1 == kmax fits a fused launch, kmax + 1 does not
    assert pol.psfm_host_solve_clean(kmax, kmax - 1, 0, 0, kmax) == 1
    assert pol.psfm_host_solve_clean(kmax + 1, kmax, 0, 0, kmax) == 0
    assert pol.psfm_host_solve_clean(3, 2, 0, 1, kmax) == 0 and pol.psfm_host_solve_clean(3, 2, FAILURE, 0, kmax) == 0


def test_mode_of_the_next_window(pol):
    unclean, ok, none = solve(2, dogleg=1), solve(2), Q(0, 0, -1, 0)
    t = tally(pol, [unclean] + [ok] * 7, 8)
    assert (t["n_solved"], t["n_unclean"], t["mode_next"]) == (8, 1, 0)          # 1 * 8 > 8 is false: fused
    t = tally(pol, [unclean] + [ok] * 6, 8)
    assert (t["n_solved"], t["n_unclean"], t["mode_next"]) == (7, 1, 1)          # 8 > 7: the launch chain
    assert tally(pol, [ok] * 5, 8)["mode_next"] == 0
    # frames without a solve count in neither number
    t = tally(pol, [unclean] + [ok] * 6 + [none] * 9, 8)
    assert (t["n_solved"], t["n_unclean"], t["mode_next"]) == (7, 1, 1)
    t = tally(pol, [none] * 3, 8)
    assert (t["n_solved"], t["n_unclean"]) == (0, 0)


def test_device_paced_k(pol):
    kmax = 8
    assert tally(pol, [], kmax)["k_device_paced"] == 2 and tally(pol, [Q(0, 0, -1, 0)] * 4, kmax)["k_device_paced"] == 2
    assert tally(pol, [solve(2), solve(4), solve(4), solve(2)], kmax)["k_device_paced"] == 3      # bins 3 and 5 tie: the smaller
    t = tally(pol, [solve(19)] * 5 + [solve(3)], kmax)
    assert t["hist"][15] == 5 and t["hist"][4] == 1 and t["k_device_paced"] == 4                   # need 20 -> bin 15, never chosen
    assert tally(pol, [solve(kmax - 1)] * 2 + [solve(2)], kmax)["k_device_paced"] == kmax           # bin kmax can win
    t = tally(pol, [solve(kmax)] * 3 + [solve(2)], kmax)
    assert t["hist"][kmax + 1] == 3 and t["k_device_paced"] == 3                                    # bin kmax + 1 cannot
    # bins 0 and 1 are never chosen either: a window of solves that accepted no step speculates 2
    assert tally(pol, [solve(0)] * 4, kmax)["k_device_paced"] == 2
    # an unclean solve counts in the histogram like a clean one (its bin is what it accepted)
    assert tally(pol, [solve(3, dogleg=1)] * 2 + [solve(2)], kmax)["k_device_paced"] == 4


def test_host_paced_k_and_unroll(pol):
    assert tally(pol, [solve(5)], 8, k_prev=3)["k_host_paced"] == 6              # growth: the new value at once
    assert tally(pol, [solve(5)], 8, k_prev=6)["k_host_paced"] == 6              # the need met exactly: K stays

    def decay(window, k):
        seen = []
        for _ in range(4):
            k = tally(pol, window, 8, k_prev=k)["k_host_paced"]
            seen.append(k)
        return seen
    # decay: K gives up half the distance to the need, rounded up -- k - (k - k_need + 1) // 2.
    # k_need = 2 (distances 6, 3, 1): 8 -> 5 -> 3 -> 2, where it stays.  The chain 8 -> 5 -> 4 -> 3 is the one of k_need = 3
    # (distances 5, 2, 1), pinned beside it.
    assert decay([solve(1)], 8) == [5, 3, 2, 2]
    assert decay([solve(2)], 8) == [5, 4, 3, 3]
    assert decay([Q(0, 0, -1, 0)], 8) == [5, 3, 2, 2]                            # (no solve in the window: k_need is still 2)
    # unclean solves do not raise k_need; k_need starts at 2
    assert tally(pol, [solve(6, dogleg=1)], 8)["k_need"] == 2 and tally(pol, [solve(6)], 8)["k_need"] == 7
    # unroll: max_it + 1 within [4, 64], up at once, down half the way
    assert tally(pol, [Q(0, 0, -1, 0)], 8, unroll_prev=4)["unroll_next"] == 4    # max_it = 0
    assert tally(pol, [solve(1)], 8, unroll_prev=4)["unroll_next"] == 4          # 2 + 1 clamps at 4
    assert tally(pol, [Q(200, 199, 3, 0)], 8, unroll_prev=6)["unroll_next"] == 64
    assert tally(pol, [Q(63, 62, 0, 0)], 8, unroll_prev=6)["unroll_next"] == 64 and tally(pol, [Q(62, 61, 0, 0)], 8, unroll_prev=6)["unroll_next"] == 63
    assert tally(pol, [Q(9, 8, 0, 0)], 8, unroll_prev=6)["unroll_next"] == 10
    assert [tally(pol, [solve(1)], 8, unroll_prev=p)["unroll_next"] for p in (64, 34, 19, 11, 7, 5, 4)] == [34, 19, 11, 7, 5, 4, 4]
    # max_it counts frames without a solve too
    assert tally(pol, [Q(30, 0, -1, 0), solve(2)], 8)["max_it"] == 30


def test_windows(pol):
    assert [pol.psfm_host_window_launches(left, 16) for left in (1, 15, 16, 17, 100)] == [3, 17, 18, 18, 18]      # min(left, check) + 2
    assert pol.psfm_host_window_reach(1, 18, 100) == 18 and pol.psfm_host_window_reach(90, 12, 99) == 99
    assert pol.psfm_host_window_reach(82, 18, 99) == 99 and pol.psfm_host_window_reach(81, 18, 99) == 98          # clamps at n_last exactly
    assert pol.psfm_host_window_reach(1, 3, 1) == 1
    for f_top, n_launch, n_last in itertools.product((1, 5, 40), (3, 10, 18), (1, 7, 22, 57, 400)):
        assert pol.psfm_host_window_reach(f_top, n_launch, n_last) == min(f_top + n_launch - 1, n_last)
    assert pol.psfm_host_k_now(0, 5) == 5 and pol.psfm_host_k_now(3, 5) == 3 and pol.psfm_host_k_now(8, 2) == 8


def test_resume_k(pol):
    kmax = 8
    assert pol.psfm_host_resume_fused_k(1, 1, 0, 3, kmax) == 0                   # device-paced
    assert pol.psfm_host_resume_fused_k(0, 0, 0, 3, kmax) == 0                   # the window was chain
    assert pol.psfm_host_resume_fused_k(1, 0, 4, 4, kmax) == 0                   # solver_K > 0: a forced K
    assert pol.psfm_host_resume_fused_k(1, 0, 0, kmax, kmax) == 0                # nothing above kmax to try
    assert pol.psfm_host_resume_fused_k(1, 0, 0, 3, kmax) == 5
    assert pol.psfm_host_resume_fused_k(1, 0, 0, 7, kmax) == 8 and pol.psfm_host_resume_fused_k(1, 0, 0, 6, kmax) == 8
    for fused, seq, forced, k_used, km in itertools.product((0, 1), (0, 1), (0, 3), range(1, 9), (4, 8)):
        want = min(k_used + 2, km) if (fused and not seq and forced == 0 and k_used < km) else 0
        assert pol.psfm_host_resume_fused_k(fused, seq, forced, k_used, km) == want


def test_batch_leaves_on_stall(pol):
    first = 17
    assert pol.psfm_host_batch_leaves_on_stall(0, first + 7, first) == 1         # fewer than eight solves in front of the stalled one
    assert pol.psfm_host_batch_leaves_on_stall(0, first + 8, first) == 0
    assert pol.psfm_host_batch_leaves_on_stall(0, first, first) == 1
    assert pol.psfm_host_batch_leaves_on_stall(0, -1, first) == 0                # nothing stalled
    for stalled in range(first, first + 20):
        assert pol.psfm_host_batch_leaves_on_stall(2, stalled, first) == 0      # psfm_ctx_set_solver(ctx, 2, k) keeps it in


def parent_track_loop(window, kmax, solve_K, solve_unroll, seq):
    """psfm_track_impl's checkpoint as it stood before the rules moved (csrc/psfm_api.hip:685-728 of the parent commit), line for line:
    returns (n_solved, n_unclean, solve_mode or None, solve_K, solve_unroll)."""
    solve_mode = None
    max_it, n_solved, n_unclean, k_need = 0, 0, 0, 2
    for q in window:                                                             # :686
        if q.termination >= 0:                                                   # :689
            clean = (q.dogleg_nonGN == 0 and q.termination != FAILURE and                                        # :695
                     (q.iterations == q.successful_steps + 1 or                                                  # :696
                      (q.termination == GRADIENT_TOL and q.iterations == q.successful_steps)) and                # :697
                     q.successful_steps + 1 <= kmax)                                                             # :698
            n_solved += 1                                                        # :699
            if not clean:                                                        # :700
                n_unclean += 1
            elif q.successful_steps + 1 > k_need:                                # :701
                k_need = q.successful_steps + 1
        if q.iterations > max_it:                                                # :706
            max_it = q.iterations
    if n_solved > 0:                                                             # :708
        solve_mode = 1 if n_unclean * 8 > n_solved else 0                        # :709
        if seq:                                                                  # :710
            hist = [0] * 16                                                      # :713
            for q in window:                                                     # :714
                if q.termination >= 0:                                           # :715
                    hist[q.successful_steps + 1 if q.successful_steps + 1 < 15 else 15] += 1
            best = 2                                                             # :716
            for b in range(2, kmax + 1):                                         # :717
                if hist[b] > hist[best]:
                    best = b
            solve_K = best                                                       # :718
        else:
            solve_K = k_need if k_need > solve_K else solve_K - (solve_K - k_need + 1) // 2                      # :720
    want = max_it + 1                                                            # :726
    want = 4 if want < 4 else (64 if want > 64 else want)                        # :727
    solve_unroll = want if want > solve_unroll else solve_unroll - (solve_unroll - want + 1) // 2               # :728
    return n_solved, n_unclean, solve_mode, solve_K, solve_unroll


def parent_batch_loop(window, kmax, solve_K):
    """batch_run's checkpoint of one sequence as it stood (csrc/psfm_batch.hip:405-426 of the parent commit), line for line:
    returns (n_solved, n_unclean, solve_mode or None, solve_K)."""
    solve_mode = None
    n_solved, n_unclean = 0, 0                                                   # :405
    hist = [0] * 16                                                              # :406
    for q in window:                                                             # :407
        if q.termination < 0:                                                    # :409
            continue
        clean = (q.dogleg_nonGN == 0 and q.termination != FAILURE and                                            # :412
                 (q.iterations == q.successful_steps + 1 or                                                      # :413
                  (q.termination == GRADIENT_TOL and q.iterations == q.successful_steps)) and                    # :414
                 q.successful_steps + 1 <= kmax)                                                                 # :415
        n_solved += 1                                                            # :416
        if not clean:                                                            # :417
            n_unclean += 1
        hist[q.successful_steps + 1 if q.successful_steps + 1 < 15 else 15] += 1                                 # :418
    if n_solved > 0:                                                             # :421
        solve_mode = 1 if n_unclean * 8 > n_solved else 0                        # :422
        best = 2                                                                 # :423
        for b in range(2, kmax + 1):                                             # :424
            if hist[b] > hist[best]:
                best = b
        solve_K = best                                                           # :425
    return n_solved, n_unclean, solve_mode, solve_K


def test_tally_equals_the_two_loops_it_replaced(pol):
    rng = random.Random(20261020)
    modes = set()
    for _ in range(4000):
        kmax = rng.choice((8, 8, 4))
        window = []
        for _ in range(rng.randint(1, 18)):
            ss = rng.choice((0, 1, 2, 2, 3, 3, 4, 5, 6, 7, 8, 9, 13, 14, 15, 20, 70))
            window.append(Q(ss + rng.choice((-1, 0, 1, 1, 1, 1, 2)), ss, rng.choice((-1, 0, 0, 0, 1, 2, 2, 3, 4, 5)), int(rng.random() < 0.1)))
        k_prev, unroll_prev = rng.randint(2, kmax), rng.randint(4, 64)
        t = tally(pol, window, kmax, k_prev, unroll_prev)
        # the callers' guard: mode and K are taken from the tally only when the window had a solve
        got_mode = t["mode_next"] if t["n_solved"] > 0 else None
        for seq in (False, True):
            got_k = (t["k_device_paced"] if seq else t["k_host_paced"]) if t["n_solved"] > 0 else k_prev
            assert (t["n_solved"], t["n_unclean"], got_mode, got_k, t["unroll_next"]) == parent_track_loop(window, kmax, k_prev, unroll_prev, seq), (window, kmax)
        got_k = t["k_device_paced"] if t["n_solved"] > 0 else k_prev
        assert (t["n_solved"], t["n_unclean"], got_mode, got_k) == parent_batch_loop(window, kmax, k_prev), (window, kmax)
        assert sum(t["hist"]) == t["n_solved"]
        modes.add(got_mode)
    assert modes == {None, 0, 1}


def test_stand_alone_sweep_program(tmp_path):
    """the same file as a program of its own (what a sanitizer build -- g++ -fsanitize=address,undefined -- runs): the tally over
    20000 random windows, statistics far outside a solve's included; it exits 0 when every tally is consistent"""
    exe = str(tmp_path / "solve_policy_sweep")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-DPSFM_SOLVE_POLICY_MAIN", "-I", os.path.join(ROOT, "tests", "host", "shim"),
                    "-I", os.path.join(ROOT, "particle-sfm_amd", "csrc"), os.path.join(ROOT, "tests", "host", "solve_policy_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, text=True)
    assert r.returncode == 0 and "0 inconsistent" in r.stdout, r.stdout
