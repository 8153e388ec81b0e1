// Host build of the solve-pacing rules (particle-sfm_amd/csrc/psfm_solve_policy.h) for tests/test_solve_policy_host.py: every function
// of the header through extern "C", the window tally as a row of integers.  With -DPSFM_SOLVE_POLICY_MAIN the file is a stand-alone
// program that runs the tally over random windows (statistics far outside what a solve reports included) -- what a sanitizer build
// (g++ -fsanitize=address,undefined) checks the hist[16] indexing with.  Test infrastructure.
#include "psfm_solve_policy.h"

static psfm_solve_stats stats_of(int iterations, int successful_steps, int termination, int dogleg_nonGN)
{
    psfm_solve_stats q;
    q.iterations = iterations; q.successful_steps = successful_steps; q.termination = termination; q.dogleg_nonGN = dogleg_nonGN;
    q.initial_cost = q.final_cost = 0.0;
    return q;
}

extern "C" int psfm_host_solve_clean(int iterations, int successful_steps, int termination, int dogleg_nonGN, int kmax)
{
    return psfm_solve_clean(stats_of(iterations, successful_steps, termination, dogleg_nonGN), kmax) ? 1 : 0;
}

// stats: n rows of (iterations, successful_steps, termination, dogleg_nonGN).
// out: n_solved, n_unclean, k_need, max_it, mode_next, k_device_paced, k_host_paced(k_prev), unroll_next(unroll_prev), hist[0..15]
extern "C" void psfm_host_tally(const int* stats, int n, int kmax, int k_prev, int unroll_prev, long long* out)
{
    PsfmWindowTally t;
    for (int i = 0; i < n; ++i) t.add(stats_of(stats[4 * i], stats[4 * i + 1], stats[4 * i + 2], stats[4 * i + 3]), kmax);
    const long long v[8] = {t.n_solved, t.n_unclean, t.k_need, t.max_it, t.mode_next(), t.k_device_paced(kmax), t.k_host_paced(k_prev),
                            t.unroll_next(unroll_prev)};
    for (int i = 0; i < 8; ++i) out[i] = v[i];
    for (int i = 0; i < 16; ++i) out[8 + i] = t.hist[i];
}

extern "C" int psfm_host_k_now(int solver_K, int solve_K) { return psfm_k_now(solver_K, solve_K); }
extern "C" int psfm_host_window_launches(int left, int check) { return psfm_window_launches(left, check); }
extern "C" int psfm_host_window_reach(int f_top, int n_launch, int n_last) { return psfm_window_reach(f_top, n_launch, n_last); }
extern "C" int psfm_host_resume_fused_k(int fused_now, int seq, int solver_K, int k_used, int kmax)
{
    return psfm_resume_fused_k(fused_now != 0, seq != 0, solver_K, k_used, kmax);
}
extern "C" int psfm_host_batch_leaves_on_stall(int solver_mode, int stalled, int first_unchecked)
{
    return psfm_batch_leaves_on_stall(solver_mode, stalled, first_unchecked) ? 1 : 0;
}

#ifdef PSFM_SOLVE_POLICY_MAIN
#include <stdio.h>

int main()
{
    uint64_t x = 0x9e3779b97f4a7c15ull;      // (fixed seed)
    auto next = [&](int n) { x = x * 6364136223846793005ull + 1442695040888963407ull; return (int)((x >> 33) % (uint64_t)n); };
    unsigned long long sum = 0;
    long long bad = 0;
    for (int w = 0; w < 20000; ++w) {
        const int n = 1 + next(18), kmax = next(2) ? 8 : 4 + next(28);      // (kmax beyond the histogram's bins too)
        int stats[18 * 4];
        for (int i = 0; i < n; ++i) {
            const bool wild = next(8) == 0;
            const int ss = wild ? next(200) - 20 : next(12);
            stats[4 * i + 1] = ss;
            stats[4 * i] = ss + next(4) - 1;
            stats[4 * i + 2] = next(7) - 1;
            stats[4 * i + 3] = next(4) == 0;
        }
        long long out[24];
        psfm_host_tally(stats, n, kmax, 2 + next(7), 4 + next(61), out);
        long long h = 0;
        for (int i = 0; i < 16; ++i) h += out[8 + i];
        if (h != out[0] || out[1] > out[0] || out[5] < 2 || out[5] > 15 || out[7] < 4 || out[7] > 64) ++bad;
        for (int i = 0; i < 24; ++i) sum = sum * 31ull + (unsigned long long)out[i];
    }
    printf("solve policy sweep: 20000 windows, %lld inconsistent, checksum %llu\n", bad, sum);
    return bad ? 1 : 0;
}
#endif
