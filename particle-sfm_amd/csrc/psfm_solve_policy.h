// psfm_solve_policy.h -- how the host PACES the path-consistency solves of the frame recurrence: the one statement of the rules that
// psfm_track / psfm_connect (psfm_api.hip) and psfm_connect_batch (psfm_batch.hip) follow window by window -- whether a solve was
// "clean", whether the next window runs fused solves or the launch chain, how many iterations (K) a fused launch speculates, how many
// launches a window enqueues, how far the device can get with them, which K a stalled fused solve is retried with, when a sequence
// leaves its batch.  Pure functions of integers: no HIP, no psfm_ctx -- the CPU suite compiles this header with g++
// (tests/host/solve_policy_host.cpp) and pins every rule at its switching points.  kmax is a parameter: the callers pass
// psfm_solve_kmax().
#pragma once
#include <stdint.h>

#include "../../include/psfm.h"

// "clean": every iteration but the terminating one took the Gauss-Newton step and was accepted --
// what the fused solve speculates; it then needs successful_steps + 1 iterations in its launch
// (termination 5 = Ceres' FAILURE: the reference ignores it, trajectory_optimize.cpp:81-82, and carries on
// with the positions it had -- so does the device; the caller sees it in the solve statistics)
static inline bool psfm_solve_clean(const psfm_solve_stats& q, int kmax)
{
    return q.dogleg_nonGN == 0 && q.termination != PSFM_TERM_FAILURE &&
           (q.iterations == q.successful_steps + 1 ||
            (q.termination == PSFM_TERM_GRADIENT_TOL && q.iterations == q.successful_steps)) &&
           q.successful_steps + 1 <= kmax;
}

// The statistics of one window (the frames between two checkpoints), frame by frame, and what the next window does about them.
struct PsfmWindowTally {
    int n_solved = 0, n_unclean = 0;
    int k_need = 2;          // the largest successful_steps + 1 of the clean solves
    int max_it = 0;          // the most iterations of any frame added
    int hist[16] = {0};      // solves by min(successful_steps + 1, 15)

    void add(const psfm_solve_stats& q, int kmax)
    {
        if (q.termination >= 0) {   // -1: no track had a full buffer, nothing was solved
            ++n_solved;
            if (!psfm_solve_clean(q, kmax)) ++n_unclean;
            else if (q.successful_steps + 1 > k_need) k_need = q.successful_steps + 1;
            const int need = q.successful_steps + 1;
            ++hist[need < 0 ? 0 : (need < 15 ? need : 15)];   // (bins 0, 1 and those above kmax are never chosen)
        }
        if (q.iterations > max_it) max_it = q.iterations;
    }
    // How the next window's solves are enqueued: the fused solve (0) -- ONE launch that speculates K Gauss-Newton iterations -- or the
    // launch chain (1).  A window whose solves rejected steps / left the Gauss-Newton path (more than one in eight) sends the next
    // window to the chain, a clean window brings the fused solve back.  (Meaningful when n_solved > 0.)
    int mode_next() const { return (n_unclean * 8 > n_solved) ? 1 : 0; }
    // device-paced: an iteration more than speculated costs one more launch, not a redo -- follow the MOST COMMON
    // need of the window instead of its maximum
    int k_device_paced(int kmax) const
    {
        int best = 2;
        for (int q = 2; q <= kmax && q < 16; ++q) if (hist[q] > hist[best]) best = q;
        return best;
    }
    // host-paced: an iteration more than speculated is a redo -- K follows the accepted steps seen: up at once, down half the way
    int k_host_paced(int k_prev) const { return k_need > k_prev ? k_need : k_prev - (k_prev - k_need + 1) / 2; }
    // adapt the unroll to what this sequence needs, within [4, 64]: a solve of k iterations needs k-1 pc_iter
    // launches (pc_init does the first), so max+1 leaves two spare launches for the slowest solve seen in the
    // window (a spare launch is a no-op that costs < 1 us behind another one; a solve that still runs out raises the stall flag)
    int unroll_next(int prev) const
    {
        int want = max_it + 1;
        want = want < 4 ? 4 : (want > 64 ? 64 : want);
        return want > prev ? want : prev - (prev - want + 1) / 2;   // decays all the way
    }
};

// iterations a fused launch speculates: the forced K (psfm_ctx_set_solver) if set, else the adapted one
static inline int psfm_k_now(int solver_K, int solve_K) { return solver_K > 0 ? solver_K : solve_K; }

// launches of one device-paced window with `left` frames to go: two spare -- continuation launches of the window
static inline int psfm_window_launches(int left, int check) { return (left < check ? left : check) + 2; }

// the furthest frame the device can get to with n_launch launches from frame f_top (n_last: the last frame there is)
static inline int psfm_window_reach(int f_top, int n_launch, int n_last) { return f_top + n_launch - 1 < n_last ? f_top + n_launch - 1 : n_last; }

// a fused solve that ran out of iterations is first retried with two iterations more (the K this returns); the chain
// takes what is left (0) -- and every stalled solve of a chain window, of a device-paced window, with a forced K, or at kmax
static inline int psfm_resume_fused_k(bool fused_now, bool seq, int solver_K, int k_used, int kmax)
{
    return (fused_now && !seq && solver_K == 0 && k_used < kmax) ? (k_used + 2 < kmax ? k_used + 2 : kmax) : 0;
}

// psfm_connect_batch, a sequence whose solve of frame `stalled` stalled with fewer than eight solves of the window in front of it:
// whatever they were, the window counts as one whose solves reject steps (one in eight is the bar of mode_next) and the sequence is
// about to leave the batch -- and to be run again from its first frame by psfm_connect.  No point in redoing this solve with
// launches first.  (psfm_ctx_set_solver(ctx, 2, k) keeps a sequence in.)
static inline bool psfm_batch_leaves_on_stall(int solver_mode, int stalled, int first_unchecked)
{
    return stalled >= 0 && solver_mode != 2 && stalled - first_unchecked < 8;
}
