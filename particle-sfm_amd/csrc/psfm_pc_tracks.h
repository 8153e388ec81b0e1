// psfm_pc_tracks.h -- the per-track work the launch chain and the resident solve (psfm_solver.hip) share: iteration 0 and one trust-region
// iteration of a track whose state is in memory, the order in which the blocks' sums are added + the control step, the write-back.
#pragma once
#include "psfm_pc_params.h"

// ------------------------------------------------------------------------------------------------
// pc_init: iteration 0.  Frame mode also prepares ref1/ref2/scale (trajectory.py:173-183).
// ------------------------------------------------------------------------------------------------
// refs / scale of a track from its p0 (trajectory.py:173-183): the fp32 sampler on flow01, flow02, occ02
__device__ __forceinline__ void pc_refs(const PcParams& P, double2 p0, double2& r1, double2& r2, double& s)
{
    const PsfmTaps t = psfm_taps((float)p0.x, (float)p0.y, P.cw, P.ch, P.H, P.W);
    const PsfmTapIdx k = psfm_tap_idx(P.H, P.W, t);
    const float2 f01 = psfm_sample_flow(P.flow01, k, t);
    const float2 f02 = psfm_sample_flow(P.flow02, k, t);
    const float o02 = psfm_sample_mask(P.occ02, k, t);
    // (1.0 - occ02) * (|flow02| < 20) in fp32; numpy's norm = sqrt(u*u + v*v) without fma (trajectory.py:179)
    const float nrm = sqrtf(__fadd_rn(__fmul_rn(f02.x, f02.x), __fmul_rn(f02.y, f02.y)));
    const float sf = __fmul_rn(__fsub_rn(1.0f, o02), nrm < 20.0f ? 1.0f : 0.0f);
    s = (double)sf;
    r1 = make_double2(p0.x + (double)f01.x, p0.y + (double)f01.y);
    r2 = make_double2(p0.x + (double)f02.x, p0.y + (double)f02.y);
}

// iteration 0 of ONE track (lane i): refs / scale (frame mode: from its p0; batch mode: given), Jacobi scaling from the Jacobian
// at the start values, cost and system there (mu = min_mu); its terms go to acc[], what a solve keeps of it to o.
struct PcInit { double2 r1, r2; double s; PcConst c; double x[4]; PcSys y; };
__device__ __forceinline__ void pc_init_entry(const PcParams& P, int i, bool store, double acc[PC_NSUM], PcInit& o)
{
    const double mu = 1e-8;
    if (P.p0) {
        pc_refs(P, P.p0[i], o.r1, o.r2, o.s);
        if (store) { P.ref1[i] = o.r1; P.ref2[i] = o.r2; P.scale[i] = o.s; }
    } else {
        o.r1 = P.ref1[i]; o.r2 = P.ref2[i]; o.s = P.scale[i];
    }
    const double2 p1 = P.x1a[i], p2 = P.x2a[i];
    o.x[0] = p1.x; o.x[1] = p1.y; o.x[2] = p2.x; o.x[3] = p2.y;
    // Jacobi scaling 1/(1+sqrt(colnorm^2)) from the Jacobian at x0, computed once (trust_region_minimizer.cc)
    double r0[6], j0[4];
    pc_core_eval((const PcF2*)P.flow12, P.H, P.W, o.x, o.r1.x, o.r1.y, o.r2.x, o.r2.y, o.s, r0, j0);
    o.c = pc_core_const(o.s, j0);
    if (store) P.jscale[i] = make_double2(o.c.S0q, o.c.S1q);
    acc[SUM_CNT] += 1.0;
    acc[SUM_COST0] += pc_core_cost(r0);
    pc_core_system<true>(o.x, r0, j0, o.c, mu, pc_core_iA22(o.c, mu), acc, o.y, CH_QUD, CH_QDD);
}

// iteration 0 for this block's tracks: the block's list, then its entries
__device__ __forceinline__ void pc_init_tracks(const PcParams& P, double acc[PC_NSUM])
{
    // the chain step in front of this solve has consumed PsfmCounters::sel (positions of an earlier fused solve): the launch
    // chain works in buffer 0 from here on, whatever becomes of it
    if (P.sel && blockIdx.x == 0 && threadIdx.x == 0) *P.sel = 0;
    const int n = P.n_lanes_ptr ? min(*P.n_lanes_ptr, P.n_rows) : P.n_rows;
#pragma unroll
    for (int k = 0; k < PC_NSUM; ++k) acc[k] = 0.0;
    const int cnt = pc_build_list(P, n);
    const int* lst = P.list + (int64_t)blockIdx.x * P.list_pitch;
    for (int p = threadIdx.x; p < cnt; p += PC_BLOCK) {
        PcInit o;
        pc_init_entry(P, lst[p], true, acc, o);
    }
}

// What one launch of the chain does for ONE track whose state is in memory (lane i): the refresh form (the system at x for a
// raised mu) or the evaluate-ahead form (candidate of (a, b), its cost, the system there).  Sums into acc[].
// (Round 3 measured how early these loads can be requested -- the state with the birth frame, the next track's state under this
// track's arithmetic, a fully software-pipelined loop, two tracks per thread at a time: level or slower, profiles/EXPERIMENTS.md
// 5.2.  What helped is not streaming the state at all: psfm_pc_resident_kernel below.)
#ifndef PC_ITER_PAIR
#define PC_ITER_PAIR true   // the launch chain's taps as 16-byte pairs (psfm_pc_core.h)
#endif
__device__ __forceinline__ void pc_refresh_entry(const PcParams& P, int i, const double2* xc1, const double2* xc2, double mu, double acc[PC_NSUM])
{
    const double2 r1 = P.ref1[i], r2 = P.ref2[i];
    const double s = P.scale[i];
    const PcConst c = pc_const_load(s, P.jscale[i]);
    const double2 p1 = xc1[i], p2 = xc2[i];
    const double x[4] = {p1.x, p1.y, p2.x, p2.y};
    double r[6], jac[4];
    PcSys y;
    pc_core_eval<PC_ITER_PAIR>((const PcF2*)P.flow12, P.H, P.W, x, r1.x, r1.y, r2.x, r2.y, s, r, jac);
    pc_core_system<true>(x, r, jac, c, mu, pc_core_iA22(c, mu), acc, y, CH_QUD, CH_QDD);
}

__device__ __forceinline__ void pc_ahead_entry(const PcParams& P, int i, const double2* xc1, const double2* xc2, double2* xn1, double2* xn2,
                                               double mu, double mu_next, double a, double b, double acc[PC_NSUM])
{
    const PcF2* F12 = (const PcF2*)P.flow12;
    const double2 r1 = P.ref1[i], r2 = P.ref2[i];
    const double s = P.scale[i];
    const PcConst c = pc_const_load(s, P.jscale[i]);
    const double2 p1 = xc1[i], p2 = xc2[i];
    const double x[4] = {p1.x, p1.y, p2.x, p2.y};
    double r[6], jac[4], xp[4], unused[PC_NSUM];      // (unused: the sums at x are in the control block already)
    PcSys y;
#pragma unroll
    for (int k = 0; k < PC_NSUM; ++k) unused[k] = 0.0;
    pc_core_eval<PC_ITER_PAIR>(F12, P.H, P.W, x, r1.x, r1.y, r2.x, r2.y, s, r, jac);
    pc_core_system<false>(x, r, jac, c, mu, pc_core_iA22(c, mu), unused, y, 0, 0);
    pc_core_step<false, false>(x, r, jac, c, y, a, b, acc, xp);
    xn1[i] = make_double2(xp[0], xp[1]);
    xn2[i] = make_double2(xp[2], xp[3]);
    // the candidate's cost and, ahead of the decision, the system there (what the next iteration needs if it is accepted)
    pc_core_eval<PC_ITER_PAIR>(F12, P.H, P.W, xp, r1.x, r1.y, r2.x, r2.y, s, r, jac);
    acc[SUM_COST] += pc_core_cost(r);
    pc_core_system<true>(xp, r, jac, c, mu_next, pc_core_iA22(c, mu_next), acc, y, CH_QUD, CH_QDD);
}

// DoglegStrategy::StepAccepted: the mu of the system at a candidate that is accepted
__device__ __forceinline__ double pc_mu_next(double mu) { return fmax(1e-8, 2.0 * mu / 10.0); }

// ... for the entries p0, p0 + PC_BLOCK, ... of this block's list (the launch chain: all of them; the resident solve: the ones
// beyond the slots it keeps on chip)
__device__ __forceinline__ void pc_iter_tracks(const PcParams& P, int p0, int cur, double mu, double a, double b, bool refresh, double acc[PC_NSUM])
{
    const double2* xc1 = pc_buf1(P, cur);
    const double2* xc2 = pc_buf2(P, cur);
    double2* xn1 = pc_buf1(P, pc_other(cur));
    double2* xn2 = pc_buf2(P, pc_other(cur));
    const double mu_next = pc_mu_next(mu);
    const int cnt = P.list_n[blockIdx.x];
    const int* lst = P.list + (int64_t)blockIdx.x * P.list_pitch;
    if (refresh) {      // the system at x for the mu an invalid step has raised (rare)
        for (int p = p0; p < cnt; p += PC_BLOCK) pc_refresh_entry(P, lst[p], xc1, xc2, mu, acc);
        return;
    }
    for (int p = p0; p < cnt; p += PC_BLOCK) pc_ahead_entry(P, lst[p], xc1, xc2, xn1, xn2, mu, mu_next, a, b, acc);
}

// ------------------------------------------------------------------------------------------------
// The order in which the blocks' sums are added (every form of the chain: launches, the resident solve, the sharded export),
// with L = min(PC_LEADERS, n_blocks) and Q = ceil(ceil(n_blocks / PC_LEADERS) / 4):
//     total = ((t_0 + t_1) + t_2) + t_3,      t_j  = S_{8j} + S_{8j+1} + ... + S_{8j+7}  (those below L, in order)
//     S_x   = ((s_x0 + s_x1) + s_x2) + s_x3,  s_xj = the sums of blocks x + PC_LEADERS m, m in [j Q, (j + 1) Q), in order
// -- S_x is what ONE block of the resident solve (the "leader" x) adds up from its members' granules, the rest is what every
// block adds up from the leaders' (pc_res_allreduce): two hops, a few loads per lane in each.  SUM_GMAX by max.
// ------------------------------------------------------------------------------------------------
// (PC_LEADERS, pc_tree_q and the same order as plain arithmetic on rows -- pc_tree_totals, what the host mirror adds up with: psfm_pc_resident.h)

// Executed by the LAST block of pc_init / pc_iter to finish (detected with a ticket behind write-through partials; the loads
// here bypass the caches -- cdna_hip_programming.md G16): the reduction above, then the scalar control step on thread 0.
// totals of the launch's partial rows, in LDS (pc_totals()), valid for every thread of the block after the call
__device__ __forceinline__ double* pc_totals()
{
    __shared__ double s_tot[PC_NSUM];
    return s_tot;
}
__device__ __forceinline__ void pc_reduce_totals(double* partials, int n_blocks)
{
    __shared__ double s_sub[PC_LEADERS][4][PC_NSUM + 1];
    __shared__ double s_S[PC_LEADERS][PC_NSUM + 1];
    double* s_tot = pc_totals();
    const int L = n_blocks < PC_LEADERS ? n_blocks : PC_LEADERS;
    const int Q = pc_tree_q(n_blocks);
    // work item (x, j, k): PC_LEADERS x 4 x 16 of them, 8 per thread; ALL loads of a thread are issued before the first is used
    // (they bypass the caches: every dependent batch would be a full round trip on the tail of the launch), then added in
    // member order
    constexpr int ITEMS = PC_LEADERS * 4 * 16 / PC_BLOCK, QMAX = PC_MAX_BLOCKS / PC_LEADERS / 4;
    double pv[ITEMS][QMAX];
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        const int w = threadIdx.x + it * PC_BLOCK;
        const int k = w & 15, j = (w >> 4) & 3, x = w >> 6;
        const int cnt = (n_blocks - x + PC_LEADERS - 1) / PC_LEADERS;
#pragma unroll
        for (int u = 0; u < QMAX; ++u) {
            const int m = j * Q + u;
            pv[it][u] = (k < PC_NSUM && x < L && u < Q && m < cnt)
                            ? __hip_atomic_load(&partials[(int64_t)(x + PC_LEADERS * m) * PC_NSUM + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)
                            : 0.0;
        }
    }
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        const int w = threadIdx.x + it * PC_BLOCK;
        const int k = w & 15, j = (w >> 4) & 3, x = w >> 6;
        if (k >= PC_NSUM || x >= L) continue;
        double v = 0.0;
#pragma unroll
        for (int u = 0; u < QMAX; ++u) v = (k == SUM_GMAX) ? fmax(v, pv[it][u]) : v + pv[it][u];
        s_sub[x][j][k] = v;
    }
    __syncthreads();
    for (int w = threadIdx.x; w < PC_LEADERS * 16; w += PC_BLOCK) {
        const int k = w & 15, x = w >> 4;
        if (k >= PC_NSUM || x >= L) continue;
        const double s0 = s_sub[x][0][k], s1 = s_sub[x][1][k], s2 = s_sub[x][2][k], s3 = s_sub[x][3][k];
        s_S[x][k] = (k == SUM_GMAX) ? fmax(fmax(fmax(s0, s1), s2), s3) : ((s0 + s1) + s2) + s3;
    }
    __syncthreads();
    if (threadIdx.x < PC_NSUM) {
        const int k = threadIdx.x;
        double t[4];
        for (int j = 0; j < 4; ++j) {
            double v = 0.0;
            for (int x = 8 * j; x < 8 * j + 8 && x < L; ++x) v = (k == SUM_GMAX) ? fmax(v, s_S[x][k]) : v + s_S[x][k];
            t[j] = v;
        }
        s_tot[k] = (k == SUM_GMAX) ? fmax(fmax(fmax(t[0], t[1]), t[2]), t[3]) : ((t[0] + t[1]) + t[2]) + t[3];
    }
    __syncthreads();
}

// (force-inlined: as a called function it dragged the call ABI's register budget into the kernels -- 248 VGPRs,
// 2 waves/SIMD -- although the per-track code needs 152)
__device__ __forceinline__ void pc_reduce_and_control(PsfmSolveCtrl* __restrict__ ctrl, double* partials, int n_blocks,
                                                      int is_init, double* export_sums)
{
    pc_reduce_totals(partials, n_blocks);
    const double* s_tot = pc_totals();
    if (export_sums) {
        if (threadIdx.x < PC_NSUM) export_sums[threadIdx.x] = s_tot[threadIdx.x];
        return;
    }
    if (threadIdx.x != 0) return;
    PsfmSolveCtrl C = *ctrl;
    pc_chain_control(C, s_tot, is_init ? 0 : 1);
    C.launches += 1;
    *ctrl = C;
}

// what thread 0 of block 0 leaves behind a finished solve of the chain: the frame's statistics, PsfmCounters::sel, the lane snapshot
__device__ __forceinline__ void pc_writeback_scalars(const PcParams& P, const PsfmSolveCtrl& C)
{
    if (P.stats_dev) {
        psfm_solve_stats st;
        st.iterations = C.iteration; st.successful_steps = C.successful;
        st.termination = C.n_tracks == 0 ? -1 : C.termination; st.dogleg_nonGN = C.nonGN;
        st.initial_cost = C.initial_cost; st.final_cost = C.x_cost;
        if (C.failed) st.termination = PSFM_TERM_FAILURE;
        P.stats_dev[P.frame] = st;
    }
    if (P.sel) {
        *P.sel = 0;                                   // the iterate is (being) copied into buffer 0 right here
        if (P.n_lanes_snap) P.n_lanes_snap[(P.frame + 1) & 1] = *P.n_lanes_ptr;   // (no chain step is running: the lane count is final)
    }
}

// final: if the accepted iterate lives in the scratch pair, copy it back (frame mode: into the log); C: the final control block
__device__ __forceinline__ void pc_writeback_tracks(const PcParams& P, const PsfmSolveCtrl& C, double* out_rows)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) pc_writeback_scalars(P, C);
    const int n = P.n_lanes_ptr ? min(*P.n_lanes_ptr, P.n_rows) : P.n_rows;
    // A failed solve is not an error (the reference ignores Ceres' FAILURE, trajectory_optimize.cpp:81-82) and Ceres
    // hands the parameters back as they came in (solver.cc Minimize(), Summary::IsSolutionUsable() is false): buffer 0,
    // which the chain never writes before this point, whatever was accepted on the way -- non-finite residuals at
    // iteration 0, five invalid steps in a row or a system that lost definiteness behind accepted steps alike.
    const int cur = C.failed ? 0 : C.cur;
    if (cur == 0 && !out_rows) return;
    const double2* xc1 = pc_buf1(P, cur);
    const double2* xc2 = pc_buf2(P, cur);
    for (int i = blockIdx.x * PC_BLOCK + threadIdx.x; i < n; i += gridDim.x * PC_BLOCK) {
        if (!pc_participates(P, i, n)) continue;
        const double2 p1 = xc1[i], p2 = xc2[i];
        if (out_rows) {
            out_rows[4 * (int64_t)i + 0] = p1.x; out_rows[4 * (int64_t)i + 1] = p1.y;
            out_rows[4 * (int64_t)i + 2] = p2.x; out_rows[4 * (int64_t)i + 3] = p2.y;
        } else {
            P.x1a[i] = p1; P.x2a[i] = p2;
        }
    }
}
