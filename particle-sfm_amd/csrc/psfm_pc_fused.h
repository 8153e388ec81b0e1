// psfm_pc_fused.h -- the fused solve as device functions: what psfm_pc_fused_kernel, psfm_frame_kernel and psfm_seq_kernel
// (psfm_solver_fused.hip) and psfm_seq_batch_kernel (psfm_solver_batch.hip) run, and the replay of its control flow that
// psfm_pc_control_kernel (psfm_solver.hip) repeats on the totals of a track-sharded run.  Force-inlined; no kernels.
#pragma once
#include "psfm_pc_params.h"

// ------------------------------------------------------------------------------------------------
// pc_fused: the WHOLE solve of a frame in one launch, speculating that every trust-region iteration takes the pure
// Gauss-Newton step at mu = min_mu and is accepted -- which is what Ceres does on every solve that converges without a
// rejection.  Under that assumption nothing a track computes depends on the global scalars: thread = track runs K
// iterations in registers (the residuals / Jacobian evaluated at a candidate for its cost ARE the next iteration's
// evaluation at x: K + 1 interpolations instead of 2 K), stores the iterate after m accepted steps in buffer m, and
// every iteration's 13 sums are reduced block -> group of PC_GROUP blocks -> grid (two tickets, fixed order).  The last
// block replays Ceres' control flow over iterations 1..K with those sums, exactly as the launch chain would have
// (pc_control_step), and stops believing the speculation at the first decision that is not "Gauss-Newton step
// accepted": termination -> done, the accepted iterate is buffer `cur` (PsfmCounters::sel tells the next chain step, which
// copies it into the log on its way); anything else (rejection, dogleg interpolation, invalid step, more than K
// iterations) raises the stall flag and the host redoes this solve with the launch chain from the untouched buffer 0.
// ------------------------------------------------------------------------------------------------
// Where iterate m (the position after m accepted steps) of a fused solve lives.  A solve that goes as speculated accepts
// e = k_first - 1 steps and terminates in iteration k_first, so iterate e is written straight into buffer 0 -- the log
// slabs, where the next chain step and finalize read -- and the values the solve started from are kept in buffer e
// instead; every other iterate m sits in buffer m.
__device__ __forceinline__ int pc_phys(int m, int e) { return m == e ? 0 : (m == 0 ? e : m); }

// Ceres' control flow replayed over the sums of `n_it` speculated iterations (thread 0 of the last block, or the control
// kernel of a track-sharded run): tot[j * PC_NSUM + k].  first: the launch that started the solve (iteration 1 ..), else
// a continuation behind `C.cur` accepted steps.  pc != NULL (device-paced sequence): the outcome also says what the NEXT
// launch does -- the next frame, or more iterations of this solve when every one so far was accepted and none terminated.
// The replay proper, on a control block C in memory of the function's choice (a macro: the two functions below differ in where C lives
// and in nothing else, and the first must compile to what it always did).  Where a decision is not what was speculated, the launch chain
// redoes the solve from the values it started from, which psfm_solve_frame_resume first moves back into buffer 0; a failed solve hands
// the parameters back as they came in -- iterate 0 -- whatever it had accepted on the way (see the write-back).
#define PC_FUSED_REPLAY_BODY \
    const int base = first ? 0 : C.cur; \
    const int k_first = first ? n_it : C.k_first; \
    for (int j = 1; j <= n_it; ++j) { \
        pc_control_step(C, tot + (j - 1) * PC_NSUM, first && j == 1, base + j); \
        if (C.done) break; \
        if (!(C.fresh_x && C.cur == base + j && C.dl_fixed == 0 && C.mu == 1e-8)) break; \
    } \
    C.k_first = k_first; \
    C.launches += 1; \
    *P.ctrl = C; \
    const int e = k_first - 1; \
    if (!C.done) { \
        const bool all_accepted = C.fresh_x && C.cur == base + n_it && C.dl_fixed == 0 && C.mu == 1e-8; \
        if (pc && all_accepted && C.cur + 1 <= PC_KMAX) { \
            pc->pc_phase = 1; \
            pc->pc_owner = launch_id + 1; \
            return; \
        } \
        *P.sel = pc_phys(0, e); \
        *P.stall = P.frame + 1; \
        return; \
    } \
    *P.sel = pc_phys(C.failed ? 0 : C.cur, e); \
    if (P.stats_dev) { \
        psfm_solve_stats st; \
        st.iterations = C.iteration; st.successful_steps = C.successful; \
        st.termination = C.n_tracks == 0 ? -1 : C.termination; st.dogleg_nonGN = C.nonGN; \
        st.initial_cost = C.initial_cost; st.final_cost = C.x_cost; \
        if (C.failed) st.termination = PSFM_TERM_FAILURE; \
        P.stats_dev[P.frame] = st; \
    } \
    if (pc) { pc->pc_frame = P.frame + 1; pc->pc_phase = 0; pc->pc_owner = launch_id + 1; }
__device__ __forceinline__ void pc_fused_replay(const PcParams& P, const double* tot, int n_it, bool first, PsfmCounters* pc,
                                                int launch_id, const PsfmSolveCtrl* c_in = nullptr)
{
    PsfmSolveCtrl C = c_in ? *c_in : *P.ctrl;      // (c_in: the caller's copy of the control block, loaded with everything else it needs)
    PC_FUSED_REPLAY_BODY
}

// The same with ONE copy of the control block per block in LDS (232 bytes; thread 0 of the last block only).  The local copy above is
// kept by the compiler as a per-thread array -- 2 KB of LDS per field, and what no longer fits the LDS of four blocks per CU in scratch --
// which the batched sequence with the motion-boundary verdict (psfm_solver_batch_mb.hip) does without.
__device__ __forceinline__ void pc_fused_replay_lds(const PcParams& P, const double* tot, int n_it, bool first, PsfmCounters* pc, int launch_id)
{
    __shared__ PsfmSolveCtrl s_ctrl;
    PsfmSolveCtrl& C = s_ctrl;
    C = *P.ctrl;
    PC_FUSED_REPLAY_BODY
}

struct PcTrack {            // one track's solve state in registers
    double x[4], r[6], jac[4];
    double2 r1, r2;
    PcConst c;
    double iA22;            // 1 / (H22 (1 + mu)) at the mu the fused solve speculates
};

// (Round 4 tried a tap NEIGHBOURHOOD per track in LDS -- 3 rows x 4 columns of F12 around the start position, brought in by six
// global_load_lds_dwordx4 per lane at the setup, so that the K evaluations behind it take their taps from LDS instead of a dependent
// gather each: bit-identical, and 2 % SLOWER (frame kernel 66.7 vs 65.4 us at 1080p).  The taps of an iterate lie in the cache
// lines its predecessor touched: those gathers are L1 hits, not round trips to L2 / HBM.  profiles/EXPERIMENTS.md 6.5.)
// residuals and Jacobian of T at T.x
__device__ __forceinline__ void pc_track_eval(const PcParams& P, PcTrack& T)
{
    const PcTaps t = pc_core_taps<PC_FUSED_PAIR>((const PcF2*)P.flow12, P.H, P.W, T.x);
    pc_core_eval_taps(t, T.x, T.r1.x, T.r1.y, T.r2.x, T.r2.y, T.c.s, T.r, T.jac);
}

// sums of one trust-region iteration at T.x (already evaluated: T.r, T.jac) into v[]; the candidate goes to (xn1, xn2)[i]
// and becomes T.x, evaluated.  The same function as the launch chain's iteration, with (a, b) = (0, 1) at compile time.
__device__ __forceinline__ void pc_fused_iteration(const PcParams& P, PcTrack& T, double mu, double2* xn1, double2* xn2, int i,
                                                   double v[PC_NSUM])
{
    double xp[4];
    pc_core_iteration<true>(T.x, T.r, T.jac, T.c, mu, T.iA22, 0.0, 1.0, v, xp);
    if (xn1) {
        xn1[i] = make_double2(xp[0], xp[1]);
        xn2[i] = make_double2(xp[2], xp[3]);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) T.x[k] = xp[k];
    pc_track_eval(P, T);
    v[SUM_COST] += pc_core_cost(T.r);
}

// Sums of one iteration over the 64 tracks of a WAVE, without a block barrier (the four waves of a block stay independent
// inside the iteration loop).  Round 4: the transposed exchange tree of psfm_pc_reduce.h inside each 16-lane row (registers, DPP),
// the four row totals of a slot through 450 bytes of LDS per wave, added in row order by lane k < 13.  Fixed order.  (Rounds 2-3
// parked every lane's 13 values in LDS -- 27 KB per block, the space the tap neighbourhoods below need; PC_WAVE_PARK keeps
// that form for A/B builds.)  LDS operations of one wave execute in order, so the wave only has to wait for its own stores.
#define PC_NW (PC_BLOCK / PSFM_WAVE)
#ifndef PC_WAVE_PARK
struct PcWaveRed {
    double row[PC_NW][4][PC_NSUM + 1];
    double wsum[PC_NW][PC_KMAX][PC_NSUM];
};
__device__ __forceinline__ void pc_wave_reduce(PcWaveRed& R, const double v[PC_NSUM], int iter)
{
    const int lane = threadIdx.x & (PSFM_WAVE - 1), w = threadIdx.x / PSFM_WAVE;
    int slot;
    const double g = pc_row_tree<PC_NSUM>(v, slot);
    R.row[w][lane >> 4][slot] = g;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (lane < PC_NSUM) {
        const double q0 = R.row[w][0][lane], q1 = R.row[w][1][lane], q2 = R.row[w][2][lane], q3 = R.row[w][3][lane];
        R.wsum[w][iter][lane] = (lane == SUM_GMAX) ? fmax(fmax(fmax(q0, q1), q2), q3) : ((q0 + q1) + q2) + q3;
    }
    // (the next iteration's row stores come behind these loads in the wave's LDS queue)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
#else
#define PC_WROW 66          // row pitch in doubles: 2-way instead of 13-way bank conflicts in the quarter sums
struct PcWaveRed {
    double park[PC_NW][PC_NSUM][PC_WROW];
    double quarter[PC_NW][PC_NSUM][4];
    double wsum[PC_NW][PC_KMAX][PC_NSUM];
};
__device__ __forceinline__ void pc_wave_reduce(PcWaveRed& R, const double v[PC_NSUM], int iter)
{
    const int lane = threadIdx.x & (PSFM_WAVE - 1), w = threadIdx.x / PSFM_WAVE;
#pragma unroll
    for (int k = 0; k < PC_NSUM; ++k) R.park[w][k][lane] = v[k];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // (the max slot on its own branch: one select per addition otherwise -- 4 instructions per step instead of 1)
    const int k = lane >> 2, q = lane & 3;
    if (k < PC_NSUM && k != SUM_GMAX) {
        double t = R.park[w][k][q];
#pragma unroll
        for (int j = 1; j < 16; ++j) t += R.park[w][k][4 * j + q];
        R.quarter[w][k][q] = t;
    } else if (k == SUM_GMAX) {
        double t = R.park[w][SUM_GMAX][q];
#pragma unroll
        for (int j = 1; j < 16; ++j) t = fmax(t, R.park[w][SUM_GMAX][4 * j + q]);
        R.quarter[w][SUM_GMAX][q] = t;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (lane < PC_NSUM) {
        const double q0 = R.quarter[w][lane][0], q1 = R.quarter[w][lane][1], q2 = R.quarter[w][lane][2], q3 = R.quarter[w][lane][3];
        R.wsum[w][iter][lane] = (lane == SUM_GMAX) ? fmax(fmax(fmax(q0, q1), q2), q3) : ((q0 + q1) + q2) + q3;
    }
    // (the next iteration's park stores come behind these loads in the wave's LDS queue)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
#endif

// drain this block's write-through stores, then take a ticket: true for the last of `members` arrivals (which also
// resets the counter for the next launch)
__device__ __forceinline__ bool pc_last_arrival(unsigned* ticket, unsigned members)
{
    __shared__ int s_last2;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last2 = (t == members - 1u);
        if (s_last2) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    return s_last2 != 0;
}

// (one LDS instance for every body that reduces per wave: a kernel that contains two of them must not pay for two)
__device__ __forceinline__ PcWaveRed& pc_shared_red()
{
    __shared__ PcWaveRed s_red_storage;
    return s_red_storage;
}

// refs / scale (trajectory.py:173-183, as in psfm_pc_init_kernel) and the Jacobi scaling of a track: from its p0 and
// the values x0 its solve starts from.  Leaves T.x = x0 evaluated (T.r, T.jac); returns the cost at x0.
__device__ __forceinline__ double pc_track_setup(const PcParams& P, PcTrack& T, double2 p0, double2 p1, double2 p2, double mu)
{
    const PsfmTaps t = psfm_taps((float)p0.x, (float)p0.y, P.cw, P.ch, P.H, P.W);
    const PsfmTapIdx k = psfm_tap_idx(P.H, P.W, t);
    const float2 f01 = psfm_sample_flow(P.flow01, k, t);
    const float2 f02 = psfm_sample_flow(P.flow02, k, t);
    const float o02 = psfm_sample_mask(P.occ02, k, t);
    const float nrm = sqrtf(__fadd_rn(__fmul_rn(f02.x, f02.x), __fmul_rn(f02.y, f02.y)));
    const float sf = __fmul_rn(__fsub_rn(1.0f, o02), nrm < 20.0f ? 1.0f : 0.0f);
    T.r1 = make_double2(p0.x + (double)f01.x, p0.y + (double)f01.y);
    T.r2 = make_double2(p0.x + (double)f02.x, p0.y + (double)f02.y);
    T.x[0] = p1.x; T.x[1] = p1.y; T.x[2] = p2.x; T.x[3] = p2.y;
    T.c.s = (double)sf;
    pc_track_eval(P, T);
    // Jacobi scaling from the Jacobian at x0 (what psfm_pc_init_kernel stores in P.jscale)
    T.c = pc_core_const((double)sf, T.jac);
    T.iA22 = pc_core_iA22(T.c, mu);
    return pc_core_cost(T.r);
}

// The block's sums of n_it iterations (the waves' sums, in wave order) -> its partial row; then the two tickets: the
// last block of each group of PC_GROUP consecutive blocks adds the group's rows, the last group adds the group sums in
// group order.  Returns the totals ([n_it][PC_NSUM], in LDS) in the LAST block of the launch, NULL in every other block.
// n_active: the blocks of the launch that come here.
__device__ __forceinline__ const double* pc_grid_totals(const PcParams& P, PcWaveRed& s_red, int n_it, int n_active)
{
    const int tid = threadIdx.x;
    __syncthreads();
    if (tid < n_it * PC_NSUM) {   // the block's sums: its waves in order
        const int j = tid / PC_NSUM, k = tid - j * PC_NSUM;
        double t = s_red.wsum[0][j][k];
#pragma unroll
        for (int w = 1; w < PC_NW; ++w) t = (k == SUM_GMAX) ? fmax(t, s_red.wsum[w][j][k]) : t + s_red.wsum[w][j][k];
        __hip_atomic_store(&P.partials[((int64_t)blockIdx.x * PC_KMAX + j) * PC_NSUM + k], t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    // ---- level 1 ----
    const int n_groups = (n_active + PC_GROUP - 1) / PC_GROUP;
    const int grp = blockIdx.x / PC_GROUP;
    const int members = min(PC_GROUP, n_active - grp * PC_GROUP);
    if (!pc_last_arrival(P.gticket + 1 + grp, (unsigned)members)) return nullptr;
    __shared__ double s_half[2][PC_KMAX * PC_NSUM];
    __shared__ double s_tot[PC_KMAX][PC_NSUM];
    const int slot = tid & 127, half = tid >> 7;      // slot = j * PC_NSUM + k
    const int nslot = n_it * PC_NSUM;
    {
        double t = 0.0;
        if (slot < nslot) {
            const int j = slot / PC_NSUM, k = slot - j * PC_NSUM;
            double pv[PC_GROUP / 2];
#pragma unroll
            for (int u = 0; u < PC_GROUP / 2; ++u) {
                const int b = half * (PC_GROUP / 2) + u;
                pv[u] = b < members ? __hip_atomic_load(&P.partials[((int64_t)(grp * PC_GROUP + b) * PC_KMAX + j) * PC_NSUM + k],
                                                        __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)
                                    : 0.0;
            }
#pragma unroll
            for (int u = 0; u < PC_GROUP / 2; ++u) t = (k == SUM_GMAX) ? fmax(t, pv[u]) : t + pv[u];
            s_half[half][slot] = t;
        }
        __syncthreads();
        if (tid < nslot) {
            const int j = tid / PC_NSUM, k = tid - j * PC_NSUM;
            const double a = s_half[0][tid], b = s_half[1][tid];
            __hip_atomic_store(&P.gpart[((int64_t)grp * PC_KMAX + j) * PC_NSUM + k], (k == SUM_GMAX) ? fmax(a, b) : a + b,
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    // ---- level 2 ----
    if (!pc_last_arrival(P.gticket, (unsigned)n_groups)) return nullptr;
    {
        double t = 0.0;
        if (slot < nslot) {
            const int j = slot / PC_NSUM, k = slot - j * PC_NSUM;
            for (int g0 = half * 16; g0 < n_groups; g0 += 32) {
                double pv[16];
#pragma unroll
                for (int u = 0; u < 16; ++u)
                    pv[u] = g0 + u < n_groups ? __hip_atomic_load(&P.gpart[((int64_t)(g0 + u) * PC_KMAX + j) * PC_NSUM + k],
                                                                  __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)
                                              : 0.0;
#pragma unroll
                for (int u = 0; u < 16; ++u) t = (k == SUM_GMAX) ? fmax(t, pv[u]) : t + pv[u];
            }
            s_half[half][slot] = t;
        }
        __syncthreads();
        if (tid < nslot) {
            const int j = tid / PC_NSUM, k = tid - j * PC_NSUM;
            const double a = s_half[0][tid], b = s_half[1][tid];
            s_tot[j][k] = (k == SUM_GMAX) ? fmax(a, b) : a + b;
        }
        __syncthreads();
    }
    return &s_tot[0][0];
}

// The solve of lane i = blockIdx.x * PC_BLOCK + threadIdx.x (if `part`) from its three buffered positions, the sums of
// the launch and -- in its last block -- the control flow.  n_active: the blocks of the launch that come here (every one
// of them, whatever its lanes do: the tickets count them).  snap_next / n_lanes_live: the merged frame kernel leaves the
// lane count for the next frame's launch.  pc / launch_id: device-paced sequence (see pc_fused_replay); there the K-th
// candidate is stored too (a continuation launch starts from it).
template <bool CTRL_LDS = false>      // (true: pc_fused_replay_lds)
__device__ __forceinline__ void pc_fused_body(const PcParams& P, bool part, double2 p0, double2 p1, double2 p2, int n_active,
                                              int* snap_next, const int* n_lanes_live, PsfmCounters* pc, int launch_id, int lane0)
{
    const int K = P.K;
    const int tid = threadIdx.x;
    const int i = lane0 + tid;          // (lane0: first lane of the block's tile -- XCD-banded in the merged kernels, psfm_xcd_tile)
    const double mu = 1e-8;
    const int e = K - 1;            // (pc_phys: iterate e goes straight into the log slabs, the start values into buffer e)
    PcWaveRed& s_red = pc_shared_red();
    PcTrack T;
    double c0 = 0.0;
    if (part) {
        if (e != 0) { pc_buf1(P, e)[i] = p1; pc_buf2(P, e)[i] = p2; }
        c0 = pc_track_setup(P, T, p0, p1, p2, mu);
    }
    for (int j = 0; j < K; ++j) {
        double v[PC_NSUM];
#pragma unroll
        for (int q = 0; q < PC_NSUM; ++q) v[q] = 0.0;
        if (part) {
            // (host-paced: the K-th candidate is never read -- were it accepted, the solve would not be over and is redone)
            const bool keep = j + 1 < K || (pc != nullptr && K < PC_KMAX);
            const int m = pc_phys(j + 1, e);
            pc_fused_iteration(P, T, mu, keep ? pc_buf1(P, m) : nullptr, keep ? pc_buf2(P, m) : nullptr, i, v);
            if (j == 0) { v[SUM_CNT] = 1.0; v[SUM_COST0] = c0; }
        }
        pc_wave_reduce(s_red, v, j);
    }
    const double* tot = pc_grid_totals(P, s_red, K, n_active);
    if (!tot) return;
    if (P.export_sums) {      // track-sharded: the totals of THIS process; the control step follows the ranks' exchange
        if (tid < K * PC_NSUM) P.export_sums[tid] = tot[tid];
        if (tid == 0 && snap_next) *snap_next = *n_lanes_live;   // (merged frame launch: every block is past its chain step)
        return;
    }
    if (tid != 0) return;
    if (snap_next) *snap_next = *n_lanes_live;   // (every block is past its chain step: the count is final for this launch)
    if constexpr (CTRL_LDS) pc_fused_replay_lds(P, tot, K, true, pc, launch_id);
    else pc_fused_replay(P, tot, K, true, pc, launch_id);
}

// Device-paced sequence: MORE iterations of the solve of P.frame, behind a launch whose K iterations were all accepted
// without terminating it.  The track state is rebuilt from p0 and the start values (kept in buffer k_first - 1), the
// iterate is read from where the previous launch left it, up to two more iterations are speculated the same way.
template <bool CTRL_LDS = false>
__device__ __forceinline__ void pc_more_body(const PcParams& P, int n_active, PsfmCounters* pc, int launch_id)
{
    const PsfmSolveCtrl C0 = *P.ctrl;
    const int e = C0.k_first - 1, base = C0.cur;
    const int n_it = min(2, PC_KMAX - base);
    const int n = min(*P.n_lanes_ptr, P.n_rows);
    const int tid = threadIdx.x;
    const int i = blockIdx.x * PC_BLOCK + tid;
    const double mu = 1e-8;
    PcWaveRed& s_red = pc_shared_red();
    const bool part = pc_participates(P, i, n);
    PcTrack T;
    if (part) {
        const double2 p0 = P.p0[i];
        const double2 s1 = pc_buf1(P, pc_phys(0, e))[i], s2 = pc_buf2(P, pc_phys(0, e))[i];      // the start values
        (void)pc_track_setup(P, T, p0, s1, s2, mu);
        const double2 c1 = pc_buf1(P, pc_phys(base, e))[i], c2 = pc_buf2(P, pc_phys(base, e))[i];  // the current iterate
        T.x[0] = c1.x; T.x[1] = c1.y; T.x[2] = c2.x; T.x[3] = c2.y;
        pc_track_eval(P, T);
    }
    for (int j = 0; j < n_it; ++j) {
        double v[PC_NSUM];
#pragma unroll
        for (int q = 0; q < PC_NSUM; ++q) v[q] = 0.0;
        if (part) {
            const int m = pc_phys(base + j + 1, e);
            const bool keep = base + j + 1 <= PC_KMAX;
            pc_fused_iteration(P, T, mu, keep ? pc_buf1(P, m) : nullptr, keep ? pc_buf2(P, m) : nullptr, i, v);
        }
        pc_wave_reduce(s_red, v, j);
    }
    const double* tot = pc_grid_totals(P, s_red, n_it, n_active);
    if (!tot || tid != 0) return;
    if constexpr (CTRL_LDS) pc_fused_replay_lds(P, tot, n_it, false, pc, launch_id);
    else pc_fused_replay(P, tot, n_it, false, pc, launch_id);
}

// ------------------------------------------------------------------------------------------------
// The device-paced sequence of track_optimize: every launch is the same kernel with the same arguments (those of frame
// 1 + the strides of the per-frame stacks) and does "the next thing" the device-side program counter names --
//   phase 0  the frame kernel of pc_frame (chain step + fused solve with solve_K iterations), or
//   phase 1  more iterations of that frame's solve, when all of them were accepted and none terminated it
// -- and its control thread moves the counter on.  The host only keeps launches in the queue and looks at the counter
// at its checkpoints: a solve that needs one iteration more than the sequence's usual costs one more launch instead of
// a drained queue, a host-side redo and the no-op launches behind a stall flag.  (Solves that reject a step or leave the
// Gauss-Newton path still raise the stall flag and are redone by the launch chain.)
// launch_id: a block that is dispatched after the control thread has moved the counter on (only blocks beyond the lane
// snapshot can be) sees pc_owner != launch_id and leaves.
// ------------------------------------------------------------------------------------------------
// what one block of a device-paced launch does for ITS sequence (psfm_seq_kernel: the launch's only sequence; psfm_seq_batch_kernel:
// sequence blockIdx.y of the batch).  MB: `a.occ` walks the sequence's kill maps and the chain step forms the motion-boundary verdict
// (psfm_solver_batch_mb.hip); the solve reads the stride-2 occlusion maps only, which stay 0/1.
template <int R, bool MB = false>
__device__ __forceinline__ void psfm_seq_body(PsfmChainArgs a, PcParams P, const PsfmSeqStride st, int64_t occ2_stride, int n_flows, int launch_id)
{
    PsfmCounters* ctr = a.ctr;
    if (ctr->stall || ctr->pc_owner != launch_id) return;
    // (MB: the program counter is the same in every lane, and the form with the second verdict says so -- the frame's rebased pointers
    // are then scalars, which is what keeps this form out of scratch at four waves per SIMD)
    const int f = MB ? __builtin_amdgcn_readfirstlane(ctr->pc_frame) : ctr->pc_frame;
    const int phase = MB ? __builtin_amdgcn_readfirstlane(ctr->pc_phase) : ctr->pc_phase;
    if (f >= n_flows) return;
    psfm_chain_args_rebase(a, st, f);
    pc_params_rebase(P, st, occ2_stride, f);
    const int k = MB ? __builtin_amdgcn_readfirstlane(ctr->solve_K) : ctr->solve_K;
    P.K = k < 1 ? 1 : (k > PC_KMAX ? PC_KMAX : k);
    // the blocks that take part in the solve's tickets (as in psfm_frame_kernel).  MB: read where it is used, behind the chain step --
    // this launch writes the snapshot of the OTHER parity only -- so that it is not one more value alive across the step
#define PSFM_SEQ_N_ACTIVE() min((max(ctr->n_lanes_snap[f & 1], a.Gband) + PC_BLOCK - 1) / PC_BLOCK, (int)gridDim.x)
    if (MB) {
        if (phase == 0) {
            PsfmChainOut o;
            if (!psfm_chain_step_body<R, true, true, true>(a, o)) return;
            const int n_active = __builtin_amdgcn_readfirstlane(PSFM_SEQ_N_ACTIVE());      // (the same in every lane: a scalar)
            pc_fused_body<true>(P, o.solve, o.p0, o.p1, o.p2, n_active, &ctr->n_lanes_snap[(f + 1) & 1], &ctr->n_lanes, ctr, launch_id, o.tile);
        } else {
            const int n_active = __builtin_amdgcn_readfirstlane(PSFM_SEQ_N_ACTIVE());      // (the same in every lane: a scalar)
            if ((int)blockIdx.x >= n_active) return;
            pc_more_body<true>(P, n_active, ctr, launch_id);
        }
        return;
    }
    const int n_active = PSFM_SEQ_N_ACTIVE();
#undef PSFM_SEQ_N_ACTIVE
    if (phase == 0) {
        PsfmChainOut o;
        if (!psfm_chain_step_body<R, true, true, false>(a, o)) return;
        pc_fused_body(P, o.solve, o.p0, o.p1, o.p2, n_active, &ctr->n_lanes_snap[(f + 1) & 1], &ctr->n_lanes, ctr, launch_id, o.tile);
    } else {
        if ((int)blockIdx.x >= n_active) return;
        pc_more_body(P, n_active, ctr, launch_id);
    }
}
