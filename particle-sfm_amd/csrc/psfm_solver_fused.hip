// psfm_solver_fused.hip -- the fused form of the path-consistency solve (see psfm_solver.hip for the solve and its other forms) as
// kernels -- the solve alone, merged with the frame's chain step, paced by the device-side program counter -- and their host code.
#include <stdlib.h>
#include <hip/hip_ext.h>

#include "psfm_pc_fused.h"
#include "psfm_solver_internal.h"

template <int WAVES>
__global__ __launch_bounds__(PC_BLOCK) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES)))
void psfm_pc_fused_kernel(PcParams P)
{
    if (*P.stall) return;
    P.K = P.K < 1 ? 1 : (P.K > PC_KMAX ? PC_KMAX : P.K);      // (the host clamps it too: stated here, the range spares the iteration
                                                             // loop 37 spilled VGPRs at 4 waves per SIMD)
    const int n = P.n_lanes_ptr ? min(*P.n_lanes_ptr, P.n_rows) : P.n_rows;
    const int n_active = (n + PC_BLOCK - 1) / PC_BLOCK;        // blocks with a lane below the high-water mark
    if ((int)blockIdx.x >= n_active) return;
    const int i = blockIdx.x * PC_BLOCK + threadIdx.x;
    // (state loaded alongside the birth frame that decides whether the lane takes part: one round trip less)
    double2 p0 = make_double2(0.0, 0.0), p1 = p0, p2 = p0;
    if (i < n) { p0 = P.p0[i]; p1 = P.x1a[i]; p2 = P.x2a[i]; }
    pc_fused_body(P, pc_participates(P, i, n), p0, p1, p2, n_active, nullptr, nullptr, nullptr, 0, (int)blockIdx.x * PC_BLOCK);
}

// ------------------------------------------------------------------------------------------------
// The merged frame kernel of track_optimize (track_optimize.py:31-50, one loop iteration = ONE launch): the chain step
// of the frame for the block's lanes (births, step, marks, records -- psfm_chain_step_body) and, for the tracks that
// survive it with three buffered points, the whole path-consistency solve (pc_fused_body) -- their tail and next position
// go from the step straight into the solve, the taps of both share a round trip, one launch boundary and one pass over
// the lane state disappear.  Every block below the lane snapshot / the grid takes part in the solve's tickets.
// ------------------------------------------------------------------------------------------------
template <int R>
__global__ __launch_bounds__(PC_BLOCK) __attribute__((amdgpu_waves_per_eu(PSFM_FRAME_WAVES, PSFM_FRAME_WAVES)))
void psfm_frame_kernel(PsfmChainArgs a, PcParams P)
{
    P.K = P.K < 1 ? 1 : (P.K > PC_KMAX ? PC_KMAX : P.K);      // (clamped by the host already: the stated range keeps the loop from spilling)
    PsfmChainOut o;
    if (!psfm_chain_step_body<R, true, true>(a, o)) return;
    // (clamped to the launch's grid: a lane table that ran full leaves a snapshot beyond it -- the host ends such a run at its next
    // checkpoint, PSFM_ERR_CAPACITY; until then no launch may count on blocks that do not exist)
    const int n_active = min((max(a.ctr->n_lanes_snap[a.frame & 1], a.Gband) + PC_BLOCK - 1) / PC_BLOCK, (int)gridDim.x);
    pc_fused_body(P, o.solve, o.p0, o.p1, o.p2, n_active, &a.ctr->n_lanes_snap[(a.frame + 1) & 1], &a.ctr->n_lanes, nullptr, 0, o.tile);
}

template <int R, int WAVES>
__global__ __launch_bounds__(PC_BLOCK) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES)))
void psfm_seq_kernel(PsfmChainArgs a, PcParams P, PsfmSeqStride st, int64_t occ2_stride, int n_flows, int launch_id)
{
    psfm_seq_body<R>(a, P, st, occ2_stride, n_flows, launch_id);
}

// The fused solve's workspace, and where a launch finds it (P.partials / gticket / gpart; P.K clamped): a partial row per block, the
// tickets -- FIRST in their buffer: their place must not depend on the shape, they are zeroed once and every launch leaves them at zero
// -- and the group sums.  The tickets are zeroed when the buffer moved, or whenever the caller says so.
psfm_status pc_fused_workspace(psfm_ctx* c, const PsfmTrackDims& d, PcParams& P, int K, hipStream_t s, bool zero_tickets)
{
    psfm_status rc;
    const int n_blocks = (int)((d.cap + PC_BLOCK - 1) / PC_BLOCK);
    const int n_groups = (n_blocks + PC_GROUP - 1) / PC_GROUP;
    if ((rc = c->sol_partials.ensure(sizeof(double) * (size_t)n_blocks * PC_KMAX * PC_NSUM)) != PSFM_OK) return rc;
    const size_t tbytes = 4096 * sizeof(unsigned), gbytes = sizeof(double) * (size_t)n_groups * PC_KMAX * PC_NSUM;
    if (n_groups + 1 > 4096) { psfm_set_error("psfm_track: lane table too large for the fused solve"); return PSFM_ERR_ARG; }
    void* before = c->sol_fused.p;
    if ((rc = c->sol_fused.ensure(tbytes + gbytes)) != PSFM_OK) return rc;
    if (zero_tickets || c->sol_fused.p != before) PSFM_HIP(hipMemsetAsync(c->sol_fused.p, 0, tbytes, s));
    P.partials = c->sol_partials.as<double>();
    P.gticket = c->sol_fused.as<unsigned>();
    P.gpart = (double*)((char*)c->sol_fused.p + tbytes);
    P.K = K < 1 ? 1 : (K > PC_KMAX ? PC_KMAX : K);
    return PSFM_OK;
}

// the chain steps of track_optimize capture the iterate-buffer pointer: allocate before the first one is enqueued
psfm_status psfm_solve_prepare(psfm_ctx* c, const PsfmTrackDims& d, hipStream_t s)
{
    psfm_status rc;
    if ((rc = pc_workspace(c, d.cap, PC_KMAX)) != PSFM_OK) return rc;
    if ((rc = c->sol_stats.ensure(sizeof(psfm_solve_stats) * (size_t)(d.n_flows + 1))) != PSFM_OK) return rc;
    // The fused solve's tickets, zero at the start of every sequence.  Every launch leaves them at zero -- unless a sequence runs into
    // its lane capacity: its launches then count on more blocks than the grid has, never see their last arrival, and the tickets would
    // stay mid-count for every later sequence of this context (round 5's stress: a capacity retry that made "no progress").
    PcParams P;      // (nothing is launched here: only the buffers -- the partial rows too, which the first launch used to allocate)
    return pc_fused_workspace(c, d, P, 0, s, true);
}

// One frame's solve as ONE launch that speculates K Gauss-Newton iterations (psfm_pc_fused_kernel).  No host
// synchronisation: a solve that does not go as speculated raises the stall flag like a launch chain that ran out of
// iterations.  The accepted iterate stays in an iterate buffer; the next chain step (or psfm_solve_flush) moves it.
psfm_status psfm_solve_frame_fused(psfm_ctx* c, const PsfmTrackDims& d, const float* flow01, const float* flow12,
                                   const float* flow02, const uint8_t* occ02, int frame, int K, hipStream_t s)
{
    PcParams P;
    psfm_status rc = pc_frame_params(c, d, flow01, flow12, flow02, occ02, frame, P, s);
    if (rc != PSFM_OK) return rc;
    const int n_blocks = (int)((d.cap + PC_BLOCK - 1) / PC_BLOCK);
    if ((rc = pc_fused_workspace(c, d, P, K, s)) != PSFM_OK) return rc;
    static const int waves = getenv("PSFM_FUSED_WAVES") ? atoi(getenv("PSFM_FUSED_WAVES")) : 4;   // (round 3: 124 VGPRs, nothing spilled, once the kernel states the range of K)
    hipEvent_t e0 = nullptr, e1 = nullptr;
    c->prof.kernel_span(PSFM_PROF_SOLVER, &e0, &e1, true);   // (profiling on: exact begin / end of every fused launch)
    if (waves == 3) hipExtLaunchKernelGGL(psfm_pc_fused_kernel<3>, dim3(n_blocks), dim3(PC_BLOCK), 0, s, e0, e1, 0, P);
    else hipExtLaunchKernelGGL(psfm_pc_fused_kernel<4>, dim3(n_blocks), dim3(PC_BLOCK), 0, s, e0, e1, 0, P);
    PSFM_HIP(hipGetLastError());
    return PSFM_OK;
}

// track-sharded runs: the fused launch of psfm_solve_export (P.export_sums set: the K x 13 sums of this process, no control step)
psfm_status pc_launch_fused_export(psfm_ctx* c, const PsfmTrackDims& d, PcParams& P, int K, hipStream_t s)
{
    psfm_status rc = pc_fused_workspace(c, d, P, K, s);
    if (rc != PSFM_OK) return rc;
    const int n_blocks = (int)((d.cap + PC_BLOCK - 1) / PC_BLOCK);
    hipLaunchKernelGGL(psfm_pc_fused_kernel<4>, dim3(n_blocks), dim3(PC_BLOCK), 0, s, P);
    PSFM_HIP(hipGetLastError());
    return PSFM_OK;
}

// One loop iteration of track_optimize as ONE launch: chain step of `frame` + the fused solve of its tracks
// (psfm_frame_kernel).  flow12 = the frame's own forward flow, occ = its occlusion map.
psfm_status psfm_launch_frame(psfm_ctx* c, const PsfmTrackDims& d, const float* flow01, const float* flow12, const float* flow02,
                              const uint8_t* occ, const uint8_t* occ02, int frame, int K, hipStream_t s, double* export_sums)
{
    PcParams P;
    psfm_status rc = pc_frame_params(c, d, flow01, flow12, flow02, occ02, frame, P, s);
    if (rc != PSFM_OK) return rc;
    P.export_sums = export_sums;      // track-sharded runs: the K x 13 sums of this process instead of the control step
    const int n_blocks = (int)((d.cap + PC_BLOCK - 1) / PC_BLOCK);
    if ((rc = pc_fused_workspace(c, d, P, K, s)) != PSFM_OK) return rc;
    PsfmChainArgs a;
    psfm_fill_chain_args(c, d, flow12, occ, frame, a, s);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    c->prof.kernel_span(PSFM_PROF_SOLVER, &e0, &e1, true);
    const dim3 grid((unsigned)n_blocks), block(PC_BLOCK);
#define PSFM_FRAME_LAUNCH(R_) hipExtLaunchKernelGGL(psfm_frame_kernel<R_>, grid, block, 0, s, e0, e1, 0, a, P)
    PSFM_RATIO_DISPATCH(d.ratio, PSFM_FRAME_LAUNCH)
#undef PSFM_FRAME_LAUNCH
    PSFM_HIP(hipGetLastError());
    return PSFM_OK;
}

// The arguments every launch of a device-paced sequence carries: those of frame 1 + the strides of the per-frame stacks
// (psfm_seq_kernel gets them as kernel arguments, psfm_seq_batch_kernel from its sequence's row of the batch table).
psfm_status pc_seq_args(psfm_ctx* c, const PsfmTrackDims& d, const float* flows, const uint8_t* occ, int64_t occ_pitch,
                        const float* flows_f2, const uint8_t* occ_s2, PcParams& P, PsfmChainArgs& a, PsfmSeqStride& st, hipStream_t s)
{
    const int64_t Pix = (int64_t)d.H * d.W;
    psfm_status rc = pc_frame_params(c, d, flows, flows + Pix * 2, flows_f2, occ_s2, 1, P, s);
    if (rc != PSFM_OK) return rc;
    if ((rc = pc_fused_workspace(c, d, P, 0, s)) != PSFM_OK) return rc;      // (K: every launch takes it from PsfmCounters::solve_K)
    psfm_fill_chain_args_nolaunch(c, d, flows + Pix * 2, occ + occ_pitch, 1, a);
    a.owner_clear = 1;
    st.flow = Pix; st.occ = occ_pitch; st.cap = d.cap;          // (float2 / byte / double2 elements per frame)
    return PSFM_OK;
}

// Device-paced sequence: `n_launches` launches of psfm_seq_kernel (ids launch_id0 ..), every one with the arguments of
// frame 1 and the strides; what each of them does is decided on the device (PsfmCounters::pc_*).
psfm_status psfm_launch_seq(psfm_ctx* c, const PsfmTrackDims& d, const float* flows, const uint8_t* occ, int64_t occ_pitch,
                            const float* flows_f2, const uint8_t* occ_s2, int n_launches, int launch_id0, hipStream_t s)
{
    const int64_t Pix = (int64_t)d.H * d.W;
    PcParams P;
    PsfmChainArgs a;
    PsfmSeqStride st;
    psfm_status rc = pc_seq_args(c, d, flows, occ, occ_pitch, flows_f2, occ_s2, P, a, st, s);
    if (rc != PSFM_OK) return rc;
    const int n_blocks = (int)((d.cap + PC_BLOCK - 1) / PC_BLOCK);
    if (getenv("PSFM_SEQ_CHECK")) {     // the device-side rebase against the host's own per-frame arguments
        const int fs[] = {2, 3, 17, 254, 255, 256, 509, 510};
        for (int f : fs) {
            if (f >= d.n_flows) continue;
            PsfmChainArgs r = a, h;
            psfm_chain_args_rebase(r, st, f);
            // (no stream: the host version may launch the stamp-wrap clear, which the device-paced form does in-kernel)
            psfm_fill_chain_args_nolaunch(c, d, flows + (size_t)f * Pix * 2, occ + (size_t)f * occ_pitch, f, h);
            PcParams rp = P, hp;
            pc_params_rebase(rp, st, Pix, f);
            if ((rc = pc_frame_params(c, d, flows + (size_t)(f - 1) * Pix * 2, flows + (size_t)f * Pix * 2, flows_f2 + (size_t)(f - 1) * Pix * 2,
                                      occ_s2 + (size_t)(f - 1) * Pix, f, hp, s)) != PSFM_OK) return rc;
            const bool ok = r.flow == h.flow && r.occ == h.occ && r.log_cur == h.log_cur && r.log_next == h.log_next && r.log_prev == h.log_prev &&
                            r.blocked_cur == h.blocked_cur && r.blocked_prev == h.blocked_prev && r.stamp_cur == h.stamp_cur &&
                            r.stamp_prev == h.stamp_prev && r.surv_cur == h.surv_cur && r.surv_prev == h.surv_prev && r.sh_pop == h.sh_pop &&
                            r.sh_push == h.sh_push && r.free_pop == h.free_pop && r.free_push == h.free_push && r.frame == h.frame &&
                            rp.p0 == hp.p0 && rp.x1a == hp.x1a && rp.x2a == hp.x2a && rp.flow01 == hp.flow01 && rp.flow12 == hp.flow12 &&
                            rp.flow02 == hp.flow02 && rp.occ02 == hp.occ02 && rp.frame == hp.frame && rp.max_birth == hp.max_birth;
            if (!ok) { psfm_set_error("psfm_seq: rebased arguments of frame %d differ from the host's", f); return PSFM_ERR_ARG; }
        }
    }
    const dim3 grid((unsigned)n_blocks), block(PC_BLOCK);
    // waves per SIMD of the frame kernel: 3 (<= 168 VGPRs; leaves the register file room for the background flow_check's
    // block beside it) or 4 (<= 128 VGPRs: the solver core fits since round 3); PSFM_SEQ_WAVES overrides for measurements
    static const int seq_waves = getenv("PSFM_SEQ_WAVES") ? atoi(getenv("PSFM_SEQ_WAVES")) : PSFM_SEQ_WAVES_DEFAULT;
    for (int k = 0; k < n_launches; ++k) {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        c->prof.kernel_span(PSFM_PROF_SOLVER, &e0, &e1, true);
        const int id = launch_id0 + k;
#define PSFM_SEQ_LAUNCH4(R_) hipExtLaunchKernelGGL((psfm_seq_kernel<R_, 4>), grid, block, 0, s, e0, e1, 0, a, P, st, Pix, d.n_flows, id)
#define PSFM_SEQ_LAUNCH3(R_) hipExtLaunchKernelGGL((psfm_seq_kernel<R_, 3>), grid, block, 0, s, e0, e1, 0, a, P, st, Pix, d.n_flows, id)
        if (seq_waves == 4) { PSFM_RATIO_DISPATCH(d.ratio, PSFM_SEQ_LAUNCH4) }
        else { PSFM_RATIO_DISPATCH(d.ratio, PSFM_SEQ_LAUNCH3) }
#undef PSFM_SEQ_LAUNCH4
#undef PSFM_SEQ_LAUNCH3
    }
    PSFM_HIP(hipGetLastError());
    return PSFM_OK;
}
