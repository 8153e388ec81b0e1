// psfm_solver_internal.h -- host-side declarations the units of the path-consistency solver share.  A kernel is launched only by the
// unit that defines it; the other units call its launcher.  (What other drivers call: psfm_internal.h.)
#pragma once
#include "psfm_pc_params.h"

// ---- psfm_solver.hip: the launch chain, the resident solve, the host driver of a solve ----
psfm_status pc_workspace(psfm_ctx* c, int64_t rows, int n_buf);
psfm_status pc_frame_params(psfm_ctx* c, const PsfmTrackDims& d, const float* flow01, const float* flow12,
                            const float* flow02, const uint8_t* occ02, int frame, PcParams& P, hipStream_t s);

// A batch-mode problem (rows given, no frame recurrence) of up to `cap` rows in c's OWN solver workspace, as psfm_solve_batch sets one
// up -- pc_workspace(c, cap, 2) + pc_setup: iterate buffers, refs / jscale / scale, ctrl, ticket, partials, the lists sized for every
// row count up to cap -- with buffer 0 (x1a, x2a) in c->sol_misc.  *limit: the blocks a launch of this context's chain may use (pc_blocks).
psfm_status pc_multi_problem(psfm_ctx* c, int64_t cap, int h, int w, PcParams& P, int* limit, hipStream_t s);

// ---- psfm_solver_multi.hip: the launch chain over a table of problems (index rules: psfm_solver_multi.h) ----
// One problem of the table.  P.n_lanes_ptr: the address of the problem's row count for the current step; P.n_rows: the rows its
// buffers hold; P.flow12: map 0 of the stack the solves sample (the kernels add pc_multi_map(k) * flow_stride).
struct PcMultiRow {
    PcParams P;
    int64_t flow_stride;      // float2 elements between two maps of the stack
    int n_flows;              // steps of the problem's sequence: it takes part in steps 1 .. n_flows - 1
    int back;                 // the direction's map rule (pc_multi_map)
    int limit;                // blocks a launch may use for this problem
    int pad;
};
// what the poll leaves in pinned memory per problem
struct PcMultiPoll { PsfmSolveCtrl C; int n_rows; int pad; };
void pc_multi_launch_init(const PcMultiRow* tab, int grid_x, int n_problems, int k, hipStream_t s);
void pc_multi_launch_iter(const PcMultiRow* tab, int grid_x, int n_problems, int k, int n_launches, hipStream_t s);
void pc_multi_launch_writeback(const PcMultiRow* tab, int grid_x, int n_problems, int k, hipStream_t s);
void pc_multi_launch_poll(const PcMultiRow* tab, int n_problems, int k, PcMultiPoll* out_pinned, hipStream_t s);
// the statistics of a finished solve from its control block, as psfm_solve_batch reports them
void pc_multi_stats(const PsfmSolveCtrl* C, psfm_solve_stats* st);

// pc_finish_sync's pacing of a solve, over a table of problems: four iteration launches, one poll into pinned memory and ONE
// synchronisation; while any problem is left undone another chunk of iteration launches (6, doubling to 32) and another poll; at
// most 2 * 200 + 64 iterations past the first poll.  iter(n): enqueue n iteration launches; poll(): enqueue the poll; undone(): read
// what the poll left.  The one statement of the policy for both batch callers (psfm_query_pc_batch.hip, psfm_batch.hip), each with
// its own census counters.
struct PcPaceCensus { int32_t* fixed; int32_t* iter; int32_t* syncs; };
template <class Iter, class Poll, class Undone>
static inline psfm_status pc_multi_pace(Iter&& iter, Poll&& poll, Undone&& undone, const PcPaceCensus& n, hipStream_t s, const char* who)
{
    iter(4);
    *n.iter += 4;
    PSFM_HIP(hipGetLastError());
    int launched = 0, chunk = 6;
    for (;;) {
        poll();
        *n.fixed += 1;
        PSFM_HIP(hipGetLastError());
        PSFM_HIP(hipStreamSynchronize(s));
        *n.syncs += 1;
        if (!undone()) break;
        if (launched > 2 * 200 + 64) { psfm_set_error("%s: path-consistency solver did not terminate", who); return PSFM_ERR_SOLVER; }
        iter(chunk);
        *n.iter += chunk;
        launched += chunk;
        chunk = chunk < 32 ? chunk * 2 : 32;
    }
    return PSFM_OK;
}

// ---- psfm_solver_multi.hip, frame mode: the grid tracker's per-frame solves over a table of sequences (index rules: psfm_batch_chain.h) ----
// One sequence of the table: the solver arguments of frame 1 in the sequence's OWN context (what PsfmBatchSeqOpt holds for the fused
// batch kernel), the strides pc_params_rebase turns them into any frame's with, and the single chain's block count for that context.
struct PcMultiFrameRow { PcParams P; PsfmSeqStride st; int64_t occ2_stride; int n_flows; int n_blocks; };
// what the frame-mode poll leaves in pinned memory per sequence: the control block of the frame's solve and the sequence's counters
struct PcMultiFramePoll { PsfmSolveCtrl C; int active; int n_lanes; int overflow; int stall; };

// ---- psfm_solver_fused.hip ----
psfm_status pc_fused_workspace(psfm_ctx* c, const PsfmTrackDims& d, PcParams& P, int K, hipStream_t s, bool zero_tickets = false);
psfm_status pc_launch_fused_export(psfm_ctx* c, const PsfmTrackDims& d, PcParams& P, int K, hipStream_t s);
psfm_status pc_seq_args(psfm_ctx* c, const PsfmTrackDims& d, const float* flows, const uint8_t* occ, int64_t occ_pitch,
                        const float* flows_f2, const uint8_t* occ_s2, PcParams& P, PsfmChainArgs& a, PsfmSeqStride& st, hipStream_t s);

// LAUNCH_(R) with the kernel instantiation of the sample ratio: R = 1, 2, 4 for those ratios, 0 (the generic form) for any other
#define PSFM_RATIO_DISPATCH(ratio_, LAUNCH_) \
    switch (ratio_) { case 1: LAUNCH_(1); break; case 2: LAUNCH_(2); break; case 4: LAUNCH_(4); break; default: LAUNCH_(0); break; }
