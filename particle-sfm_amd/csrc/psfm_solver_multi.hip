// psfm_solver_multi.hip -- the launch chain of the path-consistency solver (psfm_solver.hip: pc_init, one pc_iter launch per
// trust-region iteration, the write-back) over a TABLE of problems in device memory, one grid for all of them.
//
// The chain already decides on the device (the last block of a launch reduces and runs pc_reduce_and_control), reads its row count
// from device memory (PcParams::n_lanes_ptr) and makes a launch a no-op for a solve that is done; what it lacked is a form that runs
// over many independent solves at once -- psfm_track_queries_optimize_batch has one small solve per sequence and frame, each of them
// a block or two.  Here a row of the table (PcMultiRow) is one problem: a PcParams whose ctrl, ticket, partials, list and iterate
// buffers live in that sequence's own context, the address of the sequence's row count for the current step, the block limit
// pc_blocks gives that context, and what changes from step to step (the map flow12 names).  The table is written once per direction;
// the step is a kernel argument and the kernels derive the step's pointers from it in the manner of pc_params_rebase.
//
// Grid (blocks, problems) -- the index rules and why not the flattened form: psfm_solver_multi.h.  A problem's effective block count
// is computed on the device from its row count by the rule of pc_blocks; blocks beyond it return before touching anything, and that
// count -- not gridDim.x -- goes into the list plan, the last-block ticket and the tree of the block sums.  A problem with no rows, a
// done problem and a stalled one cost a few scalar loads per block.
//
// Per-track arithmetic, list order, the tree of the block sums and the control step are the single chain's functions
// (psfm_pc_tracks.h); this unit only adds the forms of pc_build_list and pc_is_last_block that take the block count as an argument
// (pc_block_reduce names a block by blockIdx.x alone and is used as it is).  No floating-point atomics: the partials are handed off
// as in the single chain -- write-through stores, the drain, then the ticket.  No resident form, no fused form.
//
// Two forms of a table: ROW mode (above: psfm_pc_multi_*_kernel, rows written in place by the query engine, the block count derived
// on the device) and FRAME mode (psfm_pc_multi_frame_*_kernel below: a row is a SEQUENCE of the grid tracker, rebased to the frame by
// pc_params_rebase, with the single chain's block count known on the host -- index rules in psfm_batch_chain.h).
#include <string.h>

#include "psfm_pc_tracks.h"
#include "psfm_solver_internal.h"
#include "psfm_solver_multi.h"
#include "psfm_batch_chain.h"

// pc_build_list (psfm_pc_params.h) for a solve of n_blocks blocks inside a larger grid: the same plan, the same compaction
__device__ __forceinline__ int pc_build_list_nb(const PcParams& P, int n, int n_blocks)
{
    __shared__ int s_wc[PC_BLOCK / PSFM_WAVE];
    int* lst = P.list + (int64_t)blockIdx.x * P.list_pitch;
    const int lane = threadIdx.x & (PSFM_WAVE - 1), w = threadIdx.x / PSFM_WAVE;
    const PcListPlan plan = pc_list_plan((int)blockIdx.x, n_blocks, n, P.list_banded);
    const int first = plan.first, step = plan.step, band0 = plan.band0;
    int base = 0;
    for (int q = first; pc_list_chunk_ok(plan, q); q += step) {
        const int i = (band0 + q) * PC_BLOCK + (int)threadIdx.x;
        const bool part = pc_participates(P, i, n);
        const unsigned long long m = __ballot(part);
        if (lane == 0) s_wc[w] = __popcll(m);
        __syncthreads();
        int off = base, tot = 0;
#pragma unroll
        for (int qq = 0; qq < PC_BLOCK / PSFM_WAVE; ++qq) { if (qq < w) off += s_wc[qq]; tot += s_wc[qq]; }
        if (part) lst[off + __popcll(m & ((1ull << lane) - 1ull))] = i;
        base += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) P.list_n[blockIdx.x] = base;
    return base;
}

// pc_is_last_block (psfm_pc_params.h) among the n_blocks blocks of ONE problem: write-through payload -> drain -> the problem's own
// ticket (device-scope atomic); the last block reads the payload with cache-bypassing loads
__device__ __forceinline__ bool pc_is_last_block_nb(unsigned* ticket, int n_blocks)
{
    __shared__ int s_last;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's partial stores have been performed
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = (t == (unsigned)n_blocks - 1u);
        if (s_last) *ticket = 0u;   // next launch starts from zero (visible after the kernel boundary)
    }
    __syncthreads();
    return s_last != 0;
}

// The block's problem in step k: false when the block has nothing to do (the problem does not take part in the step, has no rows, or
// has fewer blocks than the grid).  P: the row's arguments rebased to the step; n: its rows; nb: its effective block count.
__device__ __forceinline__ bool pc_multi_begin(const PcMultiRow* __restrict__ tab, int k, PcParams& P, int& n, int& nb)
{
    const PcMultiRow& R = tab[blockIdx.y];
    const int n_flows = R.n_flows;
    if (!pc_multi_active(k, n_flows)) return false;
    // (the count is the same in every lane, but it comes through a pointer into memory the compiler must assume written: say so, or
    // the block count and every loop bound derived from it live in vector registers)
    n = __builtin_amdgcn_readfirstlane(pc_multi_rows(k, n_flows, *R.P.n_lanes_ptr, R.P.n_rows));
    if (!pc_multi_block_works((int)blockIdx.x, n, R.limit)) return false;
    nb = pc_multi_blocks(n, R.limit);
    P = R.P;
    P.flow12 += (int64_t)pc_multi_map(k, n_flows, R.back) * R.flow_stride;
    P.frame = k;
    return true;
}

__global__ __launch_bounds__(PC_BLOCK) void psfm_pc_multi_init_kernel(const PcMultiRow* __restrict__ tab, int k)
{
    PcParams P;
    int n, nb;
    if (!pc_multi_begin(tab, k, P, n, nb)) return;
    if (*P.stall) return;
    double acc[PC_NSUM];
#pragma unroll
    for (int q = 0; q < PC_NSUM; ++q) acc[q] = 0.0;
    const int cnt = pc_build_list_nb(P, n, nb);
    const int* lst = P.list + (int64_t)blockIdx.x * P.list_pitch;
    for (int p = threadIdx.x; p < cnt; p += PC_BLOCK) {      // (pc_init_tracks: the block's entries in list order)
        PcInit o;
        pc_init_entry(P, lst[p], true, acc, o);
    }
    pc_block_reduce(acc, P.partials);
    if (pc_is_last_block_nb(P.ticket, nb)) {
        // pc_reduce_and_control's init form, with the control block built in LDS (as the resident solve builds it): iteration 0 clears
        // the whole block first, and a private copy of it does not stay in registers behind that -- the single kernel has it in scratch
        __shared__ PsfmSolveCtrl s_C;
        pc_reduce_totals(P.partials, nb);
        if (threadIdx.x != 0) return;
        pc_chain_control(s_C, pc_totals(), 0);
        s_C.launches += 1;
        *P.ctrl = s_C;
    }
}

__global__ __launch_bounds__(PC_BLOCK) void psfm_pc_multi_iter_kernel(const PcMultiRow* __restrict__ tab, int k)
{
    PcParams P;
    int n, nb;
    if (!pc_multi_begin(tab, k, P, n, nb)) return;
    if (*P.stall) return;
    const PsfmSolveCtrl C = *P.ctrl;
    if (C.done) return;
    double acc[PC_NSUM];
#pragma unroll
    for (int q = 0; q < PC_NSUM; ++q) acc[q] = 0.0;
    pc_iter_tracks(P, (int)threadIdx.x, C.cur, C.mu, C.dl_a, C.dl_b, C.kind_next != 0, acc);
    pc_block_reduce(acc, P.partials);
    if (pc_is_last_block_nb(P.ticket, nb)) pc_reduce_and_control(P.ctrl, P.partials, nb, 0, nullptr);
}

// behind the poll that saw every problem done: the accepted iterate into buffer 0 (x1a, x2a), as pc_writeback_tracks does it -- a
// failed solve and one that accepted no step leave buffer 0 as it came in
__global__ __launch_bounds__(PC_BLOCK) void psfm_pc_multi_writeback_kernel(const PcMultiRow* __restrict__ tab, int k)
{
    PcParams P;
    int n, nb;
    if (!pc_multi_begin(tab, k, P, n, nb)) return;
    if (*P.stall) return;
    const PsfmSolveCtrl C = *P.ctrl;
    if (!C.done) return;
    const int cur = __builtin_amdgcn_readfirstlane(C.failed ? 0 : C.cur);
    if (cur == 0) return;
    const double2* xc1 = pc_buf1(P, cur);
    const double2* xc2 = pc_buf2(P, cur);
    for (int i = blockIdx.x * PC_BLOCK + threadIdx.x; i < n; i += nb * PC_BLOCK) {
        P.x1a[i] = xc1[i];
        P.x2a[i] = xc2[i];
    }
}

// one block: every problem's control block and its rows of step k into pinned host memory -- what the host decides on (is any
// problem left undone?) and the statistics of the solves, in one copy
__global__ __launch_bounds__(PC_BLOCK) void psfm_pc_multi_poll_kernel(const PcMultiRow* __restrict__ tab, int n_problems, int k,
                                                                      PcMultiPoll* __restrict__ out)
{
    static_assert(sizeof(PsfmSolveCtrl) % 8 == 0, "the control block is copied as 8-byte words");
    constexpr int WORDS = (int)(sizeof(PsfmSolveCtrl) / 8);
    for (int w = threadIdx.x; w < n_problems * (WORDS + 1); w += PC_BLOCK) {
        const int b = w / (WORDS + 1), j = w - b * (WORDS + 1);
        const PcMultiRow& R = tab[b];
        // (a problem that does not take part in the step has no row count to read, and one without rows no solve to report)
        const int n = pc_multi_active(k, R.n_flows) ? pc_multi_rows(k, R.n_flows, *R.P.n_lanes_ptr, R.P.n_rows) : 0;
        if (j == WORDS) { out[b].n_rows = n; out[b].pad = 0; }
        else ((unsigned long long*)&out[b].C)[j] = n > 0 ? ((const unsigned long long*)R.P.ctrl)[j] : 0ull;
    }
}

// ---- frame mode: the grid tracker's per-frame solves over a table of SEQUENCES (psfm_connect_batch's redo_together) ----
// A row is one sequence (PcMultiFrameRow): the solver arguments of frame 1 in the sequence's own context -- lanes with birth frames,
// p0 / x1a / x2a log slabs that move with the frame, pc_init building ref1 / ref2 / scale from flow01 / flow02 / occ02 -- rebased to
// frame f by pc_params_rebase, and the block count pc_blocks gives that context on the HOST.  That count (not one derived from the lane
// count, not gridDim.x) goes into the list plan, the ticket and the tree of the block sums: the launches of a sequence are the launches
// psfm_connect makes for it alone, block for block, and leave the same bytes.  Index rules: psfm_batch_chain.h.
__device__ __forceinline__ bool pc_frame_begin(const PcMultiFrameRow* __restrict__ tab, int f, PcParams& P, int& n, int& nb)
{
    const PcMultiFrameRow& R = tab[blockIdx.y];
    if (!pc_frame_active(f, R.n_flows)) return false;
    nb = R.n_blocks;
    if (!pc_frame_block_works((int)blockIdx.x, nb)) return false;
    P = R.P;
    pc_params_rebase(P, R.st, R.occ2_stride, f);
    if (*P.stall) return false;
    // (uniform, but read through a pointer: see pc_multi_begin)
    n = __builtin_amdgcn_readfirstlane(pc_frame_rows(*P.n_lanes_ptr, P.n_rows));
    return true;
}

__global__ __launch_bounds__(PC_BLOCK) void psfm_pc_multi_frame_init_kernel(const PcMultiFrameRow* __restrict__ tab, int f)
{
    PcParams P;
    int n, nb;
    if (!pc_frame_begin(tab, f, P, n, nb)) return;
    // (pc_init_tracks: the chain step in front has consumed PsfmCounters::sel; the chain works in buffer 0 from here on)
    if (blockIdx.x == 0 && threadIdx.x == 0) *P.sel = 0;
    double acc[PC_NSUM];
#pragma unroll
    for (int q = 0; q < PC_NSUM; ++q) acc[q] = 0.0;
    const int cnt = pc_build_list_nb(P, n, nb);
    const int* lst = P.list + (int64_t)blockIdx.x * P.list_pitch;
    for (int p = threadIdx.x; p < cnt; p += PC_BLOCK) {
        PcInit o;
        pc_init_entry(P, lst[p], true, acc, o);
    }
    pc_block_reduce(acc, P.partials);
    if (pc_is_last_block_nb(P.ticket, nb)) {
        __shared__ PsfmSolveCtrl s_C;      // (as psfm_pc_multi_init_kernel: iteration 0 clears the whole block, built in LDS)
        pc_reduce_totals(P.partials, nb);
        if (threadIdx.x != 0) return;
        pc_chain_control(s_C, pc_totals(), 0);
        s_C.launches += 1;
        *P.ctrl = s_C;
    }
}

__global__ __launch_bounds__(PC_BLOCK) void psfm_pc_multi_frame_iter_kernel(const PcMultiFrameRow* __restrict__ tab, int f)
{
    PcParams P;
    int n, nb;
    if (!pc_frame_begin(tab, f, P, n, nb)) return;
    const PsfmSolveCtrl C = *P.ctrl;
    if (C.done) return;
    double acc[PC_NSUM];
#pragma unroll
    for (int q = 0; q < PC_NSUM; ++q) acc[q] = 0.0;
    pc_iter_tracks(P, (int)threadIdx.x, C.cur, C.mu, C.dl_a, C.dl_b, C.kind_next != 0, acc);
    pc_block_reduce(acc, P.partials);
    if (pc_is_last_block_nb(P.ticket, nb)) pc_reduce_and_control(P.ctrl, P.partials, nb, 0, nullptr);
}

// behind the poll that saw every sequence's solve done: pc_writeback_tracks with the sequence's own block count -- the frame's
// statistics, PsfmCounters::sel and the lane snapshot (pc_writeback_scalars), the accepted iterate into the log slabs
__global__ __launch_bounds__(PC_BLOCK) void psfm_pc_multi_frame_writeback_kernel(const PcMultiFrameRow* __restrict__ tab, int f)
{
    PcParams P;
    int n, nb;
    if (!pc_frame_begin(tab, f, P, n, nb)) return;
    const PsfmSolveCtrl C = *P.ctrl;
    if (!C.done) return;
    if (blockIdx.x == 0 && threadIdx.x == 0) pc_writeback_scalars(P, C);
    const int cur = __builtin_amdgcn_readfirstlane(C.failed ? 0 : C.cur);
    if (cur == 0) return;
    const double2* xc1 = pc_buf1(P, cur);
    const double2* xc2 = pc_buf2(P, cur);
    for (int i = blockIdx.x * PC_BLOCK + threadIdx.x; i < n; i += nb * PC_BLOCK) {
        if (!pc_participates(P, i, n)) continue;
        P.x1a[i] = xc1[i];
        P.x2a[i] = xc2[i];
    }
}

// one block: every sequence's control block of frame f and its counters (lanes in use, overflow bits, stall flag) into pinned host
// memory -- what the host decides on, the statistics of the solves and the check of the tables, in one copy
__global__ __launch_bounds__(PC_BLOCK) void psfm_pc_multi_frame_poll_kernel(const PcMultiFrameRow* __restrict__ tab, int n_problems, int f,
                                                                            PcMultiFramePoll* __restrict__ out)
{
    constexpr int WORDS = (int)(sizeof(PsfmSolveCtrl) / 8);
    static_assert(sizeof(PcMultiFramePoll) == sizeof(PsfmSolveCtrl) + 16, "the poll row is the control block and four counters");
    for (int w = threadIdx.x; w < n_problems * (WORDS + 1); w += PC_BLOCK) {
        const int b = w / (WORDS + 1), j = w - b * (WORDS + 1);
        const PcMultiFrameRow& R = tab[b];
        const bool active = pc_frame_active(f, R.n_flows);
        if (j == WORDS) {
            const PsfmCounters* ctr = (const PsfmCounters*)R.P.n_lanes_ptr;      // (n_lanes is the first member: pc_frame_params)
            out[b].active = active ? 1 : 0; out[b].n_lanes = ctr->n_lanes; out[b].overflow = ctr->overflow; out[b].stall = ctr->stall;
        } else {
            ((unsigned long long*)&out[b].C)[j] = active ? ((const unsigned long long*)R.P.ctrl)[j] : 0ull;
        }
    }
}

// ---- host: the launchers (a kernel is launched only by the unit that defines it) ----
void pc_multi_launch_init(const PcMultiRow* tab, int grid_x, int n_problems, int k, hipStream_t s)
{
    hipLaunchKernelGGL(psfm_pc_multi_init_kernel, dim3((unsigned)grid_x, (unsigned)n_problems), dim3(PC_BLOCK), 0, s, tab, k);
}
void pc_multi_launch_iter(const PcMultiRow* tab, int grid_x, int n_problems, int k, int n_launches, hipStream_t s)
{
    for (int q = 0; q < n_launches; ++q)
        hipLaunchKernelGGL(psfm_pc_multi_iter_kernel, dim3((unsigned)grid_x, (unsigned)n_problems), dim3(PC_BLOCK), 0, s, tab, k);
}
void pc_multi_launch_writeback(const PcMultiRow* tab, int grid_x, int n_problems, int k, hipStream_t s)
{
    hipLaunchKernelGGL(psfm_pc_multi_writeback_kernel, dim3((unsigned)grid_x, (unsigned)n_problems), dim3(PC_BLOCK), 0, s, tab, k);
}
void pc_multi_launch_poll(const PcMultiRow* tab, int n_problems, int k, PcMultiPoll* out_pinned, hipStream_t s)
{
    hipLaunchKernelGGL(psfm_pc_multi_poll_kernel, dim3(1), dim3(PC_BLOCK), 0, s, tab, n_problems, k, out_pinned);
}

// ---- host, frame mode: rows, launchers and one frame's solves of the whole table (psfm_batch.hip keeps the rows opaque) ----
size_t psfm_frame_row_bytes(void) { return sizeof(PcMultiFrameRow); }
size_t psfm_frame_poll_bytes(void) { return sizeof(PcMultiFramePoll); }

// a sequence's row from its row of the fused batch table (psfm_batch_fill_seq_opt: the arguments of frame 1 and the strides)
psfm_status psfm_frame_row_fill(psfm_ctx* c, const PsfmTrackDims& d, const void* seq_opt_row_host, void* row_host, int* n_blocks)
{
    static_assert(offsetof(PsfmCounters, n_lanes) == 0, "the poll reads the counters through PcParams::n_lanes_ptr");
    const PsfmBatchSeqOpt* q = (const PsfmBatchSeqOpt*)seq_opt_row_host;
    PcMultiFrameRow* R = (PcMultiFrameRow*)row_host;
    memset(R, 0, sizeof(*R));
    R->P = q->P; R->st = q->st; R->occ2_stride = q->occ2_stride; R->n_flows = q->n_flows;
    R->n_blocks = psfm_solve_blocks(c, d);
    *n_blocks = R->n_blocks;
    if (R->n_blocks > PC_MAX_BLOCKS || R->P.list_pitch != pc_frame_list_pitch(d.cap, R->n_blocks) || R->P.frame != 1 || !R->P.sel ||
        !R->P.stall || !R->P.n_lanes_ptr || R->P.n_rows != (int)d.cap) {
        psfm_set_error("psfm_connect_batch: a sequence's solver arguments do not fit the frame-mode chain (blocks %d, list pitch %d)",
                       R->n_blocks, R->P.list_pitch);
        return PSFM_ERR_ARG;
    }
    return PSFM_OK;
}

// The solves of frame f of every sequence of the table: the init launch, pc_multi_pace's iteration launches and polls, the write-back
// launch.  poll_pinned holds what the last poll saw (psfm_frame_poll_read) when this returns.
psfm_status psfm_frame_solve_batch(const void* rows_dev, int grid_x, int n_problems, int f, void* poll_pinned, int32_t* n_fixed,
                                   int32_t* n_iter, int32_t* n_syncs, hipStream_t s)
{
    const PcMultiFrameRow* tab = (const PcMultiFrameRow*)rows_dev;
    PcMultiFramePoll* poll = (PcMultiFramePoll*)poll_pinned;
    const dim3 grid((unsigned)grid_x, (unsigned)n_problems), block(PC_BLOCK);
    hipLaunchKernelGGL(psfm_pc_multi_frame_init_kernel, grid, block, 0, s, tab, f);
    *n_fixed += 1;
    const PcPaceCensus census{n_fixed, n_iter, n_syncs};
    psfm_status st = pc_multi_pace(
        [&](int n_launches) { for (int q = 0; q < n_launches; ++q) hipLaunchKernelGGL(psfm_pc_multi_frame_iter_kernel, grid, block, 0, s, tab, f); },
        [&]() { hipLaunchKernelGGL(psfm_pc_multi_frame_poll_kernel, dim3(1), dim3(PC_BLOCK), 0, s, tab, n_problems, f, poll); },
        [&]() {
            bool undone = false;
            // (a sequence whose tables ran full is the caller's to refuse; its solve is not waited for)
            for (int i = 0; i < n_problems; ++i)
                undone = undone || (poll[i].active && !poll[i].stall && (poll[i].overflow & 7) == 0 && !poll[i].C.done);
            return undone;
        },
        census, s, "psfm_connect_batch");
    if (st != PSFM_OK) return st;
    hipLaunchKernelGGL(psfm_pc_multi_frame_writeback_kernel, grid, block, 0, s, tab, f);
    *n_fixed += 1;
    PSFM_HIP(hipGetLastError());
    return PSFM_OK;
}

// what the last poll of psfm_frame_solve_batch saw of sequence i: did it take part, the statistics of its solve (as pc_fill_stats
// fills them; 5 for a failed solve), its lanes in use, overflow bits and stall flag (raised: the kernels skipped the sequence and
// the control block is not this frame's -- the caller's to refuse)
void psfm_frame_poll_read(const void* poll_pinned, int i, int* active, psfm_solve_stats* st, int* n_lanes, int* overflow, int* stall)
{
    const PcMultiFramePoll& p = ((const PcMultiFramePoll*)poll_pinned)[i];
    *active = p.active; *n_lanes = p.n_lanes; *overflow = p.overflow; *stall = p.stall;
    memset(st, 0, sizeof(*st));
    if (!p.active) return;
    pc_multi_stats(&p.C, st);
    if (p.C.failed) st->termination = PSFM_TERM_FAILURE;
}
