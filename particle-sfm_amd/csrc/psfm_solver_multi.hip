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
#include <string.h>

#include "psfm_pc_tracks.h"
#include "psfm_solver_internal.h"
#include "psfm_solver_multi.h"

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
