// psfm_pc_params.h -- what every unit of the path-consistency solver (psfm_solver*.hip) shares: the tunables, the kernels' argument block
// (PcParams), the block-level helpers, the rows of the batch table.  Force-inlined device code; each kernel is defined by ONE unit.
#pragma once
#include "psfm_device.h"
#include "psfm_internal.h"
#include "psfm_chain_step.h"
#include "psfm_pc_core.h"
#include "psfm_pc_control.h"

#define PC_BLOCK 256
#include "psfm_pc_resident.h"
#include "psfm_pc_reduce.h"
#include "psfm_batch_chain.h"
#ifndef PC_FUSED_PAIR
#define PC_FUSED_PAIR false  // ... and the fused solve's: its lanes are neighbours in the image, and the frame kernel spills 7 VGPRs with them
#endif
#ifndef PC_MAX_BLOCKS
#define PC_MAX_BLOCKS 1024   // rows of the launch chain's partial sums
#endif
#ifndef PC_CHAIN_BLOCKS
#define PC_CHAIN_BLOCKS 512  // blocks of a launch-chain kernel: 512 measured best on the 401-frame 1080p run in round 2 (152 VGPRs, 3
                             // waves/SIMD: 66 ms; 768: 67.6, 384: 70.9, 430: 69.2, 537: 71 -- an equal number of blocks on every CU
                             // matters more than an equal number of tracks per thread)
#endif
#define PC_KMAX 8            // fused solve: most trust-region iterations speculated in one launch
#ifndef PSFM_FRAME_WAVES
#define PSFM_FRAME_WAVES 4    // psfm_frame_kernel (host-paced merged frames, the sharded engine's frames)
#endif
#ifndef PSFM_SEQ_WAVES_DEFAULT
#define PSFM_SEQ_WAVES_DEFAULT 4
#endif
#define PC_GROUP 32          // fused solve: blocks per first-level reduction group

struct PcParams {
    // geometry
    int H, W;
    float cw, ch;
    // frame mode: lanes; batch mode: rows
    const int* birth_frame;   // NULL in batch mode
    int max_birth;            // track participates iff 0 <= birth_frame <= max_birth
    const int* n_lanes_ptr;   // device count of lanes (frame mode) or NULL
    int n_rows;               // upper bound of the index range (cap or batch n)
    // iterate buffers: buffer 0 = (x1a, x2a) -- the caller's values (frame mode: the log slabs), never overwritten before
    // the write-back; buffer m >= 1 = (xs + (2m-2) * xs_stride, xs + (2m-1) * xs_stride).  The launch chain ping-pongs
    // between buffers 1 and 2; the fused solve stores the iterate after m accepted steps in buffer m.
    double2 *x1a, *x2a;
    double2* xs; int64_t xs_stride;
    const double2* p0;        // frame mode: log slab f-1
    // per-track constants
    double2 *ref1, *ref2;
    double* scale;
    double2* jscale;          // (S0^2, S1^2): squared Jacobi scaling of columns 0, 1 (columns 2, 3 need none: psfm_pc_core.h)
    const float2* flow12;
    // init-only inputs (frame mode)
    const float2* flow01;
    const float2* flow02;
    const uint8_t* occ02;
    double* partials;         // [PC_MAX_BLOCKS][PC_NSUM]
    // launch chain / resident solve: the lanes that take part in this solve, compacted per block by pc_init (pc_build_list):
    // block b's entries are list[b * list_pitch + 0 .. list_n[b]), thread t walks entries t, t + PC_BLOCK, ...
    int* list; int* list_n; int list_pitch; int list_banded;
    PsfmSolveCtrl* ctrl;
    int* stall;               // != 0: an earlier solve of this sequence ran out of unrolled iterations -> do nothing
    unsigned* ticket;         // last-block detection
    int frame;                // frame index of this solve (stall value / stats slot)
    psfm_solve_stats* stats_dev;   // per-frame statistics (frame mode) or NULL
    // fused solve (psfm_pc_fused_kernel)
    int K;                    // speculated trust-region iterations per launch (<= PC_KMAX)
    double* gpart;            // [groups][PC_KMAX][PC_NSUM] sums of PC_GROUP consecutive blocks
    unsigned* gticket;        // [groups] + 1 (top)
    int* sel;                 // PsfmCounters::sel: buffer that holds the accepted iterate of the last solve (0: the log)
    int* n_lanes_snap;        // PsfmCounters::n_lanes_snap[2] (frame mode)
    // track-sharded runs: the tracks of the solve are spread over several processes.  A launch then only EXPORTS its sums
    // ([K or 1][PC_NSUM], this process's tracks); the ranks combine them (all-gather, rank order) and every rank runs the
    // same control step on the totals (psfm_pc_control_kernel)
    double* export_sums;
};

__device__ __forceinline__ double2* pc_buf1(const PcParams& P, int m) { return m == 0 ? P.x1a : P.xs + (int64_t)(2 * m - 2) * P.xs_stride; }
__device__ __forceinline__ double2* pc_buf2(const PcParams& P, int m) { return m == 0 ? P.x2a : P.xs + (int64_t)(2 * m - 1) * P.xs_stride; }

// The per-track arithmetic (evaluation, normal equations through the 2x2 Schur complement, dogleg step, the terms of the 13
// sums) lives in psfm_pc_core.h; it is shared by the launch chain and the fused solve, so the two give the same bits.
// P.jscale holds (S0^2, S1^2): the squared Jacobi scaling of columns 0, 1.
__device__ __forceinline__ PcConst pc_const_load(double s, double2 js)
{
    PcConst c;
    c.s = s; c.S0q = js.x; c.S1q = js.y; c.H22 = fma(s, s, 1.0);
    return c;
}

// ... -> partials[blockIdx] (launch chain)
__device__ __forceinline__ void pc_block_reduce(double acc[PC_NSUM], double* __restrict__ partials)
{
    __shared__ double s_blk[PC_NSUM];
    pc_block_sums<PC_NSUM>(acc, s_blk);
    // write-through (sc0 sc1) store: the last block of the launch reads these with matching loads, so no
    // agent-scope release (an L2 write-back per block) is needed -- MI355X_MICROARCH.md, valid hand-off forms
    if (threadIdx.x < PC_NSUM)
        __hip_atomic_store(&partials[(int64_t)blockIdx.x * PC_NSUM + threadIdx.x], s_blk[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

__device__ __forceinline__ bool pc_participates(const PcParams& P, int i, int n)
{
    if (i >= n) return false;
    if (!P.birth_frame) return true;
    const int bf = P.birth_frame[i];
    return bf >= 0 && bf <= P.max_birth;
}

// The tracks of a solve, dealt to the blocks of the launch chain: block b looks at the lane chunks b, b + gridDim.x, ... (PC_BLOCK
// lanes each) and compacts the lanes that take part (ballot -> wave offsets through LDS) into ITS list, in lane order.  Every
// later launch of the solve -- pc_iter, the resident solve -- walks that list: thread t takes entries t, t + PC_BLOCK, ...; no
// launch after pc_init reads a birth frame or skips a lane, the resident solve knows how many tracks a thread will ever hold,
// and all forms add the tracks' terms in the same order.  Returns the block's count (also left in list_n[b]).
__device__ __forceinline__ int pc_build_list(const PcParams& P, int n)
{
    __shared__ int s_wc[PC_BLOCK / PSFM_WAVE];
    int* lst = P.list + (int64_t)blockIdx.x * P.list_pitch;
    const int lane = threadIdx.x & (PSFM_WAVE - 1), w = threadIdx.x / PSFM_WAVE;
    // Which chunks (pc_list_plan, psfm_pc_resident.h): by default XCD-BANDED -- the blocks of XCD x = b % 8 share the x-th eighth of the
    // chunks, so the taps of an XCD's tracks come from one band of the flow field (2 MB of 16.6 at 1080p: it stays in that XCD's 4 MB
    // L2 across the rounds of a solve) instead of from all of it.  P.list_banded == 0 or a grid that is not a multiple of 8: chunks b,
    // b + gridDim.x, ...
    const PcListPlan plan = pc_list_plan((int)blockIdx.x, (int)gridDim.x, n, P.list_banded);
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
        __syncthreads();      // (s_wc is rewritten by the next chunk; the list entries are visible to the block behind it)
    }
    if (threadIdx.x == 0) P.list_n[blockIdx.x] = base;
    return base;
}

// Publish this block's partials and find out whether it is the last one to finish: write-through payload ->
// drain -> ticket (device-scope atomic); the last block reads the payload with cache-bypassing loads.
__device__ __forceinline__ bool pc_is_last_block(unsigned* ticket)
{
    __shared__ int s_last;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's partial stores have been performed
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = (t == gridDim.x - 1u);
        if (s_last) *ticket = 0u;   // next launch starts from zero (visible after the kernel boundary)
    }
    __syncthreads();
    return s_last != 0;
}

// What changes from one frame to the next in the solver's arguments (frame mode)
__host__ __device__ inline void pc_params_rebase(PcParams& P, const PsfmSeqStride& st, int64_t occ2_stride, int f)
{
    // (the rule itself is written over any argument block in psfm_batch_chain.h, where the CPU suite compiles and runs it)
    pc_frame_rebase(P, (long long)st.cap, (long long)st.flow, (long long)occ2_stride, f);
}

// one sequence's row of the batch table (psfm_solver_batch.hip; filled by psfm_batch_fill_seq_opt)
struct PsfmBatchSeqOpt { PsfmChainArgs a; PcParams P; PsfmSeqStride st; int64_t occ2_stride; int n_flows; int pad; };
