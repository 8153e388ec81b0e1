// psfm_batch_chain.h -- the index rules of the FRAME-MODE multi-problem launch chain (psfm_pc_multi_frame_*_kernel,
// psfm_solver_multi.hip): pc_init / pc_iter / write-back of the grid tracker's per-frame solves over a table of SEQUENCES, one grid
// (blocks, sequences) for all of them -- what psfm_connect_batch runs the sequences through whose solves reject steps
// (BatchRun::redo_together, psfm_batch.hip).  Plain integer rules with no HIP in them: the CPU suite compiles this header with g++
// (tests/host/batch_chain_host.cpp) and holds every rule against the single chain's.
//
// What differs from the row-mode rules of psfm_solver_multi.h: a problem's block count is NOT derived from a row count on the device.
// It is the single chain's count for the sequence's context -- pc_blocks(ctx, lane capacity), resident budget applied -- known on the
// host and stored in the table row, so that the list plan, the last-block ticket and the tree of the block sums are those of
// psfm_connect on that context and the iterates equal its bit for bit.  The rows of a solve are lanes: min(lanes in use, capacity),
// read on the device; which of them take part is pc_participates' business (birth frames), not an index rule.
#pragma once

#ifndef PC_BLOCK
#define PC_BLOCK 256
#endif
#if defined(__HIPCC__) || defined(__CUDACC__)
#define PC_FRAME_HD __host__ __device__ __forceinline__
#else
#define PC_FRAME_HD static inline
#endif

// The single chain's block count for a context whose lane table holds `cap` lanes and whose launches may use `limit` blocks
// (PC_CHAIN_BLOCKS, or the context's resident budget when that is smaller): the rule of pc_blocks (psfm_solver.hip).
PC_FRAME_HD int pc_frame_blocks(long long cap, int limit)
{
    long long nb = (cap + PC_BLOCK - 1) / PC_BLOCK;
    if (nb > limit) nb = limit;
    return nb < 1 ? 1 : (int)nb;
}

// A sequence takes part in the solve launches of frame f when a solve can happen there (track_optimize.py:49-50: a track holds three
// positions from frame 1 on) and the sequence has that frame.  A sequence shorter than its companions does nothing beyond its end.
PC_FRAME_HD bool pc_frame_active(int f, int n_flows) { return f >= 1 && f < n_flows; }

// Does block `blk` of the grid work for a sequence whose chain has n_blocks blocks?  (gridDim.x is the table's largest count.)
PC_FRAME_HD bool pc_frame_block_works(int blk, int n_blocks) { return blk >= 0 && blk < n_blocks; }

// gridDim.x of a launch over a table: the largest block count of its sequences
PC_FRAME_HD int pc_frame_grid_x(const int* n_blocks, int n_problems)
{
    int g = 1;
    for (int b = 0; b < n_problems; ++b) if (n_blocks[b] > g) g = n_blocks[b];
    return g;
}

// The lanes a solve looks at: the count the chain step left in device memory, bounded by the lanes the tables hold
PC_FRAME_HD int pc_frame_rows(int lanes_in_use, int capacity)
{
    const int n = lanes_in_use < capacity ? lanes_in_use : capacity;
    return n < 0 ? 0 : n;
}

// The pitch of a sequence's list rows (entries per block) for a block count known on the host: what pc_setup (psfm_solver.hip) sizes
// -- ceil(chunks / n_blocks) chunks per block at the capacity, non-decreasing in the lane count, plus one chunk of head-room for the
// banded plan.  The frame-mode kernels use the pitch pc_setup left in the sequence's own arguments; the driver checks it against this.
PC_FRAME_HD int pc_frame_list_pitch(long long cap, int n_blocks)
{
    const long long chunks = (cap + PC_BLOCK - 1) / PC_BLOCK;
    return (int)(((chunks + n_blocks - 1) / n_blocks + 1) * PC_BLOCK);
}

// The rebase of a row (the solver arguments of frame `P.frame`, in the table: frame 1) to frame f, written over any argument block
// with these members so that the host suite can run it: the three log slabs move by the lane capacity, the three flow maps by one
// map, the stride-2 occlusion map by its own stride.  pc_params_rebase (psfm_pc_params.h), which every kernel calls, IS this
// function applied to PcParams: one statement of the rule.
template <class Params>
PC_FRAME_HD void pc_frame_rebase(Params& P, long long cap_stride, long long flow_stride, long long occ2_stride, int f)
{
    const long long df = (long long)f - P.frame;
    P.p0 += df * cap_stride; P.x1a += df * cap_stride; P.x2a += df * cap_stride;
    P.flow01 += df * flow_stride; P.flow12 += df * flow_stride; P.flow02 += df * flow_stride;
    P.occ02 += df * occ2_stride;
    P.frame = f;
    P.max_birth = f - 1;
}
