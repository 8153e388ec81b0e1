// psfm_solver_multi.h -- the index rules of the MULTI-PROBLEM launch chain (psfm_solver_multi.hip): pc_init / pc_iter / write-back of
// the path-consistency solver over a table of problems in device memory, one grid for all of them.  Plain integer rules with no HIP
// in them: the CPU suite compiles this header with g++ (tests/host/solver_multi_host.cpp) and runs a table of problems through them
// against each problem alone through the single chain's rules.
//
// The grid is (blocks, problems): blockIdx.y is the problem, blockIdx.x the block INSIDE the problem.  Chosen over the flattened form
// of psfm_query_batch.h because every shared function of the chain that names a block (pc_block_reduce, pc_iter_tracks, the list
// rows, the partial rows) reads blockIdx.x as "my block of this solve" -- with the problem in y they run unchanged and compile to
// what they compile to in the single kernels; only gridDim.x had to go.  A flattened grid would need a prefix of block counts that
// is known on the host, and here the block count of a problem is only known on the DEVICE (it follows the frame's row count, which
// the host never reads): gridDim.x is the most blocks any problem of the table can have, and a block beyond its problem's effective
// count returns behind a few scalar loads.
#pragma once

#ifndef PC_BLOCK
#define PC_BLOCK 256
#endif
#if defined(__HIPCC__) || defined(__CUDACC__)
#define PC_MULTI_HD __host__ __device__ __forceinline__
#else
#define PC_MULTI_HD static inline
#endif

// The effective block count of a problem with n_rows rows whose launches may use `limit` blocks: the rule of pc_blocks
// (psfm_solver.hip), clamp(ceil(n_rows / PC_BLOCK), 1, limit).  THIS count -- not gridDim.x -- goes into the list plan, the
// last-block ticket and the tree of the block sums.
PC_MULTI_HD int pc_multi_blocks(int n_rows, int limit)
{
    int nb = (n_rows + PC_BLOCK - 1) / PC_BLOCK;
    if (nb > limit) nb = limit;
    return nb < 1 ? 1 : nb;
}

// A problem takes part in step k of its direction when a solve can happen there: a track holds three positions from the second step
// on, and the sequence has n_flows steps.  (A sequence that is shorter than its companions does nothing in the steps beyond its end.)
PC_MULTI_HD bool pc_multi_active(int k, int n_flows) { return k >= 1 && k < n_flows; }

// The map the solve of step k samples (flow12: the map that was stepped through): forward map k, backward map n_flows - k - 1
PC_MULTI_HD int pc_multi_map(int k, int n_flows, int back) { return back ? n_flows - k - 1 : k; }

// The rows of a problem in step k: the count its sequence's scan left in device memory, bounded by the rows the buffers hold
PC_MULTI_HD int pc_multi_rows(int k, int n_flows, int counted, int capacity)
{
    if (!pc_multi_active(k, n_flows)) return 0;
    return counted < capacity ? counted : capacity;
}

// Does block `blk` of the grid work for a problem of n_rows rows?  No rows: no block does (no solve runs, as in the single call).
PC_MULTI_HD bool pc_multi_block_works(int blk, int n_rows, int limit) { return n_rows > 0 && blk < pc_multi_blocks(n_rows, limit); }

// gridDim.x of a launch over a table: the most blocks any of its problems can have (cap[b]: the rows its buffers hold)
PC_MULTI_HD int pc_multi_grid_x(const int* cap, const int* limit, int n_problems)
{
    int g = 1;
    for (int b = 0; b < n_problems; ++b) {
        const int nb = pc_multi_blocks(cap[b], limit[b]);
        if (nb > g) g = nb;
    }
    return g;
}

// The pitch of a problem's list rows (entries per block) that holds every row count up to `cap` under `limit`: what pc_setup
// (psfm_solver.hip) sizes for ONE row count, at its largest -- chunks per block is 1 while the chunks fit the limit and
// ceil(chunks / limit) beyond, both non-decreasing in the row count; one chunk of head-room for the banded plan.
PC_MULTI_HD int pc_multi_list_pitch(int cap, int limit)
{
    const int chunks = (cap + PC_BLOCK - 1) / PC_BLOCK;
    const int nb = pc_multi_blocks(cap, limit);
    return ((chunks + nb - 1) / nb + 1) * PC_BLOCK;
}
