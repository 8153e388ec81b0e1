// psfm_query_batch.h -- psfm_track_queries_batch (psfm_query_batch.hip): the query points of up to 64 sequences through ONE set of
// launches.  The table of sequences, the lookup a block of a flattened grid performs and the offset rule of the one scan over the
// concatenation of all sequences.  Plain C++: also compiled for the host by the CPU suite (tests/host/queries_batch_host.cpp through
// tests/host/shim).
//
// Sequence b with Q[b] queries owns ceil(Q[b] / 256) blocks of every flattened grid, numbered inside the sequence, so every block
// -- and every wave -- belongs to one sequence; it owns elements [q0[b], q0[b] + Q[b]) of the concatenated per-direction lengths.
// The lengths of all sequences are scanned once: inside each flattened block, then the block totals by one block.  A sequence reads
// the scan relative to its first block -- off[i] = local + (sum[blk] - sum[blk0[b]]) -- which is the single call's off, because the
// sums are integers added in block order and a sequence's blocks are consecutive.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define PSFM_QB_MAX 64                  // sequences per call: PSFM_BATCH_MAX (static_assert in psfm_query_batch.hip)
#define PSFM_QB_BLOCK 256               // threads per block = queries per block (PSFM_QUERY_BLOCK of psfm_query.hip)

// One sequence of a call, in device memory (64 of them do not fit the kernel arguments comfortably).  The sources are known from the
// arguments; the slab, the lengths per direction and the result buffers are filled in behind the validation, when the contexts may
// be touched.  (xy of the result is sized last and travels in the gather's kernel arguments.)
struct PsfmQbSeq {
    const float2* flows_f; const uint8_t* masks_f;      // the forward stack and its occlusion (or kill) maps; NULL: not tracked
    const float2* flows_b; const uint8_t* masks_b;      // the backward stack and ITS maps
    const double2* q_xy; const int* q_t;                // (Q)
    double2* slab;                                      // (n_flows+1, Q) time-major, in the sequence's own context (log)
    int* len_f; int* len_b;                             // (Q) points per direction: this sequence's part of the concatenation, or NULL
    int* birth; int* len; int64_t* off;                 // the result, in the sequence's own context
    int H, W, n_flows;
    unsigned Q, P;                                      // queries; pixels of a map
    float cw, ch, rcw, rch;                             // the sampler's constants (psfm_device.h)
    int blk0;                                           // first block of the sequence in every flattened grid
    int pad;
};

// The flattened grid and the concatenation: what the host builds from the query counts.
struct PsfmQbGrid {
    int blk_end[PSFM_QB_MAX];           // INCLUSIVE prefix of the block counts: blocks of sequences 0 .. b; INT32_MAX at and above n_seq
    int blk0[PSFM_QB_MAX];              // blocks of the sequences before b
    int64_t q0[PSFM_QB_MAX + 1];        // queries of the sequences before b; at and above n_seq: the queries of all sequences
    int blocks;                         // of all sequences = the grid
};

__host__ __device__ __forceinline__ int psfm_qb_blocks_of(int64_t n_q) { return (int)((n_q + PSFM_QB_BLOCK - 1) / PSFM_QB_BLOCK); }

// n_q[b] >= 0, all together below 2^28 (checked by the caller: the block count fits an int with room to spare)
inline void psfm_qb_grid(PsfmQbGrid& G, const int64_t* n_q, int n_seq)
{
    int blocks = 0;
    int64_t q = 0;
    for (int b = 0; b < PSFM_QB_MAX; b++) {
        const bool in = b < n_seq;
        G.blk0[b] = blocks;
        G.q0[b] = q;
        if (in) { blocks += psfm_qb_blocks_of(n_q[b]); q += n_q[b]; }
        G.blk_end[b] = in ? blocks : INT32_MAX;
    }
    G.q0[PSFM_QB_MAX] = q;
    G.blocks = blocks;
}

// The sequence of block `blk` (0 <= blk < blocks): the number of entries of the inclusive prefix that are <= blk.  An empty sequence
// repeats its predecessor's entry and is passed over with it; the entries at and above n_seq never count.  `blk` is block-uniform
// and the 64 entries are read at constant addresses: scalar loads and scalar compares.
__host__ __device__ __forceinline__ int psfm_qb_find(const int* __restrict__ blk_end, int blk)
{
    int n = 0;
#pragma unroll
    for (int i = 0; i < PSFM_QB_MAX; i++) n += blk_end[i] <= blk ? 1 : 0;
    return n;
}

// The query thread `thread` of block `blk` owns inside sequence b (whose first block is blk0)
__host__ __device__ __forceinline__ unsigned psfm_qb_query(int blk, int blk0, unsigned thread)
{
    return (unsigned)(blk - blk0) * PSFM_QB_BLOCK + thread;
}

// The offset rule.  local: the exclusive prefix of the lengths inside the block; sum[]: the exclusive prefix of the block totals over
// ALL flattened blocks (sum[blocks]: the points of all sequences).
__host__ __device__ __forceinline__ int64_t psfm_qb_offset(int64_t local, const int64_t* sum, int blk, int blk0)
{
    return local + (sum[blk] - sum[blk0]);
}
// ... and the points of a sequence whose blocks are [blk0, blk_end): off[Q] of its CSR (0 for an empty sequence: blk_end == blk0)
__host__ __device__ __forceinline__ int64_t psfm_qb_points(const int64_t* sum, int blk0, int blk_end) { return sum[blk_end] - sum[blk0]; }

// birth and length of a query from its directions' lengths (1 for a direction that was not tracked): psfm_query_plan_kernel's rule
__host__ __device__ __forceinline__ void psfm_qb_join(int t, int nf, int nb, int* birth, int* len)
{
    *birth = t - (nb - 1);
    *len = nb + nf - 1;
}
