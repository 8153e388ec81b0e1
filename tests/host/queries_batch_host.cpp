// HOST driver of particle-sfm_amd/csrc/psfm_query_batch.h for tests/test_queries_batch_host.py: the flattened grid of
// psfm_track_queries_batch, the lookup a block performs, and the plan + scan + offsets over the concatenation of all sequences as
// the kernels of psfm_query_batch.hip run them (block-local scan, one scan of the block totals, the add relative to the sequence's
// first block), compiled through tests/host/shim.  Test infrastructure.
#include "psfm_query_batch.h"

#include <vector>

extern "C" int psfm_host_qb_max(void) { return PSFM_QB_MAX; }
extern "C" int psfm_host_qb_block(void) { return PSFM_QB_BLOCK; }

// n_q[0 .. n_seq) -> blk_end[64], blk0[64], q0[65]; returns the blocks of all sequences
extern "C" long psfm_host_qb_grid(const long* n_q, int n_seq, int* blk_end, int* blk0, long* q0)
{
    static PsfmQbGrid G;
    int64_t n[PSFM_QB_MAX] = {0};
    for (int b = 0; b < n_seq && b < PSFM_QB_MAX; b++) n[b] = n_q[b];
    psfm_qb_grid(G, n, n_seq);
    for (int b = 0; b < PSFM_QB_MAX; b++) { blk_end[b] = G.blk_end[b]; blk0[b] = G.blk0[b]; }
    for (int b = 0; b <= PSFM_QB_MAX; b++) q0[b] = (long)G.q0[b];
    return G.blocks;
}

// every block of the grid: its sequence and the query its thread 0 owns
extern "C" void psfm_host_qb_locate(const int* blk_end, const int* blk0, int blocks, int* seq, long* first_query)
{
    for (int k = 0; k < blocks; k++) {
        seq[k] = psfm_qb_find(blk_end, k);
        first_query[k] = (long)psfm_qb_query(k, blk0[seq[k]], 0u);
    }
}

// The finish over the concatenation.  t, len_f, len_b: the queries of all sequences one behind the other (len_f / len_b NULL: that
// direction was not tracked); birth, len, off: per sequence one behind the other, off with Q[b] + 1 entries per sequence; points[b].
extern "C" void psfm_host_qb_finish(const long* n_q, int n_seq, const int* t, const int* len_f, const int* len_b, int* birth, int* len,
                                    long* off, long* points)
{
    static PsfmQbGrid G;
    int64_t n[PSFM_QB_MAX] = {0};
    for (int b = 0; b < n_seq; b++) n[b] = n_q[b];
    psfm_qb_grid(G, n, n_seq);
    std::vector<int64_t> sum((size_t)G.blocks + 1, 0);
    std::vector<long*> off_of(n_seq);
    for (int b = 0; b < n_seq; b++) off_of[b] = off + G.q0[b] + b;
    // plan: per flattened block, the prefix inside the block and the block's total
    for (int k = 0; k < G.blocks; k++) {
        const int b = psfm_qb_find(G.blk_end, k);
        int64_t run = 0;
        for (unsigned th = 0; th < PSFM_QB_BLOCK; th++) {
            const unsigned q = psfm_qb_query(k, G.blk0[b], th);
            if ((int64_t)q >= n[b]) continue;
            const int64_t g = G.q0[b] + q;
            psfm_qb_join(t[g], len_f ? len_f[g] : 1, len_b ? len_b[g] : 1, &birth[g], &len[g]);
            off_of[b][q] = (long)run;
            run += len[g];
        }
        sum[k] = run;
    }
    // scan of the block totals, in block order; the per-sequence totals
    int64_t carry = 0;
    for (int k = 0; k < G.blocks; k++) { const int64_t v = sum[k]; sum[k] = carry; carry += v; }
    sum[G.blocks] = carry;
    for (int b = 0; b < n_seq; b++) {
        points[b] = (long)psfm_qb_points(sum.data(), G.blk0[b], G.blk_end[b]);
        off_of[b][n[b]] = points[b];
    }
    // the add
    for (int k = 0; k < G.blocks; k++) {
        const int b = psfm_qb_find(G.blk_end, k);
        for (unsigned th = 0; th < PSFM_QB_BLOCK; th++) {
            const unsigned q = psfm_qb_query(k, G.blk0[b], th);
            if ((int64_t)q < n[b]) off_of[b][q] = (long)psfm_qb_offset(off_of[b][q], sum.data(), k, G.blk0[b]);
        }
    }
}
