// HOST driver of particle-sfm_amd/csrc/psfm_matches_batch.h for tests/test_matches_batch_host.py: the lookup a block of the flattened
// grids performs, the bases of the concatenation, the composed sort key and its width check, the grouping rule, and the per-element
// rules the single and the batched match-table kernels share, compiled through tests/host/shim.  Test infrastructure.
#include "psfm_matches_batch.h"

extern "C" int psfm_host_mtb_max(void) { return PSFM_MTB_MAX; }
extern "C" int psfm_host_mtb_block(void) { return PSFM_MTB_BLOCK; }

// n[0 .. n_seq) -> blk0[64], base[65]; returns the blocks of all sequences (-1: more than a launch takes)
extern "C" long psfm_host_mtb_grid(const long* n, int n_seq, long* blk0, long* base)
{
    static PsfmMtbGrid G;
    int64_t nn[PSFM_MTB_MAX] = {0}, bb[PSFM_MTB_MAX + 1];
    for (int b = 0; b < n_seq && b < PSFM_MTB_MAX; b++) nn[b] = n[b];
    psfm_mtb_grid(G, nn, n_seq);
    psfm_mtb_bases(bb, nn, n_seq);
    for (int b = 0; b < PSFM_MTB_MAX; b++) blk0[b] = G.blk0[b];
    for (int b = 0; b <= PSFM_MTB_MAX; b++) base[b] = (long)bb[b];
    return G.blocks;
}

extern "C" int psfm_host_mtb_find(const long* first, int blk)
{
    int f[PSFM_MTB_MAX];
    for (int i = 0; i < PSFM_MTB_MAX; i++) f[i] = (int)first[i];
    return psfm_mtb_find(f, blk);
}

extern "C" int psfm_host_mtb_bits(unsigned long long v) { return psfm_mtb_bits(v); }
extern "C" int psfm_host_mtb_key_bits(int n_seq, unsigned long long local_range, int* local_bits) { return psfm_mtb_key_bits(n_seq, local_range, local_bits); }
extern "C" unsigned long long psfm_host_mtb_key(int b, unsigned long long local, int local_bits) { return psfm_mtb_key(b, local, local_bits); }
extern "C" int psfm_host_mtb_key_seq(unsigned long long key, int local_bits) { return psfm_mtb_key_seq(key, local_bits); }
extern "C" unsigned long long psfm_host_mtb_key_local(unsigned long long key, int local_bits) { return key & psfm_mtb_key_mask(local_bits); }

extern "C" int psfm_host_mtb_group_end(const long* n_pts, int n, int start, long max_points, int* alone)
{
    int64_t nn[4096];
    for (int i = 0; i < n && i < 4096; i++) nn[i] = n_pts[i];
    return psfm_mtb_group_end(nn, n, start, max_points, alone);
}

// ---- the rules of one sequence ----
extern "C" long psfm_host_mt_match_count(long n, long j, int sample_k) { return (long)psfm_mt_match_count(n, j, sample_k); }

// the targets of point j of a trajectory with n kept points, in loop order; returns how many
extern "C" int psfm_host_mt_targets(long n, long j, int sample_k, long* out)
{
    int64_t reps, stride;
    psfm_mt_targets(n, sample_k, &reps, &stride);
    int m = 0;
    for (int64_t r = 0; r < reps; ++r) if (r * stride != j) out[m++] = (long)(r * stride);
    return m;
}

extern "C" void psfm_host_mt_owner(const long* off, long k, long n_pts, int* owner)
{
    static_assert(sizeof(long) == sizeof(int64_t), "LP64");
    for (long p = 0; p < n_pts; p++) owner[p] = psfm_mt_owner((const int64_t*)off, k, p);
}

extern "C" unsigned psfm_host_mt_frame_index(int f, int n_img, int* outside)
{
    bool o;
    const unsigned r = psfm_mt_frame_index(f, n_img, &o);
    *outside = o ? 1 : 0;
    return r;
}

extern "C" long psfm_host_mt_lower_bound(const unsigned long long* key, long lo, long hi, unsigned long long mask, unsigned long long v)
{
    return (long)psfm_mt_lower_bound<unsigned long long>(key, lo, hi, mask, v);
}
