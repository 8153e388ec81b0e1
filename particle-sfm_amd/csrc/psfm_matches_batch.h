// psfm_matches_batch.h -- the saved sets and the match tables of all sequences of a batch through ONE pass
// (psfm_result_filter_batch, psfm_traj_to_matches_batch, psfm_labels_to_matches_batch): the per-element rules the single kernels
// (psfm_matches.hip) and the batched kernels (psfm_matches_batch.hip) share, the lookup a block of a flattened grid performs, the
// bases of the concatenated arrays, the composed sort key and the grouping rule.  Also compiled for the host by the CPU suite
// (tests/host/matches_batch_host.cpp through tests/host/shim).
//
// The pipeline is the one of the header comment of psfm_matches.hip, run once over the concatenation of the sequences: sequence b
// owns elements [base[b], base[b + 1]) of every concatenated array and blocks [blk0[b], blk0[b + 1]) of every flattened grid, so
// the sequence is block-uniform.  Counts are one global scan; a sequence reads it at its bases and subtracts.  The two sorts carry
// the sequence above the key -- (b, frame) and (b, src * n_img[b] + tgt) -- and are stable, so inside a sequence the order is the
// single call's; what is stored (pair_key, pair_off, pair_first, keypoint indices) is sequence-local.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define PSFM_MTB_MAX 64                 // sequences per call: PSFM_BATCH_MAX (static_assert in psfm_matches_batch.hip)
#define PSFM_MTB_BLOCK 256              // threads per block = elements per block of every flattened grid

// ---- rules of one sequence (psfm_matches.hip and psfm_matches_batch.hip) ----------------------------------------------------

// owner trajectory of flat point p: the last t with off[t] <= p   (off[0] <= p < off[k])
__host__ __device__ __forceinline__ int psfm_mt_owner(const int64_t* off, int64_t k, int64_t p)
{
    int64_t lo = 0, hi = k;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (off[mid] <= p) lo = mid; else hi = mid;
    }
    return (int)lo;
}

// frame of point p of trajectory t: explicit frames (the labelled set) or birth + offset (the saved set)
__host__ __device__ __forceinline__ int psfm_mt_frame(const int* frames, const int* birth, const int64_t* off, int t, int64_t p)
{
    return frames ? frames[p] : birth[t] + (int)(p - off[t]);
}

// a frame outside the image list is flagged and filed under frame 0: never used as an index
__host__ __device__ __forceinline__ unsigned psfm_mt_frame_index(int f, int n_img, bool* outside)
{
    *outside = f < 0 || f >= n_img;
    return *outside ? 0u : (unsigned)f;
}

// matches point j of a trajectory with n kept points emits (matches_from_flow.py:83-101)
__host__ __device__ __forceinline__ int64_t psfm_mt_match_count(int64_t n, int64_t j, int sample_k)
{
    if (n <= sample_k) return n - 1;
    const int64_t stride = n / sample_k;
    return sample_k - ((j % stride == 0 && j / stride < sample_k) ? 1 : 0);
}

// ... and its targets: `reps` candidates `stride` apart, itself skipped
__host__ __device__ __forceinline__ void psfm_mt_targets(int64_t n, int sample_k, int64_t* reps, int64_t* stride)
{
    *reps = n <= sample_k ? n : sample_k;
    *stride = n <= sample_k ? 1 : n / sample_k;
}

// first s in [lo, hi) with (key[s] & mask) >= v: the frame-sorted keys of one sequence
template <class K>
__host__ __device__ __forceinline__ int64_t psfm_mt_lower_bound(const K* key, int64_t lo, int64_t hi, K mask, K v)
{
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((key[mid] & mask) < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// ---- rules of the saved set (psfm_window.hip: psfm_result_filter, and psfm_matches_batch.hip) ---------------------------------------

// main_connect_point_trajectories.py:56-61: a trajectory is saved when it has at least traj_min_len points
__host__ __device__ __forceinline__ bool psfm_flt_keep(int len, int min_len) { return len >= min_len; }

// kept trajectory r of a set is trajectory id of the result: its birth and length, and its length as the scan's input
__host__ __device__ __forceinline__ void psfm_flt_meta(int id, int64_t r, const int* birth, const int* len, int* birth_out, int* len_out,
                                                       int64_t* len64)
{
    const int ln = len[id];
    birth_out[r] = birth[id];
    len_out[r] = ln;
    len64[r] = (int64_t)ln;
}

// one wave copies the run of a kept trajectory: lane, lane + lanes, ...
__host__ __device__ __forceinline__ void psfm_flt_copy_run(const double2* xy, int64_t src, double2* xy_out, int64_t dst, int n, int lane, int lanes)
{
    for (int j = lane; j < n; j += lanes) xy_out[dst + j] = xy[src + j];
}

// ---- the batch ---------------------------------------------------------------------------------------------------------------

// One sequence of a call, in device memory (64 of them do not fit the kernel arguments).  Sources first; the bases into the
// concatenated arrays and the destinations in the sequence's own context are filled in as the host learns the sizes.
struct PsfmMtbSeq {
    const int64_t* off; const int* birth; const int* frames; const double2* xy; const uint8_t* labels;
    int64_t k, n_pts;
    int n_img, pad;
    int64_t pts0, kept0, m0;            // first point, first kept point, first match of the sequence in the concatenation
    int64_t n_kept, n_m, n_pairs;
    int64_t* kp_off; double2* kp_xy; int2* rows; int64_t* pairs;
};

// One context of a filter call.
struct PsfmFltbSeq {
    const int* birth; const int* len; const int64_t* off; const double2* xy;      // the result
    int64_t n;                          // its trajectories
    int64_t src0, kept0;                // first trajectory, first kept trajectory in the concatenation
    int64_t k;                          // kept trajectories
    int* ids; int* birth_out; int* len_out; int64_t* off_out;          // (xy_out is sized last and travels in the kernel arguments)
};

// The sequence of block `blk`: the LAST entry of `first` (all 64 entries; INT32_MAX at and above n_seq) that is <= blk.  The column
// never decreases and an empty sequence repeats its successor's entry, so that is the number of entries <= blk, less one.  `blk` is
// block-uniform and `first` lies in the kernel arguments: 64 scalar compares.
__host__ __device__ __forceinline__ int psfm_mtb_find(const int* first, int blk)
{
    int n = 0;
#pragma unroll
    for (int i = 0; i < PSFM_MTB_MAX; i++) n += first[i] <= blk ? 1 : 0;
    return n - 1;
}

// A flattened grid: sequence b with n[b] elements owns ceil(n[b] / 256) blocks, numbered inside the sequence.
struct PsfmMtbGrid {
    int blk0[PSFM_MTB_MAX];             // blocks of the sequences before this one; INT32_MAX at and above n_seq
    int blocks;                         // of all sequences = the grid; -1: more than INT32_MAX
};

inline void psfm_mtb_grid(PsfmMtbGrid& G, const int64_t* n, int n_seq)
{
    int64_t blocks = 0;
    for (int b = 0; b < PSFM_MTB_MAX; b++) {
        const bool in = b < n_seq;
        G.blk0[b] = in ? (int)(blocks < INT32_MAX ? blocks : INT32_MAX) : INT32_MAX;
        if (in) blocks += (n[b] + PSFM_MTB_BLOCK - 1) / PSFM_MTB_BLOCK;
    }
    G.blocks = blocks < INT32_MAX ? (int)blocks : -1;
}

// base[b] = sum of n[a], a < b; base[n_seq ...] = the elements of all sequences
inline void psfm_mtb_bases(int64_t* base /*[65]*/, const int64_t* n, int n_seq)
{
    int64_t sum = 0;
    for (int b = 0; b <= PSFM_MTB_MAX; b++) {
        base[b] = sum;
        if (b < n_seq) sum += n[b];
    }
}

// bits needed for values < v
__host__ __device__ __forceinline__ int psfm_mtb_bits(unsigned long long v)
{
    int b = 1;
    while (b < 64 && (1ull << b) < v) ++b;
    return b;
}

// The composed key: the sequence above `local_bits` bits of the sequence's own key.
__host__ __device__ __forceinline__ unsigned long long psfm_mtb_key(int b, unsigned long long local, int local_bits)
{
    return ((unsigned long long)b << local_bits) | local;
}
__host__ __device__ __forceinline__ int psfm_mtb_key_seq(unsigned long long key, int local_bits) { return (int)(key >> local_bits); }
__host__ __device__ __forceinline__ unsigned long long psfm_mtb_key_mask(int local_bits) { return (1ull << local_bits) - 1ull; }

// Bits of the composed key over keys < local_range in n_seq sequences; 0: it does not fit 64 bits (the shift of psfm_mtb_key needs
// local_bits < 64 as well, so a 64-bit local key is refused even for one sequence).  One sequence spends no bit on the sequence:
// its composed key is the local key, and the sorts run over the bits the single calls sort (psfm_matches.hip).
inline int psfm_mtb_key_bits(int n_seq, unsigned long long local_range, int* local_bits)
{
    const int lb = psfm_mtb_bits(local_range), sb = n_seq > 1 ? psfm_mtb_bits((unsigned long long)n_seq) : 0;
    *local_bits = lb;
    if (lb >= 64 || (local_range > 1 && (1ull << lb) < local_range)) return 0;
    return lb + sb <= 64 ? lb + sb : 0;
}

// The grouping rule of the callers: consecutive groups of at most 64 sequences and at most max_points points.  Returns the end of
// the group that starts at `start`; *alone = 1 when that is one sequence above the cap (it goes through the single entry points).
inline int psfm_mtb_group_end(const int64_t* n_pts, int n, int start, int64_t max_points, int* alone)
{
    *alone = 0;
    if (start >= n) return n;
    if (n_pts[start] > max_points) { *alone = 1; return start + 1; }
    int64_t sum = 0;
    int e = start;
    while (e < n && e - start < PSFM_MTB_MAX && n_pts[e] <= max_points && sum + n_pts[e] <= max_points) sum += n_pts[e++];
    return e;
}
