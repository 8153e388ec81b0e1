// psfm_window_batch.h -- the windows of a sequence through ONE pass of the front end of the motion classifier
// (psfm_window_sample_batch, psfm_traj_augment_batch, psfm_traj_encode_batch): the per-element rules of the window sampler, the
// table lookup a block performs and the offsets of a plan.  Shared by the kernels (psfm_window_batch.hip, psfm_augment.hip,
// psfm_encoder.hip) and the host build of the CPU suite (tests/host/window_batch_host.cpp through tests/host/shim).
//
// The sampler's rule is per (trajectory, window) and is psfm_window_sample's (psfm_window.hip): a trajectory of the result is
// eligible for window [f0, f0 + L) when it belongs to the saved set (len >= traj_min_len) and has at least min_length (and at
// least one) observations on the window's frames.  Eligible trajectories are listed in ascending id order; a window with more than
// max_num of them keeps the max_num smallest keys psfm_winb_hash(seed, id), in key order, equal keys in ascending id order.
// Window b of a call occupies rows [row0[b], row0[b] + k[b]) of every output, so its block is a contiguous (k_b, L, .) tensor.
// Every flattened grid numbers its blocks inside a window: window b owns blocks [blk0[b], blk0[b + 1]), and a block finds its
// window by psfm_winb_find over that column, as psfm_dec_batch_find does over the first-tile column.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define PSFM_WINB_MAX 64                // windows per call: PSFM_DEC_BATCH_MAX (static_assert in psfm_window_batch.hip)
#define PSFM_WINB_BLOCK 256             // threads per block of the flattened grids (elements per block of the gather and the augment)

// observations of trajectory (birth, len) on frames [f0, f0 + L)   (psfm_overlap of psfm_window.hip)
__host__ __device__ __forceinline__ int psfm_winb_overlap(int birth, int len, int f0, int L)
{
    const int lo = birth > f0 ? birth : f0;
    const int hi = (birth + len) < (f0 + L) ? (birth + len) : (f0 + L);
    return hi > lo ? hi - lo : 0;
}

// the flag of psfm_window_flag_kernel
__host__ __device__ __forceinline__ bool psfm_winb_eligible(int birth, int len, int f0, int L, int traj_min_len, int min_length)
{
    const int ov = psfm_winb_overlap(birth, len, f0, L);
    return (len >= traj_min_len) & (ov > 0) & (ov >= min_length);
}

// the key of psfm_window_hash_kernel: splitmix64 of (seed, id)
__host__ __device__ __forceinline__ unsigned long long psfm_winb_hash(unsigned long long seed, int id)
{
    unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (unsigned long long)(id + 1);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// The window of block `blk`: the LAST entry of `first` (all 64 entries; INT32_MAX at and above n_win) that is <= blk.  The column
// never decreases, and an empty window repeats its successor's entry, so that is the number of entries <= blk, less one.  `blk` is
// block-uniform and `first` lies in the kernel arguments: 64 scalar compares.
__host__ __device__ __forceinline__ int psfm_winb_find(const int* first, int blk)
{
    int n = 0;
#pragma unroll
    for (int i = 0; i < PSFM_WINB_MAX; i++) n += first[i] <= blk ? 1 : 0;
    return n - 1;
}

// The offsets of a plan or of a flattened grid: per window its first row among the rows of all windows and its first block.
struct PsfmWinbOffsets {
    int64_t row0[PSFM_WINB_MAX + 1];    // row0[b] = sum of k[a], a < b; row0[n_win ...] = the rows of all windows
    int blk0[PSFM_WINB_MAX];            // blocks of the windows before this one; INT32_MAX at and above n_win
    int64_t blocks;                     // of all windows = the grid
};

// k[0 .. n_win), `per_block` units per block, `units_per_row` units per row (the gather and the augment: n_frames elements per row,
// 256 per block; the encoder: 1 and the trajectories of a block).  A window of k rows owns ceil(k * units_per_row / per_block) blocks.
inline void psfm_winb_offsets(PsfmWinbOffsets& O, const int64_t* k, int n_win, int64_t units_per_row, int64_t per_block)
{
    int64_t rows = 0, blocks = 0;
    for (int b = 0; b < PSFM_WINB_MAX; b++) {
        const bool in = b < n_win;
        O.row0[b] = rows;
        O.blk0[b] = in ? (int)(blocks < INT32_MAX ? blocks : INT32_MAX) : INT32_MAX;
        if (in) { rows += k[b]; blocks += (k[b] * units_per_row + per_block - 1) / per_block; }
    }
    O.row0[PSFM_WINB_MAX] = rows;
    O.blocks = blocks;
}

// the cap rule: rows of a window with `count` eligible trajectories
__host__ __device__ __forceinline__ int64_t psfm_winb_rows(int64_t count, int64_t max_num) { return count > max_num ? max_num : count; }

// data_utils.py:74-89 as psfm_window_gather_kernel applies it: pt /= (raw / target); pt /= target; clip to [0,1] -- the same two f64
// divisions, in order
__host__ __device__ __forceinline__ double psfm_winb_normalise(double v, double ratio, double target)
{
    double x = v / ratio;
    x = x / target;
    return x < 0.0 ? 0.0 : (x > 1.0 ? 1.0 : x);
}
