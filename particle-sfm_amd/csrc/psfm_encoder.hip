// psfm_encoder.hip -- the motion classifier's trajectory transformer as one launch behind psfm_traj_augment.
//
// Reference: traj_oa_depth.joint_encoder = pt_transformer.forward, eval mode (motion_seg/core/network/traj_oa_depth.py:25-60):
// two 1x1 convolutions, nn.Transformer(16, 4 heads, 2 + 2 layers, feed-forward 64) per trajectory, max over the tokens.  torch
// runs it as well over a hundred launches that stream [L,K,16] and [L,K,64] activations through HBM; here a trajectory's whole
// state stays in registers and LDS: the launch reads the [10][K][L] features and the mask and writes [16][K].  The arithmetic is
// psfm_encoder.h.
#include "psfm_encoder.h"
#include "psfm_internal.h"
#include "psfm_window_batch.h"

#define PE_BLOCK 256
#define PE_WAVES (PE_BLOCK / 64)

// One lane per token, floor(64 / L) whole trajectories per wave (6 at L = 10: 60 of 64 lanes busy), so a trajectory never leaves
// its wave.  The per-token linear layers are per-lane FMAs against wave-uniform weights: `w` is read with uniform addresses, which
// the compiler turns into scalar loads, so the 63.5 KB of parameters never occupy vector registers or LDS.  The tokens of a
// trajectory meet in LDS: each lane owns one row of PSFM_ENC_ROW floats in its wave's slab (K | V of the attention that follows)
// and reads the L rows of its trajectory, the same address across the trajectory's lanes.  The block barriers on both sides of a
// row write keep the compiler and the hardware from moving LDS traffic across it; no wave reads another wave's slab.
// Lanes without a token (the wave's tail, trajectories past k) run token 0 of the wave's first trajectory and write nothing, so
// every lane reaches every barrier and no result depends on how trajectories are packed into waves or blocks.
// The body of both kernels: block `block` of the grid of a window of k trajectories, `slab` the block's PE_BLOCK rows in LDS.
__device__ __forceinline__ void psfm_enc_block(const float* __restrict__ features, const double* __restrict__ mask_absent,
                                               const float* __restrict__ w, int k, int L, int per_wave, float* __restrict__ out, int block,
                                               float* slab)
{
    const PsfmEncLane m = psfm_enc_lane((int)threadIdx.x, (int64_t)block, PE_WAVES, L, per_wave, k);
    const bool active = m.active;
    const int traj = m.traj, tok = m.tok;
    float* my_row = slab + m.my_row * PSFM_ENC_ROW;            // (written by active lanes only)
    const float* rows = slab + m.row0 * PSFM_ENC_ROW;          // rows [0, L) of the trajectory: inside the wave's part of the slab
    const int e = traj * L + tok;                              // < k * L
    const int64_t plane = (int64_t)k * L;
    float f[PSFM_ENC_IN];
#pragma unroll
    for (int c = 0; c < PSFM_ENC_IN; c++) f[c] = features[c * plane + e];
    const uint64_t pad = psfm_enc_pad_bits(__ballot(active && psfm_enc_padded(mask_absent, e)), m, L);

    PsfmEncTok s = {};
#pragma unroll 1
    for (int p = 0; p < PSFM_ENC_PHASES; p++) {
        psfm_enc_phase(p, s, w, f, rows, L, pad);
        __syncthreads();            // every lane has read the rows of the exchange before
        if (active) {
#pragma unroll
            for (int i = 0; i < 2 * PSFM_ENC_D; i++) my_row[i] = s.pub[i];
        }
        __syncthreads();
    }
    if (active)
        for (int c = tok; c < PSFM_ENC_D; c += L) out[(int64_t)c * k + traj] = psfm_enc_max(rows, L, c);
}

__global__ __launch_bounds__(PE_BLOCK) void psfm_traj_encode_kernel(const float* __restrict__ features, const double* __restrict__ mask_absent,
                                                                  const float* __restrict__ w, int k, int L, int per_wave,
                                                                  float* __restrict__ out)
{
    __shared__ float slab[PE_BLOCK * PSFM_ENC_ROW];
    psfm_enc_block(features, mask_absent, w, k, L, per_wave, out, (int)blockIdx.x, slab);
}

// ---- a batch of windows (psfm_traj_encode_batch) -------------------------------------------------------------------------------
// The table of windows, by value in the kernel arguments.  Blocks are numbered inside a window: window b owns blocks
// [blk0[b], blk0[b + 1]), a block finds it with psfm_winb_find and hands psfm_enc_lane the window's k and its own index inside the
// window, so the packing of trajectories into waves, and with it every bit, is that of psfm_traj_encode on the window alone.  The
// window costs scalar registers only: the table is read with block-uniform indices.
struct PsfmEncBatch {
    const float* features[PSFM_WINB_MAX];
    const double* mask_absent[PSFM_WINB_MAX];
    float* out[PSFM_WINB_MAX];
    int k[PSFM_WINB_MAX];
    int blk0[PSFM_WINB_MAX];            // INT32_MAX at and above n_win
    int L, per_wave;
};
static_assert(sizeof(PsfmEncBatch) + sizeof(const float*) <= 4096, "the table must fit the kernel arguments");

// (the weights stay a kernel argument of their own: a __restrict__ argument is what lets their loads stay scalar)
__global__ __launch_bounds__(PE_BLOCK) void psfm_traj_encode_batch_kernel(const PsfmEncBatch B, const float* __restrict__ w)
{
    __shared__ float slab[PE_BLOCK * PSFM_ENC_ROW];
    const int b = psfm_winb_find(B.blk0, (int)blockIdx.x);
    psfm_enc_block(B.features[b], B.mask_absent[b], w, B.k[b], B.L, B.per_wave, B.out[b], (int)blockIdx.x - B.blk0[b], slab);
}

extern "C" int psfm_traj_encode_weight_count(void) { return PSFM_ENC_WEIGHTS; }

extern "C" psfm_status psfm_traj_encode(psfm_ctx* c, const float* features, const double* mask_absent, const float* weights, int64_t k,
                                        int n_frames, float* out, void* stream)
{
    if (!c) { psfm_set_error("ctx is NULL"); return PSFM_ERR_ARG; }
    if (n_frames < 1 || n_frames > PSFM_ENC_MAX_L) {
        psfm_set_error("psfm_traj_encode: n_frames=%d, supported is 1 <= n_frames <= %d (one trajectory inside one wave)", n_frames, PSFM_ENC_MAX_L);
        return PSFM_ERR_ARG;
    }
    // 32-bit indices in the kernel: a feature index below 10*k*n_frames
    if (k < 0 || k > INT32_MAX / ((int64_t)PSFM_ENC_IN * n_frames)) {
        psfm_set_error("psfm_traj_encode: bad argument (k=%lld n_frames=%d)", (long long)k, n_frames);
        return PSFM_ERR_ARG;
    }
    if (k == 0) return PSFM_OK;
    if (!features || !mask_absent || !weights || !out) { psfm_set_error("psfm_traj_encode: NULL argument"); return PSFM_ERR_ARG; }
    PSFM_HIP(hipSetDevice(c->device));
    PsfmGate gate(c->device, 0);
    const int per_wave = 64 / n_frames, per_block = PE_WAVES * per_wave;
    hipLaunchKernelGGL(psfm_traj_encode_kernel, dim3((unsigned)((k + per_block - 1) / per_block)), dim3(PE_BLOCK), 0, (hipStream_t)stream,
                       features, mask_absent, weights, (int)k, n_frames, per_wave, out);
    PSFM_HIP(hipGetLastError());
    return PSFM_OK;
}

extern "C" psfm_status psfm_traj_encode_batch(psfm_ctx* c, int n_win, const float* const* features, const double* const* mask_absent,
                                              const float* weights, const int64_t* k, int n_frames, float* const* out, void* stream)
{
    if (!c) { psfm_set_error("ctx is NULL"); return PSFM_ERR_ARG; }
    if (n_win < 0 || n_win > PSFM_WINB_MAX) {
        psfm_set_error("psfm_traj_encode_batch: bad argument (n_win=%d, supported is 0 <= n_win <= %d)", n_win, PSFM_WINB_MAX);
        return PSFM_ERR_ARG;
    }
    if (n_frames < 1 || n_frames > PSFM_ENC_MAX_L) {
        psfm_set_error("psfm_traj_encode_batch: n_frames=%d, supported is 1 <= n_frames <= %d (one trajectory inside one wave)", n_frames,
                       PSFM_ENC_MAX_L);
        return PSFM_ERR_ARG;
    }
    if (n_win > 0 && !k) { psfm_set_error("psfm_traj_encode_batch: k is NULL"); return PSFM_ERR_ARG; }
    int64_t rows = 0;
    for (int b = 0; b < n_win; b++) {       // the single call's limits, per window
        if (k[b] < 0 || k[b] > INT32_MAX / ((int64_t)PSFM_ENC_IN * n_frames)) {
            psfm_set_error("psfm_traj_encode_batch: window %d: bad argument (k=%lld n_frames=%d)", b, (long long)k[b], n_frames);
            return PSFM_ERR_ARG;
        }
        rows += k[b];
    }
    if (rows == 0) return PSFM_OK;
    if (!features || !mask_absent || !weights || !out) { psfm_set_error("psfm_traj_encode_batch: NULL argument"); return PSFM_ERR_ARG; }
    for (int b = 0; b < n_win; b++)
        if (k[b] > 0 && (!features[b] || !mask_absent[b] || !out[b])) {
            psfm_set_error("psfm_traj_encode_batch: window %d: NULL pointer (k=%lld)", b, (long long)k[b]);
            return PSFM_ERR_ARG;
        }
    const int per_wave = 64 / n_frames, per_block = PE_WAVES * per_wave;
    static thread_local PsfmEncBatch B;
    static thread_local PsfmWinbOffsets O;
    psfm_winb_offsets(O, k, n_win, 1, per_block);
    if (O.blocks > INT32_MAX) { psfm_set_error("psfm_traj_encode_batch: %lld blocks exceed one launch", (long long)O.blocks); return PSFM_ERR_ARG; }
    for (int b = 0; b < PSFM_WINB_MAX; b++) {
        const bool in = b < n_win && k[b] > 0;
        B.features[b] = in ? features[b] : nullptr; B.mask_absent[b] = in ? mask_absent[b] : nullptr; B.out[b] = in ? out[b] : nullptr;
        B.k[b] = in ? (int)k[b] : 0;
        B.blk0[b] = O.blk0[b];
    }
    B.L = n_frames; B.per_wave = per_wave;
    PSFM_HIP(hipSetDevice(c->device));
    PsfmGate gate(c->device, 0);
    hipLaunchKernelGGL(psfm_traj_encode_batch_kernel, dim3((unsigned)O.blocks), dim3(PE_BLOCK), 0, (hipStream_t)stream, B, weights);
    PSFM_HIP(hipGetLastError());
    return PSFM_OK;
}
