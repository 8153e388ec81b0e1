// psfm_encoder.hip -- the motion classifier's trajectory transformer as one launch behind psfm_traj_augment.
//
// Reference: traj_oa_depth.joint_encoder = pt_transformer.forward, eval mode (motion_seg/core/network/traj_oa_depth.py:25-60):
// two 1x1 convolutions, nn.Transformer(16, 4 heads, 2 + 2 layers, feed-forward 64) per trajectory, max over the tokens.  torch
// runs it as well over a hundred launches that stream [L,K,16] and [L,K,64] activations through HBM; here a trajectory's whole
// state stays in registers and LDS: the launch reads the [10][K][L] features and the mask and writes [16][K].  The arithmetic is
// psfm_encoder.h.
#include "psfm_encoder.h"
#include "psfm_internal.h"

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
__global__ __launch_bounds__(PE_BLOCK) void psfm_traj_encode_kernel(const float* __restrict__ features, const double* __restrict__ mask_absent,
                                                                  const float* __restrict__ w, int k, int L, int per_wave,
                                                                  float* __restrict__ out)
{
    __shared__ float slab[PE_BLOCK * PSFM_ENC_ROW];
    const PsfmEncLane m = psfm_enc_lane((int)threadIdx.x, (int64_t)blockIdx.x, PE_WAVES, L, per_wave, k);
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
