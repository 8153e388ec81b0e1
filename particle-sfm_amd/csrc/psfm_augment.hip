// psfm_augment.hip -- the motion classifier's 10-channel input straight from the window tensors.
//
// Reference: traj_oa_depth.augment_traj (motion_seg/core/network/traj_oa_depth.py:72-114) behind the host glue of
// motion_seg/main_motion_segmentation.py:71-78 (ToTensor, .float(), permutes).  The reference runs about fifteen generic launches
// and materialises the back-projected point cloud of every pixel of every frame; this is one launch that reads what
// psfm_window_sample wrote (f64, (K,L) with l fastest) and writes the [1,10,K,L] fp32 tensor the transformer consumes.  The
// arithmetic is psfm_augment.h.
#include "psfm_augment.h"
#include "psfm_internal.h"
#include "psfm_window_batch.h"

#define PA_BLOCK 256
static_assert(PA_BLOCK == PSFM_WINB_BLOCK, "psfm_winb_offsets counts blocks of PSFM_WINB_BLOCK elements");

// one thread per (track k, window frame l), l fastest: the 24 B of input per element and each of the ten plane writes are
// consecutive across a wave.  A thread computes its own point and the point of l + 1 (a second gather: the neighbour's inputs are
// the bytes the next lane reads anyway), so no result depends on how the grid is cut into waves.  The body of both kernels: element
// e64 of a window of `total` = k * L elements.
__device__ __forceinline__ void psfm_aug_thread(const double* __restrict__ xy_norm, const double* __restrict__ mask_absent,
                                                const float* __restrict__ depth, int64_t e64, int total, int L, int h, int w,
                                                const PsfmAugKinv& K, float* __restrict__ out)
{
    if (e64 >= total) return;
    const int e = (int)e64;
    const int l = e % L;
    float v[PSFM_AUG_PLANES];
    psfm_aug_element(xy_norm, mask_absent, depth, e, l, L, h, w, K, v);
#pragma unroll
    for (int p = 0; p < PSFM_AUG_PLANES; p++) out[(int64_t)p * total + e] = v[p];
}

__global__ __launch_bounds__(PA_BLOCK) void psfm_traj_augment_kernel(const double* __restrict__ xy_norm, const double* __restrict__ mask_absent,
                                                                   const float* __restrict__ depth, int total, int L, int h, int w,
                                                                   PsfmAugKinv K, float* __restrict__ out)
{
    psfm_aug_thread(xy_norm, mask_absent, depth, (int64_t)blockIdx.x * PA_BLOCK + threadIdx.x, total, L, h, w, K, out);
}

// ---- a batch of windows (psfm_traj_augment_batch) ------------------------------------------------------------------------------
// The table of windows, by value in the kernel arguments.  Blocks are numbered inside a window (256 elements each): window b owns
// blocks [blk0[b], blk0[b + 1]) and a block finds it with psfm_winb_find, so what a thread computes and where it writes is what
// the same thread of psfm_traj_augment on that window alone does.  Entries at and above n_win: total = 0, blk0 = INT32_MAX.
struct PsfmAugBatch {
    const double* xy_norm[PSFM_WINB_MAX];
    const double* mask_absent[PSFM_WINB_MAX];
    const float* depth[PSFM_WINB_MAX];
    float* out[PSFM_WINB_MAX];
    int total[PSFM_WINB_MAX];           // k[b] * L
    int blk0[PSFM_WINB_MAX];
    PsfmAugKinv K;
    int L, h, w;
};
static_assert(sizeof(PsfmAugBatch) <= 4096, "the table must fit the kernel arguments");

__global__ __launch_bounds__(PA_BLOCK) void psfm_traj_augment_batch_kernel(const PsfmAugBatch B)
{
    const int b = psfm_winb_find(B.blk0, (int)blockIdx.x);
    psfm_aug_thread(B.xy_norm[b], B.mask_absent[b], B.depth[b], (int64_t)((int)blockIdx.x - B.blk0[b]) * PA_BLOCK + threadIdx.x, B.total[b],
                    B.L, B.h, B.w, B.K, B.out[b]);
}

extern "C" psfm_status psfm_traj_augment(psfm_ctx* c, const double* xy_norm, const double* mask_absent, const float* depth, int64_t k,
                                         int n_frames, int h, int w, const float* kinv_host, float* out, void* stream)
{
    if (!c) { psfm_set_error("ctx is NULL"); return PSFM_ERR_ARG; }
    // 32-bit indices in the kernel: a pixel index below h*w and an output index below 10*k*n_frames
    if (k < 0 || n_frames < 1 || h < 1 || w < 1 || (int64_t)h * w > INT32_MAX || k > INT32_MAX / ((int64_t)PSFM_AUG_PLANES * n_frames)) {
        psfm_set_error("psfm_traj_augment: bad argument (k=%lld n_frames=%d h=%d w=%d)", (long long)k, n_frames, h, w);
        return PSFM_ERR_ARG;
    }
    if (k == 0) return PSFM_OK;
    if (!xy_norm || !mask_absent || !depth || !kinv_host || !out) { psfm_set_error("psfm_traj_augment: NULL argument"); return PSFM_ERR_ARG; }
    PSFM_HIP(hipSetDevice(c->device));
    PsfmGate gate(c->device, 0);
    PsfmAugKinv K;
    for (int i = 0; i < 9; i++) K.m[i] = kinv_host[i];
    const int total = (int)(k * n_frames);
    hipLaunchKernelGGL(psfm_traj_augment_kernel, dim3((unsigned)(((int64_t)total + PA_BLOCK - 1) / PA_BLOCK)), dim3(PA_BLOCK), 0, (hipStream_t)stream,
                       xy_norm, mask_absent, depth, total, n_frames, h, w, K, out);
    PSFM_HIP(hipGetLastError());
    return PSFM_OK;
}

extern "C" psfm_status psfm_traj_augment_batch(psfm_ctx* c, int n_win, const double* const* xy_norm, const double* const* mask_absent,
                                               const float* const* depth, const int64_t* k, int n_frames, int h, int w, const float* kinv_host,
                                               float* const* out, void* stream)
{
    if (!c) { psfm_set_error("ctx is NULL"); return PSFM_ERR_ARG; }
    if (n_win < 0 || n_win > PSFM_WINB_MAX) {
        psfm_set_error("psfm_traj_augment_batch: bad argument (n_win=%d, supported is 0 <= n_win <= %d)", n_win, PSFM_WINB_MAX);
        return PSFM_ERR_ARG;
    }
    if (n_frames < 1 || h < 1 || w < 1 || (int64_t)h * w > INT32_MAX || (n_win > 0 && !k)) {
        psfm_set_error("psfm_traj_augment_batch: bad argument (n_frames=%d h=%d w=%d)", n_frames, h, w);
        return PSFM_ERR_ARG;
    }
    int64_t rows = 0;
    for (int b = 0; b < n_win; b++) {       // the single call's limits, per window
        if (k[b] < 0 || k[b] > INT32_MAX / ((int64_t)PSFM_AUG_PLANES * n_frames)) {
            psfm_set_error("psfm_traj_augment_batch: window %d: bad argument (k=%lld n_frames=%d)", b, (long long)k[b], n_frames);
            return PSFM_ERR_ARG;
        }
        rows += k[b];
    }
    if (rows == 0) return PSFM_OK;
    if (!xy_norm || !mask_absent || !depth || !kinv_host || !out) { psfm_set_error("psfm_traj_augment_batch: NULL argument"); return PSFM_ERR_ARG; }
    for (int b = 0; b < n_win; b++)
        if (k[b] > 0 && (!xy_norm[b] || !mask_absent[b] || !depth[b] || !out[b])) {
            psfm_set_error("psfm_traj_augment_batch: window %d: NULL pointer (k=%lld)", b, (long long)k[b]);
            return PSFM_ERR_ARG;
        }
    static thread_local PsfmAugBatch B;
    static thread_local PsfmWinbOffsets O;
    psfm_winb_offsets(O, k, n_win, n_frames, PA_BLOCK);
    if (O.blocks > INT32_MAX) { psfm_set_error("psfm_traj_augment_batch: %lld blocks exceed one launch", (long long)O.blocks); return PSFM_ERR_ARG; }
    for (int b = 0; b < PSFM_WINB_MAX; b++) {
        const bool in = b < n_win && k[b] > 0;
        B.xy_norm[b] = in ? xy_norm[b] : nullptr; B.mask_absent[b] = in ? mask_absent[b] : nullptr; B.depth[b] = in ? depth[b] : nullptr;
        B.out[b] = in ? out[b] : nullptr;
        B.total[b] = in ? (int)(k[b] * n_frames) : 0;
        B.blk0[b] = O.blk0[b];
    }
    for (int i = 0; i < 9; i++) B.K.m[i] = kinv_host[i];
    B.L = n_frames; B.h = h; B.w = w;
    PSFM_HIP(hipSetDevice(c->device));
    PsfmGate gate(c->device, 0);
    hipLaunchKernelGGL(psfm_traj_augment_batch_kernel, dim3((unsigned)O.blocks), dim3(PA_BLOCK), 0, (hipStream_t)stream, B);
    PSFM_HIP(hipGetLastError());
    return PSFM_OK;
}
