// psfm_augment.hip -- the motion classifier's 10-channel input straight from the window tensors.
//
// Reference: traj_oa_depth.augment_traj (motion_seg/core/network/traj_oa_depth.py:72-114) behind the host glue of
// motion_seg/main_motion_segmentation.py:71-78 (ToTensor, .float(), permutes).  The reference runs about fifteen generic launches
// and materialises the back-projected point cloud of every pixel of every frame; this is one launch that reads what
// psfm_window_sample wrote (f64, (K,L) with l fastest) and writes the [1,10,K,L] fp32 tensor the transformer consumes.  The
// arithmetic is psfm_augment.h.
#include "psfm_augment.h"
#include "psfm_internal.h"

#define PA_BLOCK 256

// one thread per (track k, window frame l), l fastest: the 24 B of input per element and each of the ten plane writes are
// consecutive across a wave.  A thread computes its own point and the point of l + 1 (a second gather: the neighbour's inputs are
// the bytes the next lane reads anyway), so no result depends on how the grid is cut into waves.
__global__ __launch_bounds__(PA_BLOCK) void psfm_traj_augment_kernel(const double* __restrict__ xy_norm, const double* __restrict__ mask_absent,
                                                                   const float* __restrict__ depth, int total, int L, int h, int w,
                                                                   PsfmAugKinv K, float* __restrict__ out)
{
    const int64_t e64 = (int64_t)blockIdx.x * PA_BLOCK + threadIdx.x;
    if (e64 >= total) return;
    const int e = (int)e64;
    const int l = e % L;
    float v[PSFM_AUG_PLANES];
    psfm_aug_element(xy_norm, mask_absent, depth, e, l, L, h, w, K, v);
#pragma unroll
    for (int p = 0; p < PSFM_AUG_PLANES; p++) out[(int64_t)p * total + e] = v[p];
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
