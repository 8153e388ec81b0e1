// psfm_augment.h -- the per-element arithmetic of the motion classifier's input step, shared by the kernel
// (psfm_augment.hip) and the host build of the CPU suite (tests/host/augment_host.cpp through tests/host/shim).
//
// Reference: motion_seg/core/network/traj_oa_depth.py:72-114 -- image_grid, depth_project, gather_point, augment_traj.  The
// reference back-projects EVERY pixel of every frame (depth * K_inv.bmm(grid), a [B,3,H,W,L] tensor) and then gathers N*L points
// from it; here a window element computes the one point under its trajectory.  Every operation is an individually rounded fp32
// operation in the reference's order (no FMA: a fused ray differs by 1 ulp in the 3-D channels), so the result is the reference's
// bit for bit.  Kept quirks of gather_point (:97-98): tx == 1.0 gives column w, i.e. the first pixel of the next row; ty == 1.0
// leaves the image and is clamped to the last pixel; a padded slot has coordinates 0 and carries the 3-D point of pixel 0.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define PSFM_AUG_PLANES 10

struct PsfmAugKinv { float m[9]; };   // K^-1 of image_grid (:78-82), row-major

struct PsfmAugPoint { float tx, ty, m, p0, p1, p2; };

// float -> int, truncating toward zero like torch's .to(torch.int) on the values finite flows produce ([0, h] and [0, w]); defined
// for everything else too (saturating, NaN -> 0), so that no index is formed from an undefined conversion
__device__ __forceinline__ int psfm_aug_trunc(float v)
{
    if (!(v > -2147483648.0f)) return v != v ? 0 : INT32_MIN;
    if (!(v < 2147483648.0f)) return INT32_MAX;
    return (int)v;
}

// gather_point (:97-98): (int)(ty * h) * w + (int)(tx * w), clamped to [0, h*w - 1]; formed in 64 bits, it cannot overflow
__device__ __forceinline__ int psfm_aug_pixel(float tx, float ty, int h, int w)
{
    const int iy = psfm_aug_trunc(__fmul_rn(ty, (float)h)), ix = psfm_aug_trunc(__fmul_rn(tx, (float)w));
    const int64_t idx = (int64_t)iy * w + ix, last = (int64_t)h * w - 1;
    return (int)(idx < 0 ? 0 : (idx > last ? last : idx));
}

// window element e = k * L + l: the .float() casts of main_motion_segmentation.py:75-77 and the back-projected point under it
// (depth_project :84-90 at the gathered pixel only)
__device__ __forceinline__ PsfmAugPoint psfm_aug_point(const double* __restrict__ xy_norm, const double* __restrict__ mask_absent,
                                                       const float* __restrict__ depth, int e, int l, int h, int w, const PsfmAugKinv& K)
{
    PsfmAugPoint o;
    o.tx = (float)xy_norm[2 * (int64_t)e];
    o.ty = (float)xy_norm[2 * (int64_t)e + 1];
    o.m = (float)mask_absent[e];
    const int idx = psfm_aug_pixel(o.tx, o.ty, h, w);
    const int py = idx / w, px = idx - py * w;
    const float d = depth[(int64_t)l * h * w + idx];
    const float fx = (float)px, fy = (float)py;
    const float r0 = __fadd_rn(__fadd_rn(__fmul_rn(K.m[0], fx), __fmul_rn(K.m[1], fy)), K.m[2]);
    const float r1 = __fadd_rn(__fadd_rn(__fmul_rn(K.m[3], fx), __fmul_rn(K.m[4], fy)), K.m[5]);
    const float r2 = __fadd_rn(__fadd_rn(__fmul_rn(K.m[6], fx), __fmul_rn(K.m[7], fy)), K.m[8]);
    o.p0 = __fmul_rn(d, r0); o.p1 = __fmul_rn(d, r1); o.p2 = __fmul_rn(d, r2);
    return o;
}

// augment_traj (:109-112): (v[l+1] - v[l]) * (1 - mask[l+1]) -- only the LATER frame's mask gates a motion
__device__ __forceinline__ float psfm_aug_motion(float v0, float v1, float m1)
{
    return __fmul_rn(__fsub_rn(v1, v0), __fsub_rn(1.0f, m1));
}

// the ten planes of element (k, l) of a window of L frames, in the order of the torch.cat of :113
__device__ __forceinline__ void psfm_aug_element(const double* __restrict__ xy_norm, const double* __restrict__ mask_absent,
                                                 const float* __restrict__ depth, int e, int l, int L, int h, int w, const PsfmAugKinv& K,
                                                 float out[PSFM_AUG_PLANES])
{
    const PsfmAugPoint a = psfm_aug_point(xy_norm, mask_absent, depth, e, l, h, w, K);
    out[0] = a.tx; out[1] = a.ty; out[4] = a.p0; out[5] = a.p1; out[6] = a.p2;
    out[2] = out[3] = out[7] = out[8] = out[9] = 0.0f;
    if (l + 1 < L) {     // (the last frame of a trajectory's row never reads the next row)
        const PsfmAugPoint b = psfm_aug_point(xy_norm, mask_absent, depth, e + 1, l + 1, h, w, K);
        out[2] = psfm_aug_motion(a.tx, b.tx, b.m); out[3] = psfm_aug_motion(a.ty, b.ty, b.m);
        out[7] = psfm_aug_motion(a.p0, b.p0, b.m); out[8] = psfm_aug_motion(a.p1, b.p1, b.m); out[9] = psfm_aug_motion(a.p2, b.p2, b.m);
    }
}
