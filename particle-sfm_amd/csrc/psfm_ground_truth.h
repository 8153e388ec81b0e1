// psfm_ground_truth.h -- the two per-element rules that compare trajectories with ground-truth masks, shared by the kernels
// (psfm_ground_truth.hip) and the host build of the CPU suite (tests/host/ground_truth_host.cpp through tests/host/shim).
//
// EVALUATION rule.  Reference: motion_seg/eval_traj_iou.py:53-65 (grid_sample), :70 (seg_metrics' two `> 0.5`) and :107-108.  A
// labelled trajectory point (x, y) is f64; it is rounded to fp32 (:57) and sampled with the sampler of psfm_device.h (psfm_taps:
// true division by (size-1)/2, zeros padding; psfm_blend) from the frame's ground-truth mask.  The reference's mask is
// 1.0 - png[:,:,0] / 255.0 in f64 (:49) cast to fp32 (:107): a function of the PNG's byte, so the map stays u8 here -- a quarter of
// the bytes -- and is seen through a 256-entry fp32 table: tap value = table[byte], a tap outside the image = 0.  gt = sample > 0.5f,
// pred = label != 0; a point falls into one of four classes, counted per frame as integers.
//
// VOTE rule.  Reference: scripts/prepare_flyingthings3d.py:98-107 (find_traj_label).  A present point (x, y) of column j is f64; its
// pixel is (rint(y), rint(x)) -- rint rounds half to even, which is what Python's round() does to a numpy.float64: 2.5 -> 2,
// 3.5 -> 4.  label_num += gts[j][ry][rx], summed as an INTEGER WITHOUT WRAP-AROUND: the behaviour of the reference's pinned NumPy 1.21,
// where int + numpy.uint8 widens; under NumPy 2 the u8 scalar would keep its type and wrap at 256.  total_num = the number of present
// columns; label = label_num > total_num / 2 with integer division; a row without a present column gets 0.
// Deviation: a pixel outside [0,H) x [0,W) or a non-finite coordinate is never read and raises a flag (compared in f64, before any
// conversion to int).  The reference would wrap a negative index to the other side of the map and raise IndexError on one >= H.
#pragma once
#include "psfm_device.h"

#define PSFM_GT_CLASSES 4        // per frame: tp, fp, fn, tn

// ---- evaluation ---------------------------------------------------------------------------------------------------------------------
// the sample of one point from one frame's u8 mask (H, W >= 2).  `table` may live in LDS (the kernel) or in host memory.
__device__ __forceinline__ float psfm_gt_sample(const uint8_t* __restrict__ mask, const float* table, double x, double y, float cw,
                                                float ch, int H, int W)
{
    const PsfmTaps t = psfm_taps((float)x, (float)y, cw, ch, H, W);
    const PsfmTapIdx k = psfm_tap_idx(H, W, t);
    // four byte gathers from clamped (always valid) addresses, zeroed by a select afterwards: psfm_sample_mask's form
    const uint8_t bnw = psfm_ld(mask, (unsigned)k.nw), bne = psfm_ld(mask, (unsigned)k.ne);
    const uint8_t bsw = psfm_ld(mask, (unsigned)k.sw), bse = psfm_ld(mask, (unsigned)k.se);
    const float vnw = k.inw ? table[bnw] : 0.0f, vne = k.ine ? table[bne] : 0.0f;
    const float vsw = k.isw ? table[bsw] : 0.0f, vse = k.ise ? table[bse] : 0.0f;
    return psfm_blend(vnw, vne, vsw, vse, t);
}

// 0 tp, 1 fp, 2 fn, 3 tn (pred = label != 0, gt = sample > 0.5f; a NaN sample is not > 0.5)
__device__ __forceinline__ int psfm_gt_class(uint8_t label, float sample)
{
    const bool pred = label != 0, gt = sample > 0.5f;
    return pred ? (gt ? 0 : 1) : (gt ? 2 : 3);
}

// ---- vote ---------------------------------------------------------------------------------------------------------------------------
// the pixel of a present point, or false (nothing may be read) when it lies outside the map or is not finite
__device__ __forceinline__ bool psfm_gt_vote_pixel(double x, double y, int H, int W, int* rx, int* ry)
{
    const double fx = rint(x), fy = rint(y);
    if (!(fx >= 0.0 && fx < (double)W && fy >= 0.0 && fy < (double)H)) return false;      // (NaN fails every comparison)
    *rx = (int)fx; *ry = (int)fy;
    return true;
}

// one trajectory's row: xy (L,2) f64, mask_absent (L) f64 (nonzero = padded), gts (L,H,W) u8.  Returns the label; *bad is set when a
// present point could not be read (the row's label is then unspecified).
__device__ __forceinline__ uint8_t psfm_gt_vote_row(const double* __restrict__ xy, const double* __restrict__ mask_absent,
                                                    const uint8_t* __restrict__ gts, int L, int H, int W, bool* bad)
{
    int64_t label_num = 0, total_num = 0;
    const int64_t hw = (int64_t)H * W;
    for (int j = 0; j < L; j++) {
        if (mask_absent[j] != 0.0) continue;                  // (`if mask[i,j]`: NaN is padded too)
        int rx, ry;
        if (!psfm_gt_vote_pixel(xy[2 * j], xy[2 * j + 1], H, W, &rx, &ry)) { *bad = true; continue; }
        label_num += psfm_ld(gts + j * hw, (unsigned)(ry * W + rx));
        total_num += 1;
    }
    return label_num > total_num / 2 ? 1 : 0;
}
