// psfm_motion_boundary.h -- the per-pixel motion-boundary rule, shared by the kernels (psfm_motion_boundary.hip) and the host build
// of the CPU suite (tests/host/motion_boundary_host.cpp through tests/host/shim).
//
// Reference: point_trajectory/trajectory.py:39-43 (motion_boundary) with utils.py:107-113 (gradient), on one (H,W,2) f32 flow map.
// Everything is f32 and every operation is rounded on its own (NumPy evaluates the expression array by array):
//   dx[y,x,c] = |f[y,x,c] - f[y,x+1,c]|  (0 in the last column)      dy[y,x,c] = |f[y,x,c] - f[y+1,x,c]|  (0 in the last row)
//   f_dx = (dx[..,0] + dx[..,1]) / 2   (np.mean over two f32 values; the halving is exact or rounds like the division: a scaling by 2)
//   motion = sqrt(f_dx*f_dx + f_dy*f_dy)      norm = sqrt(u*u + v*v)      mask = motion > float32(thres) * norm
// The comparison is strict and false for any NaN (inf - inf is one); subnormal intermediates are kept.  Every operation is spelled
// with a round-to-nearest intrinsic, so the result does not depend on the compiler's contraction settings; the square root is
// sqrtf, which the library's flags (no fast-math) and the host's libm both round correctly.
//
// In the chain step the mask is a second bilinear verdict beside the occlusion verdict (trajectory.py:51-53,60): both maps travel in
// ONE byte per pixel, the KILL MAP -- bit 0 occlusion, bit 1 motion boundary -- so that the step still gathers four bytes per
// sample (psfm_chain.h: psfm_step_finish<MB>).
#pragma once
#include "psfm_device.h"

#define PSFM_KILL_OCC 1u      // bit 0 of a kill-map byte: flow_check's occlusion verdict
#define PSFM_KILL_MB 2u       // bit 1: motion boundary

// f: the pixel's flow; fe / fs: its east / south neighbour's (ignored unless has_e / has_s: last column / last row)
__device__ __forceinline__ uint8_t psfm_mb_px(float2 f, float2 fe, bool has_e, float2 fs, bool has_s, float thres)
{
    const float dxu = has_e ? fabsf(__fsub_rn(f.x, fe.x)) : 0.0f, dxv = has_e ? fabsf(__fsub_rn(f.y, fe.y)) : 0.0f;
    const float dyu = has_s ? fabsf(__fsub_rn(f.x, fs.x)) : 0.0f, dyv = has_s ? fabsf(__fsub_rn(f.y, fs.y)) : 0.0f;
    const float gx = __fmul_rn(__fadd_rn(dxu, dxv), 0.5f), gy = __fmul_rn(__fadd_rn(dyu, dyv), 0.5f);
    const float motion = sqrtf(__fadd_rn(__fmul_rn(gx, gx), __fmul_rn(gy, gy)));
    const float norm = sqrtf(__fadd_rn(__fmul_rn(f.x, f.x), __fmul_rn(f.y, f.y)));
    return motion > __fmul_rn(thres, norm) ? 1 : 0;
}

// the same from the map: pixel (x, y) of one (H,W) float2 frame; neighbours outside the frame are never read
__device__ __forceinline__ uint8_t psfm_mb_at(const float2* __restrict__ flow, int x, int y, int H, int W, float thres)
{
    const bool has_e = x + 1 < W, has_s = y + 1 < H;
    const unsigned o = (unsigned)(y * W + x) * 8u;
    const float2 z = make_float2(0.0f, 0.0f);
    const float2 f = psfm_ld(flow, o);
    const float2 fe = has_e ? psfm_ld(flow, o + 8u) : z;
    const float2 fs = has_s ? psfm_ld(flow, o + (unsigned)W * 8u) : z;
    return psfm_mb_px(f, fe, has_e, fs, has_s, thres);
}
