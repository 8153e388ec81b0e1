// psfm_sparse_depth.h -- the per-element rules that turn a COLMAP model (images.bin / points3D.bin) into the sparse depth maps of
// sfm/convert.py:43-104 (save_depth_pose), shared by the kernels (psfm_sparse_depth.hip) and the host build of the CPU suite
// (tests/host/sparse_depth_host.cpp through tests/host/shim); and the bounds-checked walk over points3D.bin
// (sfm/colmap_utils/read_write_model.py:336-363), which is host code only.
//
// PIXEL rule (convert.py:88-90).  x_pix = clip(int32(np.round(x)), 0, w - 1), y_pix the same with h; np.round is round-half-to-even
// (rint in the default rounding mode: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, -0.5 -> -0).  The pixel comes from the model's xys, never from the
// projection.  DOMAIN: finite, |v| < 2^31 and rint(v) < 2^31 -- exactly the values whose rounded coordinate int32 holds; outside it
// the reference's astype(np.int32) is platform-defined, here psfm_sd_coord_ok is false and the call fails (PSFM_ERR_ARG).  The clip is
// done in f64 before the conversion, so no conversion ever overflows.
//
// DEPTH rule (convert.py:86-87).  The reference forms (K @ (R @ X + t))[2] with K's third row (0, 0, 1): for finite input that is
// R[2,:] . X + t[2] (the two zero products add +-0 to a finite sum).  BLAS picks the reference's summation order; ONE order is fixed
// here:  depth = ((r20 * X + r21 * Y) + r22 * Z) + t2, every product and sum rounded once (no FMA: built with -ffp-contract=off, and
// written with the _rn intrinsics on the device so that it does not depend on the flag).  |depth - reference| <= 4 * 2^-53 *
// (|r20 X| + |r21 Y| + |r22 Z| + |t2|) in any order, with or without FMA.
//
// WHICH observations (convert.py:75-80).  point3D_id == -1 is skipped; the others keep their order in the image's point list.
//
// DUPLICATE pixels (convert.py:91).  depth[ys, xs] = values assigns in order: the LAST observation of a pixel wins.  The winner of a
// pixel is the largest (position + 1) among its observations, position = index in the image's point list: an integer maximum, the
// same whatever order the lanes arrive in.  0 = nobody: such a pixel holds 0.0.
//
// ID lookup (convert.py:79).  points3D[idx]: ids sorted ascending (stable: equal ids keep file order), the row of an id is the LAST
// entry with that id -- the one a dict built in file order ends up holding.  An id that names no point is an error (KeyError there).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// one image of a launch: observations [obs_begin, obs_end) of the concatenated lists, row 2 of R and t[2], the camera's size, and
// where the image's (h, w) map begins in the output (in elements)
struct PsfmSdImage {
    int64_t obs_begin, obs_end;
    double r20, r21, r22, t2;
    int32_t w, h;
    int64_t out_off;
};

__device__ __forceinline__ bool psfm_sd_coord_ok(double v)
{
    return fabs(v) < 2147483648.0 && rint(v) < 2147483648.0;       // (false for NaN and +-inf)
}

// v inside the domain; n = w or h, 1 <= n < 2^31
__device__ __forceinline__ int32_t psfm_sd_pixel(double v, int32_t n)
{
    double r = rint(v);
    const double hi = (double)(n - 1);
    r = r < 0.0 ? 0.0 : r;
    r = r > hi ? hi : r;
    return (int32_t)r;
}

__device__ __forceinline__ double psfm_sd_depth(double r20, double r21, double r22, double t2, double X, double Y, double Z)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(r20, X), __dmul_rn(r21, Y)), __dmul_rn(r22, Z)), t2);
#else
    return ((r20 * X + r21 * Y) + r22 * Z) + t2;
#endif
}

// The search for the first entry above `id` in the ascending ids is branch-free with a trip count that depends on n_pts alone, so
// that a thread can run several searches side by side, one load of each per step (psfm_sparse_depth.hip): the answer stays inside
// [base, base + n], n -> n - n / 2 per step.
__device__ __forceinline__ void psfm_sd_find_step(const int64_t* __restrict__ id_sorted, int64_t id, int64_t& base, int64_t half)
{
    if (id_sorted[base + half - 1] <= id) base += half;
}

// behind the steps (n is 1, or 0 for an empty table): position of `id` (the last entry among equal ids), -1 when no point has that id
__device__ __forceinline__ int64_t psfm_sd_find_end(const int64_t* __restrict__ id_sorted, int64_t n_pts, int64_t id, int64_t base)
{
    if (n_pts > 0 && id_sorted[base] <= id) base += 1;
    return base > 0 && id_sorted[base - 1] == id ? base - 1 : -1;
}

__device__ __forceinline__ int64_t psfm_sd_find(const int64_t* __restrict__ id_sorted, int64_t n_pts, int64_t id)
{
    int64_t base = 0;
    for (int64_t n = n_pts; n > 1;) {
        const int64_t half = n >> 1;
        psfm_sd_find_step(id_sorted, id, base, half);
        n -= half;
    }
    return psfm_sd_find_end(id_sorted, n_pts, id, base);
}

// ---- points3D.bin (host only) ---------------------------------------------------------------------------------------------------
// u64 count, then per point: u64 id, 3 x f64 xyz, 3 x u8 rgb, f64 error (43 bytes), u64 track length L, L x (i32 image, i32 point2D).
// Record k starts where record k - 1 ended: a sequential chain.  Every read is checked against nbytes BEFORE it happens, with
// subtractions on the remaining byte count (no offset + length sum that could wrap).  A file must hold exactly the records its count
// announces and nothing behind them: a buffer cut anywhere, record boundaries included, is refused.  Returns -1 when the file is
// consistent, else the index of the record at which the walk stopped (0 when the count itself is cut; the count when bytes trail).
#include <string.h>

#define PSFM_SD_POINT_HEAD 43

static inline int64_t psfm_sd_points3d_walk(const unsigned char* buf, uint64_t nbytes, uint64_t* n_out, uint64_t* ids, double* xyz,
                                            double* err, uint64_t* track_len)
{
    *n_out = 0;
    if (nbytes < 8) return 0;
    uint64_t n;
    memcpy(&n, buf, 8);
    uint64_t pos = 8, left = nbytes - 8;
    if (n > left / (PSFM_SD_POINT_HEAD + 8)) return 0;              // more records than the bytes could hold (and n * 51 cannot wrap)
    for (uint64_t k = 0; k < n; ++k) {
        if (left < PSFM_SD_POINT_HEAD + 8) return (int64_t)k;
        uint64_t len;
        memcpy(&len, buf + pos + PSFM_SD_POINT_HEAD, 8);
        const uint64_t rest = left - (PSFM_SD_POINT_HEAD + 8);
        if (len > rest / 8) return (int64_t)k;
        if (ids) memcpy(ids + k, buf + pos, 8);
        if (xyz) memcpy(xyz + 3 * k, buf + pos + 8, 24);
        if (err) memcpy(err + k, buf + pos + 35, 8);
        if (track_len) track_len[k] = len;
        pos += PSFM_SD_POINT_HEAD + 8 + 8 * len;
        left = rest - 8 * len;
    }
    if (left != 0) return (int64_t)n;
    *n_out = n;
    return -1;
}
