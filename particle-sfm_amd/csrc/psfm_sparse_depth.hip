// psfm_sparse_depth.hip -- sfm/convert.py:43-104 (save_depth_pose) on the device: the observations of a COLMAP model (every keypoint
// of every registered image, with the id of its 3-D point) become one sparse depth map per image.  The per-element rules (pixel of an
// observation, depth, which observation wins a pixel, the id lookup) are psfm_sparse_depth.h; this file is the data movement:
//   fill     the maps (f64) and the winner map (u32, in the context's workspace) of the call's images are zeroed
//   winner   one lane per observation (SD_ITEMS observations per thread, SD_BLOCK apart: every load of a wave is contiguous, all of a
//            thread's loads are in flight before the first search).  Grid: (chunks of the longest image, images); a block reads its
//            image's descriptor with scalar loads.  id -> point row by a branch-free binary search in the sorted ids, the searches
//            of a thread's observations interleaved: SD_ITEMS independent loads per step (the table stays in L2 / the Infinity
//            Cache: 21 steps at 2 M points); the row is kept for the second pass; integer atomicMax of (position + 1) on the
//            observation's pixel.  An id without a point, a coordinate outside the domain and a row outside the table raise bits
//            of a flag word; the smallest missing id is kept by an integer atomicMin.
//   store    same lanes: where the winner of the pixel is this observation, gather X (24 B), depth, one 8-byte store.
// No floating-point atomics: the result does not depend on the order in which lanes arrive, two calls give identical bytes.
// Bytes per observation: 24 read + 4 written + one 4-byte atomic (winner); 20 + 4 read, and per winner 24 gathered + 8 written (store).
//
// psfm_sparse_depth_sort_ids sorts ids below 2^32 through the record sort of the finalize (psfm_sort.hip: stable, so equal ids keep
// file order); larger ids are sorted by the caller on the host and run the same kernels.
//
// The walk over points3D.bin (psfm_colmap_points3d_count / _scan) is host code in the header; the two entries never touch the GPU.
#include <vector>

#include "psfm_sparse_depth.h"
#include "psfm_internal.h"

#define SD_BLOCK 256
#define SD_ITEMS 4
#define SD_CHUNK (SD_BLOCK * SD_ITEMS)
#define SD_MAX_GRID_Y 65535
#define SD_FLAG_MISSING 1ull
#define SD_FLAG_COORD 2ull
#define SD_FLAG_ROW 4ull
#define SD_SIGN (1ull << 63)               // id ^ SD_SIGN as u64 orders like the signed id

// flag[0] bits, flag[1] smallest missing id (biased), flag[2] smallest observation index with a coordinate outside the domain
__global__ __launch_bounds__(SD_BLOCK) void sd_winner_kernel(const double2* __restrict__ obs_xy, const int64_t* __restrict__ obs_id,
                                                            const PsfmSdImage* __restrict__ img, const int64_t* __restrict__ id_sorted,
                                                            const int32_t* __restrict__ pt_row, int64_t n_pts, int64_t row_base,
                                                            unsigned* __restrict__ winner, int32_t* __restrict__ obs_row,
                                                            unsigned long long* __restrict__ flag)
{
    const PsfmSdImage d = img[blockIdx.y];
    const int64_t n = d.obs_end - d.obs_begin;
    const int64_t p0 = (int64_t)blockIdx.x * SD_CHUNK + threadIdx.x;
    if ((int64_t)blockIdx.x * SD_CHUNK >= n) return;
    int64_t id[SD_ITEMS];
    double2 xy[SD_ITEMS];
#pragma unroll
    for (int i = 0; i < SD_ITEMS; ++i) {
        const int64_t p = p0 + (int64_t)i * SD_BLOCK;
        const bool ok = p < n;
        id[i] = ok ? obs_id[d.obs_begin + p] : -1;
        xy[i] = ok ? obs_xy[d.obs_begin + p] : make_double2(0.0, 0.0);
    }
    // the searches of the thread's observations side by side: SD_ITEMS independent loads per step (psfm_sd_find, interleaved)
    int64_t base[SD_ITEMS];
#pragma unroll
    for (int i = 0; i < SD_ITEMS; ++i) base[i] = 0;
    for (int64_t m = n_pts; m > 1;) {
        const int64_t half = m >> 1;
#pragma unroll
        for (int i = 0; i < SD_ITEMS; ++i)
            if (id[i] != -1) psfm_sd_find_step(id_sorted, id[i], base[i], half);
        m -= half;
    }
#pragma unroll
    for (int i = 0; i < SD_ITEMS; ++i) {
        const int64_t p = p0 + (int64_t)i * SD_BLOCK;
        if (p >= n) continue;
        int32_t row = -1;
        if (id[i] != -1) {
            const int64_t g = psfm_sd_find_end(id_sorted, n_pts, id[i], base[i]);
            if (g >= 0) row = pt_row[g];
            if (g < 0) {
                atomicOr(&flag[0], SD_FLAG_MISSING);
                atomicMin(&flag[1], (unsigned long long)id[i] ^ SD_SIGN);
            } else if (row < 0 || (int64_t)row >= n_pts) {
                atomicOr(&flag[0], SD_FLAG_ROW);
                row = -1;
            } else if (!psfm_sd_coord_ok(xy[i].x) || !psfm_sd_coord_ok(xy[i].y)) {
                atomicOr(&flag[0], SD_FLAG_COORD);
                atomicMin(&flag[2], (unsigned long long)(d.obs_begin + p));
                row = -1;
            } else {
                const int64_t pix = d.out_off + (int64_t)psfm_sd_pixel(xy[i].y, d.h) * d.w + psfm_sd_pixel(xy[i].x, d.w);
                atomicMax(&winner[pix], (unsigned)(p + 1));
            }
        }
        obs_row[d.obs_begin + p - row_base] = row;
    }
}

__global__ __launch_bounds__(SD_BLOCK) void sd_store_kernel(const double2* __restrict__ obs_xy, const PsfmSdImage* __restrict__ img,
                                                           const double* __restrict__ pt_xyz, int64_t row_base,
                                                           const unsigned* __restrict__ winner, const int32_t* __restrict__ obs_row,
                                                           double* __restrict__ depth)
{
    const PsfmSdImage d = img[blockIdx.y];
    const int64_t n = d.obs_end - d.obs_begin;
    const int64_t p0 = (int64_t)blockIdx.x * SD_CHUNK + threadIdx.x;
    if ((int64_t)blockIdx.x * SD_CHUNK >= n) return;
    int32_t row[SD_ITEMS];
    double2 xy[SD_ITEMS];
#pragma unroll
    for (int i = 0; i < SD_ITEMS; ++i) {
        const int64_t p = p0 + (int64_t)i * SD_BLOCK;
        const bool ok = p < n;
        row[i] = ok ? obs_row[d.obs_begin + p - row_base] : -1;
        xy[i] = ok ? obs_xy[d.obs_begin + p] : make_double2(0.0, 0.0);
    }
#pragma unroll
    for (int i = 0; i < SD_ITEMS; ++i) {
        if (row[i] < 0) continue;                          // (skipped, failed, or behind the image's last observation)
        const int64_t p = p0 + (int64_t)i * SD_BLOCK;
        const int64_t pix = d.out_off + (int64_t)psfm_sd_pixel(xy[i].y, d.h) * d.w + psfm_sd_pixel(xy[i].x, d.w);
        if (winner[pix] != (unsigned)(p + 1)) continue;
        const double* X = pt_xyz + 3 * (int64_t)row[i];
        depth[pix] = psfm_sd_depth(d.r20, d.r21, d.r22, d.t2, X[0], X[1], X[2]);
    }
}

extern "C" psfm_status psfm_ctx_set_sparse_depth(psfm_ctx* c, int64_t budget_bytes, int timing)
{
    if (!c || budget_bytes < 0) { psfm_set_error("psfm_ctx_set_sparse_depth: budget_bytes must be >= 0 (0: no limit)"); return PSFM_ERR_ARG; }
    c->sd_budget = budget_bytes;
    c->sd_timing = timing != 0;
    return PSFM_OK;
}

extern "C" psfm_status psfm_ctx_get_sparse_depth_budget(psfm_ctx* c, int64_t* budget_bytes)
{
    if (!c || !budget_bytes) { psfm_set_error("psfm_ctx_get_sparse_depth_budget: NULL argument"); return PSFM_ERR_ARG; }
    *budget_bytes = c->sd_budget;
    return PSFM_OK;
}

extern "C" psfm_status psfm_sparse_depth_last_ms(psfm_ctx* c, double* ms3)
{
    if (!c || !ms3) { psfm_set_error("psfm_sparse_depth_last_ms: NULL argument"); return PSFM_ERR_ARG; }
    for (int i = 0; i < 3; ++i) ms3[i] = c->sd_ms[i];
    return PSFM_OK;
}

extern "C" psfm_status psfm_sparse_depth(psfm_ctx* c, const double* obs_xy, const int64_t* obs_id, int64_t n_obs, const void* img_desc_host,
                                         int n_img, const int64_t* pt_id_sorted, const int32_t* pt_row, const double* pt_xyz, int64_t n_pts,
                                         double* depth_out, int64_t* missing_id_host, void* stream)
{
    const char* who = "psfm_sparse_depth";
    if (!c) { psfm_set_error("ctx is NULL"); return PSFM_ERR_ARG; }
    if (missing_id_host) *missing_id_host = -1;
    if (!img_desc_host || !depth_out || n_img < 1 || n_obs < 0 || n_pts < 0 || n_pts >= (1ll << 31) ||
        (n_obs > 0 && (!obs_xy || !obs_id)) || (n_pts > 0 && (!pt_id_sorted || !pt_row || !pt_xyz))) {
        psfm_set_error("%s: bad argument (n_img=%d n_obs=%lld n_pts=%lld)", who, n_img, (long long)n_obs, (long long)n_pts);
        return PSFM_ERR_ARG;
    }
    // ---- the descriptors: every index a kernel forms from them is checked here ----
    const PsfmSdImage* img = (const PsfmSdImage*)img_desc_host;
    int64_t n_pix = 0, lo = n_obs, hi = 0, longest = 0;
    for (int i = 0; i < n_img; ++i) {
        const PsfmSdImage& d = img[i];
        if (d.obs_begin < 0 || d.obs_end < d.obs_begin || d.obs_end > n_obs || d.obs_end - d.obs_begin >= 0xffffffffll) {
            psfm_set_error("%s: image %d: observations [%lld, %lld) outside [0, %lld) or 2^32 - 1 and more", who, i, (long long)d.obs_begin,
                           (long long)d.obs_end, (long long)n_obs);
            return PSFM_ERR_ARG;
        }
        if (d.w < 1 || d.h < 1) { psfm_set_error("%s: image %d: camera of %d x %d pixels", who, i, d.w, d.h); return PSFM_ERR_ARG; }
        if (d.out_off != n_pix) {
            psfm_set_error("%s: image %d: map at element %lld, the maps of a call follow each other without gaps (expected %lld)", who, i,
                           (long long)d.out_off, (long long)n_pix);
            return PSFM_ERR_ARG;
        }
        n_pix += (int64_t)d.w * d.h;
        if (n_pix > (1ll << 40)) { psfm_set_error("%s: more than 2^40 pixels in one call", who); return PSFM_ERR_ARG; }
        if (d.obs_end > d.obs_begin) {
            if (d.obs_begin < lo) lo = d.obs_begin;
            if (d.obs_end > hi) hi = d.obs_end;
            if (d.obs_end - d.obs_begin > longest) longest = d.obs_end - d.obs_begin;
        }
        if (!(d.r20 == d.r20) || !(d.r21 == d.r21) || !(d.r22 == d.r22) || !(d.t2 == d.t2)) {
            psfm_set_error("%s: image %d: NaN in the pose", who, i);
            return PSFM_ERR_ARG;
        }
    }
    if (hi < lo) lo = hi = 0;                                         // no observation at all
    PSFM_HIP(hipSetDevice(c->device));
    PsfmGate gate(c->device, 0);
    hipStream_t s = (hipStream_t)stream;
    psfm_status st;
    // workspace: winner map | rows of the observations [lo, hi) | descriptors | flags
    const size_t a_win = ((size_t)n_pix * 4 + 255) / 256 * 256, a_row = ((size_t)(hi - lo) * 4 + 255) / 256 * 256;
    const size_t a_img = ((size_t)n_img * sizeof(PsfmSdImage) + 255) / 256 * 256;
    if ((st = c->sd_ws.ensure(a_win + a_row + a_img + 256)) != PSFM_OK) return st;
    char* w = (char*)c->sd_ws.p;
    unsigned* winner = (unsigned*)w;
    int32_t* obs_row = (int32_t*)(w + a_win);
    PsfmSdImage* img_dev = (PsfmSdImage*)(w + a_win + a_row);
    unsigned long long* flag = (unsigned long long*)(w + a_win + a_row + a_img);
    unsigned long long* h = (unsigned long long*)((char*)c->host_pinned + 416);      // [0] bits, [1] missing id, [2] observation
    hipEvent_t* ev = c->sd_events;
    const bool timing = c->sd_timing;
    if (timing) for (int i = 0; i < 4; ++i) if (!ev[i]) PSFM_HIP(hipEventCreate(&ev[i]));
    h[0] = 0; h[1] = ~0ull; h[2] = ~0ull;
    PSFM_HIP(hipMemcpyAsync(flag, h, 24, hipMemcpyHostToDevice, s));
    PSFM_HIP(hipMemcpyAsync(img_dev, img, (size_t)n_img * sizeof(PsfmSdImage), hipMemcpyHostToDevice, s));
    PSFM_HIP(hipStreamSynchronize(s));                                // (h and the caller's table may change from here on)
    if (timing) PSFM_HIP(hipEventRecord(ev[0], s));
    PSFM_HIP(hipMemsetAsync(depth_out, 0, (size_t)n_pix * 8, s));
    PSFM_HIP(hipMemsetAsync(winner, 0, (size_t)n_pix * 4, s));
    if (timing) PSFM_HIP(hipEventRecord(ev[1], s));
    const unsigned gx = (unsigned)((longest + SD_CHUNK - 1) / SD_CHUNK);
    if (gx > 0)
        for (int i0 = 0; i0 < n_img; i0 += SD_MAX_GRID_Y) {
            const unsigned gy = (unsigned)(n_img - i0 < SD_MAX_GRID_Y ? n_img - i0 : SD_MAX_GRID_Y);
            hipLaunchKernelGGL(sd_winner_kernel, dim3(gx, gy), dim3(SD_BLOCK), 0, s, (const double2*)obs_xy, obs_id, (const PsfmSdImage*)(img_dev + i0),
                               pt_id_sorted, pt_row, n_pts, lo, winner, obs_row, flag);
        }
    if (timing) PSFM_HIP(hipEventRecord(ev[2], s));
    if (gx > 0)
        for (int i0 = 0; i0 < n_img; i0 += SD_MAX_GRID_Y) {
            const unsigned gy = (unsigned)(n_img - i0 < SD_MAX_GRID_Y ? n_img - i0 : SD_MAX_GRID_Y);
            hipLaunchKernelGGL(sd_store_kernel, dim3(gx, gy), dim3(SD_BLOCK), 0, s, (const double2*)obs_xy, (const PsfmSdImage*)(img_dev + i0), pt_xyz,
                               lo, (const unsigned*)winner, (const int32_t*)obs_row, depth_out);
        }
    if (timing) PSFM_HIP(hipEventRecord(ev[3], s));
    PSFM_HIP(hipGetLastError());
    PSFM_HIP(hipMemcpyAsync(h, flag, 24, hipMemcpyDeviceToHost, s));
    PSFM_HIP(hipStreamSynchronize(s));
    if (timing)
        for (int i = 0; i < 3; ++i) {
            float ms = 0.f;
            PSFM_HIP(hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
            c->sd_ms[i] = ms;
        }
    if (h[0] & SD_FLAG_MISSING) {
        const int64_t id = (int64_t)(h[1] ^ SD_SIGN);
        if (missing_id_host) *missing_id_host = id;
        psfm_set_error("%s: an observation names 3-D point %lld, which the model does not hold", who, (long long)id);
        return PSFM_ERR_ARG;
    }
    if (h[0] & SD_FLAG_COORD) {
        psfm_set_error("%s: observation %lld has a coordinate that is not finite or does not round into int32", who, (long long)h[2]);
        return PSFM_ERR_ARG;
    }
    if (h[0] & SD_FLAG_ROW) { psfm_set_error("%s: pt_row holds a row outside [0, %lld)", who, (long long)n_pts); return PSFM_ERR_ARG; }
    return PSFM_OK;
}

// ---- ids below 2^32: the record sort ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SD_BLOCK) void sd_split_kernel(const int64_t* __restrict__ id, int64_t n, unsigned* __restrict__ key, int* __restrict__ val,
                                                           unsigned long long* __restrict__ flag)
{
    const int64_t i = (int64_t)blockIdx.x * SD_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int64_t v = id[i];
    if (v < 0 || v > 0xffffffffll) atomicOr(&flag[0], 1ull);
    key[i] = (unsigned)v;
    val[i] = (int)i;
}

__global__ __launch_bounds__(SD_BLOCK) void sd_widen_kernel(const unsigned* __restrict__ key, const int* __restrict__ val, int64_t n,
                                                           int64_t* __restrict__ id_sorted, int32_t* __restrict__ row)
{
    const int64_t i = (int64_t)blockIdx.x * SD_BLOCK + threadIdx.x;
    if (i >= n) return;
    id_sorted[i] = (int64_t)key[i];
    row[i] = val[i];
}

extern "C" psfm_status psfm_sparse_depth_sort_ids(psfm_ctx* c, const int64_t* pt_id, int64_t n_pts, int64_t* pt_id_sorted, int32_t* pt_row,
                                                  void* stream)
{
    if (!c) { psfm_set_error("ctx is NULL"); return PSFM_ERR_ARG; }
    if (n_pts < 0 || n_pts >= (1ll << 31) || (n_pts > 0 && (!pt_id || !pt_id_sorted || !pt_row))) {
        psfm_set_error("psfm_sparse_depth_sort_ids: bad argument (n_pts=%lld)", (long long)n_pts);
        return PSFM_ERR_ARG;
    }
    if (n_pts == 0) return PSFM_OK;
    PSFM_HIP(hipSetDevice(c->device));
    PsfmGate gate(c->device, 0);
    hipStream_t s = (hipStream_t)stream;
    psfm_status st;
    const int64_t n = n_pts;
    if ((st = c->sort_keys.ensure(sizeof(unsigned long long) * (size_t)n * 2)) != PSFM_OK) return st;
    if ((st = c->sort_lanes.ensure(sizeof(int) * (size_t)n * 2)) != PSFM_OK) return st;
    if ((st = c->sd_ws.ensure(256)) != PSFM_OK) return st;
    unsigned long long* flag = c->sd_ws.as<unsigned long long>();
    unsigned long long* h = (unsigned long long*)((char*)c->host_pinned + 416);
    unsigned* k0 = c->sort_keys.as<unsigned>();
    int* v0 = c->sort_lanes.as<int>();
    const unsigned grid = (unsigned)((n + SD_BLOCK - 1) / SD_BLOCK);
    PSFM_HIP(hipMemsetAsync(flag, 0, 8, s));
    hipLaunchKernelGGL(sd_split_kernel, dim3(grid), dim3(SD_BLOCK), 0, s, pt_id, n, k0, v0, flag);        // 4 passes: the input sits in half 0
    if ((st = psfm_sort_pairs32(c, k0, v0, k0 + n, v0 + n, n, 32u, s)) != PSFM_OK) return st;
    hipLaunchKernelGGL(sd_widen_kernel, dim3(grid), dim3(SD_BLOCK), 0, s, (const unsigned*)k0, (const int*)v0, n, pt_id_sorted, pt_row);
    PSFM_HIP(hipGetLastError());
    PSFM_HIP(hipMemcpyAsync(h, flag, 8, hipMemcpyDeviceToHost, s));
    PSFM_HIP(hipStreamSynchronize(s));
    if (h[0]) { psfm_set_error("psfm_sparse_depth_sort_ids: an id outside [0, 2^32): sort such ids on the host"); return PSFM_ERR_ARG; }
    return PSFM_OK;
}

// ---- points3D.bin (host only: no HIP call) ------------------------------------------------------------------------------------------
extern "C" psfm_status psfm_colmap_points3d_count(const void* buf, uint64_t nbytes, uint64_t* n)
{
    if (!n || (!buf && nbytes > 0)) { psfm_set_error("psfm_colmap_points3d_count: NULL argument"); return PSFM_ERR_ARG; }
    const int64_t bad = psfm_sd_points3d_walk((const unsigned char*)buf, nbytes, n, nullptr, nullptr, nullptr, nullptr);
    if (bad >= 0) {
        psfm_set_error("psfm_colmap_points3d_count: points3D.bin is truncated or inconsistent at record %lld (%llu bytes)", (long long)bad,
                       (unsigned long long)nbytes);
        return PSFM_ERR_ARG;
    }
    return PSFM_OK;
}

// ids_out, track_len_out (n) u64, xyz_out (n, 3) f64, err_out (n) f64, n from psfm_colmap_points3d_count of the same buffer; any may be NULL
extern "C" psfm_status psfm_colmap_points3d_scan(const void* buf, uint64_t nbytes, uint64_t* ids_out, double* xyz_out, double* err_out,
                                                 uint64_t* track_len_out)
{
    if (!buf && nbytes > 0) { psfm_set_error("psfm_colmap_points3d_scan: NULL argument"); return PSFM_ERR_ARG; }
    uint64_t n = 0;
    // first without writing: a refused file leaves the outputs untouched
    int64_t bad = psfm_sd_points3d_walk((const unsigned char*)buf, nbytes, &n, nullptr, nullptr, nullptr, nullptr);
    if (bad < 0) bad = psfm_sd_points3d_walk((const unsigned char*)buf, nbytes, &n, ids_out, xyz_out, err_out, track_len_out);
    if (bad >= 0) {
        psfm_set_error("psfm_colmap_points3d_scan: points3D.bin is truncated or inconsistent at record %lld (%llu bytes)", (long long)bad,
                       (unsigned long long)nbytes);
        return PSFM_ERR_ARG;
    }
    return PSFM_OK;
}
