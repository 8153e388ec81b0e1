// HOST driver of particle-sfm_amd/csrc/psfm_sparse_depth.h for tests/test_sparse_depth_host.py: the per-element rules of the kernels of
// psfm_sparse_depth.hip (sfm/convert.py:43-104) compiled through tests/host/shim, with plain loops where the kernels have threads and
// a plain maximum where they have an integer atomicMax; and the walk over points3D.bin, which is the library's own host code.
// Built with -ffp-contract=off.  Test infrastructure.
#include "psfm_sparse_depth.h"

extern "C" void psfm_host_sd_pixels(const double* v, long n, int size, int32_t* pix, uint8_t* ok)
{
    for (long i = 0; i < n; i++) {
        ok[i] = psfm_sd_coord_ok(v[i]) ? 1 : 0;
        pix[i] = ok[i] ? psfm_sd_pixel(v[i], size) : -1;
    }
}

// the two passes of the device over the images of `img`; returns 0, 1 (an id without a point: *missing = the smallest), 2 (coordinate)
extern "C" int psfm_host_sd_maps(const double* obs_xy, const int64_t* obs_id, const PsfmSdImage* img, int n_img, const int64_t* id_sorted,
                                 const int32_t* pt_row, const double* pt_xyz, int64_t n_pts, uint32_t* winner, double* depth, int64_t* missing)
{
    int status = 0;
    for (int k = 0; k < n_img; k++) {
        const PsfmSdImage d = img[k];
        for (int64_t q = 0; q < (int64_t)d.w * d.h; q++) { winner[d.out_off + q] = 0; depth[d.out_off + q] = 0.0; }
        for (int pass = 0; pass < 2; pass++)
            for (int64_t p = 0; p < d.obs_end - d.obs_begin; p++) {
                const int64_t id = obs_id[d.obs_begin + p];
                if (id == -1) continue;
                const int64_t g = psfm_sd_find(id_sorted, n_pts, id);
                if (g < 0) {
                    if (status != 1 || id < *missing) *missing = id;
                    status = 1;
                    continue;
                }
                const double x = obs_xy[2 * (d.obs_begin + p)], y = obs_xy[2 * (d.obs_begin + p) + 1];
                if (!psfm_sd_coord_ok(x) || !psfm_sd_coord_ok(y)) { if (status == 0) status = 2; continue; }
                const int64_t pix = d.out_off + (int64_t)psfm_sd_pixel(y, d.h) * d.w + psfm_sd_pixel(x, d.w);
                if (pass == 0) {
                    if (winner[pix] < (uint32_t)(p + 1)) winner[pix] = (uint32_t)(p + 1);
                } else if (winner[pix] == (uint32_t)(p + 1)) {
                    const double* X = pt_xyz + 3 * (int64_t)pt_row[g];
                    depth[pix] = psfm_sd_depth(d.r20, d.r21, d.r22, d.t2, X[0], X[1], X[2]);
                }
            }
    }
    return status;
}

// >= 0: the record at which the walk stopped; -1: consistent, *n records
extern "C" long psfm_host_sd_points3d(const unsigned char* buf, unsigned long nbytes, uint64_t* n, uint64_t* ids, double* xyz, double* err,
                                      uint64_t* track_len)
{
    uint64_t m = 0;
    long bad = (long)psfm_sd_points3d_walk(buf, nbytes, &m, nullptr, nullptr, nullptr, nullptr);
    if (bad < 0 && (ids || xyz || err || track_len)) bad = (long)psfm_sd_points3d_walk(buf, nbytes, &m, ids, xyz, err, track_len);
    *n = m;
    return bad;
}
