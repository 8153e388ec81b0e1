// Host build of the finalize gather's chunk rule (particle-sfm_amd/csrc/psfm_gather_exact.h through tests/host/shim) for
// tests/test_gather_exact_host.py: the class of a flow, the decision per chunk, and a lane-by-lane model of what a half-wave of
// psfm_gather_delta2_kernel computes for one trajectory -- its prefix sum in the kernel's order (or another), the two votes, the redo
// in the loop's order, the carry and the sticky flag -- with every decision taken by the header's functions.  Test infrastructure.
#include "psfm_gather_exact.h"

extern "C" int psfm_host_gx_class(float f) { return psfm_gx_class(f); }
extern "C" int psfm_host_gx_form(int gather_switch, int H, int W) { return psfm_gx_form(gather_switch, H, W); }
extern "C" int psfm_host_gx_in_range(double x, double y) { return psfm_gx_in_range(x, y); }

// the loop's own walk: p[0] = p0, p[t] = p[t - 1] + (double)f[t - 1]
extern "C" void psfm_host_gx_serial(const float* f, int n_points, double p0, double* p)
{
    p[0] = p0;
    for (int t = 1; t < n_points; ++t) p[t] = p[t - 1] + (double)f[t - 1];
}

// inclusive prefix sums of the 32 values of a chunk.  order 0: the kernel's -- four shifts inside rows of 16 lanes, then lane 15 of the
// lower row added to the upper one; order 1: sums of blocks of 8 from their far end, then block totals from the last block down
static void gx_prefix(const double* v, double* s, int order)
{
    const int K = PSFM_GX_CHUNK;
    if (order == 0) {
        double a[K], b[K];
        for (int i = 0; i < K; ++i) a[i] = v[i];
        for (int d = 1; d <= 8; d *= 2) {
            for (int i = 0; i < K; ++i) b[i] = a[i] + ((i & 15) >= d ? a[i - d] : 0.0);
            for (int i = 0; i < K; ++i) a[i] = b[i];
        }
        for (int i = 0; i < K; ++i) s[i] = a[i] + (i >= 16 ? a[15] : 0.0);
    } else {
        double tot[4];
        for (int blk = 0; blk < 4; ++blk) {
            for (int i = 0; i < 8; ++i) {
                double x = 0.0;
                for (int k = i; k >= 0; --k) x = v[8 * blk + k] + x;        // right to left
                s[8 * blk + i] = x;
            }
            tot[blk] = s[8 * blk + 7];
        }
        for (int blk = 3; blk >= 1; --blk) {
            double x = 0.0;
            for (int k = blk - 1; k >= 0; --k) x = tot[k] + x;
            for (int i = 0; i < 8; ++i) s[8 * blk + i] = x + s[8 * blk + i];
        }
    }
}

// One trajectory through the gather: n_points points, fx / fy the n_points - 1 flows behind its birth point (x0, y0).  Chunk by chunk
// as the half-wave does it: entries outside [1, len) are zero, blocked sum + base, the votes, psfm_gx_chunk_parallel, else the chunk
// in the loop's order; lane 31 carries position and flag.  forget_sticky: a WRONG evaluation that drops the flag between chunks (what
// the test shows to differ).  force_parallel: a WRONG evaluation that never redoes a chunk.  Returns the chunks redone serially.
extern "C" int psfm_host_gx_walk(const float* fx, const float* fy, int n_points, double x0, double y0, int order, int forget_sticky,
                                 int force_parallel, double* px, double* py)
{
    const int K = PSFM_GX_CHUNK;
    double bx = x0, by = y0;
    int sticky = 0, redone = 0;
    for (int k0 = 0; k0 < n_points; k0 += K) {
        float2 f[K];
        double vx[K], vy[K], sx[K], sy[K], qx[K], qy[K];
        int fine = 1, inr = 1;
        for (int i = 0; i < K; ++i) {
            const int t = k0 + i;
            f[i] = (t >= 1 && t < n_points) ? make_float2(fx[t - 1], fy[t - 1]) : make_float2(0.f, 0.f);
            vx[i] = (double)f[i].x; vy[i] = (double)f[i].y;
            fine &= psfm_gx_class2(f[i]);
        }
        gx_prefix(vx, sx, order);
        gx_prefix(vy, sy, order);
        for (int i = 0; i < K; ++i) {
            qx[i] = bx + sx[i]; qy[i] = by + sy[i];
            inr &= psfm_gx_in_range(qx[i], qy[i]);
        }
        const int par = force_parallel ? 1 : psfm_gx_chunk_parallel(sticky, fine, inr);
        if (!par) {
            double rx = bx, ry = by;
            for (int i = 0; i < K; ++i) { rx = rx + (double)f[i].x; ry = ry + (double)f[i].y; qx[i] = rx; qy[i] = ry; }
            ++redone;
        }
        for (int i = 0; i < K && k0 + i < n_points; ++i) { px[k0 + i] = qx[i]; py[k0 + i] = qy[i]; }
        bx = qx[K - 1]; by = qy[K - 1];
        sticky = forget_sticky ? 0 : (par ? 0 : 1);
    }
    return redone;
}
