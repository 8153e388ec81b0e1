// psfm_depth_display.hip -- sfm/convert.py:26-41 and :95 on the device: the sparse depth maps of one psfm_sparse_depth call (f64, in
// HBM) become their display images (RGBA u8, what plt.imsave writes).  The per-element rules (inv, the percentile interpolation, the
// digits and ranks of the selection, stretch, colour index) are psfm_depth_display.h; this file is the data movement:
//   count    one lane per pixel (DD_ITEMS pixels per thread, DD_BLOCK apart), grid (chunks of the largest image, images): valid
//            pixels per image, summed per wave by shuffles, per block in LDS, one integer atomicAdd per block.  The host reads the
//            counts (the only synchronisation in the middle of the call): they size the workspace and give the ranks.
//   compact  same lanes: the bit patterns of the valid inv go into the image's part of the workspace, a block's share at a position
//            one integer atomicAdd per block hands out.  Their order depends on the order of the blocks; nothing behind it does.
//   select   8 rounds, each two launches: hist (one lane per compacted value: a value that shares the prefix of a rank adds its next
//            digit to that rank's 256-bin LDS histogram, integer atomics; non-empty bins go to the image's global histogram of the
//            round) and pick (one block per image: every rank moves one digit on; behind the last round z1 and z2).  The launch
//            boundary is the only barrier between blocks: no block waits for another.
//   colour   the maps once more: per lane DD_QUADS groups of four pixels, aligned on the ABSOLUTE pixel index (an image's first pixel
//            is only 4-byte aligned in the output), each two 16-byte loads and one 16-byte store; the up to three pixels in front of
//            an image's first group and behind its last are written one by one by the image's first block.  The table sits in LDS.
// Launches per call: 3 + 16, whatever the number of images (more than 65535 images: per 65535).  Integer atomics only: two identical
// calls give identical bytes.  Bytes: count and compact 8 per pixel each (+ 8 written per valid pixel), select 8 x 8 per valid pixel,
// colour 8 read + 4 written per pixel.
#include <vector>

#include "psfm_sparse_depth.h"
#include "psfm_depth_display.h"
#include "psfm_internal.h"

#define DD_BLOCK 256
#define DD_ITEMS 4
#define DD_CHUNK (DD_BLOCK * DD_ITEMS)
#define DD_QUADS 2
#define DD_QCHUNK (DD_BLOCK * DD_QUADS)       // groups of four pixels per block of the colour pass
#define DD_MAX_GRID_Y 65535
#define DD_HIST (PSFM_DD_RANKS * PSFM_DD_BINS)
#define DD_CNT_STRIDE 32                    // words between the counters of two images: every counter has a 128-byte line of its own

__global__ __launch_bounds__(DD_BLOCK) void dd_count_kernel(const double* __restrict__ depth, const PsfmSdImage* __restrict__ img,
                                                           unsigned* __restrict__ cnt)
{
    const PsfmSdImage d = img[blockIdx.y];
    const int64_t n_pix = (int64_t)d.w * d.h;
    if ((int64_t)blockIdx.x * DD_CHUNK >= n_pix) return;
    const int64_t p0 = (int64_t)blockIdx.x * DD_CHUNK + threadIdx.x;
    __shared__ unsigned total;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    // a lane behind the image's end reads the image's last pixel and does not count it: the loads are unconditional, so all of a
    // thread's loads are in flight before the first compare (behind a branch the compiler issues them one after the other)
    double v[DD_ITEMS];
#pragma unroll
    for (int i = 0; i < DD_ITEMS; ++i) {
        const int64_t p = p0 + (int64_t)i * DD_BLOCK;
        v[i] = depth[d.out_off + (p < n_pix ? p : n_pix - 1)];
    }
    unsigned c = 0;
#pragma unroll
    for (int i = 0; i < DD_ITEMS; ++i)
        c += (p0 + (int64_t)i * DD_BLOCK < n_pix && psfm_dd_valid(v[i])) ? 1u : 0u;
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&total, c);
    __syncthreads();
    if (threadIdx.x == 0 && total) atomicAdd(&cnt[(size_t)blockIdx.y * DD_CNT_STRIDE], total);
}

__global__ __launch_bounds__(DD_BLOCK) void dd_compact_kernel(const double* __restrict__ depth, const PsfmSdImage* __restrict__ img,
                                                             PsfmDdState* __restrict__ state, unsigned long long* __restrict__ comp)
{
    const PsfmSdImage d = img[blockIdx.y];
    const int64_t n_pix = (int64_t)d.w * d.h;
    const unsigned n = state[blockIdx.y].n;
    if (n == 0 || (int64_t)blockIdx.x * DD_CHUNK >= n_pix) return;
    const int64_t comp_off = state[blockIdx.y].comp_off;
    const int64_t p0 = (int64_t)blockIdx.x * DD_CHUNK + threadIdx.x;
    double v[DD_ITEMS];
    unsigned c = 0;
#pragma unroll
    for (int i = 0; i < DD_ITEMS; ++i) {
        const int64_t p = p0 + (int64_t)i * DD_BLOCK;
        v[i] = p < n_pix ? depth[d.out_off + p] : 0.0;
        if (psfm_dd_valid(v[i])) ++c;
    }
    // where the thread's values go: an inclusive scan over the wave, the waves' totals through LDS, the block's base by one atomic
    unsigned incl = c;
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned t = __shfl_up(incl, off);
        if (lane >= (unsigned)off) incl += t;
    }
    __shared__ unsigned wsum[DD_BLOCK / 64];
    __shared__ unsigned base;
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    unsigned before = 0, total = 0;
#pragma unroll
    for (unsigned k = 0; k < DD_BLOCK / 64; ++k) {
        if (k < wave) before += wsum[k];
        total += wsum[k];
    }
    if (threadIdx.x == 0) base = total ? atomicAdd(&state[blockIdx.y].cursor, total) : 0u;
    __syncthreads();
    unsigned pos = base + before + incl - c;
#pragma unroll
    for (int i = 0; i < DD_ITEMS; ++i)
        if (psfm_dd_valid(v[i])) {
            if (pos < n) comp[comp_off + pos] = psfm_dd_bits(psfm_dd_inv(v[i]));       // (pos < n: the map the count pass saw)
            ++pos;
        }
}

// hist: the image's PSFM_DD_RANKS x 256 counts of this round (zeroed before the call)
__global__ __launch_bounds__(DD_BLOCK) void dd_hist_kernel(const unsigned long long* __restrict__ comp, const PsfmDdState* __restrict__ state,
                                                          unsigned* __restrict__ hist, int round)
{
    const PsfmDdState s = state[blockIdx.y];
    if ((int64_t)blockIdx.x * DD_CHUNK >= (int64_t)s.n) return;
    __shared__ unsigned h[DD_HIST];
    for (int k = threadIdx.x; k < DD_HIST; k += DD_BLOCK) h[k] = 0;
    __syncthreads();
    const int64_t p0 = (int64_t)blockIdx.x * DD_CHUNK + threadIdx.x;
    unsigned long long u[DD_ITEMS];
#pragma unroll
    for (int i = 0; i < DD_ITEMS; ++i) {
        const int64_t p = p0 + (int64_t)i * DD_BLOCK;
        u[i] = p < (int64_t)s.n ? comp[s.comp_off + p] : 0ull;
    }
#pragma unroll
    for (int i = 0; i < DD_ITEMS; ++i) {
        const int64_t p = p0 + (int64_t)i * DD_BLOCK;
        if (p >= (int64_t)s.n) continue;
        const unsigned m = psfm_dd_owners(s, u[i], round), dg = psfm_dd_digit(u[i], round);
#pragma unroll
        for (int r = 0; r < PSFM_DD_RANKS; ++r)
            if (m >> r & 1u) atomicAdd(&h[r * PSFM_DD_BINS + dg], 1u);
    }
    __syncthreads();
    unsigned* g = hist + (size_t)blockIdx.y * DD_HIST;
    for (int k = threadIdx.x; k < DD_HIST; k += DD_BLOCK)
        if (h[k]) atomicAdd(&g[k], h[k]);
}

__global__ __launch_bounds__(DD_BLOCK) void dd_pick_kernel(PsfmDdState* __restrict__ state, const unsigned* __restrict__ hist, int round)
{
    __shared__ unsigned h[DD_HIST];
    const unsigned* g = hist + (size_t)blockIdx.x * DD_HIST;
    for (int k = threadIdx.x; k < DD_HIST; k += DD_BLOCK) h[k] = g[k];
    __syncthreads();
    if (threadIdx.x != 0) return;
    PsfmDdState s = state[blockIdx.x];
    if (s.n == 0) return;
    psfm_dd_advance(&s, h, round);
    state[blockIdx.x] = s;
}

__device__ __forceinline__ unsigned dd_pixel(const unsigned* table, double d, double z1, double z2) { return table[psfm_dd_index(d, z1, z2)]; }

// table: 256 entries + the bad one, a pixel's four bytes as one little-endian word
__global__ __launch_bounds__(DD_BLOCK) void dd_colour_kernel(const double* __restrict__ depth, const PsfmSdImage* __restrict__ img,
                                                            const PsfmDdState* __restrict__ state, const unsigned* __restrict__ table,
                                                            unsigned* __restrict__ rgba)
{
    const PsfmSdImage d = img[blockIdx.y];
    if (state[blockIdx.y].n == 0) return;                                 // (no image: its bytes stay what they are)
    const double z1 = state[blockIdx.y].z[0], z2 = state[blockIdx.y].z[1];
    const int64_t begin = d.out_off, end = d.out_off + (int64_t)d.w * d.h;
    const int64_t q0 = (begin + 3) >> 2, q1 = end >> 2;                  // whole groups of four: [q0, q1) in absolute group numbers
    const int64_t nq = q1 > q0 ? q1 - q0 : 0;
    const int64_t first = (int64_t)blockIdx.x * DD_QCHUNK;
    if (blockIdx.x > 0 && first >= nq) return;
    __shared__ unsigned t[PSFM_DD_BINS + 1];
    for (int k = threadIdx.x; k < PSFM_DD_BINS + 1; k += DD_BLOCK) t[k] = table[k];
    __syncthreads();
    double2 v[DD_QUADS][2];
#pragma unroll
    for (int i = 0; i < DD_QUADS; ++i) {
        const int64_t q = first + (int64_t)i * DD_BLOCK + threadIdx.x;
        if (q < nq) {
            const double2* src = (const double2*)(depth + ((q0 + q) << 2));         // 32-byte aligned
            v[i][0] = src[0];
            v[i][1] = src[1];
        }
    }
#pragma unroll
    for (int i = 0; i < DD_QUADS; ++i) {
        const int64_t q = first + (int64_t)i * DD_BLOCK + threadIdx.x;
        if (q < nq) {
            uint4 o;
            o.x = dd_pixel(t, v[i][0].x, z1, z2);
            o.y = dd_pixel(t, v[i][0].y, z1, z2);
            o.z = dd_pixel(t, v[i][1].x, z1, z2);
            o.w = dd_pixel(t, v[i][1].y, z1, z2);
            *(uint4*)(rgba + ((q0 + q) << 2)) = o;                                   // 16-byte aligned
        }
    }
    if (blockIdx.x == 0) {
        // the image's first block: the pixels in front of the first whole group (threads 0..2) and behind the last (64..66)
        const int64_t head_end = (q0 << 2) < end ? (q0 << 2) : end;
        const int64_t tail_begin = (q1 << 2) > head_end ? (q1 << 2) : head_end;
        int64_t p = -1;
        if (threadIdx.x < 3) { p = begin + threadIdx.x; if (p >= head_end) p = -1; }
        else if (threadIdx.x >= 64 && threadIdx.x < 67) { p = tail_begin + (threadIdx.x - 64); if (p >= end) p = -1; }
        if (p >= 0) rgba[p] = dd_pixel(t, depth[p], z1, z2);
    }
}

extern "C" psfm_status psfm_ctx_set_depth_display(psfm_ctx* c, int timing)
{
    if (!c) { psfm_set_error("psfm_ctx_set_depth_display: ctx is NULL"); return PSFM_ERR_ARG; }
    c->dd_timing = timing != 0;
    return PSFM_OK;
}

extern "C" psfm_status psfm_depth_display_last_ms(psfm_ctx* c, double* ms4)
{
    if (!c || !ms4) { psfm_set_error("psfm_depth_display_last_ms: NULL argument"); return PSFM_ERR_ARG; }
    for (int i = 0; i < 4; ++i) ms4[i] = c->dd_ms[i];
    return PSFM_OK;
}

extern "C" int psfm_depth_display_chunk(void) { return DD_CHUNK; }

extern "C" psfm_status psfm_depth_display(psfm_ctx* c, const double* depth, const void* img_desc_host, int n_img, double pc,
                                          const uint8_t* table_host, const uint8_t* bad_rgba_host, uint8_t* rgba_out, int64_t* n_valid_out,
                                          double* z_out, void* stream)
{
    const char* who = "psfm_depth_display";
    if (!c) { psfm_set_error("ctx is NULL"); return PSFM_ERR_ARG; }
    if (!depth || !img_desc_host || !table_host || !bad_rgba_host || !rgba_out || n_img < 1) {
        psfm_set_error("%s: NULL argument or n_img < 1 (n_img=%d)", who, n_img);
        return PSFM_ERR_ARG;
    }
    if (!(pc >= 0.0 && pc <= 100.0)) { psfm_set_error("%s: pc = %g is not in [0, 100]", who, pc); return PSFM_ERR_ARG; }
    if (((uintptr_t)depth & 15) || ((uintptr_t)rgba_out & 15)) {
        psfm_set_error("%s: depth and rgba_out must be 16-byte aligned", who);
        return PSFM_ERR_ARG;
    }
    // ---- the descriptors: every index a kernel forms from them is checked here ----
    const PsfmSdImage* img = (const PsfmSdImage*)img_desc_host;
    int64_t n_pix = 0, largest = 0;
    for (int i = 0; i < n_img; ++i) {
        const PsfmSdImage& d = img[i];
        if (d.w < 1 || d.h < 1) { psfm_set_error("%s: image %d: camera of %d x %d pixels", who, i, d.w, d.h); return PSFM_ERR_ARG; }
        if ((int64_t)d.w * d.h >= (1ll << 31)) { psfm_set_error("%s: image %d: 2^31 pixels or more", who, i); return PSFM_ERR_ARG; }
        if (d.out_off != n_pix) {
            psfm_set_error("%s: image %d: map at element %lld, the maps of a call follow each other without gaps (expected %lld)", who, i,
                           (long long)d.out_off, (long long)n_pix);
            return PSFM_ERR_ARG;
        }
        n_pix += (int64_t)d.w * d.h;
        if (n_pix > (1ll << 40)) { psfm_set_error("%s: more than 2^40 pixels in one call", who); return PSFM_ERR_ARG; }
        if ((int64_t)d.w * d.h > largest) largest = (int64_t)d.w * d.h;
    }
    PSFM_HIP(hipSetDevice(c->device));
    PsfmGate gate(c->device, 0);
    hipStream_t s = (hipStream_t)stream;
    psfm_status st;
    // workspace: counts | histograms of the 8 rounds | state | descriptors | table
    auto up = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t a_cnt = up((size_t)n_img * DD_CNT_STRIDE * 4), a_hist = up((size_t)PSFM_DD_ROUNDS * n_img * DD_HIST * 4);
    const size_t a_state = up((size_t)n_img * sizeof(PsfmDdState)), a_img = up((size_t)n_img * sizeof(PsfmSdImage));
    if ((st = c->dd_ws.ensure(a_cnt + a_hist + a_state + a_img + 2048)) != PSFM_OK) return st;
    char* w = (char*)c->dd_ws.p;
    unsigned* cnt = (unsigned*)w;
    unsigned* hist = (unsigned*)(w + a_cnt);
    PsfmDdState* state = (PsfmDdState*)(w + a_cnt + a_hist);
    PsfmSdImage* img_dev = (PsfmSdImage*)(w + a_cnt + a_hist + a_state);
    unsigned* table = (unsigned*)(w + a_cnt + a_hist + a_state + a_img);
    unsigned table_words[PSFM_DD_BINS + 1];
    memcpy(table_words, table_host, 4 * PSFM_DD_BINS);
    memcpy(table_words + PSFM_DD_BINS, bad_rgba_host, 4);
    hipEvent_t* ev = c->dd_events;
    const bool timing = c->dd_timing;
    if (timing) for (int i = 0; i < 6; ++i) if (!ev[i]) PSFM_HIP(hipEventCreate(&ev[i]));
    PSFM_HIP(hipMemcpyAsync(img_dev, img, (size_t)n_img * sizeof(PsfmSdImage), hipMemcpyHostToDevice, s));
    PSFM_HIP(hipMemcpyAsync(table, table_words, sizeof(table_words), hipMemcpyHostToDevice, s));
    PSFM_HIP(hipMemsetAsync(w, 0, a_cnt + a_hist, s));
    PSFM_HIP(hipStreamSynchronize(s));                                // (the caller's tables and table_words may change from here on)
    // ---- count ----
    const unsigned gx = (unsigned)((largest + DD_CHUNK - 1) / DD_CHUNK);
    if (timing) PSFM_HIP(hipEventRecord(ev[0], s));
    for (int i0 = 0; i0 < n_img; i0 += DD_MAX_GRID_Y) {
        const unsigned gy = (unsigned)(n_img - i0 < DD_MAX_GRID_Y ? n_img - i0 : DD_MAX_GRID_Y);
        hipLaunchKernelGGL(dd_count_kernel, dim3(gx, gy), dim3(DD_BLOCK), 0, s, depth, (const PsfmSdImage*)(img_dev + i0), cnt + (size_t)i0 * DD_CNT_STRIDE);
    }
    if (timing) PSFM_HIP(hipEventRecord(ev[1], s));
    PSFM_HIP(hipGetLastError());
    std::vector<unsigned> lines((size_t)n_img * DD_CNT_STRIDE), n_valid((size_t)n_img);
    PSFM_HIP(hipMemcpyAsync(lines.data(), cnt, lines.size() * 4, hipMemcpyDeviceToHost, s));        // (one copy, 128 bytes per image)
    PSFM_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < n_img; ++i) n_valid[i] = lines[(size_t)i * DD_CNT_STRIDE];
    std::vector<PsfmDdState> hs((size_t)n_img);
    int64_t total = 0;
    unsigned most = 0;
    for (int i = 0; i < n_img; ++i) {
        memset(&hs[i], 0, sizeof(PsfmDdState));
        psfm_dd_state_init(&hs[i], n_valid[i], pc);
        hs[i].comp_off = total;
        total += n_valid[i];
        if (n_valid[i] > most) most = n_valid[i];
        if (n_valid_out) n_valid_out[i] = n_valid[i];
        if (z_out) z_out[2 * i] = z_out[2 * i + 1] = 0.0;
    }
    for (int i = 0; i < 4; ++i) c->dd_ms[i] = 0.0;
    if (total == 0) return PSFM_OK;                                       // no image at all
    if ((st = c->dd_comp.ensure((size_t)total * 8)) != PSFM_OK) return st;
    unsigned long long* comp = c->dd_comp.as<unsigned long long>();
    PSFM_HIP(hipMemcpyAsync(state, hs.data(), (size_t)n_img * sizeof(PsfmDdState), hipMemcpyHostToDevice, s));
    PSFM_HIP(hipStreamSynchronize(s));
    // ---- compact ----
    if (timing) PSFM_HIP(hipEventRecord(ev[2], s));
    for (int i0 = 0; i0 < n_img; i0 += DD_MAX_GRID_Y) {
        const unsigned gy = (unsigned)(n_img - i0 < DD_MAX_GRID_Y ? n_img - i0 : DD_MAX_GRID_Y);
        hipLaunchKernelGGL(dd_compact_kernel, dim3(gx, gy), dim3(DD_BLOCK), 0, s, depth, (const PsfmSdImage*)(img_dev + i0), state + i0, comp);
    }
    if (timing) PSFM_HIP(hipEventRecord(ev[3], s));
    // ---- select ----
    const unsigned gs = (unsigned)(((int64_t)most + DD_CHUNK - 1) / DD_CHUNK);
    for (int round = 0; round < PSFM_DD_ROUNDS; ++round) {
        unsigned* hr = hist + (size_t)round * n_img * DD_HIST;
        for (int i0 = 0; i0 < n_img; i0 += DD_MAX_GRID_Y) {
            const unsigned gy = (unsigned)(n_img - i0 < DD_MAX_GRID_Y ? n_img - i0 : DD_MAX_GRID_Y);
            hipLaunchKernelGGL(dd_hist_kernel, dim3(gs, gy), dim3(DD_BLOCK), 0, s, (const unsigned long long*)comp, (const PsfmDdState*)(state + i0),
                               hr + (size_t)i0 * DD_HIST, round);
        }
        hipLaunchKernelGGL(dd_pick_kernel, dim3((unsigned)n_img), dim3(DD_BLOCK), 0, s, state, (const unsigned*)hr, round);
    }
    if (timing) PSFM_HIP(hipEventRecord(ev[4], s));
    // ---- colour ----
    const unsigned gc = (unsigned)((largest / 4 + DD_QCHUNK) / DD_QCHUNK);            // (at least one block: heads and tails)
    for (int i0 = 0; i0 < n_img; i0 += DD_MAX_GRID_Y) {
        const unsigned gy = (unsigned)(n_img - i0 < DD_MAX_GRID_Y ? n_img - i0 : DD_MAX_GRID_Y);
        hipLaunchKernelGGL(dd_colour_kernel, dim3(gc, gy), dim3(DD_BLOCK), 0, s, depth, (const PsfmSdImage*)(img_dev + i0),
                           (const PsfmDdState*)(state + i0), (const unsigned*)table, (unsigned*)rgba_out);
    }
    if (timing) PSFM_HIP(hipEventRecord(ev[5], s));
    PSFM_HIP(hipGetLastError());
    PSFM_HIP(hipMemcpyAsync(hs.data(), state, (size_t)n_img * sizeof(PsfmDdState), hipMemcpyDeviceToHost, s));
    PSFM_HIP(hipStreamSynchronize(s));
    if (timing) {
        const int span[4][2] = {{0, 1}, {2, 3}, {3, 4}, {4, 5}};
        for (int i = 0; i < 4; ++i) {
            float ms = 0.f;
            PSFM_HIP(hipEventElapsedTime(&ms, ev[span[i][0]], ev[span[i][1]]));
            c->dd_ms[i] = ms;
        }
    }
    if (z_out)
        for (int i = 0; i < n_img; ++i)
            if (hs[i].n) { z_out[2 * i] = hs[i].z[0]; z_out[2 * i + 1] = hs[i].z[1]; }
    return PSFM_OK;
}
