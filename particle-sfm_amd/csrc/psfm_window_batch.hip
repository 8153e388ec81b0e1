// psfm_window_batch.hip -- psfm_window_sample for all windows of one context in ONE pass: psfm_window_sample_batch.
//
// psfm_window_sample (psfm_window.hip) selects one window per call and is called twice per window (count, then fill): two passes
// over all trajectories, two compactions, above the cap two hashes and two 64-bit sorts, three stream synchronisations.  Here one
// PLAN selects for up to 64 windows at once and is kept in the context, and a FILL is one gather launch over the rows of all windows:
//   count    one pass over the trajectories; per (window, block) the number of eligible trajectories (ballots, no atomics)
//   scan     one exclusive scan over the window-major (window, block) counts: the place of every block's first eligible trajectory
//            in the concatenated pre-cap lists, and with it every window's count
//   -- the ONE synchronisation: the windows' first rows come to the host; k[b] = min(count[b], max_num_tracks) --
//   compact  the same pass again writes the eligible ids of every window, ascending, at the scanned places
//   cap      per window above the cap: psfm_window_sample's hash and its stable 64-bit radix sort over that window's ids
//   gather   one launch over the flattened rows of all windows, blocks numbered inside a window (psfm_window_batch.h)
// The rules are psfm_window_batch.h; every window's rows are byte for byte what psfm_window_sample gives for it.
#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "psfm_decoder_batch.h"
#include "psfm_device.h"
#include "psfm_internal.h"
#include "psfm_window_batch.h"

static_assert(PSFM_WINB_MAX == PSFM_DEC_BATCH_MAX, "one bound for the windows of a call");
static_assert(PSFM_WINB_MAX == 64, "psfm_ctx::winb holds 64 windows");
#define PWB_BLOCK PSFM_WINB_BLOCK
#define PWB_WAVES (PWB_BLOCK / PSFM_WAVE)

// the windows of a call as the selection sees them; by value in the kernel arguments
struct PsfmWinbWindows {
    int frame0[PSFM_WINB_MAX];
    int n_win, L, traj_min_len, min_length;
};

// Block `blockIdx.x` covers trajectories [256 blk, 256 blk + 256).  cnt[b * nblk + blk] = its eligible trajectories for window b;
// cnt[n_win * nblk] = 0, so that the exclusive scan leaves the total there.
__global__ __launch_bounds__(PWB_BLOCK) void psfm_winb_count_kernel(const int* __restrict__ birth, const int* __restrict__ len, int64_t n,
                                                                  const PsfmWinbWindows W, int64_t nblk, int64_t* __restrict__ cnt)
{
    __shared__ int wave_cnt[PWB_WAVES][PSFM_WINB_MAX];
    const int64_t i = (int64_t)blockIdx.x * PWB_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & (PSFM_WAVE - 1), wave = threadIdx.x / PSFM_WAVE;
    const bool in = i < n;
    const int bi = in ? birth[i] : 0, ln = in ? len[i] : 0;
    for (int b = 0; b < W.n_win; b++) {
        const unsigned long long m = __ballot(in && psfm_winb_eligible(bi, ln, W.frame0[b], W.L, W.traj_min_len, W.min_length));
        if (lane == 0) wave_cnt[wave][b] = __popcll(m);
    }
    __syncthreads();
    if ((int)threadIdx.x < W.n_win) {
        int s = 0;
#pragma unroll
        for (int w = 0; w < PWB_WAVES; w++) s += wave_cnt[w][threadIdx.x];
        cnt[(int64_t)threadIdx.x * nblk + blockIdx.x] = s;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) cnt[(int64_t)W.n_win * nblk] = 0;
}

// first[b] = the first row of window b in the concatenated pre-cap lists, b = 0 .. n_win (the last: all rows)
__global__ void psfm_winb_first_kernel(const int64_t* __restrict__ scan, int64_t nblk, int n_win, int64_t* __restrict__ first)
{
    const int b = threadIdx.x;
    if (b <= n_win) first[b] = scan[(int64_t)b * nblk];
}

// The pass of the count kernel again: an eligible trajectory goes to scan[b * nblk + blk] + (eligible ones before it in the block),
// so a window's ids are ascending.  Every place is below `total` (the scan's last entry), which the host has read.
__global__ __launch_bounds__(PWB_BLOCK) void psfm_winb_compact_kernel(const int* __restrict__ birth, const int* __restrict__ len, int64_t n,
                                                                    const PsfmWinbWindows W, int64_t nblk, const int64_t* __restrict__ scan,
                                                                    int64_t total, int* __restrict__ sel)
{
    __shared__ int wave_cnt[PWB_WAVES][PSFM_WINB_MAX];
    const int64_t i = (int64_t)blockIdx.x * PWB_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & (PSFM_WAVE - 1), wave = threadIdx.x / PSFM_WAVE;
    const bool in = i < n;
    const int bi = in ? birth[i] : 0, ln = in ? len[i] : 0;
    for (int b = 0; b < W.n_win; b++) {
        const unsigned long long m = __ballot(in && psfm_winb_eligible(bi, ln, W.frame0[b], W.L, W.traj_min_len, W.min_length));
        if (lane == 0) wave_cnt[wave][b] = __popcll(m);
    }
    __syncthreads();
    for (int b = 0; b < W.n_win; b++) {
        const bool e = in && psfm_winb_eligible(bi, ln, W.frame0[b], W.L, W.traj_min_len, W.min_length);
        const unsigned long long m = __ballot(e);          // (every lane of the wave is here)
        if (e) {
            int before = __popcll(m & (((unsigned long long)1 << lane) - 1));
            for (int w = 0; w < wave; w++) before += wave_cnt[w][b];
            const int64_t at = scan[(int64_t)b * nblk + blockIdx.x] + before;
            if (at < total) sel[at] = (int)i;
        }
    }
}

// psfm_window_hash_kernel over one window's ids
__global__ __launch_bounds__(PWB_BLOCK) void psfm_winb_hash_kernel(const int* __restrict__ ids, int64_t k, unsigned long long seed,
                                                                 unsigned long long* __restrict__ keys)
{
    const int64_t i = (int64_t)blockIdx.x * PWB_BLOCK + threadIdx.x;
    if (i >= k) return;
    keys[i] = psfm_winb_hash(seed, ids[i]);
}

// the windows of a call as the gather sees them; by value in the kernel arguments
struct PsfmWinbGather {
    const int* src[PSFM_WINB_MAX];      // the window's selected ids
    int64_t k[PSFM_WINB_MAX];
    int64_t row0[PSFM_WINB_MAX];        // rows of the windows before this one
    int blk0[PSFM_WINB_MAX];            // blocks of the windows before this one (INT32_MAX at and above n_win)
    int frame0[PSFM_WINB_MAX];
    const int* birth; const int* len; const int64_t* off; const double2* xy;
    int L, normalise;
    double ratio_w, ratio_h, in_w, in_h;
    int* ids_out; double2* xy_raw; double2* xy_norm; double* mask_absent;
};
static_assert(sizeof(PsfmWinbGather) <= 4096, "the table must fit the kernel arguments");
static_assert(sizeof(PsfmWinbWindows) + 64 <= 4096, "the table must fit the kernel arguments");

// psfm_window_gather_kernel with the window looked up: one thread per (row, window frame j) of its window, j fastest
__global__ __launch_bounds__(PWB_BLOCK) void psfm_winb_gather_kernel(const PsfmWinbGather a)
{
    const int b = psfm_winb_find(a.blk0, (int)blockIdx.x);
    const int64_t e = (int64_t)((int)blockIdx.x - a.blk0[b]) * PWB_BLOCK + threadIdx.x;      // inside the window
    if (e >= a.k[b] * a.L) return;
    const int64_t k = e / a.L;
    const int j = (int)(e - k * a.L);
    const int id = a.src[b][k];
    const int t = a.frame0[b] + j, bi = a.birth[id];
    const bool present = (t >= bi) & (t < bi + a.len[id]);
    double2 p = make_double2(0.0, 0.0);
    if (present) p = a.xy[a.off[id] + (t - bi)];
    const int64_t row = a.row0[b] + k, g = a.row0[b] * a.L + e;       // among the rows (elements) of all windows
    if (j == 0 && a.ids_out) a.ids_out[row] = id;
    if (a.xy_raw) a.xy_raw[g] = p;
    if (a.mask_absent) a.mask_absent[g] = present ? 0.0 : 1.0;
    if (a.xy_norm) a.xy_norm[g] = make_double2(psfm_winb_normalise(p.x, a.ratio_w, a.in_w), psfm_winb_normalise(p.y, a.ratio_h, a.in_h));
}

// The selection for all windows, kept in c->winb / c->winb_ws.  Synchronises `s` once.
static psfm_status psfm_winb_plan(psfm_ctx* c, int n_win, const int* frame0, int n_frames, int traj_min_len, int min_length,
                                  int64_t max_num, const uint64_t* seed, hipStream_t s)
{
    auto& P = c->winb;
    P.valid = false;
    P.res_gen = c->res_gen; P.n_win = n_win; P.n_frames = n_frames; P.traj_min_len = traj_min_len; P.min_length = min_length;
    P.max_num = max_num;
    for (int b = 0; b < PSFM_WINB_MAX; b++) {
        P.frame0[b] = b < n_win ? frame0[b] : 0; P.seed[b] = b < n_win ? seed[b] : 0; P.k[b] = 0; P.src[b] = 0;
    }
    const int64_t n = c->res_n_traj;
    if (n == 0 || n_win == 0) { P.valid = true; return PSFM_OK; }
    psfm_status st;
    if (!c->winb_host) PSFM_HIP(hipHostMalloc(&c->winb_host, (PSFM_WINB_MAX + 1) * sizeof(int64_t), hipHostMallocDefault));
    int64_t* h_first = (int64_t*)c->winb_host;
    PsfmWinbWindows W;
    for (int b = 0; b < PSFM_WINB_MAX; b++) W.frame0[b] = P.frame0[b];
    W.n_win = n_win; W.L = n_frames; W.traj_min_len = traj_min_len; W.min_length = min_length;
    const int64_t nblk = (n + PWB_BLOCK - 1) / PWB_BLOCK;
    const size_t cells = (size_t)n_win * (size_t)nblk + 1;
    // scratch of this call: counts | their scan | the windows' first rows
    const size_t o_scan = (8 * cells + 255) / 256 * 256, o_first = 2 * o_scan, total_ws = o_first + 8 * (PSFM_WINB_MAX + 1);
    if ((st = c->win_ws.ensure(total_ws)) != PSFM_OK) return st;
    int64_t* cnt = (int64_t*)c->win_ws.p;
    int64_t* scan = (int64_t*)((char*)c->win_ws.p + o_scan);
    int64_t* d_first = (int64_t*)((char*)c->win_ws.p + o_first);
    size_t scan_bytes = 0;
    PSFM_HIP(rocprim::exclusive_scan(nullptr, scan_bytes, cnt, scan, (int64_t)0, cells, rocprim::plus<int64_t>(), s));
    if ((st = c->sort_tmp.ensure(scan_bytes)) != PSFM_OK) return st;
    hipLaunchKernelGGL(psfm_winb_count_kernel, dim3((unsigned)nblk), dim3(PWB_BLOCK), 0, s, c->res_birth.as<int>(), c->res_len.as<int>(), n,
                       W, nblk, cnt);
    PSFM_HIP(hipGetLastError());
    PSFM_HIP(rocprim::exclusive_scan(c->sort_tmp.p, scan_bytes, cnt, scan, (int64_t)0, cells, rocprim::plus<int64_t>(), s));
    hipLaunchKernelGGL(psfm_winb_first_kernel, dim3(1), dim3(2 * PSFM_WAVE), 0, s, scan, nblk, n_win, d_first);
    PSFM_HIP(hipGetLastError());
    PSFM_HIP(hipMemcpyAsync(h_first, d_first, (size_t)(n_win + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    PSFM_HIP(hipStreamSynchronize(s));          // the one synchronisation of a plan
    const int64_t total = h_first[n_win];
    if (total == 0) { P.valid = true; return PSFM_OK; }
    bool any_capped = false;
    int64_t first[PSFM_WINB_MAX + 1];
    for (int b = 0; b <= n_win; b++) first[b] = h_first[b];
    for (int b = 0; b < n_win; b++) any_capped |= first[b + 1] - first[b] > max_num;
    // kept: selected ids (total i32) | above the cap: ids in key order (total i32) | keys in, keys out (2 total u64)
    const size_t o_ids2 = (4 * (size_t)total + 255) / 256 * 256, o_keys = 2 * o_ids2, o_keys2 = o_keys + 8 * (size_t)total,
                 kept = any_capped ? o_keys2 + 8 * (size_t)total : o_ids2;
    if ((st = c->winb_ws.ensure(kept)) != PSFM_OK) return st;
    int* sel = (int*)c->winb_ws.p;
    hipLaunchKernelGGL(psfm_winb_compact_kernel, dim3((unsigned)nblk), dim3(PWB_BLOCK), 0, s, c->res_birth.as<int>(), c->res_len.as<int>(), n,
                       W, nblk, scan, total, sel);
    PSFM_HIP(hipGetLastError());
    if (any_capped) {
        int* ids2 = (int*)((char*)c->winb_ws.p + o_ids2);
        unsigned long long* keys = (unsigned long long*)((char*)c->winb_ws.p + o_keys);
        unsigned long long* keys2 = (unsigned long long*)((char*)c->winb_ws.p + o_keys2);
        size_t tmp_max = 0;
        for (int b = 0; b < n_win; b++) {
            const int64_t cb = first[b + 1] - first[b];
            if (cb <= max_num) continue;
            size_t tmp = 0;
            PSFM_HIP(rocprim::radix_sort_pairs(nullptr, tmp, keys, keys2, sel, ids2, (size_t)cb, 0u, 64u, s));
            if (tmp > tmp_max) tmp_max = tmp;
        }
        if ((st = c->sort_tmp.ensure(tmp_max)) != PSFM_OK) return st;
        for (int b = 0; b < n_win; b++) {          // trajectory_base.cpp:150-153, with a seed: psfm_window_sample's hash and its sort
            const int64_t cb = first[b + 1] - first[b], at = first[b];
            if (cb <= max_num) continue;
            hipLaunchKernelGGL(psfm_winb_hash_kernel, dim3((unsigned)((cb + PWB_BLOCK - 1) / PWB_BLOCK)), dim3(PWB_BLOCK), 0, s, sel + at, cb,
                               (unsigned long long)P.seed[b], keys + at);
            PSFM_HIP(hipGetLastError());
            size_t tmp = tmp_max;
            PSFM_HIP(rocprim::radix_sort_pairs(c->sort_tmp.p, tmp, keys + at, keys2 + at, sel + at, ids2 + at, (size_t)cb, 0u, 64u, s));
        }
    }
    for (int b = 0; b < n_win; b++) {
        const int64_t cb = first[b + 1] - first[b];
        P.k[b] = psfm_winb_rows(cb, max_num);
        P.src[b] = (cb > max_num ? o_ids2 : 0) + 4 * (size_t)first[b];
    }
    P.valid = true;
    return PSFM_OK;
}

static bool psfm_winb_plan_matches(const psfm_ctx* c, int n_win, const int* frame0, int n_frames, int traj_min_len, int min_length,
                                   int64_t max_num, const uint64_t* seed)
{
    const auto& P = c->winb;
    if (!P.valid || P.res_gen != c->res_gen || P.n_win != n_win || P.n_frames != n_frames || P.traj_min_len != traj_min_len ||
        P.min_length != min_length || P.max_num != max_num) return false;
    for (int b = 0; b < n_win; b++)
        if (P.frame0[b] != frame0[b] || P.seed[b] != seed[b]) return false;
    return true;
}

extern "C" psfm_status psfm_window_sample_batch(psfm_ctx* c, int n_win, const int* frame0, int n_frames, int traj_min_len, int min_length,
                                                int64_t max_num_tracks, const uint64_t* seed, int raw_h, int raw_w, int in_h, int in_w,
                                                int64_t capacity, int32_t* ids_out, double* xy_raw, double* xy_norm, double* mask_absent,
                                                int64_t* k_host, void* stream)
{
    if (!c) { psfm_set_error("ctx is NULL"); return PSFM_ERR_ARG; }
    if (n_win < 0 || n_win > PSFM_WINB_MAX) {
        psfm_set_error("psfm_window_sample_batch: bad argument (n_win=%d, supported is 0 <= n_win <= %d)", n_win, PSFM_WINB_MAX);
        return PSFM_ERR_ARG;
    }
    if (n_frames < 1 || max_num_tracks < 0 || capacity < 0 || (n_win > 0 && (!k_host || !frame0 || !seed)) ||
        (xy_norm && (raw_h < 1 || raw_w < 1 || in_h < 1 || in_w < 1))) {
        psfm_set_error("psfm_window_sample_batch: bad argument (n_frames=%d max_num_tracks=%lld capacity=%lld)", n_frames,
                       (long long)max_num_tracks, (long long)capacity);
        return PSFM_ERR_ARG;
    }
    for (int b = 0; b < n_win; b++)
        if ((int64_t)frame0[b] + n_frames > INT32_MAX) {       // (the window's last frame is formed in 32 bits)
            psfm_set_error("psfm_window_sample_batch: window %d: frame0=%d n_frames=%d leaves the 32-bit frame range", b, frame0[b], n_frames);
            return PSFM_ERR_ARG;
        }
    if (psfm_set_result_refuses(c, traj_min_len, "psfm_window_sample_batch")) return PSFM_ERR_ARG;
    PSFM_HIP(hipSetDevice(c->device));
    PsfmGate gate(c->device, 0);
    hipStream_t s = (hipStream_t)stream;
    const bool fill = ids_out || xy_raw || xy_norm || mask_absent;
    psfm_status st;
    if (!fill || !psfm_winb_plan_matches(c, n_win, frame0, n_frames, traj_min_len, min_length, max_num_tracks, seed))
        if ((st = psfm_winb_plan(c, n_win, frame0, n_frames, traj_min_len, min_length, max_num_tracks, seed, s)) != PSFM_OK) return st;
    const auto& P = c->winb;
    PsfmWinbOffsets O;
    psfm_winb_offsets(O, P.k, n_win, n_frames, PWB_BLOCK);
    const int64_t rows = O.row0[PSFM_WINB_MAX];
    if (fill && rows > capacity) {
        psfm_set_error("psfm_window_sample_batch: %lld trajectories selected over %d windows, output capacity %lld", (long long)rows, n_win,
                       (long long)capacity);
        return PSFM_ERR_CAPACITY;
    }
    if (O.blocks > INT32_MAX) {
        psfm_set_error("psfm_window_sample_batch: %lld rows of %d frames exceed one launch; pass fewer windows per call", (long long)rows, n_frames);
        return PSFM_ERR_ARG;
    }
    for (int b = 0; b < n_win; b++) k_host[b] = P.k[b];
    if (!fill || rows == 0) return PSFM_OK;
    static thread_local PsfmWinbGather a;
    for (int b = 0; b < PSFM_WINB_MAX; b++) {
        const bool in = b < n_win && P.k[b] > 0;
        a.src[b] = in ? (const int*)((const char*)c->winb_ws.p + P.src[b]) : nullptr;
        a.k[b] = b < n_win ? P.k[b] : 0; a.row0[b] = O.row0[b]; a.blk0[b] = O.blk0[b]; a.frame0[b] = P.frame0[b];
    }
    a.birth = c->res_birth.as<int>(); a.len = c->res_len.as<int>(); a.off = c->res_off.as<int64_t>(); a.xy = c->res_xy.as<double2>();
    a.L = n_frames;
    a.normalise = xy_norm != nullptr;
    a.ratio_w = a.normalise ? (double)raw_w / (double)in_w : 1.0;
    a.ratio_h = a.normalise ? (double)raw_h / (double)in_h : 1.0;
    a.in_w = (double)in_w; a.in_h = (double)in_h;
    a.ids_out = ids_out; a.xy_raw = (double2*)xy_raw; a.xy_norm = (double2*)xy_norm; a.mask_absent = mask_absent;
    hipLaunchKernelGGL(psfm_winb_gather_kernel, dim3((unsigned)O.blocks), dim3(PWB_BLOCK), 0, s, a);
    PSFM_HIP(hipGetLastError());
    return PSFM_OK;
}
