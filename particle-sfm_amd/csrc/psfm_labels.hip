// psfm_labels.hip -- motion_seg/main_motion_segmentation.py:89-129 on the device: the network's per-window, per-trajectory
// predictions merged into the labelled trajectory set that sfm/matches_from_flow.py consumes.
//
// The reference walks every row of every window in Python (:92-112): the row's valid points (mask == 0) enter a dict keyed by the
// trajectory id -- a new key takes all of them (:100-103), a known key only the points whose frame it does not hold yet (:105-112) --
// and every point carries the row's prediction.  The saved dict (:122-129) therefore lists the trajectories in order of first
// appearance (window, then row), a point's label is the prediction of the FIRST window that covered it, and a trajectory that was
// not sampled in some window has a gap in its frames there.
//
// Here the same set is built over the saved set that psfm_result_filter left in HBM (ascending ids, frames birth .. birth + len - 1):
//   state  per saved point, u8       255 = not in the labelled set, 0 static, 1 dynamic
//   first  per saved trajectory, u32 sequence number (rows of earlier windows + row) of the row that brought it in, 0xffffffff = none
// A window is ONE asynchronous launch (psfm_labels_merge_window), so it can sit in the stream right behind the network's output;
// launches are ordered by the stream and ids are unique inside a window, so no atomics are needed.  Finish counts the labelled points
// per trajectory, orders the trajectories by `first` (psfm_sort.hip), scans, and gathers ids / off / frame_ids / xy / labels as a CSR.
#include <rocprim/device/device_scan.hpp>

#include "psfm_device.h"
#include "psfm_internal.h"

#define PL_BLOCK 256
#define PL_GROUP 16                 // lanes per window row / per trajectory: a window has ~10 frames, a trajectory ~25 points
#define PL_UNSET 0xffffffffu
#define PL_NONE 255

static unsigned pl_grid(int64_t n) { return (unsigned)((n + PL_BLOCK - 1) / PL_BLOCK); }

// One group of PL_GROUP lanes per window row.  Lane 0 of the group finds the trajectory's row in the saved set (binary search of the
// id, once per row) and broadcasts it; the lanes then take the row's frames inside the window -- consecutive bytes of `state`.
__global__ __launch_bounds__(PL_BLOCK) void pl_merge_kernel(const int* __restrict__ ids, const uint8_t* __restrict__ pred, int64_t k_rows,
                                                           int64_t f0, int64_t f1, unsigned rows_before, const int* __restrict__ sids,
                                                           int64_t k_saved, const int* __restrict__ birth, const int* __restrict__ len,
                                                           const int64_t* __restrict__ off, uint8_t* __restrict__ state,
                                                           unsigned* __restrict__ first, int* __restrict__ flag)
{
    const int64_t g = ((int64_t)blockIdx.x * PL_BLOCK + threadIdx.x) / PL_GROUP;
    const int sub = threadIdx.x & (PL_GROUP - 1);
    int r = -1;
    if (sub == 0 && g < k_rows) {
        const int id = ids[g];
        int64_t lo = 0, hi = k_saved;          // first saved row with sids[row] >= id
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (sids[mid] < id) lo = mid + 1; else hi = mid;
        }
        if (lo < k_saved && sids[lo] == id) r = (int)lo;
        else *flag = 1;                        // an id outside the saved set: reported by psfm_labels_finish
    }
    r = __shfl(r, 0, PL_GROUP);
    if (r < 0) return;
    const int64_t b = birth[r], e = b + len[r];
    const int64_t lo = b > f0 ? b : f0, hi = e < f1 ? e : f1;
    if (hi <= lo) return;                      // no point in the window: the row is ignored
    const uint8_t v = pred[g] != 0 ? 1 : 0;
    const int64_t base = off[r] - b;
    for (int64_t f = lo + sub; f < hi; f += PL_GROUP)
        if (state[base + f] == PL_NONE) state[base + f] = v;      // the first window that covers a point decides (:105-112)
    if (sub == 0 && first[r] == PL_UNSET) first[r] = rows_before + (unsigned)g;
}

// One group per saved trajectory: its labelled points, and its sort record (first, row) -- rows never seen get the key `sentinel`
// (= the total number of rows, above every sequence number) so that the sort needs only the bits of that value.
__global__ __launch_bounds__(PL_BLOCK) void pl_count_kernel(const uint8_t* __restrict__ state, const int64_t* __restrict__ off, int64_t k,
                                                           const unsigned* __restrict__ first, unsigned sentinel, int* __restrict__ cnt,
                                                           unsigned* __restrict__ key, int* __restrict__ val)
{
    const int64_t t = ((int64_t)blockIdx.x * PL_BLOCK + threadIdx.x) / PL_GROUP;
    const int sub = threadIdx.x & (PL_GROUP - 1);
    int n = 0;
    if (t < k) {
        const int64_t o = off[t], m = off[t + 1] - o;
        for (int64_t j = sub; j < m; j += PL_GROUP) n += state[o + j] != PL_NONE ? 1 : 0;
    }
#pragma unroll
    for (int d = PL_GROUP / 2; d > 0; d >>= 1) n += __shfl_xor(n, d, PL_GROUP);
    if (sub == 0 && t < k) {
        const unsigned f = first[t];
        cnt[t] = n;
        key[t] = f == PL_UNSET ? sentinel : f;
        val[t] = (int)t;
    }
}

// s-th trajectory in order of first appearance: its id, its point count for the scan; the last one that was seen sets n_traj
__global__ __launch_bounds__(PL_BLOCK) void pl_order_kernel(const unsigned* __restrict__ key_s, const int* __restrict__ val_s, int64_t k,
                                                           unsigned sentinel, const int* __restrict__ cnt, const int* __restrict__ sids,
                                                           int64_t* __restrict__ cnt64, int* __restrict__ ids_out, int64_t* __restrict__ n_traj)
{
    const int64_t s = (int64_t)blockIdx.x * PL_BLOCK + threadIdx.x;
    if (s > k) return;
    if (s == k) { cnt64[s] = 0; return; }
    const bool seen = key_s[s] < sentinel;
    const int t = val_s[s];
    cnt64[s] = seen ? (int64_t)cnt[t] : 0;
    ids_out[s] = sids[t];
    if (seen && (s + 1 == k || key_s[s + 1] >= sentinel)) *n_traj = s + 1;
}

// One group per labelled trajectory: its points with a label, in time order, to their place in the CSR.  16 points per step; a
// point's position is the number of labelled points before it (ballot of the wave, the group's 16 bits of it).
__global__ __launch_bounds__(PL_BLOCK) void pl_gather_kernel(const int* __restrict__ val_s, int64_t n_traj, const int64_t* __restrict__ off,
                                                            const int* __restrict__ birth, const uint8_t* __restrict__ state,
                                                            const double2* __restrict__ xy, const int64_t* __restrict__ off_out,
                                                            int* __restrict__ frames, double2* __restrict__ xy_out, uint8_t* __restrict__ labels)
{
    const int64_t s = ((int64_t)blockIdx.x * PL_BLOCK + threadIdx.x) / PL_GROUP;
    const int sub = threadIdx.x & (PL_GROUP - 1);
    const int shift = (threadIdx.x & (PSFM_WAVE - 1)) & ~(PL_GROUP - 1);
    if (s >= n_traj) return;
    const int t = val_s[s];
    const int64_t o = off[t], m = off[t + 1] - o;
    const int b = birth[t];
    int64_t dst = off_out[s];
    for (int64_t j0 = 0; j0 < m; j0 += PL_GROUP) {
        const int64_t j = j0 + sub;
        const uint8_t st = j < m ? state[o + j] : (uint8_t)PL_NONE;
        const bool have = st != PL_NONE;
        const unsigned gm = (unsigned)((__ballot(have) >> shift) & 0xffffull);
        if (have) {
            const int64_t q = dst + __popc(gm & ((1u << sub) - 1u));
            frames[q] = b + (int)j;
            xy_out[q] = xy[o + j];
            labels[q] = st;
        }
        dst += __popc(gm);
    }
}

static int pl_bits(unsigned long long v)   // bits needed for values < v
{
    int b = 1;
    while (b < 64 && (1ull << b) < v) ++b;
    return b;
}

// the labels of this context belong to the saved set it holds now
static psfm_status pl_check(psfm_ctx* c, const char* who)
{
    if (!c) { psfm_set_error("ctx is NULL"); return PSFM_ERR_ARG; }
    if (!c->lb_active) { psfm_set_error("%s: no psfm_labels_begin on this context", who); return PSFM_ERR_ARG; }
    if (c->lb_gen != c->res_gen) {
        psfm_set_error("%s: the saved set changed since psfm_labels_begin (psfm_track / psfm_connect / psfm_result_filter ran)", who);
        return PSFM_ERR_ARG;
    }
    return PSFM_OK;
}

extern "C" psfm_status psfm_labels_begin(psfm_ctx* c, void* stream)
{
    if (!c) { psfm_set_error("ctx is NULL"); return PSFM_ERR_ARG; }
    c->lb_active = c->lb_finished = false;
    if (c->flt_n_traj <= 0 || c->flt_n_points <= 0) {
        psfm_set_error("psfm_labels_begin: no saved set in the context (run psfm_result_filter first)");
        return PSFM_ERR_ARG;
    }
    PSFM_HIP(hipSetDevice(c->device));
    PsfmGate gate(c->device, 0);
    hipStream_t s = (hipStream_t)stream;
    psfm_status st;
    if ((st = c->lb_state.ensure((size_t)c->flt_n_points)) != PSFM_OK) return st;
    if ((st = c->lb_first.ensure(4 * (size_t)c->flt_n_traj)) != PSFM_OK) return st;
    if ((st = c->lb_flag.ensure(256)) != PSFM_OK) return st;
    PSFM_HIP(hipMemsetAsync(c->lb_state.p, 0xff, (size_t)c->flt_n_points, s));
    PSFM_HIP(hipMemsetAsync(c->lb_first.p, 0xff, 4 * (size_t)c->flt_n_traj, s));
    PSFM_HIP(hipMemsetAsync(c->lb_flag.p, 0, 256, s));
    c->lb_gen = c->res_gen;
    c->lb_rows = 0;
    c->lb_n_traj = c->lb_n_points = 0;
    c->lb_active = true;
    return PSFM_OK;
}

extern "C" psfm_status psfm_labels_merge_window(psfm_ctx* c, int frame0, int n_frames, const int32_t* ids_dev, const uint8_t* pred_dev,
                                                int64_t k, void* stream)
{
    psfm_status st;
    if ((st = pl_check(c, "psfm_labels_merge_window")) != PSFM_OK) return st;
    if (n_frames < 1 || k < 0 || (k > 0 && (!ids_dev || !pred_dev))) {
        psfm_set_error("psfm_labels_merge_window: bad argument (n_frames=%d k=%lld)", n_frames, (long long)k);
        return PSFM_ERR_ARG;
    }
    if (c->lb_rows + k >= 0xffffffffll) { psfm_set_error("psfm_labels_merge_window: more than 2^32 - 2 rows over all windows"); return PSFM_ERR_ARG; }
    if (k == 0) return PSFM_OK;
    PSFM_HIP(hipSetDevice(c->device));
    PsfmGate gate(c->device, 0);
    hipLaunchKernelGGL(pl_merge_kernel, dim3(pl_grid(k * PL_GROUP)), dim3(PL_BLOCK), 0, (hipStream_t)stream, (const int*)ids_dev, pred_dev, k,
                       (int64_t)frame0, (int64_t)frame0 + n_frames, (unsigned)c->lb_rows, (const int*)c->flt_ids.as<int>(), c->flt_n_traj,
                       (const int*)c->flt_birth.as<int>(), (const int*)c->flt_len.as<int>(), (const int64_t*)c->flt_off.as<int64_t>(),
                       c->lb_state.as<uint8_t>(), c->lb_first.as<unsigned>(), c->lb_flag.as<int>());
    PSFM_HIP(hipGetLastError());
    c->lb_rows += k;
    c->lb_finished = false;
    return PSFM_OK;
}

extern "C" psfm_status psfm_labels_finish(psfm_ctx* c, int64_t* n_traj_host, int64_t* n_points_host, void* stream)
{
    psfm_status st;
    if ((st = pl_check(c, "psfm_labels_finish")) != PSFM_OK) return st;
    if (!n_traj_host || !n_points_host) { psfm_set_error("psfm_labels_finish: NULL argument"); return PSFM_ERR_ARG; }
    PSFM_HIP(hipSetDevice(c->device));
    PsfmGate gate(c->device, 0);
    hipStream_t s = (hipStream_t)stream;
    *n_traj_host = *n_points_host = 0;
    c->lb_finished = false;
    c->lb_n_traj = c->lb_n_points = 0;
    const int64_t k = c->flt_n_traj;
    if (k >= 0x7fffffffll) { psfm_set_error("psfm_labels_finish: more than 2^31 saved trajectories"); return PSFM_ERR_ARG; }
    int64_t* h = (int64_t*)((char*)c->host_pinned + 256);      // [0] n_traj, [1] n_points, [2] unknown-id flag
    if (c->lb_rows == 0) {                                     // no window: the empty set
        if ((st = c->lb_off.ensure(8)) != PSFM_OK) return st;
        PSFM_HIP(hipMemsetAsync(c->lb_off.p, 0, 8, s));
        PSFM_HIP(hipStreamSynchronize(s));
        c->lb_finished = true;
        return PSFM_OK;
    }
    const unsigned sentinel = (unsigned)c->lb_rows;
    const unsigned end_bit = (unsigned)pl_bits((unsigned long long)sentinel + 1ull);
    // workspace: counts (k i32) | sort halves: keys 0, values 0, keys 1, values 1 (k each) | n_traj (i64)
    const size_t a4 = ((size_t)k * 4 + 255) / 256 * 256;
    if ((st = c->lb_ws.ensure(5 * a4 + 256)) != PSFM_OK) return st;
    char* w = (char*)c->lb_ws.p;
    int* cnt = (int*)w;
    unsigned* k0 = (unsigned*)(w + a4); int* v0 = (int*)(w + 2 * a4);
    unsigned* k1 = (unsigned*)(w + 3 * a4); int* v1 = (int*)(w + 4 * a4);
    int64_t* d_ntraj = (int64_t*)(w + 5 * a4);
    if ((st = c->lb_ids.ensure(4 * (size_t)k)) != PSFM_OK) return st;
    if ((st = c->lb_off.ensure(8 * (size_t)(k + 1))) != PSFM_OK) return st;
    if ((st = c->scan_tmp.ensure(8 * (size_t)(k + 1))) != PSFM_OK) return st;
    const bool in1 = (psfm_sort_pairs32_passes(end_bit) & 1) != 0;       // where the sort wants its input
    PSFM_HIP(hipMemsetAsync(d_ntraj, 0, 8, s));
    hipLaunchKernelGGL(pl_count_kernel, dim3(pl_grid(k * PL_GROUP)), dim3(PL_BLOCK), 0, s, (const uint8_t*)c->lb_state.as<uint8_t>(),
                       (const int64_t*)c->flt_off.as<int64_t>(), k, (const unsigned*)c->lb_first.as<unsigned>(), sentinel, cnt,
                       in1 ? k1 : k0, in1 ? v1 : v0);
    if ((st = psfm_sort_pairs32(c, k0, v0, k1, v1, k, end_bit, s)) != PSFM_OK) return st;
    hipLaunchKernelGGL(pl_order_kernel, dim3(pl_grid(k + 1)), dim3(PL_BLOCK), 0, s, (const unsigned*)k0, (const int*)v0, k, sentinel,
                       (const int*)cnt, (const int*)c->flt_ids.as<int>(), c->scan_tmp.as<int64_t>(), c->lb_ids.as<int>(), d_ntraj);
    {
        size_t bytes = 0;
        PSFM_HIP(rocprim::exclusive_scan(nullptr, bytes, (int64_t*)nullptr, (int64_t*)nullptr, (int64_t)0, (size_t)(k + 1), rocprim::plus<int64_t>(), s));
        if ((st = c->sort_tmp.ensure(bytes)) != PSFM_OK) return st;
        PSFM_HIP(rocprim::exclusive_scan(c->sort_tmp.p, bytes, c->scan_tmp.as<int64_t>(), c->lb_off.as<int64_t>(), (int64_t)0, (size_t)(k + 1),
                                         rocprim::plus<int64_t>(), s));
    }
    h[2] = 0;
    PSFM_HIP(hipMemcpyAsync(h, d_ntraj, 8, hipMemcpyDeviceToHost, s));
    PSFM_HIP(hipMemcpyAsync(h + 1, c->lb_off.as<int64_t>() + k, 8, hipMemcpyDeviceToHost, s));
    PSFM_HIP(hipMemcpyAsync(h + 2, c->lb_flag.p, 4, hipMemcpyDeviceToHost, s));
    PSFM_HIP(hipStreamSynchronize(s));
    if ((int)(h[2] & 0xffffffff) != 0) { psfm_set_error("psfm_labels_finish: a window named a trajectory id that is not in the saved set"); return PSFM_ERR_ARG; }
    const int64_t n_traj = h[0], n_points = h[1];
    if ((st = c->lb_frames.ensure(4 * (size_t)(n_points > 0 ? n_points : 1))) != PSFM_OK) return st;
    if ((st = c->lb_xy.ensure(16 * (size_t)(n_points > 0 ? n_points : 1))) != PSFM_OK) return st;
    if ((st = c->lb_labels.ensure((size_t)(n_points > 0 ? n_points : 1))) != PSFM_OK) return st;
    if (n_traj > 0) {
        hipLaunchKernelGGL(pl_gather_kernel, dim3(pl_grid(n_traj * PL_GROUP)), dim3(PL_BLOCK), 0, s, (const int*)v0, n_traj,
                           (const int64_t*)c->flt_off.as<int64_t>(), (const int*)c->flt_birth.as<int>(), (const uint8_t*)c->lb_state.as<uint8_t>(),
                           (const double2*)c->flt_xy.as<double2>(), (const int64_t*)c->lb_off.as<int64_t>(), c->lb_frames.as<int>(),
                           c->lb_xy.as<double2>(), c->lb_labels.as<uint8_t>());
        PSFM_HIP(hipGetLastError());
        PSFM_HIP(hipStreamSynchronize(s));
    }
    c->lb_n_traj = n_traj; c->lb_n_points = n_points;
    *n_traj_host = n_traj; *n_points_host = n_points;
    c->lb_finished = true;
    return PSFM_OK;
}

// off (k+1) must run from 0 to n_points without stepping back: the match-table kernels index by it
__global__ __launch_bounds__(PL_BLOCK) void pl_check_off_kernel(const int64_t* __restrict__ off, int64_t k, int64_t n_points, int* __restrict__ flag)
{
    const int64_t t = (int64_t)blockIdx.x * PL_BLOCK + threadIdx.x;
    if (t > k) return;
    const int64_t a = off[t];
    const bool bad = t == 0 ? a != 0 : (a < off[t - 1] || (t == k && a != n_points));
    if (bad) *flag = 1;
}

// A labelled set from elsewhere (a labelled track.npy, labels of another classifier): the caller's CSR becomes the context's
// labelled set, as if psfm_labels_finish had built it.
extern "C" psfm_status psfm_labels_set(psfm_ctx* c, int64_t n_traj, int64_t n_points, const int32_t* ids, const int64_t* off,
                                       const int32_t* frame_ids, const double* xy, const uint8_t* labels, void* stream)
{
    if (!c) { psfm_set_error("ctx is NULL"); return PSFM_ERR_ARG; }
    if (n_traj < 0 || n_points < 0 || n_traj >= 0x7fffffffll || !off || (n_traj > 0 && !ids) || (n_points > 0 && (!frame_ids || !xy || !labels))) {
        psfm_set_error("psfm_labels_set: bad argument (n_traj=%lld n_points=%lld)", (long long)n_traj, (long long)n_points);
        return PSFM_ERR_ARG;
    }
    PSFM_HIP(hipSetDevice(c->device));
    PsfmGate gate(c->device, 0);
    hipStream_t s = (hipStream_t)stream;
    psfm_status st;
    c->lb_active = c->lb_finished = false;         // (a merge in progress ends here)
    c->lb_n_traj = c->lb_n_points = 0;
    if ((st = c->lb_ids.ensure(4 * (size_t)(n_traj > 0 ? n_traj : 1))) != PSFM_OK) return st;
    if ((st = c->lb_off.ensure(8 * (size_t)(n_traj + 1))) != PSFM_OK) return st;
    if ((st = c->lb_frames.ensure(4 * (size_t)(n_points > 0 ? n_points : 1))) != PSFM_OK) return st;
    if ((st = c->lb_xy.ensure(16 * (size_t)(n_points > 0 ? n_points : 1))) != PSFM_OK) return st;
    if ((st = c->lb_labels.ensure((size_t)(n_points > 0 ? n_points : 1))) != PSFM_OK) return st;
    if ((st = c->lb_flag.ensure(256)) != PSFM_OK) return st;
    if (n_traj > 0) PSFM_HIP(hipMemcpyAsync(c->lb_ids.p, ids, 4 * (size_t)n_traj, hipMemcpyDefault, s));
    PSFM_HIP(hipMemcpyAsync(c->lb_off.p, off, 8 * (size_t)(n_traj + 1), hipMemcpyDefault, s));
    if (n_points > 0) {
        PSFM_HIP(hipMemcpyAsync(c->lb_frames.p, frame_ids, 4 * (size_t)n_points, hipMemcpyDefault, s));
        PSFM_HIP(hipMemcpyAsync(c->lb_xy.p, xy, 16 * (size_t)n_points, hipMemcpyDefault, s));
        PSFM_HIP(hipMemcpyAsync(c->lb_labels.p, labels, (size_t)n_points, hipMemcpyDefault, s));
    }
    int* flag = c->lb_flag.as<int>() + 1;           // (word 0 is the merge's unknown-id flag)
    int64_t* h = (int64_t*)((char*)c->host_pinned + 256);
    h[0] = 0;
    PSFM_HIP(hipMemsetAsync(flag, 0, 4, s));
    hipLaunchKernelGGL(pl_check_off_kernel, dim3(pl_grid(n_traj + 1)), dim3(PL_BLOCK), 0, s, (const int64_t*)c->lb_off.as<int64_t>(), n_traj, n_points, flag);
    PSFM_HIP(hipGetLastError());
    PSFM_HIP(hipMemcpyAsync(h, flag, 4, hipMemcpyDeviceToHost, s));
    PSFM_HIP(hipStreamSynchronize(s));
    if ((int)(h[0] & 0xffffffff) != 0) { psfm_set_error("psfm_labels_set: off does not run from 0 to n_points=%lld in ascending order", (long long)n_points); return PSFM_ERR_ARG; }
    c->lb_n_traj = n_traj; c->lb_n_points = n_points;
    c->lb_finished = true;
    return PSFM_OK;
}

// the labelled set is a copy of its own: it stays readable after the saved set it was built from is gone
static psfm_status pl_finished(psfm_ctx* c, const char* who)
{
    if (!c) { psfm_set_error("ctx is NULL"); return PSFM_ERR_ARG; }
    if (!c->lb_finished) { psfm_set_error("%s: no labelled set in the context (psfm_labels_finish)", who); return PSFM_ERR_ARG; }
    return PSFM_OK;
}

extern "C" psfm_status psfm_labels_device(psfm_ctx* c, const int32_t** ids, const int64_t** off, const int32_t** frame_ids, const double** xy,
                                          const uint8_t** labels)
{
    psfm_status st;
    if ((st = pl_finished(c, "psfm_labels_device")) != PSFM_OK) return st;
    if (ids) *ids = c->lb_ids.as<int32_t>();
    if (off) *off = c->lb_off.as<int64_t>();
    if (frame_ids) *frame_ids = c->lb_frames.as<int32_t>();
    if (xy) *xy = c->lb_xy.as<double>();
    if (labels) *labels = c->lb_labels.as<uint8_t>();
    return PSFM_OK;
}

// hipMemcpyDefault: the destinations may be host buffers or device buffers (what LabelMerger.finish hands out as torch tensors)
extern "C" psfm_status psfm_labels_copy(psfm_ctx* c, int32_t* ids_out, int64_t* off_out, int32_t* frame_ids_out, double* xy_out,
                                        uint8_t* labels_out, void* stream)
{
    psfm_status st;
    if ((st = pl_finished(c, "psfm_labels_copy")) != PSFM_OK) return st;
    PSFM_HIP(hipSetDevice(c->device));
    PsfmGate gate(c->device, 0);
    hipStream_t s = (hipStream_t)stream;
    const int64_t k = c->lb_n_traj, n = c->lb_n_points;
    if (ids_out && k > 0) PSFM_HIP(hipMemcpyAsync(ids_out, c->lb_ids.p, 4 * (size_t)k, hipMemcpyDefault, s));
    if (off_out) PSFM_HIP(hipMemcpyAsync(off_out, c->lb_off.p, 8 * (size_t)(k + 1), hipMemcpyDefault, s));
    if (frame_ids_out && n > 0) PSFM_HIP(hipMemcpyAsync(frame_ids_out, c->lb_frames.p, 4 * (size_t)n, hipMemcpyDefault, s));
    if (xy_out && n > 0) PSFM_HIP(hipMemcpyAsync(xy_out, c->lb_xy.p, 16 * (size_t)n, hipMemcpyDefault, s));
    if (labels_out && n > 0) PSFM_HIP(hipMemcpyAsync(labels_out, c->lb_labels.p, (size_t)n, hipMemcpyDefault, s));
    PSFM_HIP(hipStreamSynchronize(s));
    return PSFM_OK;
}

extern "C" psfm_status psfm_labels_to_matches(psfm_ctx* c, int n_img, int sample_k, int remove_dynamic, int64_t* n_kp_host,
                                              int64_t* n_matches_host, int64_t* n_pairs_host, void* stream)
{
    psfm_status st;
    if ((st = pl_finished(c, "psfm_labels_to_matches")) != PSFM_OK) return st;
    PsfmMatchSrc src;
    src.who = "psfm_labels_to_matches";
    src.k = c->lb_n_traj; src.n_pts = c->lb_n_points;
    src.off = c->lb_off.as<int64_t>(); src.frames = c->lb_frames.as<int>(); src.xy = c->lb_xy.as<double2>();
    src.labels = remove_dynamic ? c->lb_labels.as<uint8_t>() : nullptr;       // matches_from_flow.py:71-74
    return psfm_match_tables(c, src, n_img, sample_k, n_kp_host, n_matches_host, n_pairs_host, (hipStream_t)stream);
}
