// psfm_query.hip -- psfm_track_queries: caller-given query points (x, y, t) tracked through a flow stack on the device.
//
// The semantics are the reference's own functions with no new rule: per query the body of track.py:37-47 -- grid_sample of the flow
// (trajectory.py:25-37) and step_forward (trajectory.py:45-62; the motion-boundary form of :60 when the context has the option on) --
// repeated until the first step that is not alive or the end of the stack.  The per-lane loop is psfm_query.h (the CPU suite compiles
// the same text); the step is the arithmetic of psfm_chain.h that the chain kernels run.
//
//   psfm_query_validate_kernel   first query with a non-finite coordinate or a frame outside [0, n_flows] (one atomic minimum)
//   psfm_query_track_kernel      one lane per query, one launch per direction: a chain of dependent gathers per lane -- per step
//                                4 x 8 B flow taps, 4 mask bytes, one 16 B store into the time-major slab (n_flows+1, Q) kept in the
//                                context's log buffer.  No LDS, no atomics, no barrier: occupancy (8 waves per SIMD) hides the latency
//   psfm_query_plan_kernel       birth = t - (len_b - 1), len = len_b + len_f - 1; the lengths scanned inside each block
//   psfm_query_scan_kernel       ... the block totals scanned by one block, in index order
//   psfm_query_offsets_kernel    ... and added: off (Q + 1) i64.  Integer sums in a fixed order: identical calls give identical bytes
//   psfm_query_gather_kernel     slab rows birth .. birth + len - 1 of every query into the CSR: reads coalesced along q, 16 B stores
#include "psfm_device.h"
#include <cstring>

#include "psfm_internal.h"
#include "psfm_query.h"

#define PSFM_QUERY_BLOCK 256

__global__ __launch_bounds__(PSFM_QUERY_BLOCK) void psfm_query_validate_kernel(const double2* __restrict__ q_xy, const int* __restrict__ q_t,
                                                                               unsigned Q, int n_flows, unsigned long long* __restrict__ first_bad)
{
    const unsigned q = blockIdx.x * PSFM_QUERY_BLOCK + threadIdx.x;
    if (q >= Q) return;
    const double2 p = q_xy[q];
    const int t = q_t[q];
    const bool finite = fabs(p.x) <= 1.7976931348623157e308 && fabs(p.y) <= 1.7976931348623157e308;   // (NaN fails both)
    if (!finite || t < 0 || t > n_flows) atomicMin(first_bad, (unsigned long long)q);
}

template <bool MB, bool BACK>
__global__ __launch_bounds__(PSFM_QUERY_BLOCK) __attribute__((amdgpu_waves_per_eu(8, 8))) void psfm_query_track_kernel(PsfmQueryArgs a)
{
    const unsigned q = blockIdx.x * PSFM_QUERY_BLOCK + threadIdx.x;
    const bool has_query = q < a.Q;
    double2 p = make_double2(0.0, 0.0);
    int t = 0;
    if (has_query) {
        p = a.q_xy[q];
        t = a.q_t[q];
        psfm_st(a.slab + (size_t)t * a.Q, q * 16u, p);        // the (t, q) entry is the query itself, in either direction
    }
    const int n = psfm_query_walk<MB, BACK>(a, has_query, p, t, q);
    if (has_query) a.len[q] = n;
}

// exclusive prefix of v over the block's threads (in thread order) and the block's total
__device__ __forceinline__ int64_t psfm_query_block_scan(int64_t v, int64_t* total)
{
    __shared__ int64_t s_wave[PSFM_QUERY_BLOCK / PSFM_WAVE];
    const int lane = psfm_lane_id(), wave = (int)threadIdx.x / PSFM_WAVE;
    int64_t inc = v;
#pragma unroll
    for (int d = 1; d < PSFM_WAVE; d <<= 1) {
        const int64_t u = __shfl_up(inc, d, PSFM_WAVE);
        if (lane >= d) inc += u;
    }
    if (lane == PSFM_WAVE - 1) s_wave[wave] = inc;
    __syncthreads();
    int64_t base = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < PSFM_QUERY_BLOCK / PSFM_WAVE; ++k) {
        if (k < wave) base += s_wave[k];
        tot += s_wave[k];
    }
    __syncthreads();                                         // (the scan kernel calls this in a loop)
    *total = tot;
    return base + inc - v;
}

// len_f / len_b: NULL for a direction that was not tracked (one point: the query).  off[q]: the prefix inside the block, for now.
__global__ __launch_bounds__(PSFM_QUERY_BLOCK) void psfm_query_plan_kernel(const int* __restrict__ q_t, const int* __restrict__ len_f,
                                                                           const int* __restrict__ len_b, unsigned Q, int* __restrict__ birth,
                                                                           int* __restrict__ len, int64_t* __restrict__ off,
                                                                           int64_t* __restrict__ block_sum)
{
    const unsigned q = blockIdx.x * PSFM_QUERY_BLOCK + threadIdx.x;
    int n = 0;
    if (q < Q) {
        const int nf = len_f ? len_f[q] : 1, nb = len_b ? len_b[q] : 1;
        n = nb + nf - 1;
        birth[q] = q_t[q] - (nb - 1);
        len[q] = n;
    }
    int64_t total;
    const int64_t before = psfm_query_block_scan((int64_t)n, &total);
    if (q < Q) off[q] = before;
    if (threadIdx.x == 0) block_sum[blockIdx.x] = total;
}

// one block: block_sum[b] <- sum of the blocks before b; off[Q] <- the number of points
__global__ __launch_bounds__(PSFM_QUERY_BLOCK) void psfm_query_scan_kernel(int64_t* __restrict__ block_sum, unsigned n_blocks, unsigned Q,
                                                                           int64_t* __restrict__ off)
{
    int64_t carry = 0;
    for (unsigned b0 = 0; b0 < n_blocks; b0 += PSFM_QUERY_BLOCK) {
        const unsigned b = b0 + threadIdx.x;
        const int64_t v = b < n_blocks ? block_sum[b] : 0;
        int64_t total;
        const int64_t before = psfm_query_block_scan(v, &total);
        if (b < n_blocks) block_sum[b] = carry + before;
        carry += total;
    }
    if (threadIdx.x == 0) off[Q] = carry;
}

__global__ __launch_bounds__(PSFM_QUERY_BLOCK) void psfm_query_offsets_kernel(const int64_t* __restrict__ block_sum, unsigned Q,
                                                                              int64_t* __restrict__ off)
{
    const unsigned q = blockIdx.x * PSFM_QUERY_BLOCK + threadIdx.x;
    if (q < Q) off[q] += block_sum[blockIdx.x];
}

__global__ __launch_bounds__(PSFM_QUERY_BLOCK) void psfm_query_gather_kernel(const double2* __restrict__ slab, const int* __restrict__ birth,
                                                                             const int* __restrict__ len, const int64_t* __restrict__ off,
                                                                             unsigned Q, int n_flows, double2* __restrict__ out)
{
    const unsigned q = blockIdx.x * PSFM_QUERY_BLOCK + threadIdx.x;
    const bool has_query = q < Q;
    const int b = has_query ? birth[q] : n_flows + 1;
    const int e = has_query ? b + len[q] : 0;                 // one past the last frame
    const int64_t o = has_query ? off[q] : 0;
    const int f_lo = psfm_query_wave_min(b), f_hi = -psfm_query_wave_min(-e);
    for (int f = f_lo; f < f_hi; ++f)                         // (wave-uniform bounds; the row base is a scalar)
        if ((f >= b) & (f < e)) out[o + (f - b)] = psfm_ld(slab + (size_t)f * Q, q * 16u);
}

// first query with a non-finite coordinate or a frame outside [0, n_flows]: PSFM_ERR_ARG naming it (`who`: the entry point), else PSFM_OK
psfm_status psfm_query_refuse(psfm_ctx* c, const char* who, const double* q_xy, const int32_t* q_t, unsigned Q, int n_flows,
                              unsigned long long* first_bad, hipStream_t s)
{
    if (Q == 0) return PSFM_OK;
    unsigned long long* hq = (unsigned long long*)((char*)c->host_pinned + 448);
    const unsigned nblk = (Q + PSFM_QUERY_BLOCK - 1) / PSFM_QUERY_BLOCK;
    PSFM_HIP(hipMemsetAsync(first_bad, 0xff, sizeof(unsigned long long), s));
    hipLaunchKernelGGL(psfm_query_validate_kernel, dim3(nblk), dim3(PSFM_QUERY_BLOCK), 0, s, (const double2*)q_xy, q_t, Q, n_flows, first_bad);
    PSFM_HIP(hipGetLastError());
    PSFM_HIP(hipMemcpyAsync(&hq[0], first_bad, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    PSFM_HIP(hipStreamSynchronize(s));
    if (hq[0] != ~0ull) {
        psfm_set_error("%s: query %llu has a non-finite coordinate or a frame outside [0, %d]", who, hq[0], n_flows);
        return PSFM_ERR_ARG;
    }
    return PSFM_OK;
}

// The finish of a query result (Q > 0): births and lengths from the directions' lengths (NULL: not tracked), offsets, the slab's rows
// (c->log) gathered into the CSR; *n_points: its points.  bsum: (blocks + 1) i64 of scan storage.  Synchronises s.
psfm_status psfm_query_finish(psfm_ctx* c, const int32_t* q_t, const int* len_f, const int* len_b, unsigned Q, int n_flows, int64_t* bsum,
                              int64_t* n_points, hipStream_t s)
{
    psfm_status st;
    unsigned long long* hq = (unsigned long long*)((char*)c->host_pinned + 448);
    const unsigned nblk = (Q + PSFM_QUERY_BLOCK - 1) / PSFM_QUERY_BLOCK;
    c->prof.begin(PSFM_PROF_FINALIZE, s);                       // lengths -> offsets -> CSR as the finalize
    hipLaunchKernelGGL(psfm_query_plan_kernel, dim3(nblk), dim3(PSFM_QUERY_BLOCK), 0, s, q_t, len_f, len_b, Q,
                       c->res_birth.as<int>(), c->res_len.as<int>(), c->res_off.as<int64_t>(), bsum);
    hipLaunchKernelGGL(psfm_query_scan_kernel, dim3(1), dim3(PSFM_QUERY_BLOCK), 0, s, bsum, nblk, Q, c->res_off.as<int64_t>());
    hipLaunchKernelGGL(psfm_query_offsets_kernel, dim3(nblk), dim3(PSFM_QUERY_BLOCK), 0, s, (const int64_t*)bsum, Q, c->res_off.as<int64_t>());
    PSFM_HIP(hipGetLastError());
    PSFM_HIP(hipMemcpyAsync(&hq[1], c->res_off.as<int64_t>() + Q, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    PSFM_HIP(hipStreamSynchronize(s));
    const int64_t npts = (int64_t)hq[1];
    if ((st = c->res_xy.ensure(sizeof(double2) * (size_t)(npts > 0 ? npts : 1))) != PSFM_OK) return st;
    hipLaunchKernelGGL(psfm_query_gather_kernel, dim3(nblk), dim3(PSFM_QUERY_BLOCK), 0, s, c->log.as<double2>(), c->res_birth.as<int>(),
                       c->res_len.as<int>(), c->res_off.as<int64_t>(), Q, n_flows, c->res_xy.as<double2>());
    c->prof.end(s);
    PSFM_HIP(hipGetLastError());
    PSFM_HIP(hipStreamSynchronize(s));
    c->prof.collect();
    *n_points = npts;
    return PSFM_OK;
}

template <bool BACK>
static void psfm_launch_query_track(const PsfmQueryArgs& a, bool mb, hipStream_t s)
{
    const dim3 grid((a.Q + PSFM_QUERY_BLOCK - 1) / PSFM_QUERY_BLOCK), block(PSFM_QUERY_BLOCK);
    if (mb) hipLaunchKernelGGL((psfm_query_track_kernel<true, BACK>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((psfm_query_track_kernel<false, BACK>), grid, block, 0, s, a);
}

extern "C" psfm_status psfm_track_queries(psfm_ctx* c, const float* flows_f, const uint8_t* occ_f, const float* flows_b, const uint8_t* occ_b,
                                          int n_flows, int h, int w, const double* q_xy, const int32_t* q_t, int64_t n_q,
                                          psfm_track_info* info, void* stream)
{
    if (!c) { psfm_set_error("ctx is NULL"); return PSFM_ERR_ARG; }
    // ---- arguments: before any allocation or launch ----
    if ((!flows_f && !flows_b) || (flows_f != nullptr) != (occ_f != nullptr) || (flows_b != nullptr) != (occ_b != nullptr)) {
        psfm_set_error("psfm_track_queries: give at least one stack, and every stack with its occlusion maps");
        return PSFM_ERR_ARG;
    }
    if (n_flows < 1 || !psfm_frame_ok(h, w)) {
        psfm_set_error("psfm_track_queries: bad argument (n_flows=%d h=%d w=%d)", n_flows, h, w);
        return PSFM_ERR_ARG;
    }
    // a frame row of the slab -- 16 bytes per query -- stays below 4 GB (32-bit lane offsets)
    if (n_q < 0 || n_q >= ((int64_t)1 << 28) || (n_q > 0 && (!q_xy || !q_t))) {
        psfm_set_error("psfm_track_queries: bad argument (n_q=%lld: 0 <= n_q < 2^28, q_xy and q_t on the device)", (long long)n_q);
        return PSFM_ERR_ARG;
    }
    PSFM_HIP(hipSetDevice(c->device));
    PsfmGate gate(c->device, 0);
    hipStream_t s = (hipStream_t)stream;
    psfm_status st;
    const unsigned Q = (unsigned)n_q;
    const size_t P = (size_t)h * w;
    const unsigned nblk = (Q + PSFM_QUERY_BLOCK - 1) / PSFM_QUERY_BLOCK;

    // ---- workspace: first refused query | len_f | len_b | block totals of the length scan ----
    const size_t o_lenf = 64, o_lenb = o_lenf + (((size_t)Q * 4 + 63) & ~(size_t)63), o_bsum = o_lenb + (((size_t)Q * 4 + 63) & ~(size_t)63);
    if ((st = c->qr_ws.ensure(o_bsum + (size_t)(nblk + 1) * sizeof(int64_t))) != PSFM_OK) return st;
    char* ws = c->qr_ws.as<char>();
    unsigned long long* first_bad = (unsigned long long*)ws;

    // ---- refusals: a non-finite coordinate, a frame outside [0, n_flows] -- before anything is tracked ----
    if ((st = psfm_query_refuse(c, "psfm_track_queries", q_xy, q_t, Q, n_flows, first_bad, s)) != PSFM_OK) return st;

    // ---- from here on the call replaces the result (and the lane tables of an unfinished sharded run: the slab lives in the log) ----
    psfm_shard_abandon(c);
    c->res_gen++;
    c->solve_stats.clear();
    c->res_n_traj = c->res_n_points = 0;
    c->res_n_flows = n_flows;
    c->res_is_query = true;
    c->res_is_set = false;
    const size_t nq1 = Q > 0 ? Q : 1;
    if ((st = c->log.ensure(sizeof(double2) * (size_t)(n_flows + 1) * nq1)) != PSFM_OK) return st;
    if ((st = c->res_birth.ensure(sizeof(int) * nq1)) != PSFM_OK) return st;
    if ((st = c->res_len.ensure(sizeof(int) * nq1)) != PSFM_OK) return st;
    if ((st = c->res_off.ensure(sizeof(int64_t) * ((size_t)Q + 1))) != PSFM_OK) return st;
    if (Q == 0) {
        PSFM_HIP(hipMemsetAsync(c->res_off.p, 0, sizeof(int64_t), s));
        PSFM_HIP(hipStreamSynchronize(s));
    } else {
        const bool mb = c->mb_enable;
        const uint8_t* mask_f = occ_f;
        const uint8_t* mask_b = occ_b;
        if (mb) {   // the kill maps (bit 0 occlusion, bit 1 motion boundary) of each stack being sampled, from that stack's own flows
            if ((st = c->kill.ensure((size_t)n_flows * P * 2)) != PSFM_OK) return st;
            uint8_t* kf = c->kill.as<uint8_t>();
            uint8_t* kb = kf + (size_t)n_flows * P;
            if (flows_f) {
                if ((st = psfm_launch_motion_boundary(flows_f, occ_f, n_flows, h, w, c->mb_thres, kf, s)) != PSFM_OK) return st;
                mask_f = kf;
            }
            if (flows_b) {
                if ((st = psfm_launch_motion_boundary(flows_b, occ_b, n_flows, h, w, c->mb_thres, kb, s)) != PSFM_OK) return st;
                mask_b = kb;
            }
        }
        PsfmQueryArgs a;
        a.q_xy = (const double2*)q_xy; a.q_t = q_t; a.slab = c->log.as<double2>();
        a.H = h; a.W = w; a.n_flows = n_flows; a.Q = Q; a.P = (unsigned)P;
        a.cw = (float)((double)(w - 1) / 2.0); a.ch = (float)((double)(h - 1) / 2.0);
        a.rcw = psfm_rcp_host(a.cw); a.rch = psfm_rcp_host(a.ch);
        int* len_f = flows_f ? (int*)(ws + o_lenf) : nullptr;
        int* len_b = flows_b ? (int*)(ws + o_lenb) : nullptr;
        c->prof.begin(PSFM_PROF_CHAIN, s);                      // (psfm_ctx_set_profiling: the tracking launches count as the chain step)
        if (flows_f) {
            a.flows = (const float2*)flows_f; a.masks = mask_f; a.len = len_f;
            psfm_launch_query_track<false>(a, mb, s);
        }
        if (flows_b) {
            a.flows = (const float2*)flows_b; a.masks = mask_b; a.len = len_b;
            psfm_launch_query_track<true>(a, mb, s);
        }
        c->prof.end(s);
        PSFM_HIP(hipGetLastError());
        int64_t npts = 0;
        if ((st = psfm_query_finish(c, q_t, len_f, len_b, Q, n_flows, (int64_t*)(ws + o_bsum), &npts, s)) != PSFM_OK) return st;
        c->res_n_traj = (int64_t)Q;
        c->res_n_points = npts;
    }
    if (info) {
        memset(info, 0, sizeof(*info));
        info->n_traj = c->res_n_traj;
        info->n_points = c->res_n_points;
        info->n_lanes_peak = (int64_t)Q;
        info->lane_capacity = (int64_t)Q;
        info->chain_mode = 4;
    }
    return PSFM_OK;
}
