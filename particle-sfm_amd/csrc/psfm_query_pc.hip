// psfm_query_pc.hip -- psfm_track_queries_optimize: caller-given query points (x, y, t) tracked through a flow stack with the stride-2
// path-consistency solve of track_optimize.py:49-50 after every step -- what every grid trajectory of psfm_track gets, for query tracks.
//
// The semantics are the reference's own with no new rule: IncrementalTrajectorySet(buffer_size=3) fed with the queries of every frame
// (new_traj_all takes any points), then the body of track_optimize.py:37-50.  The solve of a frame is JOINT over the call's queries
// (Ceres' trust-region loop is global: one cost, one step decision), a device-wide dependency per frame -- so this engine is a loop of
// launches over frames, not one walk per lane as psfm_query.hip.  The per-lane text is psfm_query_pc.h (the CPU suite compiles it).
//
//   psfm_query_pc_init_kernel     the query itself into slab row t, one point per direction
//   per frame and direction:
//   psfm_query_pc_step_kernel     one lane per query: the lanes whose tail is this frame take the step of psfm_chain.h (the slow form in
//                                 a wave that holds a first step, as psfm_query_walk) -- 16 B load, 8 taps, 16 B store -- and decide
//                                 whether they are a row of this frame's solve; rows per wave from a ballot
//   psfm_query_pc_scan_kernel     one block: the rows in the waves before every wave and their total, integer sums in index order
//                                 (no block waits for another: the launch boundary does the ordering).  The host reads the total
//   psfm_query_pc_rows_kernel     the rows compacted in query order -- uv12, ref1, ref2, scale, owner: the f64 sums of the solve have
//                                 one order -- with the refs / scale arithmetic of pc_refs
//   psfm_solve_batch              the solve psfm_optimize_location runs, on those arrays (no solver kernel is touched)
//   psfm_query_pc_scatter_kernel  its result back into the two slab rows of the owners
//   A frame with no row runs no solve (the reference's np.stack([]) raises there).
// The finish -- births, lengths, offsets, CSR -- is psfm_query.hip's.
#include "psfm_device.h"
#include <cstring>

#include "psfm_internal.h"
#include "psfm_query_pc.h"

#define PSFM_QPC_BLOCK 256

__global__ __launch_bounds__(PSFM_QPC_BLOCK) void psfm_query_pc_init_kernel(const double2* __restrict__ q_xy, const int* __restrict__ q_t,
                                                                            unsigned Q, double2* __restrict__ slab, int* __restrict__ len_f,
                                                                            int* __restrict__ len_b)
{
    const unsigned q = blockIdx.x * PSFM_QPC_BLOCK + threadIdx.x;
    if (q >= Q) return;
    psfm_st(slab + (size_t)q_t[q] * Q, q * 16u, q_xy[q]);     // the (t, q) entry is the query itself, in either direction
    len_f[q] = 1;
    len_b[q] = 1;
}

template <bool MB>
__global__ __launch_bounds__(PSFM_QPC_BLOCK) __attribute__((amdgpu_waves_per_eu(8, 8))) void psfm_query_pc_step_kernel(PsfmQueryPcFrame a)
{
    const unsigned q = blockIdx.x * PSFM_QPC_BLOCK + threadIdx.x;
    const bool has_query = q < a.Q;
    int t = 0, n = 0;
    if (has_query) { t = a.q_t[q]; n = a.len[q]; }
    const bool take = has_query & psfm_query_pc_tail_at(t, n, a.from, a.dir);
    bool row = false;
    if (psfm_query_any(take)) {
        const bool slow = psfm_query_any(take & (n == 1));    // a caller-given position: the tap geometry with the true division
        if (take) {
            if (slow) row = psfm_query_pc_step<MB, false>(a, q, n);
            else row = psfm_query_pc_step<MB, true>(a, q, n);
        }
    }
    const unsigned long long rows = __ballot(row);
    if (psfm_lane_id() == 0) a.wave_cnt[q / PSFM_WAVE] = __popcll(rows);   // (every wave of the grid: the scan reads no stale count)
}

// one block: wave_cnt[k] <- rows in the waves before k (index order); *total <- rows of the frame
__global__ __launch_bounds__(PSFM_QPC_BLOCK) void psfm_query_pc_scan_kernel(int* __restrict__ wave_cnt, unsigned n_waves, int* __restrict__ total)
{
    __shared__ int s_wave[PSFM_QPC_BLOCK / PSFM_WAVE];
    const int lane = psfm_lane_id(), wave = (int)threadIdx.x / PSFM_WAVE;
    int carry = 0;
    for (unsigned k0 = 0; k0 < n_waves; k0 += PSFM_QPC_BLOCK) {
        const unsigned k = k0 + threadIdx.x;
        const int v = k < n_waves ? wave_cnt[k] : 0;
        int inc = v;
#pragma unroll
        for (int d = 1; d < PSFM_WAVE; d <<= 1) {
            const int u = __shfl_up(inc, d, PSFM_WAVE);
            if (lane >= d) inc += u;
        }
        if (lane == PSFM_WAVE - 1) s_wave[wave] = inc;
        __syncthreads();
        int base = 0, tot = 0;
#pragma unroll
        for (int j = 0; j < PSFM_QPC_BLOCK / PSFM_WAVE; ++j) {
            if (j < wave) base += s_wave[j];
            tot += s_wave[j];
        }
        __syncthreads();
        if (k < n_waves) wave_cnt[k] = carry + base + inc - v;
        carry += tot;
    }
    if (threadIdx.x == 0) *total = carry;
}

__global__ __launch_bounds__(PSFM_QPC_BLOCK) void psfm_query_pc_rows_kernel(PsfmQueryPcFrame a, PsfmQueryPcRows r)
{
    const unsigned q = blockIdx.x * PSFM_QPC_BLOCK + threadIdx.x;
    const bool has_query = q < a.Q;
    int t = 0, n = 0;
    if (has_query) { t = a.q_t[q]; n = a.len[q]; }
    const bool row = has_query & psfm_query_pc_is_row(a, t, n);
    const unsigned long long rows = __ballot(row);
    if (row) psfm_query_pc_row(a, r, q, (unsigned)(a.wave_cnt[q / PSFM_WAVE] + psfm_rank_in(rows)));
}

__global__ __launch_bounds__(PSFM_QPC_BLOCK) void psfm_query_pc_scatter_kernel(PsfmQueryPcFrame a, const double2* __restrict__ out,
                                                                               const int* __restrict__ owner, unsigned n_rows)
{
    const unsigned i = blockIdx.x * PSFM_QPC_BLOCK + threadIdx.x;
    if (i < n_rows) psfm_query_pc_scatter(a, out, owner, i);
}

static inline size_t psfm_qpc_pad(size_t b) { return (b + 63) & ~(size_t)63; }

extern "C" psfm_status psfm_track_queries_optimize(psfm_ctx* c, const float* flows_f, const uint8_t* occ_f, const float* flows_f2,
                                                   const uint8_t* occ_f2, const float* flows_b, const uint8_t* occ_b, const float* flows_b2,
                                                   const uint8_t* occ_b2, int n_flows, int h, int w, const double* q_xy, const int32_t* q_t,
                                                   int64_t n_q, psfm_track_info* info, void* stream)
{
    if (!c) { psfm_set_error("ctx is NULL"); return PSFM_ERR_ARG; }
    // ---- arguments: before any allocation or launch ----
    if ((!flows_f && !flows_b) || (flows_f != nullptr) != (occ_f != nullptr) || (flows_b != nullptr) != (occ_b != nullptr)) {
        psfm_set_error("psfm_track_queries_optimize: give at least one stack, and every stack with its occlusion maps");
        return PSFM_ERR_ARG;
    }
    if (n_flows < 1 || !psfm_frame_ok(h, w)) {
        psfm_set_error("psfm_track_queries_optimize: bad argument (n_flows=%d h=%d w=%d)", n_flows, h, w);
        return PSFM_ERR_ARG;
    }
    // a direction is its four pointers or none of them; with one flow no solve can happen and the stride-2 pointers may be NULL
    const bool s2_f_bad = (flows_f2 != nullptr) != (occ_f2 != nullptr) || (!flows_f && flows_f2) || (flows_f && !flows_f2 && n_flows >= 2);
    const bool s2_b_bad = (flows_b2 != nullptr) != (occ_b2 != nullptr) || (!flows_b && flows_b2) || (flows_b && !flows_b2 && n_flows >= 2);
    if (s2_f_bad || s2_b_bad) {
        psfm_set_error("psfm_track_queries_optimize: every stride-1 stack needs its stride-2 stack and that stack's occlusion maps (n_flows=%d)",
                       n_flows);
        return PSFM_ERR_ARG;
    }
    // a frame row of the slab -- 16 bytes per query -- stays below 4 GB (32-bit lane offsets)
    if (n_q < 0 || n_q >= ((int64_t)1 << 28) || (n_q > 0 && (!q_xy || !q_t))) {
        psfm_set_error("psfm_track_queries_optimize: bad argument (n_q=%lld: 0 <= n_q < 2^28, q_xy and q_t on the device)", (long long)n_q);
        return PSFM_ERR_ARG;
    }
    PSFM_HIP(hipSetDevice(c->device));
    // the gate of psfm_optimize_location: exclusive if no other psfm call is in flight, and the solves may then run as resident launches
    PsfmGate gate(c->device, (c->chain_mode == 1 || c->resident_budget > 0) ? 0 : 1);
    hipStream_t s = (hipStream_t)stream;
    psfm_status st;
    const unsigned Q = (unsigned)n_q;
    const size_t P = (size_t)h * w;
    const unsigned nblk = (Q + PSFM_QPC_BLOCK - 1) / PSFM_QPC_BLOCK;
    const unsigned n_waves = nblk * (PSFM_QPC_BLOCK / PSFM_WAVE);
    int* h_total = (int*)((char*)c->host_pinned + 464);       // (448, 456: the first refused query, the points of the result)

    // ---- workspace: first refused query | len_f | len_b | block totals of the length scan | rows per wave, their total | the rows ----
    const size_t o_lenf = 64, o_lenb = o_lenf + psfm_qpc_pad((size_t)Q * 4), o_bsum = o_lenb + psfm_qpc_pad((size_t)Q * 4);
    const size_t o_wave = o_bsum + psfm_qpc_pad((size_t)(nblk + 1) * sizeof(int64_t)), o_total = o_wave + psfm_qpc_pad((size_t)n_waves * 4);
    const size_t o_owner = o_total + 64, o_uv = o_owner + psfm_qpc_pad((size_t)Q * 4), o_ref1 = o_uv + (size_t)Q * 32;
    const size_t o_ref2 = o_ref1 + (size_t)Q * 16, o_scale = o_ref2 + (size_t)Q * 16, o_out = o_scale + psfm_qpc_pad((size_t)Q * 8);
    if ((st = c->qr_ws.ensure(o_out + (size_t)Q * 32 + 64)) != PSFM_OK) return st;
    char* ws = c->qr_ws.as<char>();

    // ---- refusals: a non-finite coordinate, a frame outside [0, n_flows] -- before anything is tracked ----
    if ((st = psfm_query_refuse(c, "psfm_track_queries_optimize", q_xy, q_t, Q, n_flows, (unsigned long long*)ws, s)) != PSFM_OK) return st;

    // ---- from here on the call replaces the result (and the lane tables of an unfinished sharded run: the slab lives in the log) ----
    psfm_shard_abandon(c);
    c->res_gen++;
    c->solve_stats.clear();
    c->res_n_traj = c->res_n_points = 0;
    c->res_n_flows = n_flows;
    c->res_is_query = true;
    c->res_is_set = false;
    c->pc_persist_ok = gate.exclusive || c->resident_budget > 0;
    c->pc_giveups = 0;
    c->n_resident = c->n_iter_launches = 0;
    const size_t nq1 = Q > 0 ? Q : 1;
    if ((st = c->log.ensure(sizeof(double2) * (size_t)(n_flows + 1) * nq1)) != PSFM_OK) return st;
    if ((st = c->res_birth.ensure(sizeof(int) * nq1)) != PSFM_OK) return st;
    if ((st = c->res_len.ensure(sizeof(int) * nq1)) != PSFM_OK) return st;
    if ((st = c->res_off.ensure(sizeof(int64_t) * ((size_t)Q + 1))) != PSFM_OK) return st;
    int64_t iterations = 0;
    if (Q == 0) {
        PSFM_HIP(hipMemsetAsync(c->res_off.p, 0, sizeof(int64_t), s));
        PSFM_HIP(hipStreamSynchronize(s));
    } else {
        const bool mb = c->mb_enable;
        const uint8_t* mask_f = occ_f;
        const uint8_t* mask_b = occ_b;
        if (mb) {   // the kill maps (bit 0 occlusion, bit 1 motion boundary) of each stride-1 stack, from that stack's own flows
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
        int* len_f = (int*)(ws + o_lenf);
        int* len_b = (int*)(ws + o_lenb);
        int* d_total = (int*)(ws + o_total);
        double2* slab = c->log.as<double2>();
        double* out = (double*)(ws + o_out);
        PsfmQueryPcRows r;
        r.uv12 = (double2*)(ws + o_uv); r.ref1 = (double2*)(ws + o_ref1); r.ref2 = (double2*)(ws + o_ref2);
        r.scale = (double*)(ws + o_scale); r.owner = (int*)(ws + o_owner);
        PsfmQueryPcFrame a;
        memset(&a, 0, sizeof(a));
        a.fr.H = h; a.fr.W = w;
        a.fr.cw = (float)((double)(w - 1) / 2.0); a.fr.ch = (float)((double)(h - 1) / 2.0);
        a.fr.rcw = psfm_rcp_host(a.fr.cw); a.fr.rch = psfm_rcp_host(a.fr.ch);
        a.q_t = q_t; a.wave_cnt = (int*)(ws + o_wave); a.Q = Q;
        const dim3 grid(nblk), block(PSFM_QPC_BLOCK);
        hipLaunchKernelGGL(psfm_query_pc_init_kernel, grid, block, 0, s, (const double2*)q_xy, q_t, Q, slab, len_f, len_b);
        PSFM_HIP(hipGetLastError());
        for (int back = 0; back < 2; ++back) {
            const float2* flows = (const float2*)(back ? flows_b : flows_f);
            const float2* flows2 = (const float2*)(back ? flows_b2 : flows_f2);
            const uint8_t* masks = back ? mask_b : mask_f;
            const uint8_t* occ2 = back ? occ_b2 : occ_f2;
            if (!flows) continue;
            a.len = back ? len_b : len_f;
            a.dir = back ? -1 : 1;
            for (int k = 0; k < n_flows; ++k) {
                // forward: from frame k through map k; backward: from frame n_flows - k through map n_flows - k - 1 (frame f+1 -> f)
                const int from = back ? n_flows - k : k, to = from + a.dir, map = back ? from - 1 : from;
                a.from = from;
                a.fr.flow = flows + (size_t)map * P; a.fr.occ = masks + (size_t)map * P;
                a.row_p1 = slab + (size_t)from * Q; a.row_p2 = slab + (size_t)to * Q;
                a.row_p0 = nullptr; a.flow01 = a.flow02 = nullptr; a.occ02 = nullptr;
                if (k >= 1) {   // p0 one frame before `from`: the stride-1 map it was stepped through, the stride-2 map from its frame
                    const int p0 = from - a.dir, map01 = back ? from : from - 1, map02 = from - 1;
                    a.row_p0 = slab + (size_t)p0 * Q;
                    a.flow01 = flows + (size_t)map01 * P; a.flow02 = flows2 + (size_t)map02 * P; a.occ02 = occ2 + (size_t)map02 * P;
                }
                c->prof.begin(PSFM_PROF_CHAIN, s);
                if (mb) hipLaunchKernelGGL(psfm_query_pc_step_kernel<true>, grid, block, 0, s, a);
                else hipLaunchKernelGGL(psfm_query_pc_step_kernel<false>, grid, block, 0, s, a);
                c->prof.end(s);
                PSFM_HIP(hipGetLastError());
                if (k < 1) continue;
                hipLaunchKernelGGL(psfm_query_pc_scan_kernel, dim3(1), block, 0, s, a.wave_cnt, n_waves, d_total);
                PSFM_HIP(hipGetLastError());
                PSFM_HIP(hipMemcpyAsync(h_total, d_total, sizeof(int), hipMemcpyDeviceToHost, s));
                PSFM_HIP(hipStreamSynchronize(s));
                const int n_rows = *h_total;
                if (n_rows <= 0) continue;                      // no row: no solve
                if ((unsigned)n_rows > Q) { psfm_set_error("psfm_track_queries_optimize: %d rows of %u queries", n_rows, Q); return PSFM_ERR_HIP; }
                hipLaunchKernelGGL(psfm_query_pc_rows_kernel, grid, block, 0, s, a, r);
                PSFM_HIP(hipGetLastError());
                psfm_solve_stats ss;
                memset(&ss, 0, sizeof(ss));
                c->prof.begin(PSFM_PROF_SOLVER, s);
                st = psfm_solve_batch(c, (const double*)r.uv12, (const double*)r.ref1, (const double*)r.ref2, r.scale, (const float*)a.fr.flow,
                                      n_rows, w, h, out, &ss, s);
                c->prof.end(s);
                if (st != PSFM_OK) return st;
                c->solve_stats.push_back(ss);
                iterations += ss.iterations;
                hipLaunchKernelGGL(psfm_query_pc_scatter_kernel, dim3(((unsigned)n_rows + PSFM_QPC_BLOCK - 1) / PSFM_QPC_BLOCK), block, 0, s, a,
                                   (const double2*)out, (const int*)r.owner, (unsigned)n_rows);
                PSFM_HIP(hipGetLastError());
            }
        }
        int64_t npts = 0;
        if ((st = psfm_query_finish(c, q_t, flows_f ? len_f : nullptr, flows_b ? len_b : nullptr, Q, n_flows, (int64_t*)(ws + o_bsum), &npts,
                                    s)) != PSFM_OK)
            return st;
        c->res_n_traj = (int64_t)Q;
        c->res_n_points = npts;
    }
    if (info) {
        memset(info, 0, sizeof(*info));
        info->n_traj = c->res_n_traj;
        info->n_points = c->res_n_points;
        info->n_lanes_peak = (int64_t)Q;
        info->lane_capacity = (int64_t)Q;
        info->solver_iterations = iterations;
        info->n_solves = (int32_t)c->solve_stats.size();
        info->chain_mode = 5;
    }
    return PSFM_OK;
}
