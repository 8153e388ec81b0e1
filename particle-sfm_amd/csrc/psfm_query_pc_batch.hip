// psfm_query_pc_batch.hip -- psfm_track_queries_optimize_batch: the query points of up to 64 sequences (any frame sizes, any lengths)
// tracked with the stride-2 path-consistency solve after every step, through ONE set of launches per step.
//
// psfm_track_queries_optimize on a small video is its fixed cost: per frame a step launch, a one-block scan, a 4-byte copy with a
// synchronisation, a rows launch, three device-to-device copies, pc_init, four or more single-block iteration launches, one or more
// further synchronisations, the write-back and the scatter -- a few thousand host round trips around solves of one block each for a
// directory of 64 clips.  Here a step of ALL sequences is
//   psfm_qpb_step_kernel        one lane per query over the flattened blocks (psfm_query_batch.h): the single kernel's body, its
//                               arguments derived from the sequence's row of the table and the step number (psfm_query_pc_batch.h);
//                               a sequence that has no such step does nothing
//   psfm_qpb_scan_kernel        one block per sequence: rows in the waves before every wave, and the sequence's row count -- which
//                               stays in device memory: the host never reads it
//   psfm_qpb_rows_kernel        the rows compacted in query order straight into the solver's buffers of the sequence's own context
//   pc_multi init / iter        the launch chain over the table of problems, one grid for all (psfm_solver_multi.hip)
//   pc_multi poll               every control block into pinned memory, ONE synchronisation; the host launches further chunks of
//                               iterations until no problem is left undone -- pc_finish_sync's policy, applied to the batch -- and
//                               takes the solves' statistics from the same copy
//   pc_multi write-back, psfm_qpb_scatter_kernel   the result into the two slab rows of the owners
// Everything around the frame loop -- the refusals, what happens to the contexts, the kill maps of the motion-boundary option, the one
// length scan and the one CSR gather for all contexts -- is psfm_track_queries_batch's (psfm_qb_run, psfm_query_batch.hip).
// Every context ends up with what psfm_track_queries_optimize leaves in it on its sequence alone.
#include "psfm_device.h"
#include <cstring>

#include "psfm_internal.h"
#include "psfm_solver_internal.h"
#include "psfm_solver_multi.h"
#include "psfm_query_pc_batch.h"

#define QPB_BLOCK PSFM_QB_BLOCK
static_assert(QPB_BLOCK == PC_BLOCK, "one block size for the query grids and the solver's");

// a field of the block's table row as a scalar (qb_uniform of psfm_query_batch.hip)
__device__ __forceinline__ int qpb_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ unsigned qpb_uniform(unsigned v) { return (unsigned)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ float qpb_uniform(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
template <class T>
__device__ __forceinline__ T* qpb_uniform(T* p)
{
    const unsigned long long v = (unsigned long long)p;
    const unsigned lo = qpb_uniform((unsigned)v), hi = qpb_uniform((unsigned)(v >> 32));
    // ... and a pointer into GLOBAL memory, as a kernel argument is known to be: a pointer read from a table is generic to the compiler,
    // and every access through it a flat instruction with a 64-bit address per lane in place of scalar base + 32-bit lane offset
    typedef __attribute__((address_space(1))) T* G;
    return (T*)(G)(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ void qpb_uniform_frame(PsfmQueryPcFrame& a)
{
    a.fr.flow = qpb_uniform(a.fr.flow); a.fr.occ = qpb_uniform(a.fr.occ);
    a.flow01 = qpb_uniform(a.flow01); a.flow02 = qpb_uniform(a.flow02); a.occ02 = qpb_uniform(a.occ02);
    a.q_t = qpb_uniform(a.q_t); a.len = qpb_uniform(a.len); a.wave_cnt = qpb_uniform(a.wave_cnt);
    a.row_p0 = qpb_uniform(a.row_p0); a.row_p1 = qpb_uniform(a.row_p1); a.row_p2 = qpb_uniform(a.row_p2);
    a.Q = qpb_uniform(a.Q); a.from = qpb_uniform(a.from); a.dir = qpb_uniform(a.dir);
    a.fr.H = qpb_uniform(a.fr.H); a.fr.W = qpb_uniform(a.fr.W);
    a.fr.cw = qpb_uniform(a.fr.cw); a.fr.ch = qpb_uniform(a.fr.ch); a.fr.rcw = qpb_uniform(a.fr.rcw); a.fr.rch = qpb_uniform(a.fr.rch);
}

// the block's sequence (a scalar) and its row
#define QPB_LOCATE()                                                                                    \
    const int b = qpb_uniform(psfm_qb_find(blk_end, (int)blockIdx.x));                                  \
    const PsfmQpbSeq& S = tab[b]

// the query itself into slab row t, one point per direction (psfm_query_pc_init_kernel)
__global__ __launch_bounds__(QPB_BLOCK) void psfm_qpb_init_kernel(const PsfmQpbSeq* __restrict__ tab, const int* __restrict__ blk_end)
{
    QPB_LOCATE();
    const unsigned Q = qpb_uniform(S.Q);
    const unsigned q = psfm_qb_query((int)blockIdx.x, qpb_uniform(S.blk0), threadIdx.x);
    if (q >= Q) return;
    psfm_st(S.slab + (size_t)S.q_t[q] * Q, q * 16u, S.q_xy[q]);
    if (S.dir[0].len) S.dir[0].len[q] = 1;
    if (S.dir[1].len) S.dir[1].len[q] = 1;
}

// psfm_query_pc_step_kernel's body on the block's sequence
template <bool MB>
__global__ __launch_bounds__(QPB_BLOCK) __attribute__((amdgpu_waves_per_eu(8, 8))) void psfm_qpb_step_kernel(
    const PsfmQpbSeq* __restrict__ tab, const int* __restrict__ blk_end, int k, int back)
{
    QPB_LOCATE();
    if (!psfm_qpb_steps(k, qpb_uniform(S.n_flows))) return;          // the sequence has ended: nothing of it is touched
    PsfmQueryPcFrame a;
    psfm_qpb_frame(S, k, back, a);
    qpb_uniform_frame(a);
    const unsigned q = psfm_qb_query((int)blockIdx.x, qpb_uniform(S.blk0), threadIdx.x);
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
    if (psfm_lane_id() == 0) a.wave_cnt[q / PSFM_WAVE] = __popcll(rows);   // (every wave of the sequence's blocks)
}

// one block per sequence: psfm_query_pc_scan_kernel on the sequence's waves; the total stays on the device.  A sequence that has no
// solve in this step (it has ended, or has no query) gets the count 0.
__global__ __launch_bounds__(QPB_BLOCK) void psfm_qpb_scan_kernel(const PsfmQpbSeq* __restrict__ tab, int k)
{
    __shared__ int s_wave[QPB_BLOCK / PSFM_WAVE];
    const PsfmQpbSeq& S = tab[blockIdx.x];
    const unsigned n_waves = pc_multi_active(k, S.n_flows) ? (unsigned)S.n_blk * (QPB_BLOCK / PSFM_WAVE) : 0u;
    int* wave_cnt = S.wave_cnt;
    const int lane = psfm_lane_id(), wave = (int)threadIdx.x / PSFM_WAVE;
    int carry = 0;
    for (unsigned k0 = 0; k0 < n_waves; k0 += QPB_BLOCK) {
        const unsigned i = k0 + threadIdx.x;
        const int v = i < n_waves ? wave_cnt[i] : 0;
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
        for (int j = 0; j < QPB_BLOCK / PSFM_WAVE; ++j) {
            if (j < wave) base += s_wave[j];
            tot += s_wave[j];
        }
        __syncthreads();
        if (i < n_waves) wave_cnt[i] = carry + base + inc - v;
        carry += tot;
    }
    if (threadIdx.x == 0) *S.n_rows = carry;
}

__global__ __launch_bounds__(QPB_BLOCK) void psfm_qpb_rows_kernel(const PsfmQpbSeq* __restrict__ tab, const int* __restrict__ blk_end, int k,
                                                                   int back)
{
    QPB_LOCATE();
    if (!pc_multi_active(k, qpb_uniform(S.n_flows))) return;
    PsfmQueryPcFrame a;
    psfm_qpb_frame(S, k, back, a);
    qpb_uniform_frame(a);
    const unsigned q = psfm_qb_query((int)blockIdx.x, qpb_uniform(S.blk0), threadIdx.x);
    const bool has_query = q < a.Q;
    int t = 0, n = 0;
    if (has_query) { t = a.q_t[q]; n = a.len[q]; }
    const bool row = has_query & psfm_query_pc_is_row(a, t, n);
    const unsigned long long rows = __ballot(row);
    // (a rank is below the sequence's row count, which is at most Q: the rows the solver's buffers hold)
    if (row) psfm_qpb_row(a, S, q, (unsigned)(a.wave_cnt[q / PSFM_WAVE] + psfm_rank_in(rows)));
}

__global__ __launch_bounds__(QPB_BLOCK) void psfm_qpb_scatter_kernel(const PsfmQpbSeq* __restrict__ tab, const int* __restrict__ blk_end, int k,
                                                                      int back)
{
    QPB_LOCATE();
    if (!pc_multi_active(k, qpb_uniform(S.n_flows))) return;
    const unsigned i = psfm_qb_query((int)blockIdx.x, qpb_uniform(S.blk0), threadIdx.x);
    const int n_rows = *S.n_rows;
    const unsigned n = n_rows < 0 ? 0u : ((unsigned)n_rows < S.Q ? (unsigned)n_rows : S.Q);
    if (i >= n) return;
    PsfmQueryPcFrame a;
    psfm_qpb_frame(S, k, back, a);
    psfm_qpb_scatter(a, S, i);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
namespace {
struct QpbUpload {
    PsfmQpbSeq seq[PSFM_QB_MAX];
    PcMultiRow rows[2][PSFM_QB_MAX];            // the table of problems of each direction
};
struct QpbStaging {
    QpbUpload up;
    PcMultiPoll poll[PSFM_QB_MAX];              // what the poll kernel writes, read behind the synchronisation
};
struct QpbArgs {
    const float* const* flows[2];                                    // stride-1 (given or NULL for the whole batch)
    const float* const* flows2[2]; const uint8_t* const* occ2[2];    // stride-2
    const int* n_flows;
};
}  // namespace

#define QPB_WHO "psfm_track_queries_optimize_batch"
#define QPB_FIXED(n) do { own->qpb_fixed += (n); } while (0)
#define QPB_LAUNCH(kernel, grid, ...)                                                                    \
    do {                                                                                                 \
        hipLaunchKernelGGL(kernel, dim3((unsigned)(grid)), dim3(QPB_BLOCK), 0, s, __VA_ARGS__);          \
        QPB_FIXED(1);                                                                                    \
    } while (0)

// the stride-2 arguments: a direction is its four arrays or none of them; per sequence its four pointers -- with one flow no solve can
// happen and the stride-2 pointers may be NULL
static psfm_status qpb_check(void* user, int i)
{
    const QpbArgs& A = *(const QpbArgs*)user;
    for (int d = 0; d < 2; ++d) {
        const char* name = d ? "backward" : "forward";
        if (i < 0) {
            if ((A.flows2[d] != nullptr) != (A.occ2[d] != nullptr) || (!A.flows[d] && A.flows2[d])) {
                psfm_set_error(QPB_WHO ": the %s stride-2 stacks come with their occlusion maps and with the %s stride-1 stacks, or not at all",
                               name, name);
                return PSFM_ERR_ARG;
            }
            continue;
        }
        if (!A.flows[d]) continue;
        const float* f2 = A.flows2[d] ? A.flows2[d][i] : nullptr;
        const uint8_t* o2 = A.occ2[d] ? A.occ2[d][i] : nullptr;
        if ((f2 != nullptr) != (o2 != nullptr) || (!f2 && A.n_flows[i] >= 2)) {
            psfm_set_error(QPB_WHO ": sequence %d: the %s stride-1 stack needs its stride-2 stack and that stack's occlusion maps (n_flows=%d)",
                           i, name, A.n_flows[i]);
            return PSFM_ERR_ARG;
        }
    }
    return PSFM_OK;
}

static psfm_status qpb_track(void* user, const PsfmQbRun& run)
{
    const QpbArgs& A = *(const QpbArgs*)user;
    psfm_ctx* own = run.own;
    hipStream_t s = run.s;
    const int n_seq = run.n_seq, blocks = run.blocks;
    psfm_status st;
    if (!own->qpb_host) PSFM_HIP(hipHostMalloc(&own->qpb_host, sizeof(QpbStaging), hipHostMallocDefault));
    QpbStaging* hs = (QpbStaging*)own->qpb_host;
    const size_t wave_bytes = (((size_t)blocks * (QPB_BLOCK / PSFM_WAVE)) * sizeof(int) + 63) & ~(size_t)63;
    if ((st = own->qpb_tab.ensure(sizeof(QpbUpload))) != PSFM_OK) return st;
    if ((st = own->qpb_ws.ensure(wave_bytes + PSFM_QB_MAX * sizeof(int))) != PSFM_OK) return st;
    QpbUpload* du = own->qpb_tab.as<QpbUpload>();
    int* d_wave = own->qpb_ws.as<int>();
    int* d_rows = (int*)(own->qpb_ws.as<char>() + wave_bytes);
    PSFM_HIP(hipMemsetAsync(d_rows, 0, PSFM_QB_MAX * sizeof(int), s));
    QPB_FIXED(1);

    memset(&hs->up, 0, sizeof(hs->up));
    int cap[PSFM_QB_MAX], limit[PSFM_QB_MAX], max_flows = 0;
    for (int i = 0; i < n_seq; ++i) {
        const PsfmQbSeq& B = run.tab_host[i];
        PsfmQpbSeq& S = hs->up.seq[i];
        S.dir[0].flows = B.flows_f; S.dir[0].masks = B.masks_f; S.dir[0].len = B.len_f;
        S.dir[1].flows = B.flows_b; S.dir[1].masks = B.masks_b; S.dir[1].len = B.len_b;
        for (int d = 0; d < 2; ++d) {
            S.dir[d].flows2 = A.flows2[d] ? (const float2*)A.flows2[d][i] : nullptr;
            S.dir[d].occ2 = A.occ2[d] ? A.occ2[d][i] : nullptr;
        }
        S.q_xy = B.q_xy; S.q_t = B.q_t; S.slab = B.slab;
        S.H = B.H; S.W = B.W; S.n_flows = B.n_flows; S.Q = B.Q; S.P = B.P;
        S.cw = B.cw; S.ch = B.ch; S.rcw = B.rcw; S.rch = B.rch;
        S.blk0 = B.blk0; S.n_blk = psfm_qb_blocks_of((int64_t)B.Q);
        S.wave_cnt = d_wave + (size_t)B.blk0 * (QPB_BLOCK / PSFM_WAVE);
        S.n_rows = d_rows + i;
        cap[i] = 0; limit[i] = 1;
        for (int d = 0; d < 2; ++d) {                            // (a sequence without queries: a problem that never takes part)
            PcMultiRow& R = hs->up.rows[d][i];
            R.P.n_lanes_ptr = d_rows + i;
            R.limit = 1;
        }
        if (B.Q == 0) continue;
        psfm_ctx* c = run.ctxs[i];
        PcParams P;
        if ((st = pc_multi_problem(c, (int64_t)B.Q, B.H, B.W, P, &limit[i], s)) != PSFM_OK) return st;
        if ((st = c->qpb_owner.ensure(sizeof(int) * (size_t)B.Q)) != PSFM_OK) return st;
        cap[i] = (int)B.Q;
        P.n_lanes_ptr = d_rows + i;
        S.x1 = P.x1a; S.x2 = P.x2a; S.ref1 = P.ref1; S.ref2 = P.ref2; S.scale = P.scale; S.owner = c->qpb_owner.as<int>();
        for (int d = 0; d < 2; ++d) {
            if (!S.dir[d].flows) continue;
            PcMultiRow& R = hs->up.rows[d][i];
            R.P = P;
            R.P.flow12 = S.dir[d].flows;
            R.flow_stride = (int64_t)B.P;
            R.n_flows = B.n_flows; R.back = d; R.limit = limit[i];
        }
        if (B.n_flows > max_flows) max_flows = B.n_flows;
    }
    const int grid_x = pc_multi_grid_x(cap, limit, n_seq);
    PSFM_HIP(hipMemcpyAsync(du, &hs->up, sizeof(QpbUpload), hipMemcpyHostToDevice, s));
    QPB_FIXED(1);
    const PsfmQpbSeq* dseq = du->seq;
    const int* dend = run.blk_end;
    QPB_LAUNCH(psfm_qpb_init_kernel, blocks, dseq, dend);
    PSFM_HIP(hipGetLastError());
    for (int back = 0; back < 2; ++back) {
        if (!A.flows[back]) continue;
        const PcMultiRow* drows = du->rows[back];
        for (int k = 0; k < max_flows; ++k) {
            if (run.mb) QPB_LAUNCH(psfm_qpb_step_kernel<true>, blocks, dseq, dend, k, back);
            else QPB_LAUNCH(psfm_qpb_step_kernel<false>, blocks, dseq, dend, k, back);
            PSFM_HIP(hipGetLastError());
            if (k < 1) continue;
            QPB_LAUNCH(psfm_qpb_scan_kernel, n_seq, dseq, k);
            QPB_LAUNCH(psfm_qpb_rows_kernel, blocks, dseq, dend, k, back);
            pc_multi_launch_init(drows, grid_x, n_seq, k, s);
            QPB_FIXED(1);
            // pc_finish_sync's policy over the batch (pc_multi_pace): poll, and while any problem is left undone another chunk of iterations
            const PcPaceCensus census{&own->qpb_fixed, &own->qpb_iter, &own->qpb_syncs};
            st = pc_multi_pace([&](int n_launches) { pc_multi_launch_iter(drows, grid_x, n_seq, k, n_launches, s); },
                               [&]() { pc_multi_launch_poll(drows, n_seq, k, hs->poll, s); },
                               [&]() {
                                   bool undone = false;
                                   for (int i = 0; i < n_seq; ++i) undone = undone || (hs->poll[i].n_rows > 0 && !hs->poll[i].C.done);
                                   return undone;
                               },
                               census, s, QPB_WHO);
            if (st != PSFM_OK) return st;
            pc_multi_launch_writeback(drows, grid_x, n_seq, k, s);
            QPB_FIXED(1);
            QPB_LAUNCH(psfm_qpb_scatter_kernel, blocks, dseq, dend, k, back);
            PSFM_HIP(hipGetLastError());
            for (int i = 0; i < n_seq; ++i) {
                if (hs->poll[i].n_rows <= 0) continue;                // no row: no solve
                psfm_solve_stats ss;
                memset(&ss, 0, sizeof(ss));
                pc_multi_stats(&hs->poll[i].C, &ss);
                run.ctxs[i]->solve_stats.push_back(ss);
            }
        }
    }
    return PSFM_OK;
}

extern "C" psfm_status psfm_track_queries_optimize_batch(psfm_ctx* const* ctxs, int n_seq, const float* const* flows_f,
                                                         const uint8_t* const* occ_f, const float* const* flows_f2,
                                                         const uint8_t* const* occ_f2, const float* const* flows_b,
                                                         const uint8_t* const* occ_b, const float* const* flows_b2,
                                                         const uint8_t* const* occ_b2, const int* n_flows, const int* h, const int* w,
                                                         const double* const* q_xy, const int32_t* const* q_t, const int64_t* n_q,
                                                         psfm_track_info* infos_host, void* stream)
{
    QpbArgs A;
    memset(&A, 0, sizeof(A));
    A.flows[0] = flows_f; A.flows2[0] = flows_f2; A.occ2[0] = occ_f2;
    A.flows[1] = flows_b; A.flows2[1] = flows_b2; A.occ2[1] = occ_b2;
    A.n_flows = n_flows;
    PsfmQbHooks hooks;
    hooks.who = QPB_WHO; hooks.chain_mode = 7; hooks.check = qpb_check; hooks.track = qpb_track; hooks.user = &A;
    psfm_ctx* own = (ctxs && n_seq >= 1) ? ctxs[0] : nullptr;
    if (own) own->qpb_fixed = own->qpb_iter = own->qpb_syncs = 0;
    psfm_status st = psfm_qb_run(ctxs, n_seq, flows_f, occ_f, flows_b, occ_b, n_flows, h, w, q_xy, q_t, n_q, infos_host, stream, &hooks);
    if (st != PSFM_OK) return st;
    own->qpb_fixed += own->qb_launches;          // (the frame around the loop: table copy, validation, length scan, offsets, gather)
    own->qpb_syncs += own->qb_syncs;
    if (infos_host)
        for (int i = 0; i < n_seq; ++i) {
            int64_t it = 0;
            for (const psfm_solve_stats& q : ctxs[i]->solve_stats) it += q.iterations;
            infos_host[i].solver_iterations = it;
            infos_host[i].n_solves = (int32_t)ctxs[i]->solve_stats.size();
        }
    return PSFM_OK;
}

extern "C" psfm_status psfm_query_pc_batch_census(psfm_ctx* c, int32_t* launches_fixed, int32_t* launches_iter, int32_t* host_syncs)
{
    if (!c) { psfm_set_error("ctx is NULL"); return PSFM_ERR_ARG; }
    if (launches_fixed) *launches_fixed = c->qpb_fixed;
    if (launches_iter) *launches_iter = c->qpb_iter;
    if (host_syncs) *host_syncs = c->qpb_syncs;
    return PSFM_OK;
}
