// psfm_query_batch.hip -- psfm_track_queries_batch: the query points of up to 64 sequences (any frame sizes, any lengths) tracked
// through ONE set of launches.
//
// A small video with a few hundred queries fills one or two blocks of the device, and a psfm_track_queries call on it is its fixed
// cost: allocations, six to eight launches of a few blocks and three host synchronisations.  Here that cost is paid once per batch.
// The grids are flattened (psfm_query_batch.h): sequence b owns ceil(Q[b] / 256) blocks numbered inside the sequence, a block finds
// its sequence by a search in the inclusive prefix of the block counts, fills a PsfmQueryArgs from its row of the table of sequences
// in device memory and runs the UNCHANGED per-lane loop of the single call (psfm_query_walk, psfm_query.h).  Every context ends up
// with the bytes psfm_track_queries leaves in it.
//
//   psfm_query_batch_validate_kernel   per sequence the first query with a non-finite coordinate or a frame outside [0, n_flows[b]]
//                                      (one integer minimum per sequence: the only atomics of the unit)
//   psfm_query_batch_track_kernel      one lane per query, one launch per direction over the flattened blocks: the single kernel's
//                                      body, its arguments read from the table as scalars.  No LDS, no atomics, no barrier
//   psfm_query_batch_plan_kernel       birth, len, and the lengths scanned inside each flattened block
//   psfm_query_batch_scan_kernel       ... the block totals of ALL sequences scanned by one block, in block order; then per sequence
//                                      off[Q] and the point total the host reads back
//   psfm_query_batch_offsets_kernel    ... and added, relative to the sequence's first block: off of every context
//   psfm_query_batch_gather_kernel     slab rows -> the CSR of every context, through the table
// Integer sums in a fixed order: identical calls give identical bytes.  Three host synchronisations (validation, point totals, end);
// apart from the kill maps of the motion-boundary option (one launch per stack) the launches do not depend on the number of sequences.
#include "psfm_device.h"
#include <cstring>

#include "psfm_internal.h"
#include "psfm_query.h"
#include "psfm_query_batch.h"

static_assert(PSFM_QB_MAX == PSFM_BATCH_MAX, "one bound for every batch entry point");
#define QB_BLOCK PSFM_QB_BLOCK

// A field of the block's table row as a scalar.  The row's address is block-uniform, but the walk is only as cheap as the single
// kernel's when the compiler KNOWS that what it holds is the same in every lane (psfm_query_uniform, psfm_query.h): the slab row
// base, the map bases and the sampler constants then live in scalar registers, as kernel arguments do.
__device__ __forceinline__ int qb_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ unsigned qb_uniform(unsigned v) { return (unsigned)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ float qb_uniform(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
template <class T>
__device__ __forceinline__ T* qb_uniform(T* p)
{
    const unsigned long long v = (unsigned long long)p;
    const unsigned lo = qb_uniform((unsigned)v), hi = qb_uniform((unsigned)(v >> 32));
    return (T*)(((unsigned long long)hi << 32) | lo);
}

// the block's sequence (a scalar) and its row
#define QB_LOCATE()                                                                                     \
    const int b = qb_uniform(psfm_qb_find(blk_end, (int)blockIdx.x));                                   \
    const PsfmQbSeq& S = tab[b]

__global__ __launch_bounds__(QB_BLOCK) void psfm_query_batch_validate_kernel(const PsfmQbSeq* __restrict__ tab, const int* __restrict__ blk_end,
                                                                             unsigned long long* __restrict__ first_bad)
{
    QB_LOCATE();
    const unsigned q = psfm_qb_query((int)blockIdx.x, S.blk0, threadIdx.x);
    if (q >= S.Q) return;
    const double2 p = S.q_xy[q];
    const int t = S.q_t[q];
    const bool finite = fabs(p.x) <= 1.7976931348623157e308 && fabs(p.y) <= 1.7976931348623157e308;   // (NaN fails both)
    if (!finite || t < 0 || t > S.n_flows) atomicMin(&first_bad[b], (unsigned long long)q);
}

template <bool MB, bool BACK>
__global__ __launch_bounds__(QB_BLOCK) __attribute__((amdgpu_waves_per_eu(8, 8))) void psfm_query_batch_track_kernel(
    const PsfmQbSeq* __restrict__ tab, const int* __restrict__ blk_end)
{
    QB_LOCATE();
    PsfmQueryArgs a;                                           // (every field read before the first store, every one a scalar)
    a.flows = qb_uniform(BACK ? S.flows_b : S.flows_f);
    a.masks = qb_uniform(BACK ? S.masks_b : S.masks_f);
    a.q_xy = qb_uniform(S.q_xy); a.q_t = qb_uniform(S.q_t);
    a.slab = qb_uniform(S.slab);
    a.len = qb_uniform(BACK ? S.len_b : S.len_f);
    a.H = qb_uniform(S.H); a.W = qb_uniform(S.W); a.n_flows = qb_uniform(S.n_flows);
    a.Q = qb_uniform(S.Q); a.P = qb_uniform(S.P);
    a.cw = qb_uniform(S.cw); a.ch = qb_uniform(S.ch); a.rcw = qb_uniform(S.rcw); a.rch = qb_uniform(S.rch);
    const unsigned q = psfm_qb_query((int)blockIdx.x, qb_uniform(S.blk0), threadIdx.x);
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

// exclusive prefix of v over the block's threads (in thread order) and the block's total: psfm_query_block_scan of psfm_query.hip
__device__ __forceinline__ int64_t qb_block_scan(int64_t v, int64_t* total)
{
    __shared__ int64_t s_wave[QB_BLOCK / PSFM_WAVE];
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
    for (int k = 0; k < QB_BLOCK / PSFM_WAVE; ++k) {
        if (k < wave) base += s_wave[k];
        tot += s_wave[k];
    }
    __syncthreads();                                         // (the scan kernel calls this in a loop)
    *total = tot;
    return base + inc - v;
}

// off[q]: the prefix inside the block, for now
__global__ __launch_bounds__(QB_BLOCK) void psfm_query_batch_plan_kernel(const PsfmQbSeq* __restrict__ tab, const int* __restrict__ blk_end,
                                                                         int64_t* __restrict__ block_sum)
{
    QB_LOCATE();
    const unsigned q = psfm_qb_query((int)blockIdx.x, S.blk0, threadIdx.x);
    int n = 0;
    if (q < S.Q) {
        int birth;
        psfm_qb_join(S.q_t[q], S.len_f ? S.len_f[q] : 1, S.len_b ? S.len_b[q] : 1, &birth, &n);
        S.birth[q] = birth;
        S.len[q] = n;
    }
    int64_t total;
    const int64_t before = qb_block_scan((int64_t)n, &total);
    if (q < S.Q) S.off[q] = before;
    if (threadIdx.x == 0) block_sum[blockIdx.x] = total;
}

// one block: block_sum[k] <- sum of the flattened blocks before k, block_sum[n_blocks] <- the points of all sequences; then per
// sequence (one thread each) off[Q] of its CSR and its point total for the host
__global__ __launch_bounds__(QB_BLOCK) void psfm_query_batch_scan_kernel(const PsfmQbSeq* __restrict__ tab, const int* __restrict__ blk_end,
                                                                         int n_seq, int64_t* __restrict__ block_sum, unsigned n_blocks,
                                                                         int64_t* __restrict__ totals)
{
    int64_t carry = 0;
    for (unsigned b0 = 0; b0 < n_blocks; b0 += QB_BLOCK) {
        const unsigned k = b0 + threadIdx.x;
        const int64_t v = k < n_blocks ? block_sum[k] : 0;
        int64_t total;
        const int64_t before = qb_block_scan(v, &total);
        if (k < n_blocks) block_sum[k] = carry + before;
        carry += total;
    }
    if (threadIdx.x == 0) block_sum[n_blocks] = carry;
    __syncthreads();                                         // (the block's own stores to global memory, read below)
    const int b = threadIdx.x;
    if (b < n_seq) {
        const PsfmQbSeq& S = tab[b];
        const int64_t n = psfm_qb_points(block_sum, S.blk0, blk_end[b]);
        S.off[S.Q] = n;
        totals[b] = n;
    }
}

__global__ __launch_bounds__(QB_BLOCK) void psfm_query_batch_offsets_kernel(const PsfmQbSeq* __restrict__ tab, const int* __restrict__ blk_end,
                                                                            const int64_t* __restrict__ block_sum)
{
    QB_LOCATE();
    const unsigned q = psfm_qb_query((int)blockIdx.x, S.blk0, threadIdx.x);
    if (q < S.Q) S.off[q] = psfm_qb_offset(S.off[q], block_sum, (int)blockIdx.x, S.blk0);
}

struct PsfmQbOut { double2* p[PSFM_QB_MAX]; };              // every context's res_xy, sized behind the second synchronisation

__global__ __launch_bounds__(QB_BLOCK) void psfm_query_batch_gather_kernel(const PsfmQbSeq* __restrict__ tab, const int* __restrict__ blk_end,
                                                                           PsfmQbOut out)
{
    QB_LOCATE();
    const unsigned Q = qb_uniform(S.Q);
    const int n_flows = qb_uniform(S.n_flows);
    const double2* slab = qb_uniform(S.slab);
    double2* xy = qb_uniform(out.p[b]);
    const unsigned q = psfm_qb_query((int)blockIdx.x, qb_uniform(S.blk0), threadIdx.x);
    const bool has_query = q < Q;
    const int b0 = has_query ? S.birth[q] : n_flows + 1;
    const int e = has_query ? b0 + S.len[q] : 0;                // one past the last frame
    const int64_t o = has_query ? S.off[q] : 0;
    const int f_lo = psfm_query_wave_min(b0), f_hi = -psfm_query_wave_min(-e);
    for (int f = f_lo; f < f_hi; ++f)                         // (wave-uniform bounds; the row base is a scalar)
        if ((f >= b0) & (f < e)) xy[o + (f - b0)] = psfm_ld(slab + (size_t)f * Q, q * 16u);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
// pinned staging of the owner: what one copy brings to the device -- the table of sequences | the inclusive block prefix | the
// per-sequence "first refused query" slots, all ones -- and behind it what the synchronisations read back: the slots | the point totals
namespace {
struct QbUpload {
    PsfmQbSeq tab[PSFM_QB_MAX];
    int blk_end[PSFM_QB_MAX];
    unsigned long long first_bad[PSFM_QB_MAX];
};
struct QbStaging {
    QbUpload up;
    unsigned long long bad[PSFM_QB_MAX];
    int64_t totals[PSFM_QB_MAX];
};
}  // namespace

#define QB_LAUNCH(kernel, grid, ...)                                                                     \
    do {                                                                                                 \
        hipLaunchKernelGGL(kernel, dim3((unsigned)(grid)), dim3(QB_BLOCK), 0, s, __VA_ARGS__);           \
        ++own->qb_launches;                                                                              \
    } while (0)
#define QB_COPY(dst, src, bytes, kind) do { PSFM_HIP(hipMemcpyAsync(dst, src, bytes, kind, s)); ++own->qb_launches; } while (0)
#define QB_SYNC() do { PSFM_HIP(hipGetLastError()); PSFM_HIP(hipStreamSynchronize(s)); ++own->qb_syncs; } while (0)

template <bool BACK>
static void qb_launch_track(psfm_ctx* own, const PsfmQbSeq* tab, const int* blk_end, int blocks, bool mb, hipStream_t s)
{
    if (mb) QB_LAUNCH((psfm_query_batch_track_kernel<true, BACK>), blocks, tab, blk_end);
    else QB_LAUNCH((psfm_query_batch_track_kernel<false, BACK>), blocks, tab, blk_end);
}

// The call.  hooks == NULL: psfm_track_queries_batch.  With hooks (psfm_track_queries_optimize_batch, psfm_query_pc_batch.hip) the
// arguments are checked further, sequence by sequence in the same pass, and the caller's frame loop runs in place of the two tracking
// launches; everything around them -- staging, refusals, what happens to the contexts, the one length scan and the one CSR gather
// for all contexts -- is this function's.
psfm_status psfm_qb_run(psfm_ctx* const* ctxs, int n_seq, const float* const* flows_f, const uint8_t* const* occ_f,
                        const float* const* flows_b, const uint8_t* const* occ_b, const int* n_flows, const int* h, const int* w,
                        const double* const* q_xy, const int32_t* const* q_t, const int64_t* n_q, psfm_track_info* infos_host, void* stream,
                        const PsfmQbHooks* hooks)
{
    const char* who = hooks ? hooks->who : "psfm_track_queries_batch";
    // ---- arguments: before any allocation or launch ----
    if (!ctxs || n_seq < 1 || n_seq > PSFM_BATCH_MAX) {
        psfm_set_error("%s: bad argument (n_seq=%d of 1..%d)", who, n_seq, PSFM_BATCH_MAX);
        return PSFM_ERR_ARG;
    }
    for (int i = 0; i < n_seq; ++i) {
        if (!ctxs[i] || !ctxs[0] || ctxs[i]->device != ctxs[0]->device) {
            psfm_set_error("%s: context %d is NULL or on another device", who, i);
            return PSFM_ERR_ARG;
        }
        for (int j = 0; j < i; ++j)
            if (ctxs[j] == ctxs[i]) { psfm_set_error("%s: context %d given twice (one per sequence)", who, i); return PSFM_ERR_ARG; }
    }
    if ((!flows_f && !flows_b) || (flows_f != nullptr) != (occ_f != nullptr) || (flows_b != nullptr) != (occ_b != nullptr)) {
        psfm_set_error("%s: give at least one stack per sequence, and every stack with its occlusion maps", who);
        return PSFM_ERR_ARG;
    }
    psfm_status st;
    if (hooks && (st = hooks->check(hooks->user, -1)) != PSFM_OK) return st;
    if (!n_flows || !h || !w || !n_q) { psfm_set_error("%s: NULL argument (n_flows, h, w, n_q: one entry per sequence)", who); return PSFM_ERR_ARG; }
    int64_t nq[PSFM_QB_MAX], N = 0;
    for (int i = 0; i < n_seq; ++i) {
        if ((flows_f && (!flows_f[i] || !occ_f[i])) || (flows_b && (!flows_b[i] || !occ_b[i]))) {
            psfm_set_error("%s: sequence %d: a stack or its occlusion maps are NULL (a direction is given for the whole batch)", who, i);
            return PSFM_ERR_ARG;
        }
        if (n_flows[i] < 1 || !psfm_frame_ok(h[i], w[i])) {
            psfm_set_error("%s: sequence %d: bad argument (n_flows=%d h=%d w=%d)", who, i, n_flows[i], h[i], w[i]);
            return PSFM_ERR_ARG;
        }
        if (n_q[i] < 0 || (n_q[i] > 0 && (!q_xy || !q_t || !q_xy[i] || !q_t[i]))) {
            psfm_set_error("%s: sequence %d: bad argument (n_q=%lld: n_q >= 0, q_xy and q_t on the device)", who, i, (long long)n_q[i]);
            return PSFM_ERR_ARG;
        }
        // the 32-bit lane offset of a slab row (16 bytes per query) and the block count of the flattened grid
        if (n_q[i] >= ((int64_t)1 << 28) || (N += n_q[i]) >= ((int64_t)1 << 28)) {
            psfm_set_error("%s: sequence %d: 2^28 or more queries in the batch", who, i);
            return PSFM_ERR_ARG;
        }
        nq[i] = n_q[i];
        if (hooks && (st = hooks->check(hooks->user, i)) != PSFM_OK) return st;
        if (ctxs[i]->mb_enable != ctxs[0]->mb_enable) {      // (one kernel form per launch: all sequences with the second verdict, or none)
            psfm_set_error("%s: context %d has the motion-boundary option %s, context 0 has it %s: it must be "
                           "on every context or on none (each with its own threshold)", who, i, ctxs[i]->mb_enable ? "on" : "off",
                           ctxs[0]->mb_enable ? "on" : "off");
            return PSFM_ERR_ARG;
        }
    }
    psfm_ctx* own = ctxs[0];
    PSFM_HIP(hipSetDevice(own->device));
    PsfmGate gate(own->device, 0);
    hipStream_t s = (hipStream_t)stream;
    own->qb_launches = own->qb_syncs = 0;
    const bool mb = own->mb_enable;

    // ---- the owner's staging and workspace (no context's result lives there) ----
    PsfmQbGrid G;
    psfm_qb_grid(G, nq, n_seq);
    const int blocks = G.blocks;
    if (!own->qb_host) PSFM_HIP(hipHostMalloc(&own->qb_host, sizeof(QbStaging), hipHostMallocDefault));
    QbStaging* hs = (QbStaging*)own->qb_host;
    const size_t len_bytes = ((size_t)N * 4 + 63) & ~(size_t)63;
    const size_t o_lenb = len_bytes, o_bsum = 2 * len_bytes, o_tot = o_bsum + (size_t)(blocks + 1) * sizeof(int64_t);
    if ((st = own->qb_tab.ensure(sizeof(QbUpload))) != PSFM_OK) return st;
    if ((st = own->qb_ws.ensure(o_tot + PSFM_QB_MAX * sizeof(int64_t))) != PSFM_OK) return st;
    QbUpload* du = own->qb_tab.as<QbUpload>();
    const PsfmQbSeq* dtab = du->tab;
    const int* dend = du->blk_end;
    char* ws = own->qb_ws.as<char>();
    int64_t* bsum = (int64_t*)(ws + o_bsum);
    int64_t* dtot = (int64_t*)(ws + o_tot);

    memset(&hs->up, 0, sizeof(hs->up));
    memset(hs->up.first_bad, 0xff, sizeof(hs->up.first_bad));
    for (int i = 0; i < PSFM_QB_MAX; ++i) hs->up.blk_end[i] = G.blk_end[i];
    for (int i = 0; i < n_seq; ++i) {
        PsfmQbSeq& S = hs->up.tab[i];
        S.q_xy = nq[i] > 0 ? (const double2*)q_xy[i] : nullptr; S.q_t = nq[i] > 0 ? q_t[i] : nullptr;
        S.H = h[i]; S.W = w[i]; S.n_flows = n_flows[i]; S.Q = (unsigned)nq[i]; S.P = (unsigned)((size_t)h[i] * w[i]);
        S.cw = (float)((double)(w[i] - 1) / 2.0); S.ch = (float)((double)(h[i] - 1) / 2.0);
        S.rcw = psfm_rcp_host(S.cw); S.rch = psfm_rcp_host(S.ch);
        S.blk0 = G.blk0[i];
    }

    // ---- refusals: a non-finite coordinate, a frame outside [0, n_flows] -- before anything is tracked ----
    if (blocks > 0) {
        QB_COPY(du, &hs->up, sizeof(QbUpload), hipMemcpyHostToDevice);
        QB_LAUNCH(psfm_query_batch_validate_kernel, blocks, dtab, dend, du->first_bad);
        QB_COPY(hs->bad, du->first_bad, sizeof(hs->bad), hipMemcpyDeviceToHost);
        QB_SYNC();
        for (int i = 0; i < n_seq; ++i)
            if (hs->bad[i] != ~0ull) {
                psfm_set_error("%s: sequence %d: query %llu has a non-finite coordinate or a frame outside [0, %d]", who, i, hs->bad[i],
                               n_flows[i]);
                return PSFM_ERR_ARG;
            }
    }

    // ---- from here on the call replaces every context's result (and the lane tables of an unfinished sharded run: the slab lives in
    // the log) ----
    for (int i = 0; i < n_seq; ++i) {
        psfm_ctx* c = ctxs[i];
        psfm_shard_abandon(c);
        c->res_gen++;
        c->solve_stats.clear();
        c->res_n_traj = c->res_n_points = 0;
        c->res_n_flows = n_flows[i];
        c->res_is_query = true;
        c->res_is_set = false;
    }
    for (int i = 0; i < n_seq; ++i) {
        psfm_ctx* c = ctxs[i];
        const size_t nq1 = nq[i] > 0 ? (size_t)nq[i] : 1, P = (size_t)h[i] * w[i];
        if ((st = c->log.ensure(sizeof(double2) * (size_t)(n_flows[i] + 1) * nq1)) != PSFM_OK) return st;
        if ((st = c->res_birth.ensure(sizeof(int) * nq1)) != PSFM_OK) return st;
        if ((st = c->res_len.ensure(sizeof(int) * nq1)) != PSFM_OK) return st;
        if ((st = c->res_off.ensure(sizeof(int64_t) * ((size_t)nq[i] + 1))) != PSFM_OK) return st;
        PsfmQbSeq& S = hs->up.tab[i];
        S.flows_f = flows_f ? (const float2*)flows_f[i] : nullptr; S.masks_f = flows_f ? occ_f[i] : nullptr;
        S.flows_b = flows_b ? (const float2*)flows_b[i] : nullptr; S.masks_b = flows_b ? occ_b[i] : nullptr;
        if (mb && nq[i] > 0) {   // the kill maps (bit 0 occlusion, bit 1 motion boundary) of each stack being sampled, from that stack's own flows
            if ((st = c->kill.ensure((size_t)n_flows[i] * P * 2)) != PSFM_OK) return st;
            uint8_t* kf = c->kill.as<uint8_t>();
            uint8_t* kb = kf + (size_t)n_flows[i] * P;
            if (flows_f) {
                if ((st = psfm_launch_motion_boundary(flows_f[i], occ_f[i], n_flows[i], h[i], w[i], c->mb_thres, kf, s)) != PSFM_OK) return st;
                S.masks_f = kf;
            }
            if (flows_b) {
                if ((st = psfm_launch_motion_boundary(flows_b[i], occ_b[i], n_flows[i], h[i], w[i], c->mb_thres, kb, s)) != PSFM_OK) return st;
                S.masks_b = kb;
            }
        }
        S.slab = c->log.as<double2>();
        S.len_f = flows_f ? (int*)ws + G.q0[i] : nullptr;
        S.len_b = flows_b ? (int*)(ws + o_lenb) + G.q0[i] : nullptr;
        S.birth = c->res_birth.as<int>(); S.len = c->res_len.as<int>(); S.off = c->res_off.as<int64_t>();
    }
    QB_COPY(du, &hs->up, sizeof(QbUpload), hipMemcpyHostToDevice);
    if (blocks > 0) {
        own->prof.begin(PSFM_PROF_CHAIN, s);                    // (psfm_ctx_set_profiling on the owner: the tracking launches count as the chain step)
        if (hooks) {
            PsfmQbRun run;
            run.own = own; run.ctxs = ctxs; run.n_seq = n_seq; run.tab_host = hs->up.tab; run.tab = dtab; run.blk_end = dend;
            run.blocks = blocks; run.mb = mb; run.s = s;
            if ((st = hooks->track(hooks->user, run)) != PSFM_OK) return st;
        } else {
            if (flows_f) qb_launch_track<false>(own, dtab, dend, blocks, mb, s);
            if (flows_b) qb_launch_track<true>(own, dtab, dend, blocks, mb, s);
        }
        own->prof.end(s);
        PSFM_HIP(hipGetLastError());
        own->prof.begin(PSFM_PROF_FINALIZE, s);                 // lengths -> offsets -> CSR as the finalize
        QB_LAUNCH(psfm_query_batch_plan_kernel, blocks, dtab, dend, bsum);
    }
    QB_LAUNCH(psfm_query_batch_scan_kernel, 1, dtab, dend, n_seq, bsum, (unsigned)blocks, dtot);
    if (blocks > 0) QB_LAUNCH(psfm_query_batch_offsets_kernel, blocks, dtab, dend, (const int64_t*)bsum);
    QB_COPY(hs->totals, dtot, sizeof(int64_t) * (size_t)n_seq, hipMemcpyDeviceToHost);
    QB_SYNC();
    PsfmQbOut out;
    memset(&out, 0, sizeof(out));
    for (int i = 0; i < n_seq; ++i) {
        const int64_t npts = hs->totals[i];
        if ((st = ctxs[i]->res_xy.ensure(sizeof(double2) * (size_t)(npts > 0 ? npts : 1))) != PSFM_OK) return st;
        out.p[i] = ctxs[i]->res_xy.as<double2>();
    }
    if (blocks > 0) {
        QB_LAUNCH(psfm_query_batch_gather_kernel, blocks, dtab, dend, out);
        own->prof.end(s);
    }
    QB_SYNC();
    own->prof.collect();
    for (int i = 0; i < n_seq; ++i) {
        psfm_ctx* c = ctxs[i];
        c->res_n_traj = nq[i];
        c->res_n_points = hs->totals[i];
        if (infos_host) {
            psfm_track_info* info = &infos_host[i];
            memset(info, 0, sizeof(*info));
            info->n_traj = c->res_n_traj;
            info->n_points = c->res_n_points;
            info->n_lanes_peak = nq[i];
            info->lane_capacity = nq[i];
            info->chain_mode = hooks ? hooks->chain_mode : 6;
        }
    }
    return PSFM_OK;
}

extern "C" psfm_status psfm_track_queries_batch(psfm_ctx* const* ctxs, int n_seq, const float* const* flows_f, const uint8_t* const* occ_f,
                                                const float* const* flows_b, const uint8_t* const* occ_b, const int* n_flows, const int* h,
                                                const int* w, const double* const* q_xy, const int32_t* const* q_t, const int64_t* n_q,
                                                psfm_track_info* infos_host, void* stream)
{
    return psfm_qb_run(ctxs, n_seq, flows_f, occ_f, flows_b, occ_b, n_flows, h, w, q_xy, q_t, n_q, infos_host, stream, nullptr);
}

extern "C" psfm_status psfm_query_batch_census(psfm_ctx* c, int32_t* launches, int32_t* host_syncs)
{
    if (!c) { psfm_set_error("ctx is NULL"); return PSFM_ERR_ARG; }
    if (launches) *launches = c->qb_launches;
    if (host_syncs) *host_syncs = c->qb_syncs;
    return PSFM_OK;
}
