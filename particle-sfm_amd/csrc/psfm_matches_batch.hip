// psfm_matches_batch.hip -- the saved sets (psfm_result_filter) and the match tables (psfm_traj_to_matches / psfm_labels_to_matches)
// of up to 64 sequences through ONE set of launches.
//
// Small sequences already share their frame launches (psfm_connect_batch) and the classifier's passes; the step behind them ran once
// per context: two host synchronisations for the filter and four for the tables, every one of them behind kernels of a few blocks.
// Here the pipeline of the header comment of psfm_matches.hip runs once over the concatenation of the sequences
// (psfm_matches_batch.h): flattened grids with blocks numbered inside a sequence, one global scan per count, the two stable sorts
// with the sequence above the key, and every output written straight into its context's own flt_* / mt_* buffers through a table of
// sequences in device memory that the host refreshes after each synchronisation has told it the sizes.  The number of
// synchronisations (2 and 4, the single calls') and of launches, copies and memsets does not depend on the number of sequences.
// Every context ends up with the bytes the single calls leave in it; the intermediates live once, in ctxs[0].
// Integer arithmetic and integer flags only; no block waits for another; two identical calls give identical bytes.
#include <string.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "psfm_device.h"
#include "psfm_internal.h"
#include "psfm_matches_batch.h"

static_assert(PSFM_MTB_MAX == PSFM_BATCH_MAX, "one bound for every batch entry point");
#define PMB_BLOCK PSFM_MTB_BLOCK
typedef unsigned long long pmb_u64;

// the block's sequence and the element of that sequence this thread owns
#define PMB_LOCATE(G)                                                                  \
    const int b = psfm_mtb_find((G).blk0, (int)blockIdx.x);                            \
    const int64_t i = (int64_t)((int)blockIdx.x - (G).blk0[b]) * PMB_BLOCK + threadIdx.x

// ---- the match tables ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PMB_BLOCK) void pmb_keep_kernel(const PsfmMtbSeq* __restrict__ tab, PsfmMtbGrid G, int64_t n_all,
                                                            int64_t* __restrict__ keep)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) keep[n_all] = 0;      // (the scan's total)
    PMB_LOCATE(G);
    const PsfmMtbSeq& S = tab[b];
    if (i >= S.n_pts) return;
    keep[S.pts0 + i] = !(S.labels && S.labels[i] != 0) ? 1 : 0;
}

// what a synchronisation reads back: per sequence the difference of a scan at its bases, and its bad-frame flag
__global__ __launch_bounds__(PSFM_MTB_MAX) void pmb_sizes_kernel(const PsfmMtbSeq* __restrict__ tab, int n_seq, int which,
                                                                const int64_t* __restrict__ scan, const int* __restrict__ bad,
                                                                int64_t* __restrict__ out)
{
    const int b = threadIdx.x;
    if (b >= n_seq) return;
    const PsfmMtbSeq& S = tab[b];
    const int64_t lo = which == 0 ? S.pts0 : (which == 1 ? S.kept0 : S.m0);
    const int64_t n = which == 0 ? S.n_pts : (which == 1 ? S.n_kept : S.n_m);
    out[b] = scan[lo + n] - scan[lo];
    out[PSFM_MTB_MAX + b] = bad ? (int64_t)bad[b] : 0;
}

// kept point q (index in the concatenation of the kept points): its (sequence, frame) key, its point, its trajectory
__global__ __launch_bounds__(PMB_BLOCK) void pmb_compact_kernel(const PsfmMtbSeq* __restrict__ tab, PsfmMtbGrid G,
                                                               const int64_t* __restrict__ q_of, int fbits, pmb_u64* __restrict__ kfr,
                                                               int64_t* __restrict__ kpt, int* __restrict__ ktraj,
                                                               unsigned* __restrict__ iota, int* __restrict__ bad)
{
    PMB_LOCATE(G);
    const PsfmMtbSeq& S = tab[b];
    if (i >= S.n_pts || (S.labels && S.labels[i] != 0)) return;
    const int64_t q = q_of[S.pts0 + i];
    const int t = psfm_mt_owner(S.off, S.k, i);
    bool outside;
    const unsigned f = psfm_mt_frame_index(psfm_mt_frame(S.frames, S.birth, S.off, t, i), S.n_img, &outside);
    if (outside) bad[b] = 1;
    kfr[q] = psfm_mtb_key(b, f, fbits);
    kpt[q] = i;
    ktraj[q] = t;
    iota[q] = (unsigned)q;
}

// fsorted == NULL: the zero-filled kp_off of a sequence that keeps nothing (or of a refused call)
__global__ __launch_bounds__(PMB_BLOCK) void pmb_kp_off_kernel(const PsfmMtbSeq* __restrict__ tab, PsfmMtbGrid G,
                                                              const pmb_u64* __restrict__ fsorted, int fbits)
{
    PMB_LOCATE(G);
    const PsfmMtbSeq& S = tab[b];
    if (i > S.n_img) return;
    S.kp_off[i] = fsorted ? psfm_mt_lower_bound<pmb_u64>(fsorted, S.kept0, S.kept0 + S.n_kept, psfm_mtb_key_mask(fbits), (pmb_u64)i) - S.kept0 : 0;
}

__global__ __launch_bounds__(PMB_BLOCK) void pmb_kp_kernel(const PsfmMtbSeq* __restrict__ tab, PsfmMtbGrid G,
                                                          const pmb_u64* __restrict__ fsorted, const unsigned* __restrict__ order,
                                                          const int64_t* __restrict__ kpt, int fbits, int* __restrict__ kp_ind)
{
    PMB_LOCATE(G);
    const PsfmMtbSeq& S = tab[b];
    if (i >= S.n_kept) return;
    const unsigned q = order[S.kept0 + i];
    kp_ind[q] = (int)(i - S.kp_off[fsorted[S.kept0 + i] & psfm_mtb_key_mask(fbits)]);
    S.kp_xy[i] = S.xy[kpt[q]];
}

__global__ __launch_bounds__(PMB_BLOCK) void pmb_count_kernel(const PsfmMtbSeq* __restrict__ tab, PsfmMtbGrid G, int64_t n_all,
                                                             const int* __restrict__ ktraj, const int64_t* __restrict__ q_of, int sample_k,
                                                             int64_t* __restrict__ m_cnt)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) m_cnt[n_all] = 0;
    PMB_LOCATE(G);
    const PsfmMtbSeq& S = tab[b];
    if (i >= S.n_kept) return;
    const int64_t q = S.kept0 + i;
    const int t = ktraj[q];
    const int64_t t0 = q_of[S.pts0 + S.off[t]];
    m_cnt[q] = psfm_mt_match_count(q_of[S.pts0 + S.off[t + 1]] - t0, q - t0, sample_k);
}

__global__ __launch_bounds__(PMB_BLOCK) void pmb_emit_kernel(const PsfmMtbSeq* __restrict__ tab, PsfmMtbGrid G, const int* __restrict__ ktraj,
                                                            const int64_t* __restrict__ q_of, int sample_k, const int64_t* __restrict__ m_off,
                                                            const pmb_u64* __restrict__ kfr, const int* __restrict__ kp_ind, int fbits,
                                                            int pbits, pmb_u64* __restrict__ key, pmb_u64* __restrict__ val,
                                                            int2* __restrict__ rows_u)
{
    PMB_LOCATE(G);
    const PsfmMtbSeq& S = tab[b];
    if (i >= S.n_kept) return;
    const int64_t q = S.kept0 + i;
    const int t = ktraj[q];
    const int64_t t0 = q_of[S.pts0 + S.off[t]];
    const int64_t n = q_of[S.pts0 + S.off[t + 1]] - t0, j = q - t0;
    int64_t reps, stride;
    psfm_mt_targets(n, sample_k, &reps, &stride);
    int64_t e = m_off[q];
    const pmb_u64 fmask = psfm_mtb_key_mask(fbits), fsrc = kfr[q] & fmask;
    const int ksrc = kp_ind[q];
    for (int64_t r = 0; r < reps; ++r) {
        const int64_t tl = r * stride;
        if (tl == j) continue;
        const int64_t tq = t0 + tl;
        key[e] = psfm_mtb_key(b, fsrc * (pmb_u64)S.n_img + (kfr[tq] & fmask), pbits);
        val[e] = (pmb_u64)e;
        rows_u[e] = make_int2(ksrc, kp_ind[tq]);
        ++e;
    }
}

__global__ __launch_bounds__(PMB_BLOCK) void pmb_rows_kernel(const PsfmMtbSeq* __restrict__ tab, PsfmMtbGrid G, int64_t n_all,
                                                            const pmb_u64* __restrict__ key_s, const pmb_u64* __restrict__ val_s,
                                                            const int2* __restrict__ rows_u, int64_t* __restrict__ flag)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) flag[n_all] = 0;
    PMB_LOCATE(G);
    const PsfmMtbSeq& S = tab[b];
    if (i >= S.n_m) return;
    const int64_t s = S.m0 + i;
    S.rows[i] = rows_u[val_s[s]];
    flag[s] = (i == 0 || key_s[s] != key_s[s - 1]) ? 1 : 0;       // (the composed key: equal pair keys of neighbouring sequences stay apart)
}

__global__ __launch_bounds__(PMB_BLOCK) void pmb_pairs_kernel(const PsfmMtbSeq* __restrict__ tab, PsfmMtbGrid G,
                                                             const pmb_u64* __restrict__ key_s, const pmb_u64* __restrict__ val_s,
                                                             const int64_t* __restrict__ gid, int pbits)
{
    PMB_LOCATE(G);
    const PsfmMtbSeq& S = tab[b];
    if (i >= S.n_m) return;
    const int64_t s = S.m0 + i, np = S.n_pairs;
    int64_t* pair_key = S.pairs; int64_t* pair_off = S.pairs + np; int64_t* pair_first = S.pairs + 2 * np + 1;
    if (i == 0) pair_off[np] = S.n_m;
    if (i == 0 || key_s[s] != key_s[s - 1]) {
        const int64_t g = gid[s] - gid[S.m0];
        pair_key[g] = (int64_t)(key_s[s] & psfm_mtb_key_mask(pbits));
        pair_off[g] = i;
        pair_first[g] = (int64_t)val_s[s] - S.m0;
    }
}

// ---- the saved sets --------------------------------------------------------------------------------------------------------------
#define PFB_LOCATE(G)                                                                  \
    const int b = psfm_mtb_find((G).blk0, (int)blockIdx.x);                            \
    const int64_t i = (int64_t)((int)blockIdx.x - (G).blk0[b]) * PMB_BLOCK + threadIdx.x

__global__ __launch_bounds__(PMB_BLOCK) void pfb_flag_kernel(const PsfmFltbSeq* __restrict__ tab, PsfmMtbGrid G, int64_t n_all, int min_len,
                                                            int64_t* __restrict__ flag)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) flag[n_all] = 0;
    PFB_LOCATE(G);
    const PsfmFltbSeq& S = tab[b];
    if (i >= S.n) return;
    flag[S.src0 + i] = psfm_flt_keep(S.len[i], min_len) ? 1 : 0;
}

// which 0: kept trajectories (scan over the flags of all trajectories); 1: kept points (scan over the kept lengths)
__global__ __launch_bounds__(PSFM_MTB_MAX) void pfb_sizes_kernel(const PsfmFltbSeq* __restrict__ tab, int n_seq, int which,
                                                                const int64_t* __restrict__ scan, int64_t* __restrict__ out)
{
    const int b = threadIdx.x;
    if (b >= n_seq) return;
    const PsfmFltbSeq& S = tab[b];
    const int64_t lo = which == 0 ? S.src0 : S.kept0, n = which == 0 ? S.n : S.k;
    out[b] = scan[lo + n] - scan[lo];
}

__global__ __launch_bounds__(PMB_BLOCK) void pfb_meta_kernel(const PsfmFltbSeq* __restrict__ tab, PsfmMtbGrid G, int64_t k_all, int min_len,
                                                            const int64_t* __restrict__ fq, int64_t* __restrict__ len64)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) len64[k_all] = 0;
    PFB_LOCATE(G);
    const PsfmFltbSeq& S = tab[b];
    if (i >= S.n) return;
    if (!psfm_flt_keep(S.len[i], min_len)) return;
    const int64_t r = fq[S.src0 + i] - fq[S.src0];        // rank among the kept trajectories of the sequence: ascending id order
    S.ids[r] = (int)i;
    psfm_flt_meta((int)i, r, S.birth, S.len, S.birth_out, S.len_out, len64 + S.kept0);
}

// the grid covers k + 1 entries of every sequence that keeps a trajectory
__global__ __launch_bounds__(PMB_BLOCK) void pfb_off_kernel(const PsfmFltbSeq* __restrict__ tab, PsfmMtbGrid G, const int64_t* __restrict__ lscan)
{
    PFB_LOCATE(G);
    const PsfmFltbSeq& S = tab[b];
    if (i > S.k) return;
    S.off_out[i] = lscan[S.kept0 + i] - lscan[S.kept0];
}

struct PfbXyOut { double2* p[PSFM_MTB_MAX]; };

// one wave per kept trajectory copies its run; the grid covers 64 lanes per kept trajectory
__global__ __launch_bounds__(PMB_BLOCK) void pfb_copy_kernel(const PsfmFltbSeq* __restrict__ tab, PsfmMtbGrid G, PfbXyOut out)
{
    const int b = psfm_mtb_find(G.blk0, (int)blockIdx.x);
    const PsfmFltbSeq& S = tab[b];
    const int lane = threadIdx.x & (PSFM_WAVE - 1);
    const int64_t t = (int64_t)((int)blockIdx.x - G.blk0[b]) * (PMB_BLOCK / PSFM_WAVE) + threadIdx.x / PSFM_WAVE;
    if (t >= S.k) return;
    const int id = S.ids[t];
    const int n = S.len[id];
    const int64_t src = S.off[id], dst = S.off_out[t];
    psfm_flt_copy_run(S.xy, src, out.p[b], dst, n, lane, PSFM_WAVE);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
namespace {
struct Census {
    psfm_ctx* own;
    void launch() { ++own->mtb_launches; }
    void sync() { ++own->mtb_syncs; }
};
}  // namespace

#define PMB_LAUNCH(kernel, grid, block, ...)                                                                   \
    do {                                                                                                       \
        hipLaunchKernelGGL(kernel, dim3((unsigned)(grid)), dim3(block), 0, s, __VA_ARGS__);                    \
        cz.launch();                                                                                           \
    } while (0)
#define PMB_COPY(dst, src, bytes, kind) do { PSFM_HIP(hipMemcpyAsync(dst, src, bytes, kind, s)); cz.launch(); } while (0)
#define PMB_SYNC() do { PSFM_HIP(hipGetLastError()); PSFM_HIP(hipStreamSynchronize(s)); cz.sync(); } while (0)

static psfm_status pmb_scan(psfm_ctx* own, int64_t* in, int64_t* out, size_t n, hipStream_t s)
{
    size_t bytes = 0;
    psfm_status st;
    PSFM_HIP(rocprim::exclusive_scan(nullptr, bytes, (int64_t*)nullptr, (int64_t*)nullptr, (int64_t)0, n, rocprim::plus<int64_t>(), s));
    if ((st = own->sort_tmp.ensure(bytes)) != PSFM_OK) return st;
    PSFM_HIP(rocprim::exclusive_scan(own->sort_tmp.p, bytes, in, out, (int64_t)0, n, rocprim::plus<int64_t>(), s));
    return PSFM_OK;
}

template <class V>
static psfm_status pmb_sort(psfm_ctx* own, pmb_u64* k_in, pmb_u64* k_out, V* v_in, V* v_out, size_t n, int bits, hipStream_t s)
{
    size_t bytes = 0;
    psfm_status st;
    PSFM_HIP(rocprim::radix_sort_pairs(nullptr, bytes, k_in, k_out, v_in, v_out, n, 0, bits, s));
    if ((st = own->sort_tmp.ensure(bytes)) != PSFM_OK) return st;
    PSFM_HIP(rocprim::radix_sort_pairs(own->sort_tmp.p, bytes, k_in, k_out, v_in, v_out, n, 0, bits, s));
    return PSFM_OK;
}

// the checks of psfm_connect_batch: 1 .. 64 contexts, none NULL, none twice, one device
static psfm_status pmb_check_ctxs(const char* who, psfm_ctx* const* ctxs, int n_seq)
{
    if (!ctxs || n_seq < 1 || n_seq > PSFM_BATCH_MAX) {
        psfm_set_error("%s: bad argument (n_seq=%d of at most %d)", who, n_seq, PSFM_BATCH_MAX);
        return PSFM_ERR_ARG;
    }
    for (int i = 0; i < n_seq; ++i) {
        if (!ctxs[i] || !ctxs[0] || ctxs[i]->device != ctxs[0]->device) { psfm_set_error("%s: context %d is NULL or on another device", who, i); return PSFM_ERR_ARG; }
        for (int j = 0; j < i; ++j) if (ctxs[j] == ctxs[i]) { psfm_set_error("%s: context %d given twice (one per sequence)", who, i); return PSFM_ERR_ARG; }
    }
    return PSFM_OK;
}

// pinned staging of the owner: the table of sequences, then 2 x 64 read-back words
static const size_t PMB_TAB_BYTES = (sizeof(PsfmMtbSeq) > sizeof(PsfmFltbSeq) ? sizeof(PsfmMtbSeq) : sizeof(PsfmFltbSeq)) * PSFM_MTB_MAX;
static const size_t PMB_SIZES_BYTES = 2 * PSFM_MTB_MAX * sizeof(int64_t);

static psfm_status pmb_staging(psfm_ctx* own)
{
    if (!own->mtb_host) PSFM_HIP(hipHostMalloc(&own->mtb_host, PMB_TAB_BYTES + PMB_SIZES_BYTES, hipHostMallocDefault));
    psfm_status st;
    if ((st = own->mtb_tab.ensure(PMB_TAB_BYTES)) != PSFM_OK) return st;
    return own->mtb_sizes.ensure(PMB_SIZES_BYTES + 4 * PSFM_MTB_MAX);      // sizes | flags read back, then the kernels' bad-frame flags
}

static unsigned pmb_blocks(const PsfmMtbGrid& G) { return (unsigned)G.blocks; }

// The pipeline over the sources `src` describes; both routes run it and differ only in where a point's frame and label come from.
static psfm_status pmb_tables(const char* who, psfm_ctx* const* ctxs, int n_seq, const PsfmMatchSrc* src, const int* n_img, int sample_k,
                              int64_t* n_kp_host, int64_t* n_matches_host, int64_t* n_pairs_host, hipStream_t s)
{
    psfm_ctx* own = ctxs[0];
    const int B = n_seq;
    int64_t npts[PSFM_MTB_MAX], nimg1[PSFM_MTB_MAX], nk[PSFM_MTB_MAX], nm[PSFM_MTB_MAX], base[PSFM_MTB_MAX + 1];
    int64_t P = 0;
    int img_max = 1;
    for (int b = 0; b < B; ++b) {
        if (n_img[b] < 1) { psfm_set_error("%s: sequence %d: bad argument (n_img=%d)", who, b, n_img[b]); return PSFM_ERR_ARG; }
        npts[b] = (src[b].k == 0 || src[b].n_pts == 0) ? 0 : src[b].n_pts;
        nimg1[b] = (int64_t)n_img[b] + 1;
        P += npts[b];
        if (P >= 0xffffffffll) { psfm_set_error("%s: sequence %d: more than 2^32 points in the batch", who, b); return PSFM_ERR_ARG; }
        if (n_img[b] > img_max) img_max = n_img[b];
    }
    int fbits = 0, pbits = 0;
    const int fkey = psfm_mtb_key_bits(B, (pmb_u64)img_max, &fbits);
    const int pkey = psfm_mtb_key_bits(B, (pmb_u64)img_max * (pmb_u64)img_max, &pbits);
    if (!fkey || !pkey) {
        int b0 = 0;
        while (n_img[b0] != img_max) ++b0;
        psfm_set_error("%s: sequence %d: the sort key of %d sequences of up to n_img=%d images does not fit 64 bits", who, b0, B, img_max);
        return PSFM_ERR_ARG;
    }
    // ---- nothing has been touched so far ----
    PSFM_HIP(hipSetDevice(own->device));
    PsfmGate gate(own->device, 0);
    Census cz{own};
    own->mtb_syncs = own->mtb_launches = 0;
    psfm_status st;
    if ((st = pmb_staging(own)) != PSFM_OK) return st;
    PsfmMtbSeq* htab = (PsfmMtbSeq*)own->mtb_host;
    int64_t* hsz = (int64_t*)((char*)own->mtb_host + PMB_TAB_BYTES);
    PsfmMtbSeq* dtab = own->mtb_tab.as<PsfmMtbSeq>();
    int64_t* dsz = own->mtb_sizes.as<int64_t>();
    int* bad = (int*)((char*)own->mtb_sizes.p + PMB_SIZES_BYTES);
    psfm_mtb_bases(base, npts, B);
    for (int b = 0; b < B; ++b) {
        psfm_ctx* c = ctxs[b];
        n_kp_host[b] = n_matches_host[b] = n_pairs_host[b] = 0;
        c->mt_n_kp = c->mt_n_m = c->mt_n_pairs = 0; c->mt_n_img = n_img[b];
        c->db_src_live = false;
        if ((st = c->mt_kp_off.ensure(8 * (size_t)(n_img[b] + 1))) != PSFM_OK) return st;
        PsfmMtbSeq& S = htab[b];
        memset(&S, 0, sizeof(S));
        S.off = src[b].off; S.birth = src[b].birth; S.frames = src[b].frames; S.xy = src[b].xy; S.labels = src[b].labels;
        S.k = src[b].k; S.n_pts = npts[b]; S.n_img = n_img[b];
        S.pts0 = base[b];
        S.kp_off = c->mt_kp_off.as<int64_t>();
    }
    PsfmMtbGrid g_pts, g_img, g_kept, g_m;
    psfm_mtb_grid(g_pts, npts, B);
    psfm_mtb_grid(g_img, nimg1, B);
    if (g_pts.blocks < 0 || g_img.blocks < 0) { psfm_set_error("%s: more blocks than a launch takes", who); return PSFM_ERR_ARG; }
    PMB_COPY(dtab, htab, sizeof(PsfmMtbSeq) * (size_t)B, hipMemcpyHostToDevice);
    PMB_LAUNCH(pmb_kp_off_kernel, pmb_blocks(g_img), PMB_BLOCK, (const PsfmMtbSeq*)dtab, g_img, (const pmb_u64*)nullptr, fbits);
    if (P == 0) { PMB_SYNC(); return PSFM_OK; }
    // ---- keep + compaction ----
    if ((st = own->mt_q.ensure(8 * (size_t)(P + 1))) != PSFM_OK) return st;
    if ((st = own->scan_tmp.ensure(8 * (size_t)(P + 1))) != PSFM_OK) return st;
    int64_t* q_of = own->mt_q.as<int64_t>();
    PMB_LAUNCH(pmb_keep_kernel, pmb_blocks(g_pts), PMB_BLOCK, (const PsfmMtbSeq*)dtab, g_pts, P, own->scan_tmp.as<int64_t>());
    if ((st = pmb_scan(own, own->scan_tmp.as<int64_t>(), q_of, (size_t)(P + 1), s)) != PSFM_OK) return st;
    PMB_LAUNCH(pmb_sizes_kernel, 1, PSFM_MTB_MAX, (const PsfmMtbSeq*)dtab, B, 0, (const int64_t*)q_of, (const int*)nullptr, dsz);
    PMB_COPY(hsz, dsz, PMB_SIZES_BYTES, hipMemcpyDeviceToHost);
    PMB_SYNC();
    int64_t K = 0;
    for (int b = 0; b < B; ++b) {
        psfm_ctx* c = ctxs[b];
        nk[b] = hsz[b];
        htab[b].kept0 = K; htab[b].n_kept = nk[b];
        K += nk[b];
        c->mt_n_kp = nk[b];
        n_kp_host[b] = nk[b];
        if (nk[b] > 0 && (st = c->mt_kp_xy.ensure(16 * (size_t)nk[b])) != PSFM_OK) return st;
        htab[b].kp_xy = c->mt_kp_xy.as<double2>();
    }
    if (K == 0) return PSFM_OK;
    psfm_mtb_grid(g_kept, nk, B);
    // per kept point: key (sequence, frame), flat point, trajectory, keypoint index; frame-sorted copies
    const size_t a4 = ((size_t)K * 4 + 255) / 256 * 256, a8 = ((size_t)K * 8 + 255) / 256 * 256;
    if ((st = own->mt_pts.ensure(3 * a8 + 4 * a4)) != PSFM_OK) return st;
    char* w = (char*)own->mt_pts.p;
    pmb_u64* kfr = (pmb_u64*)w; pmb_u64* fsorted = (pmb_u64*)(w + a8); int64_t* kpt = (int64_t*)(w + 2 * a8);
    unsigned* iota = (unsigned*)(w + 3 * a8); unsigned* order = (unsigned*)(w + 3 * a8 + a4); int* ktraj = (int*)(w + 3 * a8 + 2 * a4);
    int* kp_ind = (int*)(w + 3 * a8 + 3 * a4);
    PMB_COPY(dtab, htab, sizeof(PsfmMtbSeq) * (size_t)B, hipMemcpyHostToDevice);
    PSFM_HIP(hipMemsetAsync(bad, 0, 4 * PSFM_MTB_MAX, s)); cz.launch();
    PMB_LAUNCH(pmb_compact_kernel, pmb_blocks(g_pts), PMB_BLOCK, (const PsfmMtbSeq*)dtab, g_pts, (const int64_t*)q_of, fbits, kfr, kpt, ktraj,
               iota, bad);
    if ((st = pmb_sort(own, kfr, fsorted, iota, order, (size_t)K, fkey, s)) != PSFM_OK) return st;
    PMB_LAUNCH(pmb_kp_off_kernel, pmb_blocks(g_img), PMB_BLOCK, (const PsfmMtbSeq*)dtab, g_img, (const pmb_u64*)fsorted, fbits);
    PMB_LAUNCH(pmb_kp_kernel, pmb_blocks(g_kept), PMB_BLOCK, (const PsfmMtbSeq*)dtab, g_kept, (const pmb_u64*)fsorted, (const unsigned*)order,
               (const int64_t*)kpt, fbits, kp_ind);
    // ---- matches: count, scan, emit in loop order ----
    if ((st = own->mt_moff.ensure(8 * (size_t)(K + 1))) != PSFM_OK) return st;
    if ((st = own->scan_tmp.ensure(8 * (size_t)(K + 1))) != PSFM_OK) return st;
    int64_t* m_off = own->mt_moff.as<int64_t>();
    PMB_LAUNCH(pmb_count_kernel, pmb_blocks(g_kept), PMB_BLOCK, (const PsfmMtbSeq*)dtab, g_kept, K, (const int*)ktraj, (const int64_t*)q_of,
               sample_k, own->scan_tmp.as<int64_t>());
    if ((st = pmb_scan(own, own->scan_tmp.as<int64_t>(), m_off, (size_t)(K + 1), s)) != PSFM_OK) return st;
    PMB_LAUNCH(pmb_sizes_kernel, 1, PSFM_MTB_MAX, (const PsfmMtbSeq*)dtab, B, 1, (const int64_t*)m_off, (const int*)bad, dsz);
    PMB_COPY(hsz, dsz, PMB_SIZES_BYTES, hipMemcpyDeviceToHost);
    PMB_SYNC();
    for (int b = 0; b < B; ++b) {
        if (hsz[PSFM_MTB_MAX + b] == 0) continue;
        // every context of the call is left with empty tables
        for (int a = 0; a < B; ++a) { ctxs[a]->mt_n_kp = 0; n_kp_host[a] = 0; }
        PMB_LAUNCH(pmb_kp_off_kernel, pmb_blocks(g_img), PMB_BLOCK, (const PsfmMtbSeq*)dtab, g_img, (const pmb_u64*)nullptr, fbits);
        PMB_SYNC();
        psfm_set_error("%s: sequence %d: a trajectory has a frame outside [0, n_img=%d)", who, b, n_img[b]);
        return PSFM_ERR_ARG;
    }
    int64_t M = 0;
    for (int b = 0; b < B; ++b) {
        psfm_ctx* c = ctxs[b];
        nm[b] = hsz[b];
        htab[b].m0 = M; htab[b].n_m = nm[b];
        M += nm[b];
        c->mt_n_m = nm[b];
        n_matches_host[b] = nm[b];
        if (nm[b] > 0 && (st = c->mt_rows.ensure(8 * (size_t)nm[b])) != PSFM_OK) return st;
        htab[b].rows = c->mt_rows.as<int2>();
    }
    if (M == 0) return PSFM_OK;
    psfm_mtb_grid(g_m, nm, B);
    if (g_m.blocks < 0) { psfm_set_error("%s: more blocks than a launch takes", who); return PSFM_ERR_ARG; }
    const size_t m8 = ((size_t)M * 8 + 255) / 256 * 256;
    if ((st = own->mt_keys.ensure(5 * m8)) != PSFM_OK) return st;
    char* mk = (char*)own->mt_keys.p;
    pmb_u64* key = (pmb_u64*)mk; pmb_u64* key_s = (pmb_u64*)(mk + m8); pmb_u64* val = (pmb_u64*)(mk + 2 * m8); pmb_u64* val_s = (pmb_u64*)(mk + 3 * m8);
    int2* rows_u = (int2*)(mk + 4 * m8);
    PMB_COPY(dtab, htab, sizeof(PsfmMtbSeq) * (size_t)B, hipMemcpyHostToDevice);
    PMB_LAUNCH(pmb_emit_kernel, pmb_blocks(g_kept), PMB_BLOCK, (const PsfmMtbSeq*)dtab, g_kept, (const int*)ktraj, (const int64_t*)q_of, sample_k,
               (const int64_t*)m_off, (const pmb_u64*)kfr, (const int*)kp_ind, fbits, pbits, key, val, rows_u);
    if ((st = pmb_sort(own, key, key_s, val, val_s, (size_t)M, pkey, s)) != PSFM_OK) return st;
    // ---- rows in (sequence, pair, loop) order; pair boundaries ----
    if ((st = own->scan_tmp.ensure(8 * (size_t)(M + 1))) != PSFM_OK) return st;
    if ((st = own->mt_gid.ensure(8 * (size_t)(M + 1))) != PSFM_OK) return st;
    int64_t* gid = own->mt_gid.as<int64_t>();
    PMB_LAUNCH(pmb_rows_kernel, pmb_blocks(g_m), PMB_BLOCK, (const PsfmMtbSeq*)dtab, g_m, M, (const pmb_u64*)key_s, (const pmb_u64*)val_s,
               (const int2*)rows_u, own->scan_tmp.as<int64_t>());
    if ((st = pmb_scan(own, own->scan_tmp.as<int64_t>(), gid, (size_t)(M + 1), s)) != PSFM_OK) return st;
    PMB_LAUNCH(pmb_sizes_kernel, 1, PSFM_MTB_MAX, (const PsfmMtbSeq*)dtab, B, 2, (const int64_t*)gid, (const int*)nullptr, dsz);
    PMB_COPY(hsz, dsz, PMB_SIZES_BYTES, hipMemcpyDeviceToHost);
    PMB_SYNC();
    for (int b = 0; b < B; ++b) {
        psfm_ctx* c = ctxs[b];
        const int64_t np = hsz[b];
        htab[b].n_pairs = np;
        c->mt_n_pairs = np;
        n_pairs_host[b] = np;
        if (nm[b] > 0 && (st = c->mt_pairs.ensure(8 * (size_t)(3 * np + 1))) != PSFM_OK) return st;
        htab[b].pairs = c->mt_pairs.as<int64_t>();
    }
    PMB_COPY(dtab, htab, sizeof(PsfmMtbSeq) * (size_t)B, hipMemcpyHostToDevice);
    PMB_LAUNCH(pmb_pairs_kernel, pmb_blocks(g_m), PMB_BLOCK, (const PsfmMtbSeq*)dtab, g_m, (const pmb_u64*)key_s, (const pmb_u64*)val_s,
               (const int64_t*)gid, pbits);
    PMB_SYNC();
    return PSFM_OK;
}

extern "C" psfm_status psfm_traj_to_matches_batch(psfm_ctx* const* ctxs, int n_seq, const int* n_img, int sample_k,
                                                  const uint8_t* const* labels_dev, int64_t* n_kp_host, int64_t* n_matches_host,
                                                  int64_t* n_pairs_host, void* stream)
{
    const char* who = "psfm_traj_to_matches_batch";
    psfm_status st;
    if ((st = pmb_check_ctxs(who, ctxs, n_seq)) != PSFM_OK) return st;
    if (!n_img || !n_kp_host || !n_matches_host || !n_pairs_host || sample_k < 1) {
        psfm_set_error("%s: bad argument (sample_k=%d)", who, sample_k);
        return PSFM_ERR_ARG;
    }
    PsfmMatchSrc src[PSFM_MTB_MAX];
    for (int b = 0; b < n_seq; ++b) {
        psfm_ctx* c = ctxs[b];
        src[b].k = c->flt_n_traj; src[b].n_pts = c->flt_n_points;
        src[b].off = c->flt_off.as<int64_t>(); src[b].birth = c->flt_birth.as<int>(); src[b].xy = c->flt_xy.as<double2>();
        src[b].labels = labels_dev ? labels_dev[b] : nullptr;
    }
    return pmb_tables(who, ctxs, n_seq, src, n_img, sample_k, n_kp_host, n_matches_host, n_pairs_host, (hipStream_t)stream);
}

extern "C" psfm_status psfm_labels_to_matches_batch(psfm_ctx* const* ctxs, int n_seq, const int* n_img, int sample_k, int remove_dynamic,
                                                    int64_t* n_kp_host, int64_t* n_matches_host, int64_t* n_pairs_host, void* stream)
{
    const char* who = "psfm_labels_to_matches_batch";
    psfm_status st;
    if ((st = pmb_check_ctxs(who, ctxs, n_seq)) != PSFM_OK) return st;
    if (!n_img || !n_kp_host || !n_matches_host || !n_pairs_host || sample_k < 1) {
        psfm_set_error("%s: bad argument (sample_k=%d)", who, sample_k);
        return PSFM_ERR_ARG;
    }
    PsfmMatchSrc src[PSFM_MTB_MAX];
    for (int b = 0; b < n_seq; ++b) {
        psfm_ctx* c = ctxs[b];
        if (!c->lb_finished) { psfm_set_error("%s: sequence %d: no labelled set in the context (psfm_labels_finish)", who, b); return PSFM_ERR_ARG; }
        src[b].k = c->lb_n_traj; src[b].n_pts = c->lb_n_points;
        src[b].off = c->lb_off.as<int64_t>(); src[b].frames = c->lb_frames.as<int>(); src[b].xy = c->lb_xy.as<double2>();
        src[b].labels = remove_dynamic ? c->lb_labels.as<uint8_t>() : nullptr;       // matches_from_flow.py:71-74
    }
    return pmb_tables(who, ctxs, n_seq, src, n_img, sample_k, n_kp_host, n_matches_host, n_pairs_host, (hipStream_t)stream);
}

extern "C" psfm_status psfm_labels_sizes(psfm_ctx* c, int64_t* n_traj, int64_t* n_points)
{
    if (!c) { psfm_set_error("ctx is NULL"); return PSFM_ERR_ARG; }
    if (!c->lb_finished) { psfm_set_error("psfm_labels_sizes: no labelled set in the context (psfm_labels_finish)"); return PSFM_ERR_ARG; }
    if (n_traj) *n_traj = c->lb_n_traj;
    if (n_points) *n_points = c->lb_n_points;
    return PSFM_OK;
}

extern "C" psfm_status psfm_result_filter_batch(psfm_ctx* const* ctxs, int n_seq, int traj_min_len, int64_t* n_traj_host,
                                                int64_t* n_points_host, void* stream)
{
    const char* who = "psfm_result_filter_batch";
    psfm_status st;
    if ((st = pmb_check_ctxs(who, ctxs, n_seq)) != PSFM_OK) return st;
    if (!n_traj_host || !n_points_host) { psfm_set_error("%s: NULL argument", who); return PSFM_ERR_ARG; }
    for (int b = 0; b < n_seq; ++b) if (psfm_set_result_refuses(ctxs[b], traj_min_len, who)) return PSFM_ERR_ARG;
    const int B = n_seq;
    int64_t n[PSFM_MTB_MAX], k[PSFM_MTB_MAX], k1[PSFM_MTB_MAX], kw[PSFM_MTB_MAX], base[PSFM_MTB_MAX + 1];
    int64_t N = 0;
    for (int b = 0; b < B; ++b) {
        n[b] = ctxs[b]->res_n_traj;
        N += n[b];
        if (N >= 0x7fffffffll) { psfm_set_error("%s: sequence %d: more than 2^31 trajectories in the batch", who, b); return PSFM_ERR_ARG; }
    }
    psfm_ctx* own = ctxs[0];
    hipStream_t s = (hipStream_t)stream;
    PSFM_HIP(hipSetDevice(own->device));
    PsfmGate gate(own->device, 0);
    Census cz{own};
    own->mtb_syncs = own->mtb_launches = 0;
    for (int b = 0; b < B; ++b) {
        psfm_ctx* c = ctxs[b];
        n_traj_host[b] = n_points_host[b] = 0;
        c->flt_n_traj = c->flt_n_points = 0;
        c->res_gen++;        // (a new saved set: labels merged over the previous one are void, psfm_labels_begin)
    }
    if (N == 0) return PSFM_OK;
    if ((st = pmb_staging(own)) != PSFM_OK) return st;
    PsfmFltbSeq* htab = (PsfmFltbSeq*)own->mtb_host;
    int64_t* hsz = (int64_t*)((char*)own->mtb_host + PMB_TAB_BYTES);
    PsfmFltbSeq* dtab = own->mtb_tab.as<PsfmFltbSeq>();
    int64_t* dsz = own->mtb_sizes.as<int64_t>();
    psfm_mtb_bases(base, n, B);
    for (int b = 0; b < B; ++b) {
        psfm_ctx* c = ctxs[b];
        if (n[b] > 0 && (st = c->flt_ids.ensure(4 * (size_t)n[b])) != PSFM_OK) return st;
        PsfmFltbSeq& S = htab[b];
        memset(&S, 0, sizeof(S));
        S.birth = c->res_birth.as<int>(); S.len = c->res_len.as<int>(); S.off = c->res_off.as<int64_t>(); S.xy = c->res_xy.as<double2>();
        S.n = n[b]; S.src0 = base[b];
        S.ids = c->flt_ids.as<int>();
    }
    PsfmMtbGrid g_n, g_k1, g_w;
    psfm_mtb_grid(g_n, n, B);
    if ((st = own->scan_tmp.ensure(8 * (size_t)(N + 1))) != PSFM_OK) return st;
    if ((st = own->win_ws.ensure(8 * (size_t)(N + 1))) != PSFM_OK) return st;
    int64_t* fq = own->win_ws.as<int64_t>();
    PMB_COPY(dtab, htab, sizeof(PsfmFltbSeq) * (size_t)B, hipMemcpyHostToDevice);
    PMB_LAUNCH(pfb_flag_kernel, pmb_blocks(g_n), PMB_BLOCK, (const PsfmFltbSeq*)dtab, g_n, N, traj_min_len, own->scan_tmp.as<int64_t>());
    if ((st = pmb_scan(own, own->scan_tmp.as<int64_t>(), fq, (size_t)(N + 1), s)) != PSFM_OK) return st;
    PMB_LAUNCH(pfb_sizes_kernel, 1, PSFM_MTB_MAX, (const PsfmFltbSeq*)dtab, B, 0, (const int64_t*)fq, dsz);
    PMB_COPY(hsz, dsz, PMB_SIZES_BYTES, hipMemcpyDeviceToHost);
    PMB_SYNC();
    int64_t K = 0;
    for (int b = 0; b < B; ++b) {
        psfm_ctx* c = ctxs[b];
        k[b] = hsz[b];
        k1[b] = k[b] > 0 ? k[b] + 1 : 0;
        kw[b] = k[b] * PSFM_WAVE;
        htab[b].kept0 = K; htab[b].k = k[b];
        K += k[b];
        c->flt_n_traj = k[b];
        n_traj_host[b] = k[b];
        if (k[b] > 0) {
            if ((st = c->flt_birth.ensure(4 * (size_t)k[b])) != PSFM_OK) return st;
            if ((st = c->flt_len.ensure(4 * (size_t)k[b])) != PSFM_OK) return st;
            if ((st = c->flt_off.ensure(8 * (size_t)(k[b] + 1))) != PSFM_OK) return st;
        }
        htab[b].birth_out = c->flt_birth.as<int>(); htab[b].len_out = c->flt_len.as<int>(); htab[b].off_out = c->flt_off.as<int64_t>();
    }
    if (K == 0) return PSFM_OK;
    psfm_mtb_grid(g_k1, k1, B);
    psfm_mtb_grid(g_w, kw, B);
    if (g_w.blocks < 0) { psfm_set_error("%s: more blocks than a launch takes", who); return PSFM_ERR_ARG; }
    if ((st = own->mtb_len.ensure(8 * (size_t)(K + 1))) != PSFM_OK) return st;
    int64_t* len64 = own->mtb_len.as<int64_t>();
    int64_t* lscan = own->scan_tmp.as<int64_t>();        // (the flags are spent; K <= N)
    PMB_COPY(dtab, htab, sizeof(PsfmFltbSeq) * (size_t)B, hipMemcpyHostToDevice);
    PMB_LAUNCH(pfb_meta_kernel, pmb_blocks(g_n), PMB_BLOCK, (const PsfmFltbSeq*)dtab, g_n, K, traj_min_len, (const int64_t*)fq, len64);
    if ((st = pmb_scan(own, len64, lscan, (size_t)(K + 1), s)) != PSFM_OK) return st;
    PMB_LAUNCH(pfb_off_kernel, pmb_blocks(g_k1), PMB_BLOCK, (const PsfmFltbSeq*)dtab, g_k1, (const int64_t*)lscan);
    PMB_LAUNCH(pfb_sizes_kernel, 1, PSFM_MTB_MAX, (const PsfmFltbSeq*)dtab, B, 1, (const int64_t*)lscan, dsz);
    PMB_COPY(hsz, dsz, PMB_SIZES_BYTES, hipMemcpyDeviceToHost);
    PMB_SYNC();
    PfbXyOut out;
    for (int b = 0; b < PSFM_MTB_MAX; ++b) out.p[b] = nullptr;
    for (int b = 0; b < B; ++b) {
        psfm_ctx* c = ctxs[b];
        if (k[b] == 0) continue;
        const int64_t np_keep = hsz[b];
        c->flt_n_points = np_keep;
        n_points_host[b] = np_keep;
        if ((st = c->flt_xy.ensure(16 * (size_t)(np_keep > 0 ? np_keep : 1))) != PSFM_OK) return st;
        out.p[b] = c->flt_xy.as<double2>();
    }
    // (the destinations go by value: the table is not refreshed a third time, so nothing of this call is in flight from the pinned
    // staging when it returns -- like psfm_result_filter, it does not wait for the copy)
    PMB_LAUNCH(pfb_copy_kernel, pmb_blocks(g_w), PMB_BLOCK, (const PsfmFltbSeq*)dtab, g_w, out);
    PSFM_HIP(hipGetLastError());
    return PSFM_OK;
}

extern "C" psfm_status psfm_matches_batch_census(psfm_ctx* c, int32_t* host_syncs, int32_t* launches)
{
    if (!c) { psfm_set_error("ctx is NULL"); return PSFM_ERR_ARG; }
    if (host_syncs) *host_syncs = c->mtb_syncs;
    if (launches) *launches = c->mtb_launches;
    return PSFM_OK;
}
