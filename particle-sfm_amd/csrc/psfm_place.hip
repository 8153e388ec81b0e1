// psfm_place.hip -- finalize of the persistent loop, placed form: scan of the loop's birth masks, placement of the records by birth
// order, ONE stable radix pass on `last`.  What it computes, why it equals the four-pass sort, and every index: psfm_place.h.
//
// The pass's two kernels are siblings of psfm_sort_hist_kernel / psfm_sort_scatter_kernel (psfm_sort.hip: the structure, the stable
// wave-striped tile order and the measurements behind both are described there) with the digit taken from the top byte of the VALUE,
// where the placement put `last` beside the lane, instead of cut out of the key.  They live here so that the kernels of
// psfm_sort.hip, which every other path runs, stay the code they were.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "psfm_device.h"
#include "psfm_internal.h"
#include "psfm_place.h"

#define PL_BLOCK 256
#define PL_NW (PL_BLOCK / PSFM_WAVE)

// exclusive prefix of `mine` over the block's threads (in thread order) and the block's sum; s_w: PL_NW words of LDS
__device__ __forceinline__ int psfm_place_block_scan(int mine, int* s_w, int* sum)
{
    const int tid = threadIdx.x, lane = tid & (PSFM_WAVE - 1), wave = tid / PSFM_WAVE;
    int inc = mine;
#pragma unroll
    for (int o = 1; o < PSFM_WAVE; o <<= 1) {
        const int v = __shfl_up(inc, o);
        if (lane >= o) inc += v;
    }
    if (lane == PSFM_WAVE - 1) s_w[wave] = inc;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < PL_NW; ++w) { const int v = s_w[w]; if (w < wave) base += v; tot += v; }
    *sum = tot;
    return base + inc - mine;
}

// Block = frame b (row b of the mask table): start[b][vb] = births of frame b in the virtual blocks below vb, total[b] = births of
// frame b.  Row 0 is implied (psfm_place_count): only its total, G, is needed.  A thread takes `per` consecutive blocks of the row.
__global__ __launch_bounds__(PL_BLOCK) void psfm_place_scan_kernel(const unsigned long long* __restrict__ bmask, int G, int n_flows,
                                                                   int* __restrict__ start, int* __restrict__ total)
{
    __shared__ int s_w[PL_NW];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (b == 0) { if (tid == 0) total[0] = G; return; }
    const int gb = psfm_place_blocks(G);
    const int per = (gb + PL_BLOCK - 1) / PL_BLOCK;
    const int v0 = min(tid * per, gb), v1 = min(v0 + per, gb);
    int mine = 0;
    for (int v = v0; v < v1; ++v) mine += psfm_place_count(bmask, G, n_flows, b, v);
    int tot;
    int run = psfm_place_block_scan(mine, s_w, &tot);
    int* out = start + (int64_t)b * gb;
    for (int v = v0; v < v1; ++v) { out[v] = run; run += psfm_place_count(bmask, G, n_flows, b, v); }
    if (tid == 0) total[b] = tot;
}

// Block b = segment b of the loop (b == nblk: the shared tail), as in psfm_compact_segments_kernel, which this kernel replaces: every
// record (64-bit key, lane) goes to its position by (birth, rank among the births of its frame) in the one pass's input, as a 32-bit
// triangular key and last : lane.  The positions are a permutation of [0, n): nothing is counted here, no atomics.  A record whose
// fields point outside the tables or whose grid point the masks do not show as born (never seen; the masks and the records
// disagreeing would do it) is dropped, not stored out of bounds.
__global__ __launch_bounds__(PL_BLOCK) void psfm_place_records_kernel(
    const unsigned long long* __restrict__ fin_keys, const int* __restrict__ fin_lanes, const int2* __restrict__ seg_info, int nblk,
    int seg_cap, const PsfmCounters* __restrict__ ctr, int spill_cap, const unsigned long long* __restrict__ bmask,
    const int* __restrict__ start, const int* __restrict__ total, int G, int n_flows, PsfmKeyFmt fmt, unsigned* __restrict__ keys,
    int* __restrict__ vals, int64_t n)
{
    __shared__ int s_base[PSFM_PLACE_MAX_TIMES];
    __shared__ int s_w[PL_NW];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int gb = psfm_place_blocks(G), gw = psfm_place_words(G);
    {   // births of all frames in front of frame `tid`
        int tot;
        const int mine = tid < n_flows ? total[tid] : 0;
        s_base[tid] = psfm_place_block_scan(mine, s_w, &tot);
    }
    __syncthreads();
    const int count = b < nblk ? seg_info[b].x : min(ctr->spill_cnt, spill_cap);
    const long long src = (long long)b * seg_cap;
    // four records per thread in flight, in two rounds of loads: the records, then (from their fields) the four mask words of the
    // record's virtual block and frame -- one 32-byte sector -- and the block's start out of the table
    for (int i0 = 0; i0 < count; i0 += 4 * PL_BLOCK) {
        unsigned long long k[4];
        int l[4], last[4], bf[4], idx[4], st[4];
        ulonglong2 m[4][2];
        bool ok[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u * PL_BLOCK + tid;
            k[u] = i < count ? fin_keys[src + i] : 0ull;
            l[u] = i < count ? fin_lanes[src + i] : 0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u * PL_BLOCK + tid;
            psfm_key64_fields(k[u], fmt.shift_b, fmt.shift_d, &last[u], &bf[u], &idx[u]);
            ok[u] = i < count && bf[u] < n_flows && last[u] < PSFM_PLACE_MAX_TIMES && idx[u] < G &&
                    (unsigned)l[u] < (1u << PSFM_PLACE_LANE_BITS);
            const bool look = ok[u] && bf[u] > 0;
            const ulonglong2* row = (const ulonglong2*)(bmask + (int64_t)bf[u] * gw + (int64_t)PSFM_PLACE_VB_WORDS * (idx[u] / PSFM_PLACE_VB));
            m[u][0] = look ? row[0] : make_ulonglong2(0ull, 0ull);
            m[u][1] = look ? row[1] : make_ulonglong2(0ull, 0ull);
            st[u] = look ? start[(int64_t)bf[u] * gb + idx[u] / PSFM_PLACE_VB] : 0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (!ok[u]) continue;
            int64_t pos = idx[u];
            if (bf[u] > 0) {
                const unsigned long long w[PSFM_PLACE_VB_WORDS] = {m[u][0].x, m[u][0].y, m[u][1].x, m[u][1].y};
                if (!psfm_place_born(w, idx[u])) continue;
                pos = psfm_place_pos(s_base[bf[u]], st[u], psfm_place_ordinal(w, idx[u]));
            }
            if (pos >= 0 && pos < n) {
                keys[pos] = psfm_key32(k[u], fmt);
                vals[pos] = psfm_place_pack(l[u], last[u]);
            }
        }
    }
}

// ---- the one pass: stable, 8-bit digit `last`, tiles of 4096 keys read wave-striped (psfm_sort.hip) ----
#define PL_ITEMS 16
#define PL_TILE (PL_BLOCK * PL_ITEMS)
#define PL_WSPAN (PL_ITEMS * PSFM_WAVE)
#define PL_GROUP 8
#define PL_DIGITS 256
#define PL_GCHUNK 64
#define PL_HWAVES 2
#define PL_HREP 4                             // copies of a tile's counter row (a power of two)
#define PL_HBLOCK (PL_GROUP * PL_HWAVES * PSFM_WAVE)
#define PL_HITEMS (PL_TILE / (PL_HWAVES * PSFM_WAVE))
#define PL_PAD (PL_DIGITS - 1)                // digit of a tile's padding: last <= n_flows <= 255, and padding sits behind the tile's keys

__device__ __forceinline__ unsigned long long pl_match8(unsigned d)
{
    unsigned long long peers = ~0ull;
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
        const bool on = (d >> bit) & 1u;
        const unsigned long long m = __ballot(on);
        peers &= on ? m : ~m;
    }
    return peers;
}

// H.  Block = group of PL_GROUP tiles: per tile the digit counts as exclusive prefixes over the tiles of the group, their sum per group
__global__ __launch_bounds__(PL_HBLOCK) void psfm_place_hist_kernel(const int* __restrict__ vals, int64_t n, unsigned* __restrict__ cnt,
                                                                    unsigned* __restrict__ grp, int nb)
{
    __shared__ unsigned s_h[PL_GROUP][PL_HREP][PL_DIGITS];
    const int tid = threadIdx.x, lane = tid & (PSFM_WAVE - 1), wave = tid / PSFM_WAVE;
    for (int q = tid; q < PL_GROUP * PL_HREP * PL_DIGITS; q += PL_HBLOCK) (&s_h[0][0][0])[q] = 0u;
    const int t = wave / PL_HWAVES, part = wave % PL_HWAVES;
    const int b = blockIdx.x * PL_GROUP + t;
    const int64_t tile0 = (int64_t)b * PL_TILE;
    const int nv = b < nb ? (int)(n - tile0 < PL_TILE ? n - tile0 : PL_TILE) : 0;
    int k[PL_HITEMS];
#pragma unroll
    for (int i = 0; i < PL_HITEMS; ++i) {
        const int off = (part * PL_HITEMS + i) * PSFM_WAVE + lane;
        k[i] = off < nv ? vals[tile0 + off] : 0;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < PL_HITEMS; ++i) {
        // one LDS add per key on PL_HREP copies of the row, one add for a round whose digits all agree (psfm_sort_hist_kernel's way;
        // matching the lanes by digit first, the scatter kernel's way, measured the same here: 22.3 against 22.7 us)
        const int off = (part * PL_HITEMS + i) * PSFM_WAVE + lane;
        const bool ok = off < nv;
        const unsigned d = psfm_place_digit(k[i]);
        const unsigned long long valid = __ballot(ok);
        const unsigned d0 = (unsigned)__builtin_amdgcn_readfirstlane((int)d);
        if (__ballot(ok && d == d0) == valid) {
            if (lane == 0 && valid) atomicAdd(&s_h[t][0][d0], (unsigned)__popcll(valid));
        } else if (ok) {
            atomicAdd(&s_h[t][lane & (PL_HREP - 1)][d], 1u);
        }
    }
    __syncthreads();
    if (tid < PL_DIGITS) {
        unsigned run = 0;
#pragma unroll
        for (int q = 0; q < PL_GROUP; ++q) {
            unsigned c = 0;
#pragma unroll
            for (int rep = 0; rep < PL_HREP; ++rep) c += s_h[q][rep][tid];
            if (blockIdx.x * PL_GROUP + q < nb) cnt[(int64_t)(blockIdx.x * PL_GROUP + q) * PL_DIGITS + tid] = run;
            run += c;
        }
        grp[blockIdx.x * PL_DIGITS + tid] = run;
    }
}

// S.  Block = tile.  The values arrive as last : lane and leave as the bare lane.
__global__ __launch_bounds__(PL_BLOCK) void psfm_place_scatter_kernel(const unsigned* __restrict__ kin, const int* __restrict__ vin,
                                                                      unsigned* __restrict__ kout, int* __restrict__ vout, int64_t n,
                                                                      const unsigned* __restrict__ cnt, const unsigned* __restrict__ grp,
                                                                      int ngrp)
{
    __shared__ unsigned s_k[PL_TILE];
    __shared__ int s_v[PL_TILE];
    __shared__ unsigned s_wc[PL_NW][PL_DIGITS];
    __shared__ int s_delta[PL_DIGITS];
    __shared__ unsigned s_wsum[2][PL_NW];
    const int tid = threadIdx.x, lane = tid & (PSFM_WAVE - 1), wave = tid / PSFM_WAVE;
    const int b = blockIdx.x;
    const int64_t tile0 = (int64_t)b * PL_TILE;
    const int nv = (int)(n - tile0 < PL_TILE ? n - tile0 : PL_TILE);
#pragma unroll
    for (int w = 0; w < PL_NW; ++w) s_wc[w][tid] = 0u;
    unsigned k[PL_ITEMS];
    int v[PL_ITEMS];
#pragma unroll
    for (int i = 0; i < PL_ITEMS; ++i) {
        const int off = wave * PL_WSPAN + i * PSFM_WAVE + lane;
        const bool ok = off < nv;
        k[i] = ok ? kin[tile0 + off] : 0u;
        v[i] = ok ? vin[tile0 + off] : psfm_place_pack(0, PL_PAD);      // padding: the largest digit, behind every key of the tile
    }
    unsigned before = cnt[(int64_t)b * PL_DIGITS + tid], all = 0;
    {
        const int g = b / PL_GROUP;
        for (int q0 = 0; q0 < ngrp; q0 += PL_GCHUNK) {
            unsigned row[PL_GCHUNK];
#pragma unroll
            for (int u = 0; u < PL_GCHUNK; ++u) row[u] = q0 + u < ngrp ? grp[(q0 + u) * PL_DIGITS + tid] : 0u;
#pragma unroll
            for (int u = 0; u < PL_GCHUNK; ++u) { all += row[u]; if (q0 + u < g) before += row[u]; }
        }
    }
    __syncthreads();
    unsigned r[PL_ITEMS];      // rank among the elements of the digit in the wave, in (round, lane) order
    {
        const unsigned long long lower = (1ull << lane) - 1ull;
#pragma unroll
        for (int i = 0; i < PL_ITEMS; ++i) {
            const unsigned d = psfm_place_digit(v[i]);
            const unsigned long long peers = pl_match8(d);
            const unsigned old = s_wc[wave][d];
            const unsigned long long below = peers & lower;
            r[i] = old + (unsigned)__popcll(below);
            if (below == 0ull) s_wc[wave][d] = old + (unsigned)__popcll(peers);
            __builtin_amdgcn_wave_barrier();
        }
    }
    __syncthreads();
    {
        unsigned c[PL_NW], mine = 0;
#pragma unroll
        for (int w = 0; w < PL_NW; ++w) { c[w] = s_wc[w][tid]; mine += c[w]; }
        unsigned inc_t = mine, inc_a = all;
#pragma unroll
        for (int o = 1; o < PSFM_WAVE; o <<= 1) {
            const unsigned a = __shfl_up(inc_t, o), g2 = __shfl_up(inc_a, o);
            if (lane >= o) { inc_t += a; inc_a += g2; }
        }
        if (lane == PSFM_WAVE - 1) { s_wsum[0][wave] = inc_t; s_wsum[1][wave] = inc_a; }
        __syncthreads();
        unsigned base_t = 0, base_a = 0;
#pragma unroll
        for (int w = 0; w < PL_NW; ++w) if (w < wave) { base_t += s_wsum[0][w]; base_a += s_wsum[1][w]; }
        const unsigned dstart = base_t + inc_t - mine;
        const unsigned gstart = base_a + inc_a - all;
        unsigned run = dstart;
#pragma unroll
        for (int w = 0; w < PL_NW; ++w) { s_wc[w][tid] = run; run += c[w]; }
        s_delta[tid] = (int)(gstart + before) - (int)dstart;
    }
    __syncthreads();
    // the tile in digit order in LDS; it leaves as runs of equal digits
#pragma unroll
    for (int i = 0; i < PL_ITEMS; ++i) {
        const unsigned q = s_wc[wave][psfm_place_digit(v[i])] + r[i];
        s_k[q] = k[i];
        s_v[q] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < PL_ITEMS; ++j) {
        const int q = j * PL_BLOCK + tid;
        if (q < nv) {
            const int val = s_v[q];
            const int64_t pos = (int64_t)s_delta[psfm_place_digit(val)] + q;
            kout[pos] = s_k[q];
            vout[pos] = psfm_place_lane(val);
        }
    }
}

// where the scan's tables sit in c->place_tab behind the loop's masks
static int* psfm_place_starts(psfm_ctx* c, const PsfmTrackDims& d) { return (int*)(c->place_tab.as<unsigned long long>() + psfm_place_table_words(d.n_flows, d.G)); }

// scan + placement: the loop's n records -> the second halves of sort_keys / sort_lanes (one pass: odd, it ends in the first halves)
psfm_status psfm_place_records(psfm_ctx* c, const PsfmTrackDims& d, const PsfmFinForm& f, int64_t n, hipStream_t s)
{
    const unsigned long long* bmask = c->place_tab.as<unsigned long long>();
    int* start = psfm_place_starts(c, d);
    int* total = start + (int64_t)(d.n_flows + 1) * psfm_place_blocks(d.G);
    hipLaunchKernelGGL(psfm_place_scan_kernel, dim3((unsigned)d.n_flows), dim3(PL_BLOCK), 0, s, bmask, (int)d.G, d.n_flows, start, total);
    hipLaunchKernelGGL(psfm_place_records_kernel, dim3((unsigned)(d.nblk + 1)), dim3(PL_BLOCK), 0, s,
                       (const unsigned long long*)c->fin_keys.as<unsigned long long>(), (const int*)c->fin_lanes.as<int>(),
                       (const int2*)c->seg_info.as<int2>(), d.nblk, d.seg_cap, (const PsfmCounters*)c->counters.as<PsfmCounters>(), d.spill_cap,
                       bmask, (const int*)start, (const int*)total, (int)d.G, d.n_flows, f.fmt,
                       c->sort_keys.as<unsigned>() + n, c->sort_lanes.as<int>() + n, n);
    PSFM_HIP(hipGetLastError());
    return PSFM_OK;
}

// masks | starts | totals
size_t psfm_place_table_bytes(const PsfmTrackDims& d)
{
    return sizeof(unsigned long long) * (size_t)psfm_place_table_words(d.n_flows, d.G) +
           sizeof(int) * ((size_t)(d.n_flows + 1) * psfm_place_blocks(d.G) + PSFM_PLACE_MAX_TIMES);
}

// the one pass on `last` (the top byte of the values): (k_half1, v_half1) -> (k_half0, v_half0 as bare lanes).  n < 2^31.  Uses c->sort_tmp.
psfm_status psfm_place_sort(psfm_ctx* c, unsigned* k_half0, int* v_half0, const unsigned* k_half1, const int* v_half1, int64_t n, hipStream_t s)
{
    if (n <= 0) return PSFM_OK;
    const int64_t nb = (n + PL_TILE - 1) / PL_TILE;
    const int64_t ngrp = (nb + PL_GROUP - 1) / PL_GROUP;
    const size_t cnt_bytes = sizeof(unsigned) * PL_DIGITS * (size_t)nb;
    const size_t grp_bytes = sizeof(unsigned) * PL_DIGITS * (size_t)ngrp;
    psfm_status st = c->sort_tmp.ensure(cnt_bytes + grp_bytes);
    if (st != PSFM_OK) return st;
    unsigned* cnt = c->sort_tmp.as<unsigned>();
    unsigned* grp = (unsigned*)((char*)c->sort_tmp.p + cnt_bytes);
    hipLaunchKernelGGL(psfm_place_hist_kernel, dim3((unsigned)ngrp), dim3(PL_HBLOCK), 0, s, v_half1, n, cnt, grp, (int)nb);
    hipLaunchKernelGGL(psfm_place_scatter_kernel, dim3((unsigned)nb), dim3(PL_BLOCK), 0, s, k_half1, v_half1, k_half0, v_half0, n,
                       (const unsigned*)cnt, (const unsigned*)grp, (int)ngrp);
    PSFM_HIP(hipGetLastError());
    return PSFM_OK;
}
