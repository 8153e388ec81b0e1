// psfm_sort64.hip -- the record sort of psfm_sort.hip for keys of up to 64 bits: stable LSD radix sort of (64-bit key, lane) pairs,
// 8 bits per pass, only the passes the key's used bits need.
//
// Who needs it: psfm_key_fmt() (psfm_finalize.hip) packs (death step, birth frame, birth grid index) into 32 bits when the triangular
// number of (death, birth) fits beside the grid index; long or dense sequences (1080p x 401 frames at r = 2: 37 key bits; 480 x 640 x
// 1000 frames dense: 39) and batches whose sequence number does not fit beside a 32-bit key keep the three fields in a 64-bit word.
// Those went through rocPRIM's device sort, whose nine fill launches per sort are what psfm_sort.hip was written to remove; COLMAP
// point ids of 2^32 and above (psfm_sfm.convert) had no device sort at all.
//
// The kernels are SIBLINGS of the two in psfm_sort.hip, in a translation unit of their own so that the 32-bit kernels -- the headline's --
// are compiled from the text they always were (as templates of one body the 32-bit instances came out with other register
// assignments and schedules: profiles/EXPERIMENTS.md 20).  The finalize runs them up to PSFM_SORT64_MAX_N records (psfm_finalize.hip):
// above, a pass is bound by bandwidth instead of its launches, and rocPRIM's sort was measured faster.  The structure is theirs, and the reasons for it are told there:
//   H  one block per GROUP of 8 tiles of 4 096 keys: digit counts of the tiles as exclusive prefixes over the group + the group's row
//   S  one block per tile: wave-striped reads ((wave, round, lane) order is memory order: every pass is stable), ranks by eight-ballot
//      digit matching with one LDS counter row per wave, the tile put in order in LDS and written out as runs of equal digits
//   two launches per pass, no global atomics, no fills, nothing to zero between passes; a pass moves 2 x n x 12 B.
// What differs:
//   - H reads ONE digit per key per pass, and a digit never straddles a 32-bit word (8 | 32): it loads only the word that holds the
//     digit (stride-8 loads: the same lines, but half the registers -- 32 keys per thread are in flight -- and the 32-bit counting code);
//   - S keeps the 4 096-key tile: keys + lanes are 48 KB of LDS, 53 KB with the counter rows (under the 64 KB static limit), 131 VGPRs;
//   - the tile padding key is all ones in 64 bits, so that padding lands behind every real key of its tile in every pass.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "psfm_device.h"
#include "psfm_internal.h"

#define PS64_BLOCK 256
#define PS64_ITEMS 16
#define PS64_TILE (PS64_BLOCK * PS64_ITEMS)
#define PS64_NW (PS64_BLOCK / PSFM_WAVE)
#define PS64_WSPAN (PS64_ITEMS * PSFM_WAVE)      // elements of a tile one wave reads
#define PS64_GROUP 8                             // tiles per group row
#define PS64_DIGITS 256
#define PS64_GCHUNK 64                           // group rows the scatter kernel has in flight at once
#define PS64_HWAVES 2
#define PS64_HREP 4                              // copies of a tile's counter row (a power of two)
#define PS64_HBLOCK (PS64_GROUP * PS64_HWAVES * PSFM_WAVE)
#define PS64_HITEMS (PS64_TILE / (PS64_HWAVES * PSFM_WAVE))

typedef unsigned long long ps_key64;

// lanes of the wave whose digit equals mine (every lane of the wave takes part)
__device__ __forceinline__ unsigned long long ps64_match8(unsigned d)
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

// H.  `words`: the keys as 32-bit words (two per key); `word`: the word of a key that holds this pass's digit, `shift` inside it.
__global__ __launch_bounds__(PS64_HBLOCK) void psfm_sort_hist64_kernel(const unsigned* __restrict__ words, int64_t n, int word, int shift,
                                                                       unsigned dmask, unsigned* __restrict__ cnt,
                                                                       unsigned* __restrict__ grp, int nb)
{
    __shared__ unsigned s_h[PS64_GROUP][PS64_HREP][PS64_DIGITS];
    const int tid = threadIdx.x, lane = tid & (PSFM_WAVE - 1), wave = tid / PSFM_WAVE;
    for (int q = tid; q < PS64_GROUP * PS64_HREP * PS64_DIGITS; q += PS64_HBLOCK) (&s_h[0][0][0])[q] = 0u;
    const int t = wave / PS64_HWAVES, part = wave % PS64_HWAVES;      // this wave's tile of the group, and which part of it
    const int b = blockIdx.x * PS64_GROUP + t;
    const int64_t tile0 = (int64_t)b * PS64_TILE;
    const int nv = b < nb ? (int)(n - tile0 < PS64_TILE ? n - tile0 : PS64_TILE) : 0;
    unsigned k[PS64_HITEMS];
#pragma unroll
    for (int i = 0; i < PS64_HITEMS; ++i) {                  // all loads in flight before the first add
        const int off = (part * PS64_HITEMS + i) * PSFM_WAVE + lane;
        k[i] = off < nv ? words[2 * (tile0 + off) + word] : 0u;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < PS64_HITEMS; ++i) {
        const int off = (part * PS64_HITEMS + i) * PSFM_WAVE + lane;
        // (as psfm_sort_hist_kernel: one LDS add per key, PS64_HREP copies of the row picked by lane, one add for a round whose keys agree)
        const bool ok = off < nv;
        const unsigned d = (k[i] >> shift) & dmask;
        const unsigned long long valid = __ballot(ok);
        const unsigned d0 = (unsigned)__builtin_amdgcn_readfirstlane((int)d);
        if (__ballot(ok && d == d0) == valid) {
            if (lane == 0 && valid) atomicAdd(&s_h[t][0][d0], (unsigned)__popcll(valid));
        } else if (ok) {
            atomicAdd(&s_h[t][lane & (PS64_HREP - 1)][d], 1u);
        }
    }
    __syncthreads();
    if (tid < PS64_DIGITS) {
        unsigned run = 0;
#pragma unroll
        for (int q = 0; q < PS64_GROUP; ++q) {
            unsigned c = 0;
#pragma unroll
            for (int rep = 0; rep < PS64_HREP; ++rep) c += s_h[q][rep][tid];
            if (blockIdx.x * PS64_GROUP + q < nb) cnt[(int64_t)(blockIdx.x * PS64_GROUP + q) * PS64_DIGITS + tid] = run;
            run += c;
        }
        grp[blockIdx.x * PS64_DIGITS + tid] = run;
    }
}

// S.  Block = tile.
__global__ __launch_bounds__(PS64_BLOCK) void psfm_sort_scatter64_kernel(const ps_key64* __restrict__ kin, const int* __restrict__ vin,
                                                                         ps_key64* __restrict__ kout, int* __restrict__ vout, int64_t n,
                                                                         int shift, unsigned dmask, const unsigned* __restrict__ cnt,
                                                                         const unsigned* __restrict__ grp, int ngrp)
{
    __shared__ ps_key64 s_k[PS64_TILE];
    __shared__ int s_v[PS64_TILE];
    __shared__ unsigned s_wc[PS64_NW][PS64_DIGITS];      // per wave: digit counts, then where that share of a digit starts in the tile
    __shared__ int s_delta[PS64_DIGITS];                 // digit -> (position in the output) - (position in the tile)
    __shared__ unsigned s_wsum[2][PS64_NW];
    const int tid = threadIdx.x, lane = tid & (PSFM_WAVE - 1), wave = tid / PSFM_WAVE;
    const int b = blockIdx.x;
    const int64_t tile0 = (int64_t)b * PS64_TILE;
    const int nv = (int)(n - tile0 < PS64_TILE ? n - tile0 : PS64_TILE);
#pragma unroll
    for (int w = 0; w < PS64_NW; ++w) s_wc[w][tid] = 0u;
    ps_key64 k[PS64_ITEMS];
    int v[PS64_ITEMS];
#pragma unroll
    for (int i = 0; i < PS64_ITEMS; ++i) {
        const int off = wave * PS64_WSPAN + i * PSFM_WAVE + lane;
        const bool ok = off < nv;
        k[i] = ok ? kin[tile0 + off] : ~0ull;      // padding: the largest digit in every pass, behind every key of the tile
        v[i] = ok ? vin[tile0 + off] : 0;
    }
    // digit `tid` of the tiles in front of this one (whole groups; the tiles of its own group: H left that prefix in the tile's row),
    // and of all tiles -- behind the tile's own loads in program order, so that those are in flight while the rows arrive
    unsigned before = cnt[(int64_t)b * PS64_DIGITS + tid], all = 0;
    {
        const int g = b / PS64_GROUP;
        for (int q0 = 0; q0 < ngrp; q0 += PS64_GCHUNK) {
            unsigned row[PS64_GCHUNK];
#pragma unroll
            for (int u = 0; u < PS64_GCHUNK; ++u) row[u] = q0 + u < ngrp ? grp[(q0 + u) * PS64_DIGITS + tid] : 0u;
#pragma unroll
            for (int u = 0; u < PS64_GCHUNK; ++u) { all += row[u]; if (q0 + u < g) before += row[u]; }
        }
    }
    __syncthreads();
    // rank of every element among the elements of its digit in its wave, in (round, lane) order
    unsigned r[PS64_ITEMS];
    {
        const unsigned long long lower = (1ull << lane) - 1ull;
#pragma unroll
        for (int i = 0; i < PS64_ITEMS; ++i) {
            const unsigned d = (unsigned)(k[i] >> shift) & dmask;
            const unsigned long long peers = ps64_match8(d);
            // every lane reads its digit's counter, the first of the peers writes it back: plain LDS accesses in program order
            const unsigned old = s_wc[wave][d];
            const unsigned long long below = peers & lower;
            r[i] = old + (unsigned)__popcll(below);
            if (below == 0ull) s_wc[wave][d] = old + (unsigned)__popcll(peers);
            __builtin_amdgcn_wave_barrier();
        }
    }
    __syncthreads();
    // thread = digit: the tile's run of the digit starts behind the smaller digits; the shares of the waves follow each other inside it
    {
        unsigned c[PS64_NW], mine = 0;
#pragma unroll
        for (int w = 0; w < PS64_NW; ++w) { c[w] = s_wc[w][tid]; mine += c[w]; }
        unsigned inc_t = mine, inc_a = all;               // inclusive scans over the digits: tile counts, global counts
#pragma unroll
        for (int o = 1; o < PSFM_WAVE; o <<= 1) {
            const unsigned a = __shfl_up(inc_t, o), g2 = __shfl_up(inc_a, o);
            if (lane >= o) { inc_t += a; inc_a += g2; }
        }
        if (lane == PSFM_WAVE - 1) { s_wsum[0][wave] = inc_t; s_wsum[1][wave] = inc_a; }
        __syncthreads();
        unsigned base_t = 0, base_a = 0;
#pragma unroll
        for (int w = 0; w < PS64_NW; ++w) if (w < wave) { base_t += s_wsum[0][w]; base_a += s_wsum[1][w]; }
        const unsigned dstart = base_t + inc_t - mine;        // first position of the digit in the ordered tile
        const unsigned gstart = base_a + inc_a - all;         // first position of the digit in the output
        unsigned run = dstart;
#pragma unroll
        for (int w = 0; w < PS64_NW; ++w) { s_wc[w][tid] = run; run += c[w]; }
        s_delta[tid] = (int)(gstart + before) - (int)dstart;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < PS64_ITEMS; ++i) {
        const unsigned d = (unsigned)(k[i] >> shift) & dmask;
        const unsigned q = s_wc[wave][d] + r[i];
        s_k[q] = k[i];
        s_v[q] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < PS64_ITEMS; ++j) {
        const int q = j * PS64_BLOCK + tid;
        if (q < nv) {
            const ps_key64 key = s_k[q];
            const int64_t pos = (int64_t)s_delta[(unsigned)(key >> shift) & dmask] + q;
            kout[pos] = key;
            vout[pos] = s_v[q];
        }
    }
}

int psfm_sort_pairs64_passes(unsigned end_bit) { return (int)((end_bit + 7u) / 8u); }

// psfm_sort_pairs32's contract for 64-bit keys: sorts n (key, value) pairs by the key bits [0, end_bit), end_bit <= 64, stable.
// `half0` / `half1`: two buffers of n entries each; the input sits in half0 when the number of passes is even, in half1 when it is odd
// (psfm_sort_pairs64_passes), and the result always ends in half0.  n < 2^31.  Uses c->sort_tmp.
psfm_status psfm_sort_pairs64(psfm_ctx* c, unsigned long long* k_half0, int* v_half0, unsigned long long* k_half1, int* v_half1, int64_t n,
                              unsigned end_bit, hipStream_t s)
{
    const int passes = psfm_sort_pairs64_passes(end_bit);
    if (n <= 0 || passes == 0) return PSFM_OK;
    const int64_t nb = (n + PS64_TILE - 1) / PS64_TILE;
    const int64_t ngrp = (nb + PS64_GROUP - 1) / PS64_GROUP;
    const size_t cnt_bytes = sizeof(unsigned) * PS64_DIGITS * (size_t)nb;
    const size_t grp_bytes = sizeof(unsigned) * PS64_DIGITS * (size_t)ngrp;
    psfm_status st = c->sort_tmp.ensure(cnt_bytes + grp_bytes);
    if (st != PSFM_OK) return st;
    unsigned* cnt = c->sort_tmp.as<unsigned>();
    unsigned* grp = (unsigned*)((char*)c->sort_tmp.p + cnt_bytes);
    ps_key64* kin = (passes & 1) ? k_half1 : k_half0;
    int* vin = (passes & 1) ? v_half1 : v_half0;
    ps_key64* kout = (passes & 1) ? k_half0 : k_half1;
    int* vout = (passes & 1) ? v_half0 : v_half1;
    for (int p = 0; p < passes; ++p) {
        // the last pass of an end_bit that is no multiple of 8 takes only the digit's bits below end_bit: the bits above are not part of the key
        const unsigned rest = end_bit - 8u * (unsigned)p;
        const unsigned dmask = rest >= 8u ? 255u : (1u << rest) - 1u;
        hipLaunchKernelGGL(psfm_sort_hist64_kernel, dim3((unsigned)ngrp), dim3(PS64_HBLOCK), 0, s, (const unsigned*)kin, n, p / 4, 8 * (p % 4),
                           dmask, cnt, grp, (int)nb);
        hipLaunchKernelGGL(psfm_sort_scatter64_kernel, dim3((unsigned)nb), dim3(PS64_BLOCK), 0, s, (const ps_key64*)kin, (const int*)vin, kout,
                           vout, n, 8 * p, dmask, (const unsigned*)cnt, (const unsigned*)grp, (int)ngrp);
        ps_key64* tk = kin; kin = kout; kout = tk;
        int* tv = vin; vin = vout; vout = tv;
    }
    PSFM_HIP(hipGetLastError());
    return PSFM_OK;
}
