// psfm_depth_display.h -- the per-element rules of the display image of a sparse depth map: sfm/convert.py:26-41
// (normalize_depth_for_display + gray2rgb) and what plt.imsave does to their result (:95), shared by the kernels
// (psfm_depth_display.hip) and the host build of the CPU suite (tests/host/depth_display_host.cpp through tests/host/shim).
//
// INV rule (:33-34).  valid = d > 0 (false for NaN); inv = 1.0 / (d + 1.0) for EVERY pixel: one f64 add, one IEEE division.  d = -1
// gives +inf and stays +inf.  A valid inv is a double in [0, 1): its bit pattern as u64 orders like its value, so the order statistics
// are found on integers.
//
// PERCENTILE rule (:35-36, np.percentile, method 'linear').  s = the valid inv ascending, n of them; for q:
//   vi = (n - 1) * (q / 100.0) (the quotient first); j = floor(vi); g = vi - j; a = s[j]; b = s[min(j + 1, n - 1)]; diff = b - a;
//   r = a + diff * g, and where g >= 0.5: r = b - diff * (1 - g).  Every operation rounded once, no FMA.
// z1 is the value for q = pc, z2 the value for q = 100 - pc (pc = 2 gives z1 < z2; the stretch below is then mirrored).
//
// SELECTION.  The four ranks of an image (j and min(j + 1, n - 1) of both q) are found by an MSB-first radix select over the bit
// patterns, 8 rounds of 8 bits: in round k a rank knows the top 8 k bits of its value (its prefix) and its position among the values
// that share them (rem); the 256-bin histogram of the next digit of those values tells the digit (the first bin whose running sum
// exceeds rem) and the new rem.  Ranks with the same prefix read the same histogram (slot = the first such rank).
//
// STRETCH rule (:38-39).  v = (inv - z2) / (z1 - z2) in f64, clamped to [0, 1] by two comparisons: NaN stays NaN (z1 == z2 and
// inv == z2: 0/0), +-inf clamp.
//
// COLOUR rule (:28, matplotlib's Colormap.__call__ on float32, then imsave's byte conversion).  v32 = (float)v, round to nearest
// even; xa = v32 * 256.0f; index = 255 where xa == 256, else xa truncated; the pixel's four bytes are table[index], NaN takes the
// table's "bad" entry.  The table is data (the colour map at 0..255 times 255, truncated, alpha 255), never a formula.
//
// On the device every f64 / f32 operation is written with its _rn intrinsic, so the rules do not depend on the contraction flag; the
// host build uses the plain operators with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIP_DEVICE_COMPILE__)
#define PSFM_DD_ADD(a, b) __dadd_rn((a), (b))
#define PSFM_DD_SUB(a, b) __dsub_rn((a), (b))
#define PSFM_DD_MUL(a, b) __dmul_rn((a), (b))
#define PSFM_DD_DIV(a, b) __ddiv_rn((a), (b))
#define PSFM_DD_FMUL(a, b) __fmul_rn((a), (b))
#else
#define PSFM_DD_ADD(a, b) ((a) + (b))
#define PSFM_DD_SUB(a, b) ((a) - (b))
#define PSFM_DD_MUL(a, b) ((a) * (b))
#define PSFM_DD_DIV(a, b) ((a) / (b))
#define PSFM_DD_FMUL(a, b) ((a) * (b))
#endif

#define PSFM_DD_RANKS 4        // j, j + 1 of pc; j, j + 1 of 100 - pc
#define PSFM_DD_ROUNDS 8       // 64 bits, 8 per round, most significant first
#define PSFM_DD_BINS 256

// What the selection keeps per image (device memory; written by the host before the first round, then by the pick step).
struct PsfmDdState {
    int64_t comp_off;                    // first of the image's n compacted bit patterns in the workspace
    uint32_t n;                          // valid pixels
    uint32_t cursor;                     // compaction: patterns handed out so far (integer atomicAdd, one per block)
    uint32_t rem[PSFM_DD_RANKS];         // position of the rank among the values that share its prefix
    uint32_t slot[PSFM_DD_RANKS];        // the histogram the rank reads: the first rank with the same prefix
    uint64_t prefix[PSFM_DD_RANKS];      // the top 8 * round bits of the rank's value; after the last round the value itself
    double g[2];                         // interpolation weights of pc and 100 - pc
    double z[2];                         // z1, z2 (written behind the last round)
};

__host__ __device__ __forceinline__ bool psfm_dd_valid(double d) { return d > 0.0; }

__host__ __device__ __forceinline__ double psfm_dd_inv(double d) { return PSFM_DD_DIV(1.0, PSFM_DD_ADD(d, 1.0)); }

__host__ __device__ __forceinline__ uint64_t psfm_dd_bits(double v)
{
    uint64_t u;
    memcpy(&u, &v, 8);
    return u;
}

__host__ __device__ __forceinline__ double psfm_dd_from_bits(uint64_t u)
{
    double v;
    memcpy(&v, &u, 8);
    return v;
}

// n >= 1, q in [0, 100]: j = floor((n - 1) * (q / 100)) in [0, n - 1], *j1 = min(j + 1, n - 1), *g in [0, 1)
__host__ __device__ __forceinline__ void psfm_dd_rank(uint32_t n, double q, uint32_t* j, uint32_t* j1, double* g)
{
    const double vi = PSFM_DD_MUL((double)(n - 1), PSFM_DD_DIV(q, 100.0));
    double f = floor(vi);
    if (f > (double)(n - 1)) f = (double)(n - 1);          // (q <= 100 keeps vi <= n - 1; a guard for the index, not a rule)
    if (f < 0.0) f = 0.0;
    *j = (uint32_t)f;
    *j1 = *j + 1 < n ? *j + 1 : n - 1;
    *g = PSFM_DD_SUB(vi, f);
}

__host__ __device__ __forceinline__ double psfm_dd_lerp(double a, double b, double g)
{
    const double diff = PSFM_DD_SUB(b, a);
    if (g >= 0.5) return PSFM_DD_SUB(b, PSFM_DD_MUL(diff, PSFM_DD_SUB(1.0, g)));
    return PSFM_DD_ADD(a, PSFM_DD_MUL(diff, g));
}

// ---- selection: digits, prefixes, the pick ------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ unsigned psfm_dd_digit(uint64_t u, int round) { return (unsigned)(u >> (56 - 8 * round)) & 255u; }

// the bits above the digit of `round` (round 0: none)
__host__ __device__ __forceinline__ uint64_t psfm_dd_prefix(uint64_t u, int round) { return round == 0 ? 0ull : u >> (64 - 8 * round); }

// hist: the 256 counts of the next digit among the values that share the rank's prefix; rem < their sum.  Returns the digit of the
// value at position rem and moves rem into that bin.  (rem >= the sum cannot happen for counts of the same data; 255 then.)
__host__ __device__ __forceinline__ unsigned psfm_dd_pick(const uint32_t* hist, uint32_t* rem)
{
    uint32_t below = 0;
    for (unsigned d = 0; d < PSFM_DD_BINS - 1; ++d) {
        const uint32_t c = hist[d];
        if (*rem - below < c) { *rem -= below; return d; }
        below += c;
    }
    *rem -= below;
    return PSFM_DD_BINS - 1;
}

// the slots of the next round: the first rank with an equal prefix
__host__ __device__ __forceinline__ void psfm_dd_slots(const uint64_t* prefix, uint32_t* slot)
{
    for (int r = 0; r < PSFM_DD_RANKS; ++r) {
        int s = r;
        for (int k = r - 1; k >= 0; --k)
            if (prefix[k] == prefix[r]) s = k;
        slot[r] = (uint32_t)s;
    }
}

// the state before round 0 (comp_off is the caller's)
__host__ __device__ __forceinline__ void psfm_dd_state_init(PsfmDdState* s, uint32_t n, double pc)
{
    s->n = n;
    s->cursor = 0;
    for (int r = 0; r < PSFM_DD_RANKS; ++r) { s->rem[r] = 0; s->slot[r] = 0; s->prefix[r] = 0; }
    s->g[0] = s->g[1] = 0.0;
    s->z[0] = s->z[1] = 0.0;
    if (n == 0) return;
    psfm_dd_rank(n, pc, &s->rem[0], &s->rem[1], &s->g[0]);
    psfm_dd_rank(n, PSFM_DD_SUB(100.0, pc), &s->rem[2], &s->rem[3], &s->g[1]);
}

// one value of the image in round `round`: bit r set = it belongs into the histogram of rank r (the rank owns its slot and the value
// shares its prefix)
__host__ __device__ __forceinline__ unsigned psfm_dd_owners(const PsfmDdState& s, uint64_t u, int round)
{
    const uint64_t p = psfm_dd_prefix(u, round);
    unsigned m = 0;
    for (int r = 0; r < PSFM_DD_RANKS; ++r)
        if (s.slot[r] == (uint32_t)r && s.prefix[r] == p) m |= 1u << r;
    return m;
}

// behind the histograms of round `round` (hist: PSFM_DD_RANKS x 256 of the image): every rank moves one digit on
__host__ __device__ __forceinline__ void psfm_dd_advance(PsfmDdState* s, const uint32_t* hist, int round)
{
    for (int r = 0; r < PSFM_DD_RANKS; ++r) {
        const unsigned d = psfm_dd_pick(hist + (size_t)s->slot[r] * PSFM_DD_BINS, &s->rem[r]);
        s->prefix[r] = (s->prefix[r] << 8) | d;
    }
    psfm_dd_slots(s->prefix, s->slot);
    if (round == PSFM_DD_ROUNDS - 1) {
        s->z[0] = psfm_dd_lerp(psfm_dd_from_bits(s->prefix[0]), psfm_dd_from_bits(s->prefix[1]), s->g[0]);
        s->z[1] = psfm_dd_lerp(psfm_dd_from_bits(s->prefix[2]), psfm_dd_from_bits(s->prefix[3]), s->g[1]);
    }
}

// ---- stretch and colour -----------------------------------------------------------------------------------------------------------------
// index into the table, 256 = the bad entry
__host__ __device__ __forceinline__ unsigned psfm_dd_index(double d, double z1, double z2)
{
    double v = PSFM_DD_DIV(PSFM_DD_SUB(psfm_dd_inv(d), z2), PSFM_DD_SUB(z1, z2));
    v = v < 0.0 ? 0.0 : v;                                  // (both comparisons are false for NaN)
    v = v > 1.0 ? 1.0 : v;
    const float v32 = (float)v;
    if (v32 != v32) return 256u;
    const float xa = PSFM_DD_FMUL(v32, 256.0f);
    return xa == 256.0f ? 255u : (unsigned)(int)xa;
}
