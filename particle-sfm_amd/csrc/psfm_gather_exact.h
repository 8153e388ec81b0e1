// psfm_gather_exact.h -- when the finalize gather may sum a trajectory's logged flows in ANY order (psfm_gather_delta2_kernel).
//
// The persistent loop logs the sampled f32 flow of every survived step; a trajectory is its birth grid point plus the running f64 sum
// p(t+1) = p(t) + (double)flow(t), and the gather has to reproduce the loop's additions bit for bit.  Re-running them in the loop's
// order is one dependent chain per trajectory.  This header states when no order is needed because no addition rounds.
//
// Claim.  Let Q = 2^-40.  Call an f32 f FINE when f == 0 or 2^-17 <= |f| < 2^8.  Let p0 be an integer with |p0| < 2^13 and f1 .. fm
// fine, m <= 32.  If every prefix p0 + f1 + .. + fk (as real numbers) has magnitude below 2^13, then every f64 addition that forms
// such a prefix -- in the loop's order, or from partial sums of consecutive fi in any association -- is exact, so all orders give
// the same bits.
// Proof.
//   1. A fine f != 0 is n * 2^(e-23) with an integer n and e >= -17, a multiple of 2^-40 = Q; so is 0, and so is the integer p0.
//   2. (double)f is exact, and sums and differences of multiples of Q are multiples of Q.
//   3. A multiple of Q of magnitude below 2^13 is k * Q with |k| < 2^53: an f64 holds it exactly.
//   4. A partial sum of at most 32 consecutive fi has magnitude below 32 * 2^8 = 2^13: by 2 and 3 it is exact however it is associated.
//   5. A prefix is p(k-1) + fk, or p0 + (partial sum), or (prefix) + (partial sum): both operands are exact multiples of Q by
//      induction, the real sum is the prefix, its magnitude is below 2^13 by assumption, so by 3 the addition does not round.
//   6. The range test may be made on the COMPUTED prefix: both operands are below 2^13, so the real sum is below 2^14; rounding is
//      monotone and 2^13 is an f64, so a real sum >= 2^13 rounds to a value >= 2^13 and is seen.
//   7. Signed zeros: p0 is +0 or nonzero, and a sum whose real value is 0 is +0 unless both operands are -0; no prefix is ever -0 in
//      either order, and adding a +0 or -0 partial sum to a prefix leaves it as it is.
//   8. The next chunk starts from the last prefix: a multiple of Q below 2^13.  Integrality of p0 is used only through 1, so the
//      claim carries over chunk by chunk -- until one addition was inexact.  From then on the position is no multiple of Q and
//      nothing above holds: the trajectory stays serial for good (the sticky flag).
//
// Frames.  Positions inside a frame of max(H, W) <= 2^12 - 2^8 stay below 2^12 after a fine step, far inside the range; larger
// frames are not examined and keep the serial gather (psfm_gx_form).
//
// This header calls nothing of the HIP runtime: the CPU suite compiles it with g++ (tests/host/gather_exact_host.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#ifndef PSFM_HD
#define PSFM_HD __host__ __device__ __forceinline__
#endif

#define PSFM_GX_CHUNK 32                        // steps of a chunk = lanes that sum one trajectory (TILE_K)
#define PSFM_GX_EXP_LO (127 - 17)               // biased exponents of the fine class: 2^-17 <= |f| < 2^8
#define PSFM_GX_EXP_HI (127 + 8)
#define PSFM_GX_POS_LIMIT 8192.0                // 2^13: every produced coordinate stays below it in magnitude
#define PSFM_GX_MAX_FRAME ((1 << 12) - (1 << 8))

// 1 when f is fine: +-0, or a normal number with 2^-17 <= |f| < 2^8.  NaN, Inf and subnormals are not.
PSFM_HD int psfm_gx_class(float f)
{
    unsigned u;
    memcpy(&u, &f, sizeof(u));
    const unsigned e = (u >> 23) & 0xffu;
    return ((u << 1) == 0u || (e >= (unsigned)PSFM_GX_EXP_LO && e < (unsigned)PSFM_GX_EXP_HI)) ? 1 : 0;
}
PSFM_HD int psfm_gx_class2(float2 f) { return psfm_gx_class(f.x) & psfm_gx_class(f.y); }

// 1 when a produced position is inside the range of the claim (a NaN is not)
PSFM_HD int psfm_gx_in_range(double x, double y)
{
    return (x > -PSFM_GX_POS_LIMIT && x < PSFM_GX_POS_LIMIT && y > -PSFM_GX_POS_LIMIT && y < PSFM_GX_POS_LIMIT) ? 1 : 0;
}

// The chunk rule.  sticky: the trajectory's flag from its earlier chunks; all_fine: psfm_gx_class2 of every flow of the chunk (the
// entries outside [1, len) count as the zeros they are read as); all_in_range: psfm_gx_in_range of every position the blocked sum
// produced.  1: the blocked sum stands.  0: the chunk is redone in the loop's order and the trajectory is flagged from here on.
PSFM_HD int psfm_gx_chunk_parallel(int sticky, int all_fine, int all_in_range) { return (!sticky && all_fine && all_in_range) ? 1 : 0; }

// Which gather a finalize runs.  gather_switch: PSFM_FIN_GATHER (1; 0: the serial kernel, psfm_gather_delta_kernel).
// 1: psfm_gather_delta2_kernel, blocked sums under the chunk rule; 0: the serial kernel.
static inline int psfm_gx_form(int gather_switch, int H, int W)
{
    return (gather_switch && H <= PSFM_GX_MAX_FRAME && W <= PSFM_GX_MAX_FRAME) ? 1 : 0;
}
