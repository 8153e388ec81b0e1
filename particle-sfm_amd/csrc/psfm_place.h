// psfm_place.h -- finalize of the persistent loop: the records placed by BIRTH ORDER, then sorted in one pass (psfm_place.hip).
//
// Trajectory ids are the rank by (last, birth, idx) (psfm_finalize.hip).  The frame loop knows two thirds of that order and the
// four-pass sort used to work it out again: thread L of the loop owns grid point L and virtual blocks (psfm_vblock) are in grid order,
// so the births of a frame, wave by wave in lane order, ARE in grid-index order.  Among the trajectories born in frame b, the one born
// at grid index idx therefore has the rank
//     (births of frame b at grid indices below idx)            (frame 0: every grid point is born, rank = idx)
// and a layout by (birth, that rank) IS sorted by (birth, idx): ONE stable radix pass on `last` (8 bits: n_flows + 1 <= 256) leaves
// (last, birth, idx), today's sorted array, bit for bit.  The loop leaves behind every wave's ballot of births -- a table of birth
// masks, one 64-bit word per 64 consecutive grid points and frame (psfm_persist.hip, "Birth order"); here
//     scan       per frame b: the births of its virtual blocks (256 grid points: four words) as exclusive starts INSIDE the frame, and
//                the frame's total
//     placement  every block sums the frames' totals in front of every frame for itself (<= 256 of them, the way the compaction summed
//                the segment counts), then  pos = base[b] + start[b][idx >> 8] + (births of the block below idx)  for each record: a
//                permutation, no atomics.  It stores the 32-bit key at pos, and beside it the lane with `last` in its top byte
//     one pass   hist + scatter on that byte (decoding `last` from the triangular key instead cost the two kernels 49 us more); the
//                scatter stores the bare lane
// instead of compaction + four passes: 4 launches for 9.
//
// This header holds the decision and the index arithmetic and calls nothing of the HIP runtime: the CPU suite compiles it with g++
// (tests/host/place_host.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "psfm_finalize_plan.h"

#define PSFM_PLACE_VB 256             // grid points of a virtual block of the loop (PP_BLOCK: psfm_persist.hip checks that it is)
#define PSFM_PLACE_VB_WORDS 4         // its waves = mask words
#define PSFM_PLACE_MAX_TIMES 256      // n_flows + 1 <= this: `last` is one 8-bit digit, the frames' totals one value per thread of a block
#define PSFM_PLACE_LANE_BITS 24       // the pass's values: last << 24 | lane

// Whether a finalize runs the placed form.  persist_ran: the records and the birth masks are the persistent loop's; f: the call's form
// plan (psfm_fin_form, unchanged by this); cap: log columns (lanes); place_switch: PSFM_FIN_PLACE (1; 0: compaction + the sort's own
// passes).  sort_form 1 is the library's sort on 32-bit keys: the key format is the 32-bit one and nobody asked for rocPRIM's sort
// (PSFM_FIN_SORT=0), of which the placed form has no use.
static inline int psfm_place_form(int persist_ran, const PsfmFinForm& f, int n_flows, int64_t n, int64_t cap, int place_switch)
{
    return (place_switch && persist_ran && f.fmt.use32 && f.sort_form == 1 && n_flows + 1 <= PSFM_PLACE_MAX_TIMES && n < (1ll << 31) &&
            cap <= (1ll << PSFM_PLACE_LANE_BITS)) ? 1 : 0;
}

// virtual blocks that own grid points, and the mask words of a frame (every wave of those blocks stores one); the mask table has the
// rows 0 .. n_flows.  Row 0 is implied (every grid point is born in frame 0) and row n_flows is empty (the loop's last frame is
// n_flows - 1): neither is ever stored or loaded.
PSFM_HD int psfm_place_blocks(int64_t G) { return (int)((G + PSFM_PLACE_VB - 1) / PSFM_PLACE_VB); }
PSFM_HD int psfm_place_words(int64_t G) { return PSFM_PLACE_VB_WORDS * psfm_place_blocks(G); }
PSFM_HD int64_t psfm_place_table_words(int n_flows, int64_t G) { return (int64_t)(n_flows + 1) * psfm_place_words(G); }
// births of frame b on the grid points of virtual block vb
PSFM_HD int psfm_place_count(const unsigned long long* bmask, int64_t G, int n_flows, int b, int vb)
{
    if (b == 0) { const int64_t r = G - (int64_t)PSFM_PLACE_VB * vb; return r >= PSFM_PLACE_VB ? PSFM_PLACE_VB : (r > 0 ? (int)r : 0); }
    if (b >= n_flows) return 0;
    const unsigned long long* w = bmask + (int64_t)b * psfm_place_words(G) + (int64_t)PSFM_PLACE_VB_WORDS * vb;
    int c = 0;
    for (int j = 0; j < PSFM_PLACE_VB_WORDS; ++j) c += __builtin_popcountll(w[j]);
    return c;
}
// births of frame b >= 1 in idx's virtual block at grid indices below idx; w: the block's four mask words of the frame
PSFM_HD int psfm_place_ordinal(const unsigned long long* w, int idx)
{
    const int q = (idx & (PSFM_PLACE_VB - 1)) >> 6, bit = idx & 63;
    int k = __builtin_popcountll(w[q] & ((1ull << bit) - 1ull));
    for (int j = 0; j < PSFM_PLACE_VB_WORDS; ++j) if (j < q) k += __builtin_popcountll(w[j]);
    return k;
}
// whether the masks say that idx was born in that frame (every record's is)
PSFM_HD int psfm_place_born(const unsigned long long* w, int idx) { return (int)((w[(idx & (PSFM_PLACE_VB - 1)) >> 6] >> (idx & 63)) & 1ull); }
// a record's position in the layout by (birth, rank): base = births of all frames before b, start = births of frame b in the virtual
// blocks below its own, k = psfm_place_ordinal
PSFM_HD int64_t psfm_place_pos(int64_t base, int start, int k) { return base + start + k; }
// the one pass's values
PSFM_HD int psfm_place_pack(int lane, int last) { return (int)(((unsigned)last << PSFM_PLACE_LANE_BITS) | (unsigned)lane); }
PSFM_HD unsigned psfm_place_digit(int packed) { return (unsigned)packed >> PSFM_PLACE_LANE_BITS; }
PSFM_HD int psfm_place_lane(int packed) { return (int)((unsigned)packed & ((1u << PSFM_PLACE_LANE_BITS) - 1u)); }

// The scan as the kernels split it, in plain loops: start[b * gb + vb] for b in [1, n_flows) (row 0 is not stored: the placement takes
// pos = idx there), total[b] for b in [0, n_flows).  What the device computes must equal this (tests/test_place_host.py runs it).
static inline void psfm_place_scan_rows(const unsigned long long* bmask, int64_t G, int n_flows, int* start, int* total)
{
    const int gb = psfm_place_blocks(G);
    for (int b = 0; b < n_flows; ++b) {
        int run = 0;
        for (int vb = 0; vb < gb; ++vb) {
            if (b > 0) start[(int64_t)b * gb + vb] = run;
            run += psfm_place_count(bmask, G, n_flows, b, vb);
        }
        total[b] = run;
    }
}
