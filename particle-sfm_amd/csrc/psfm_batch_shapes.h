// psfm_batch_shapes.h -- psfm_connect_batch over sequences of DIFFERENT frame sizes (psfm_batch.hip with h = w = 0): the rows of the
// tables its two bandwidth launches read, the rule that maps a block of their flattened grid to (sequence, chunk of the sequence's
// frame), and the batch's common key format.  Plain C++: also compiled for the host by the CPU suite
// (tests/host/batch_shapes_host.cpp through tests/host/shim).
//
// The frame launches of a batch have blockIdx.y = sequence and read every dimension from the sequence's row; a block beyond the
// sequence's lanes leaves at once.  The two launches on the side stream -- flow_check of a chunk of frame pairs and, with the
// motion-boundary option, the kill maps behind it -- are streams over the pixels of a frame, and a frame of 360 x 640 has half the
// pixels of one of 480 x 910: a grid (blocks of the largest frame, pairs, sequences) would dispatch as many idle blocks as busy ones.
// So blockIdx.x of those two is FLATTENED over the sequences:
//   * sequence i owns n[i] consecutive blocks, numbered inside the sequence: its `chunks` (one per 1024 pixels) when they are walked
//     in order, 8 * xcd_per when they are banded (64 chunks and more: local block b takes chunk (b % 8) * xcd_per + b / 8, so that
//     each XCD streams one contiguous band of rows -- psfm_xcd_chunk of psfm_track.hip, the kill map's band rule);
//   * n[i] is rounded up to a multiple of 8, so every sequence starts on a block whose index is a multiple of 8 and local block b sits
//     on XCD blockIdx.x % 8 = b % 8, which is what the banding assumes.  The spare blocks return;
//   * a sequence without maps to make (n_pairs = 0: it left the batch before the first window, or has no stride-2 stack) owns none;
//   * gridDim.x is the total; blockIdx.y stays the frame pair of the chunk range, and a sequence that has fewer pairs returns;
//   * a block finds its sequence by counting the entries of the inclusive prefix that are <= blockIdx.x (psfm_bs_find): at most 64
//     scalar compares, as psfm_qb_find of psfm_query_batch.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "psfm_device.h"

#define PSFM_BS_MAX 64                  // sequences per call: PSFM_BATCH_MAX (static_assert in psfm_batch.hip)
#define PSFM_BS_FC_PIXELS 1024          // pixels per flow_check block: PSFM_BLOCK * PSFM_FC2_UNROLL * 2 (static_assert in psfm_track.hip)
#define PSFM_BS_KM_LANES 256            // lanes per kill-map block (PSFM_MB_BLOCK) ...
#define PSFM_BS_KM_PPL 4                // ... and pixels per lane (PSFM_MB_PPL; static_asserts in psfm_motion_boundary.hip)
#define PSFM_BS_BAND_MIN 64             // chunks from which a frame is banded over the XCDs

#ifndef PSFM_HD
#define PSFM_HD __host__ __device__ __forceinline__
#endif

// forms of the kill-map launch, block-uniform by row: four pixels per lane with the row below at an even / an odd distance (16-byte /
// 8-byte loads), or one pixel per thread (P odd, or a flow stack that is not 16-byte aligned)
#define PSFM_BS_KM_LANE_WEVEN 0
#define PSFM_BS_KM_LANE_WODD 1
#define PSFM_BS_KM_PX 2

// One stack of the batch for flow_check: PsfmFcSeq (psfm_internal.h), the stack's PsfmFcParams without the threshold (one per call: a
// kernel argument), and its part of the flattened grid.  Written once per run into the owner's batch_fc.
struct PsfmFcShapeRow {
    const float* ff; const float* fb; uint8_t* occ;
    int n_pairs;                        // pairs of the stack; 0: no maps to make
    int H, W;
    float cw, ch, rcw, rch;
    PsfmFastDiv wdiv;
    int chunks, xcd_per;                // 1024-pixel chunks of a frame; > 0: chunks per XCD band
    int blk0, blk_end;                  // the sequence's blocks [blk0, blk_end) of the flattened grid (blk_end: the INCLUSIVE prefix)
};

// ... and for the kill maps: PsfmKmSeq (psfm_internal.h), the frame, the form and the stack's part of the flattened grid
struct PsfmKmShapeRow {
    const float* flows; const uint8_t* occ; uint8_t* out;
    int n; float thres;                 // frames of the stack (0: no maps to make); the sequence's own threshold
    int H, W, P;
    int chunks, xcd_per;                // 256-lane (form PSFM_BS_KM_PX: 256-pixel) chunks of a frame; > 0: chunks per XCD band
    PsfmFastDiv wdiv;
    int form;
    int blk0, blk_end;
    int pad;
};

// ---- chunks of a frame ----
PSFM_HD int psfm_bs_fc_chunks(int64_t P) { return (int)((P + PSFM_BS_FC_PIXELS - 1) / PSFM_BS_FC_PIXELS); }
PSFM_HD int psfm_bs_km_chunks(int64_t P, int form)
{
    const int64_t items = form == PSFM_BS_KM_PX ? P : (P + PSFM_BS_KM_PPL - 1) / PSFM_BS_KM_PPL;
    return (int)((items + PSFM_BS_KM_LANES - 1) / PSFM_BS_KM_LANES);
}
PSFM_HD int psfm_bs_xcd_per(int chunks) { return chunks >= PSFM_BS_BAND_MIN ? (chunks + 7) / 8 : 0; }
PSFM_HD int psfm_bs_km_form(int64_t P, int W, bool flows_al16)
{
    if ((P & 1) != 0 || !flows_al16) return PSFM_BS_KM_PX;
    return (W & 1) == 0 ? PSFM_BS_KM_LANE_WEVEN : PSFM_BS_KM_LANE_WODD;
}

// ---- blocks of a sequence, and the chunk of one of them ----
PSFM_HD int psfm_bs_blocks(int chunks, int xcd_per, int n_frames)
{
    if (n_frames <= 0) return 0;
    return ((xcd_per > 0 ? 8 * xcd_per : chunks) + 7) & ~7;
}
// local block b of a sequence -> its chunk of the frame, or -1 (a spare block)
PSFM_HD int psfm_bs_chunk(int b, int chunks, int xcd_per)
{
    const int c = xcd_per > 0 ? (b & 7) * xcd_per + (b >> 3) : b;
    return c < chunks ? c : -1;
}

// the prefix over rows whose chunks / xcd_per / frame count are set, into the rows and into blk_end[PSFM_BS_MAX] -- the INCLUSIVE
// prefix as one array of 64 entries, INT32_MAX at and above n_seq: what a block searches; returns gridDim.x
template <class Row>
static inline int psfm_bs_prefix(Row* rows, int n_seq, const int* n_frames, int* blk_end)
{
    int blocks = 0;
    for (int i = 0; i < PSFM_BS_MAX; ++i) {
        if (i >= n_seq) { blk_end[i] = INT32_MAX; continue; }
        rows[i].blk0 = blocks;
        blocks += psfm_bs_blocks(rows[i].chunks, rows[i].xcd_per, n_frames[i]);
        rows[i].blk_end = blk_end[i] = blocks;
    }
    return blocks;
}
// (frames of at most 2^29 pixels -- psfm_frame_ok -- are at most 2^21 blocks each: 64 of them fit an int)
static inline int psfm_bs_fc_prefix(PsfmFcShapeRow* rows, int n_seq, int* blk_end)
{
    int nf[PSFM_BS_MAX];
    for (int i = 0; i < n_seq; ++i) nf[i] = rows[i].n_pairs;
    return psfm_bs_prefix(rows, n_seq, nf, blk_end);
}
static inline int psfm_bs_km_prefix(PsfmKmShapeRow* rows, int n_seq, int* blk_end)
{
    int nf[PSFM_BS_MAX];
    for (int i = 0; i < n_seq; ++i) nf[i] = rows[i].n;
    return psfm_bs_prefix(rows, n_seq, nf, blk_end);
}

// The sequence of block `blk` (0 <= blk < gridDim.x): the number of inclusive prefix entries that are <= blk.  A sequence without
// blocks repeats its predecessor's entry and is passed over with it; the entries at and above n_seq never count.  `blk` is
// block-uniform and the 64 entries are read at constant addresses: a few wide scalar loads behind one wait, and scalar compares.
PSFM_HD int psfm_bs_find(const int* __restrict__ blk_end, int blk)
{
    int n = 0;
#pragma unroll
    for (int i = 0; i < PSFM_BS_MAX; ++i) n += blk_end[i] <= blk ? 1 : 0;
    return n;
}

// ---- the batch's common key format ----
// A record is  last << shift_d | birth << shift_b | grid index  (psfm_key, psfm_chain.h) and the segmented finalize sorts the records
// of all sequences with ONE format.  shift_b follows from the bits of a sequence's grid and the time bits from its length; the batch
// takes the widest of each.  Wider fields leave the ORDER of a sequence's records what it was -- (last, birth, index) compared field
// by field either way -- so trajectory ids do not change; the 32-bit form (psfm_fin_form, psfm_finalize_plan.h) is chosen from the
// common shifts and the longest sequence, i.e. only when the widest grid fits it.
struct PsfmBsKeyFmt { int shift_b, tbits, shift_d; };
static inline PsfmBsKeyFmt psfm_bs_common_key(const int* shift_b, const int* n_flows, int n_seq)
{
    PsfmBsKeyFmt k;
    int n_max = 0;
    k.shift_b = 1;
    for (int i = 0; i < n_seq; ++i) {
        if (shift_b[i] > k.shift_b) k.shift_b = shift_b[i];
        if (n_flows[i] > n_max) n_max = n_flows[i];
    }
    k.tbits = 1;
    while ((1ll << k.tbits) < (long long)n_max + 2) ++k.tbits;
    k.shift_d = k.shift_b + k.tbits;
    return k;
}
