// psfm_query_pc_batch.h -- psfm_track_queries_optimize_batch (psfm_query_pc_batch.hip): the query points of up to 64 sequences
// tracked with the stride-2 path-consistency solve after every step, through ONE set of launches per step.  The table of sequences,
// the index rules of a step (which frame is stepped from, which maps it and its solve sample) and the per-lane text that differs
// from the single call's: a row of a solve written straight into the solver's buffers.  The step itself is psfm_query_pc.h's,
// unchanged.  The grids over queries are the flattened grids of psfm_query_batch.h: sequence b owns ceil(Q[b] / 256) blocks numbered
// inside the sequence, so its blocks, its waves and its rows-per-wave counts are what the single call has.
#pragma once
#include "psfm_query_pc.h"
#include "psfm_query_batch.h"

// one direction of one sequence
struct PsfmQpbDir {
    const float2* flows; const uint8_t* masks;      // the stride-1 stack and its occlusion (motion boundary: kill) maps; NULL: not tracked
    const float2* flows2; const uint8_t* occ2;      // the stride-2 stack and ITS occlusion maps (NULL with one flow: no solve happens)
    int* len;                                       // (Q) points of this direction so far: the sequence's part of the concatenation
};

// One sequence of a call, in device memory.  The solve's buffers are the sequence's own context's (pc_multi_problem).
struct PsfmQpbSeq {
    PsfmQpbDir dir[2];                              // forward, backward
    const double2* q_xy; const int* q_t;            // (Q)
    double2* slab;                                  // (n_flows+1, Q) time-major, in the sequence's own context (log)
    double2 *x1, *x2, *ref1, *ref2;                 // rows of the step's solve, compacted in query order: p1, p2 (buffer 0 of the chain), refs
    double* scale;
    int* owner;                                     // the query of every row
    int* wave_cnt;                                  // (4 per block of the sequence) rows per wave; after the scan: rows in the waves before
    int* n_rows;                                    // rows of the step's solve: left by the scan, read by the solver and the scatter
    int H, W, n_flows;
    unsigned Q, P;                                  // queries; pixels of a map
    float cw, ch, rcw, rch;
    int blk0, n_blk;                                // first block in every flattened grid, blocks of the sequence
};

// Step k (0 .. n_flows - 1) of a direction: forward from frame k through map k; backward from frame n_flows - k through map
// n_flows - k - 1 (frame f+1 -> f).  From the second step on the lanes that hold three positions are the rows of a solve whose p0 is
// one frame before `from`: the stride-1 map it was stepped through, the stride-2 map from its frame.  (psfm_query_pc.hip's loop.)
struct PsfmQpbStep { int from, to, dir, map, p0, map01, map02; bool solve; };
__host__ __device__ __forceinline__ bool psfm_qpb_steps(int k, int n_flows) { return k >= 0 && k < n_flows; }
__host__ __device__ __forceinline__ PsfmQpbStep psfm_qpb_step(int k, int n_flows, int back)
{
    PsfmQpbStep s;
    s.dir = back ? -1 : 1;
    s.from = back ? n_flows - k : k;
    s.to = s.from + s.dir;
    s.map = back ? s.from - 1 : s.from;
    s.solve = k >= 1;
    s.p0 = s.from - s.dir;
    s.map01 = back ? s.from : s.from - 1;
    s.map02 = s.from - 1;
    return s;
}

// the single call's frame arguments for step k of sequence S
__host__ __device__ __forceinline__ void psfm_qpb_frame(const PsfmQpbSeq& S, int k, int back, PsfmQueryPcFrame& a)
{
    const PsfmQpbDir& D = S.dir[back ? 1 : 0];
    const PsfmQpbStep s = psfm_qpb_step(k, S.n_flows, back);
    const size_t P = S.P, Q = S.Q;
    a.fr.H = S.H; a.fr.W = S.W; a.fr.cw = S.cw; a.fr.ch = S.ch; a.fr.rcw = S.rcw; a.fr.rch = S.rch;
    a.fr.flow = D.flows + (size_t)s.map * P; a.fr.occ = D.masks + (size_t)s.map * P;
    a.q_t = S.q_t; a.wave_cnt = S.wave_cnt; a.Q = S.Q; a.len = D.len;
    a.from = s.from; a.dir = s.dir;
    a.row_p1 = S.slab + (size_t)s.from * Q; a.row_p2 = S.slab + (size_t)s.to * Q;
    a.row_p0 = nullptr; a.flow01 = a.flow02 = nullptr; a.occ02 = nullptr;
    if (s.solve) {
        a.row_p0 = S.slab + (size_t)s.p0 * Q;
        a.flow01 = D.flows + (size_t)s.map01 * P; a.flow02 = D.flows2 + (size_t)s.map02 * P; a.occ02 = D.occ2 + (size_t)s.map02 * P;
    }
}

// row `rank` of the solve from lane q, as psfm_query_pc_row forms it, written where the solver reads it: p1 -> x1, p2 -> x2 (no
// interleaved uv12 that a load kernel splits, no copies of the refs)
__device__ __forceinline__ void psfm_qpb_row(const PsfmQueryPcFrame& a, const PsfmQpbSeq& S, unsigned q, unsigned rank)
{
    const double2 p0 = psfm_ld(a.row_p0, q * 16u), p1 = psfm_ld(a.row_p1, q * 16u), p2 = psfm_ld(a.row_p2, q * 16u);
    double2 r1, r2;
    double s;
    psfm_query_pc_refs(a, p0, r1, r2, s);
    S.x1[rank] = p1;
    S.x2[rank] = p2;
    S.ref1[rank] = r1;
    S.ref2[rank] = r2;
    S.scale[rank] = s;
    S.owner[rank] = (int)q;
}

// what the solve made of row `rank` goes back to its owner (psfm_query_pc_scatter, from buffer 0 of the chain)
__device__ __forceinline__ void psfm_qpb_scatter(const PsfmQueryPcFrame& a, const PsfmQpbSeq& S, unsigned rank)
{
    const unsigned q = (unsigned)S.owner[rank];
    psfm_st(a.row_p1, q * 16u, S.x1[rank]);
    psfm_st(a.row_p2, q * 16u, S.x2[rank]);
}
