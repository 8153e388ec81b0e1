// psfm_query_pc.h -- one lane's work in a frame of psfm_track_queries_optimize (psfm_query_pc.hip): caller-given query points carried
// through a flow stack as psfm_query.h carries them, with the stride-2 path-consistency solve of track_optimize.py:49-50 after every step.
// A solve is joint over the call's queries (Ceres' trust-region loop is global), so the engine is a loop of launches over frames and a
// lane's state between two launches is in memory: its positions in the time-major slab (row f of query q at f * Q + q) and len[q], the
// points of this direction so far.  The lane's tail is at frame t + dir * (len - 1); a lane whose tail is the frame being stepped from
// takes part, every other lane has ended (or not begun).
//   step   psfm_step_issue + psfm_step_finish<MB, FAST> of psfm_chain.h on the tail (trajectory.py:45-62); alive: the new position goes
//          into the slab row of the next frame.  The lane is a ROW of this frame's solve when it is alive and now holds three positions
//          p0, p1, p2 (optimize_buffer, trajectory.py:165-169)
//   row    uv12 = (p1, p2), ref1 = p0 + flow01(p0), ref2 = p0 + flow02(p0), scale = (1 - occ02(p0)) * (|flow02| < 20) in fp32
//          (trajectory.py:173-183): the arithmetic of pc_refs (psfm_pc_tracks.h), rows compacted in query order
// The host build of the CPU suite compiles this text (tests/host/queries_pc_host.cpp), one lane per wave.
#pragma once
#include "psfm_query.h"

struct PsfmQueryPcFrame {
    PsfmQueryFrame fr;            // the map being stepped through and its occlusion (MB: kill) map
    const float2* flow01;         // the maps of this frame's solve (all NULL: no solve, no lane is a row):
    const float2* flow02;         // stride-1 map p0 was stepped through, stride-2 map from p0's frame, ITS occlusion map
    const uint8_t* occ02;
    const int* q_t;               // (Q) query frames
    double2* row_p0;              // slab rows of the frames of p0 (NULL without a solve), p1 (the tails) and p2 (the new positions)
    double2* row_p1;
    double2* row_p2;
    int* len;                     // (Q) points of this direction so far, the query included
    int* wave_cnt;                // (waves of the launch) rows per wave; after the scan: rows in the waves before
    unsigned Q;
    int from, dir;                // the frame being stepped from; +1 forward, -1 backward
};

// the compacted rows of a solve, as psfm_solve_batch takes them, and the query every row belongs to
struct PsfmQueryPcRows {
    double2* uv12;                // (n, 2): p1, p2
    double2* ref1;
    double2* ref2;
    double* scale;
    int* owner;
};

__device__ __forceinline__ bool psfm_query_pc_tail_at(int t, int n, int frame, int dir) { return t + dir * (n - 1) == frame; }

// a lane whose tail is at a.from takes its step; returns whether it is a row of this frame's solve
template <bool MB, bool FAST>
__device__ __forceinline__ bool psfm_query_pc_step(const PsfmQueryPcFrame& a, unsigned q, int n)
{
    const double2 p = psfm_ld(a.row_p1, q * 16u);
    const PsfmStep s = psfm_query_step<MB, FAST>(a.fr, p);
    if (!s.alive) return false;                            // trajectory.py:138-147: the track ends at its last alive position
    psfm_st(a.row_p2, q * 16u, s.next);
    a.len[q] = n + 1;
    return (a.flow01 != nullptr) & (n + 1 >= 3);
}

// after the step launch of a frame: is the lane a row of its solve?  (its tail is the new frame and it holds three positions)
__device__ __forceinline__ bool psfm_query_pc_is_row(const PsfmQueryPcFrame& a, int t, int n)
{
    return (a.flow01 != nullptr) & (n >= 3) & psfm_query_pc_tail_at(t, n, a.from + a.dir, a.dir);
}

// refs / scale from p0: pc_refs of psfm_pc_tracks.h, the fp32 sampler with the true division on flow01, flow02 and occ02
__device__ __forceinline__ void psfm_query_pc_refs(const PsfmQueryPcFrame& a, double2 p0, double2& r1, double2& r2, double& s)
{
    const PsfmTaps t = psfm_taps((float)p0.x, (float)p0.y, a.fr.cw, a.fr.ch, a.fr.H, a.fr.W);
    const PsfmTapIdx k = psfm_tap_idx(a.fr.H, a.fr.W, t);
    const float2 f01 = psfm_sample_flow(a.flow01, k, t);
    const float2 f02 = psfm_sample_flow(a.flow02, k, t);
    const float o02 = psfm_sample_mask(a.occ02, k, t);
    // (1.0 - occ02) * (|flow02| < 20) in fp32; numpy's norm = sqrt(u*u + v*v) without fma (trajectory.py:179)
    const float nrm = sqrtf(__fadd_rn(__fmul_rn(f02.x, f02.x), __fmul_rn(f02.y, f02.y)));
    const float sf = __fmul_rn(__fsub_rn(1.0f, o02), nrm < 20.0f ? 1.0f : 0.0f);
    s = (double)sf;
    r1 = make_double2(p0.x + (double)f01.x, p0.y + (double)f01.y);
    r2 = make_double2(p0.x + (double)f02.x, p0.y + (double)f02.y);
}

// row `rank` of the solve from lane q: three 16-byte position loads, four 16-byte stores, the scale, the owner
__device__ __forceinline__ void psfm_query_pc_row(const PsfmQueryPcFrame& a, const PsfmQueryPcRows& r, unsigned q, unsigned rank)
{
    const double2 p0 = psfm_ld(a.row_p0, q * 16u), p1 = psfm_ld(a.row_p1, q * 16u), p2 = psfm_ld(a.row_p2, q * 16u);
    double2 r1, r2;
    double s;
    psfm_query_pc_refs(a, p0, r1, r2, s);
    r.uv12[2 * (size_t)rank] = p1;                         // (n < 2^28 rows of 32 bytes: 64-bit offsets)
    r.uv12[2 * (size_t)rank + 1] = p2;
    r.ref1[rank] = r1;
    r.ref2[rank] = r2;
    r.scale[rank] = s;
    r.owner[rank] = (int)q;
}

// what the solve made of row `rank` goes back to its owner: p1 and p2 (the next step starts from the optimised p2)
__device__ __forceinline__ void psfm_query_pc_scatter(const PsfmQueryPcFrame& a, const double2* out, const int* owner, unsigned rank)
{
    const unsigned q = (unsigned)owner[rank];
    psfm_st(a.row_p1, q * 16u, out[2 * (size_t)rank]);
    psfm_st(a.row_p2, q * 16u, out[2 * (size_t)rank + 1]);
}
