// psfm_query.h -- one lane's frame loop of psfm_track_queries (psfm_query.hip): a caller-given position (x, y) at frame t carried through
// a flow stack by the body of track.py:37-47 -- grid_sample of the flow (trajectory.py:25-37), step_forward (trajectory.py:45-62) -- until
// the first step that is not alive or the end of the stack.  No grid, no births, no occupancy map: a query interacts with no other track.
// The step is psfm_step_issue + psfm_step_finish<MB> of psfm_chain.h; the host build of the CPU suite compiles this text
// (tests/host/queries_host.cpp), with one lane per wave.
#pragma once
#include "psfm_chain.h"

// what the lanes of a wave agree on: does any lane ..., the smallest value over the wave, a value every lane holds as a scalar.
// (Without psfm_query_uniform the compiler rebuilds the slab row inside the region where a lane takes part from the lane's own t,
// which equals f there: two 64-bit VALU multiply-adds per store instead of one.)
#if defined(__HIPCC__)
__device__ __forceinline__ bool psfm_query_any(bool b) { return __ballot(b) != 0ull; }
__device__ __forceinline__ int psfm_query_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int psfm_query_wave_min(int v)
{
#pragma unroll
    for (int d = 1; d < PSFM_WAVE; d <<= 1) v = min(v, __shfl_xor(v, d, PSFM_WAVE));
    return psfm_query_uniform(v);      // every lane holds the minimum: say so, and what is built on it stays scalar
}
#else
static inline bool psfm_query_any(bool b) { return b; }
static inline int psfm_query_uniform(int v) { return v; }
static inline int psfm_query_wave_min(int v) { return v; }
#endif

struct PsfmQueryArgs {
    const float2* flows;          // the stack being sampled, (n_flows,H,W,2): forward flows, or backward flows (map f: frame f+1 -> f)
    const uint8_t* masks;         // ITS occlusion maps (n_flows,H,W), or its kill maps (MB: bit 0 occlusion, bit 1 motion boundary)
    const double2* q_xy;          // (Q) query positions
    const int* q_t;               // (Q) query frames, 0 <= t <= n_flows (validated before the launch)
    double2* slab;                // (n_flows+1, Q) positions by ABSOLUTE frame: row f of query q at f * Q + q; a row stays below 4 GB
    int* len;                     // (Q) points of this direction, the query included (>= 1)
    int H, W, n_flows;
    unsigned Q, P;                // queries; pixels of a map (H W < 2^29: psfm_frame_ok)
    float cw, ch, rcw, rch;
};

// one map of the stack as psfm_step_issue / psfm_step_finish read it
struct PsfmQueryFrame {
    const float2* flow; const uint8_t* occ;
    int H, W; float cw, ch, rcw, rch;
};

// FAST = false for a wave in which some lane takes its FIRST step: the caller's coordinates are arbitrary, so the tap geometry is built
// with the true division.  Later positions satisfy 0 < x < W-1, 0 < y < H-1 -- the domain on which psfm_div_r is the true quotient bit
// for bit -- so either form gives them the same bits, and a wave of later steps only takes the short one.
template <bool MB, bool FAST>
__device__ __forceinline__ PsfmStep psfm_query_step(const PsfmQueryFrame& fr, double2 p)
{
    const PsfmStepLoads L = psfm_step_issue<FAST>(fr, p);      // four 8-byte flow taps + four mask bytes behind one wait
    return psfm_step_finish<MB, FAST>(fr, p, L);
}

// The lane's walk.  BACK = false: a query at frame t samples map t and moves to frame t+1, up to frame n_flows (track.py:37-47).
// BACK = true: the same recurrence on the backward stack -- a query at frame t samples map t-1 and moves to frame t-1, down to frame 0.
// The wave runs over absolute frames in lock-step: from the first frame any of its lanes starts at, a lane takes part from its own t
// while it is alive, and the wave leaves when no lane has anything left (all tests on `f` and on ballots: wave-uniform).  Every alive
// step stores the new position (16 bytes) into the slab row of its frame: row base scalar, lane offset 32 bits.
// Returns the number of points of this direction (the query itself is point one; the caller has stored it).
template <bool MB, bool BACK>
__device__ __forceinline__ int psfm_query_walk(const PsfmQueryArgs& a, bool has_query, double2 p, int t, unsigned q)
{
    bool live = has_query & (BACK ? t > 0 : t < a.n_flows);
    bool first = true;
    int n = 1;
    // steps are counted from the wave's first frame: step k of the wave is absolute frame f0 + k (forward) / f0 - k (backward)
    const int f0 = BACK ? a.n_flows - psfm_query_wave_min(live ? a.n_flows - t : a.n_flows)
                        : psfm_query_wave_min(live ? t : a.n_flows);
    int f = f0;
    while (psfm_query_any(live)) {
        const bool take = live & (t == f);
        const int map = BACK ? f - 1 : f, to = BACK ? f - 1 : f + 1;
        if (psfm_query_any(take)) {            // (map is in [0, n_flows) here: a taking lane has 0 < f (BACK) / f < n_flows)
            PsfmQueryFrame fr;
            fr.flow = a.flows + (size_t)map * a.P; fr.occ = a.masks + (size_t)map * a.P;
            fr.H = a.H; fr.W = a.W; fr.cw = a.cw; fr.ch = a.ch; fr.rcw = a.rcw; fr.rch = a.rch;
            double2* row = a.slab + (size_t)(unsigned)psfm_query_uniform(to) * a.Q;
            const bool slow = psfm_query_any(take & first);
            if (take) {
                PsfmStep s;
                if (slow) s = psfm_query_step<MB, false>(fr, p);
                else s = psfm_query_step<MB, true>(fr, p);
                first = false;
                if (s.alive) {
                    p = s.next; t = to; ++n;
                    psfm_st(row, q * 16u, p);
                    live = BACK ? t > 0 : t < a.n_flows;
                } else {
                    live = false;              // trajectory.py:138-147: the track ends at its last alive position
                }
            }
        }
        f = to;
    }
    return n;
}
