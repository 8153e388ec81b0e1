// HOST driver of particle-sfm_amd/csrc/psfm_query_pc.h for tests/test_queries_pc_host.py: one frame of psfm_track_queries_optimize as
// its kernels run it -- every lane's step and row decision, the rows compacted in query order, the scatter behind the solve -- compiled
// through tests/host/shim, one lane per wave (a wave's ballot is the lane's own value), with plain loops where the kernels have threads
// and a running count where they have the scan.  Built with -ffp-contract=off.  Test infrastructure.
#include "psfm_query_pc.h"

static PsfmQueryPcFrame frame_args(const float* flow, const uint8_t* masks, const float* flow01, const float* flow02, const uint8_t* occ02,
                                   int h, int w, const int* q_t, long n_q, double* slab, int* len, int from, int dir)
{
    PsfmQueryPcFrame a;
    a.fr.flow = (const float2*)flow; a.fr.occ = masks; a.fr.H = h; a.fr.W = w;
    a.fr.cw = (float)((w - 1) / 2.0); a.fr.ch = (float)((h - 1) / 2.0);
    a.fr.rcw = psfm_rcp_host(a.fr.cw); a.fr.rch = psfm_rcp_host(a.fr.ch);
    a.flow01 = (const float2*)flow01; a.flow02 = (const float2*)flow02; a.occ02 = occ02;
    a.q_t = q_t; a.Q = (unsigned)n_q; a.len = len; a.wave_cnt = nullptr; a.from = from; a.dir = dir;
    double2* s = (double2*)slab;
    a.row_p1 = s + (size_t)from * a.Q; a.row_p2 = s + (size_t)(from + dir) * a.Q;
    a.row_p0 = flow01 ? s + (size_t)(from - dir) * a.Q : nullptr;
    return a;
}

// One frame: slab (frames, Q, 2) f64 by frame and len (Q) are updated in place; took (Q): 0 the lane did not step, 1 it stepped and is
// not alive, 2 alive.  flow01 == NULL: no solve.  Returns the number of rows written to uv12 (.,4), ref1, ref2 (.,2), scale, owner.
extern "C" int psfm_host_query_pc_frame(const float* flow, const uint8_t* masks, const float* flow01, const float* flow02,
                                        const uint8_t* occ02, int h, int w, const int* q_t, long n_q, int mb, int from, int dir, double* slab,
                                        int* len, uint8_t* took, double* uv12, double* ref1, double* ref2, double* scale, int* owner)
{
    const PsfmQueryPcFrame a = frame_args(flow, masks, flow01, flow02, occ02, h, w, q_t, n_q, slab, len, from, dir);
    PsfmQueryPcRows r;
    r.uv12 = (double2*)uv12; r.ref1 = (double2*)ref1; r.ref2 = (double2*)ref2; r.scale = scale; r.owner = owner;
    unsigned n_rows = 0;
    for (unsigned q = 0; q < a.Q; q++) {
        const int t = q_t[q], n = len[q];
        took[q] = 0;
        bool row = false;
        if (psfm_query_pc_tail_at(t, n, a.from, a.dir)) {
            const bool slow = psfm_query_any(n == 1);
            if (mb) row = slow ? psfm_query_pc_step<true, false>(a, q, n) : psfm_query_pc_step<true, true>(a, q, n);
            else row = slow ? psfm_query_pc_step<false, false>(a, q, n) : psfm_query_pc_step<false, true>(a, q, n);
            took[q] = len[q] == n + 1 ? 2 : 1;
        }
        // (the rows kernel decides again, from what the step launch left in memory: the two must agree)
        if (psfm_query_pc_is_row(a, t, len[q]) != row) return -1;
        if (row) psfm_query_pc_row(a, r, q, n_rows++);
    }
    return (int)n_rows;
}

extern "C" void psfm_host_query_pc_scatter(int h, int w, long n_q, int from, int dir, double* slab, const double* out, const int* owner,
                                           int n_rows)
{
    const PsfmQueryPcFrame a = frame_args(nullptr, nullptr, nullptr, nullptr, nullptr, h, w, nullptr, n_q, slab, nullptr, from, dir);
    for (int i = 0; i < n_rows; i++) psfm_query_pc_scatter(a, (const double2*)out, owner, (unsigned)i);
}
