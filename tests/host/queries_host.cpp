// HOST driver of particle-sfm_amd/csrc/psfm_query.h for tests/test_queries_host.py: the per-lane frame loop of psfm_query_track_kernel
// compiled through tests/host/shim, one lane per wave (the wave's ballots and minima are the lane's own values), with a plain loop
// where the kernel has threads.  Built with -ffp-contract=off: every *_rn intrinsic is the IEEE operation it names.  Test infrastructure.
#include "psfm_query.h"

// One direction over every query.  masks: the stack's occlusion maps (mb == 0) or its kill maps (mb != 0); slab (n_flows+1, Q, 2) f64
// by absolute frame; len (Q): points of this direction, the query included.
extern "C" void psfm_host_track_queries(const float* flows, const uint8_t* masks, int n_flows, int h, int w, const double* q_xy,
                                        const int* q_t, long n_q, int mb, int back, double* slab, int* len)
{
    PsfmQueryArgs a;
    a.flows = (const float2*)flows; a.masks = masks;
    a.q_xy = (const double2*)q_xy; a.q_t = q_t; a.slab = (double2*)slab; a.len = len;
    a.H = h; a.W = w; a.n_flows = n_flows; a.Q = (unsigned)n_q; a.P = (unsigned)(h * w);
    a.cw = (float)((w - 1) / 2.0); a.ch = (float)((h - 1) / 2.0);
    a.rcw = psfm_rcp_host(a.cw); a.rch = psfm_rcp_host(a.ch);
    for (unsigned q = 0; q < a.Q; q++) {
        const double2 p = a.q_xy[q];
        const int t = q_t[q];
        psfm_st(a.slab + (size_t)t * a.Q, q * 16u, p);
        int n;
        if (mb) n = back ? psfm_query_walk<true, true>(a, true, p, t, q) : psfm_query_walk<true, false>(a, true, p, t, q);
        else n = back ? psfm_query_walk<false, true>(a, true, p, t, q) : psfm_query_walk<false, false>(a, true, p, t, q);
        len[q] = n;
    }
}
