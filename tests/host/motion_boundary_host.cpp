// HOST driver of particle-sfm_amd/csrc/psfm_motion_boundary.h and of psfm_step_finish<MB> (psfm_chain.h) for
// tests/test_motion_boundary_host.py: the arithmetic of psfm_mb_kernel and of the chain step's two verdicts (trajectory.py:39-43,
// :45-62) compiled through tests/host/shim, with plain loops where the kernels have threads.  Built with -ffp-contract=off: every
// *_rn intrinsic is the IEEE operation it names.  Test infrastructure.
#include "psfm_motion_boundary.h"
#include "psfm_chain.h"

// flows (n,H,W,2) f32, occ (n,H,W) u8 or NULL -> out (n,H,W): 0/1, or the kill map (occ != 0) | mb << 1
extern "C" void psfm_host_motion_boundary(const float* flows, const uint8_t* occ, int n, int h, int w, float thres, uint8_t* out)
{
    for (int f = 0; f < n; f++) {
        const float2* F = (const float2*)flows + (int64_t)f * h * w;
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                const int64_t p = (int64_t)f * h * w + y * w + x;
                const unsigned v = psfm_mb_at(F, x, y, h, w, thres);
                out[p] = (uint8_t)(occ ? ((occ[p] != 0 ? PSFM_KILL_OCC : 0u) | (v ? PSFM_KILL_MB : 0u)) : v);
            }
    }
}

struct HostFrame {
    const float2* flow; const uint8_t* occ;
    int H, W; float cw, ch, rcw, rch;
};

// one step of every position: `mask` is the occlusion map (mb == 0) or the kill map (mb != 0)
extern "C" void psfm_host_step(const float* flow, const uint8_t* mask, int h, int w, const double* xy, long n, int mb, double* next,
                               uint8_t* alive, float* flow_sample)
{
    HostFrame a;
    a.flow = (const float2*)flow; a.occ = mask; a.H = h; a.W = w;
    a.cw = (float)((w - 1) / 2.0); a.ch = (float)((h - 1) / 2.0);
    a.rcw = psfm_rcp_host(a.cw); a.rch = psfm_rcp_host(a.ch);
    for (long i = 0; i < n; i++) {
        const double2 p = make_double2(xy[2 * i], xy[2 * i + 1]);
        const PsfmStepLoads L = psfm_step_issue(a, p);
        const PsfmStep s = mb ? psfm_step_finish<true>(a, p, L) : psfm_step_finish<false>(a, p, L);
        next[2 * i] = s.next.x; next[2 * i + 1] = s.next.y;
        alive[i] = s.alive ? 1 : 0;
        flow_sample[2 * i] = s.flow.x; flow_sample[2 * i + 1] = s.flow.y;
    }
}
