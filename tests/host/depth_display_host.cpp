// HOST driver of particle-sfm_amd/csrc/psfm_depth_display.h for tests/test_depth_display_host.py: the per-element rules of the kernels
// of psfm_depth_display.hip (sfm/convert.py:26-41 and :95) compiled through tests/host/shim, with plain loops where the kernels have
// threads and plain additions where they have integer atomics.  Built with -ffp-contract=off.  Test infrastructure.
#include <vector>

#include "psfm_depth_display.h"

extern "C" void psfm_host_dd_rank(uint32_t n, double q, uint32_t* j, uint32_t* j1, double* g) { psfm_dd_rank(n, q, j, j1, g); }

extern "C" double psfm_host_dd_lerp(double a, double b, double g) { return psfm_dd_lerp(a, b, g); }

// The four passes of the device over one map.  table: 256 words + the bad one.  Returns the number of valid pixels; 0: rgba, z and
// sel are left untouched.  sel: the four selected bit patterns (j, j + 1 of pc; j, j + 1 of 100 - pc).
extern "C" int64_t psfm_host_dd_image(const double* depth, int64_t n_pix, double pc, const uint32_t* table, uint32_t* rgba, double* z,
                                      uint64_t* sel)
{
    uint32_t n = 0;
    for (int64_t p = 0; p < n_pix; p++)
        if (psfm_dd_valid(depth[p])) n++;
    if (n == 0) return 0;
    std::vector<uint64_t> comp;
    comp.reserve(n);
    for (int64_t p = n_pix - 1; p >= 0; p--)                               // (any order: the selection does not depend on it)
        if (psfm_dd_valid(depth[p])) comp.push_back(psfm_dd_bits(psfm_dd_inv(depth[p])));
    PsfmDdState s;
    memset(&s, 0, sizeof(s));
    psfm_dd_state_init(&s, n, pc);
    std::vector<uint32_t> hist(PSFM_DD_RANKS * PSFM_DD_BINS);
    for (int round = 0; round < PSFM_DD_ROUNDS; round++) {
        for (uint32_t& c : hist) c = 0;
        for (uint64_t u : comp) {
            const unsigned m = psfm_dd_owners(s, u, round), dg = psfm_dd_digit(u, round);
            for (int r = 0; r < PSFM_DD_RANKS; r++)
                if (m >> r & 1u) hist[r * PSFM_DD_BINS + dg]++;
        }
        psfm_dd_advance(&s, hist.data(), round);
    }
    for (int r = 0; r < PSFM_DD_RANKS; r++) sel[r] = s.prefix[r];
    z[0] = s.z[0];
    z[1] = s.z[1];
    for (int64_t p = 0; p < n_pix; p++) rgba[p] = table[psfm_dd_index(depth[p], s.z[0], s.z[1])];
    return n;
}
