// Stand-alone host check of the tap-PAIR flow sampler (particle-sfm_amd/csrc/psfm_device.h through tests/host/shim) against the
// four-tap sampler it replaces in the persistent loop's fused flow_check slices.
//  * The sampler: for every map width W in [2, 6], height H in [2, 3], every north-west tap column x0 in [-3, W + 2] and row y0 in
//    [-3, H + 2], a set of fractions, and maps whose pixels carry distinct sentinel values -- all finite, then with each pixel in
//    turn NaN, +Inf, -Inf -- the two-channel sample must have the same BITS, and the pair's base and picks must be the stated rule
//    (xb = min(max(x0, 0), W - 2); west = x0 > xb ? hi : lo; east = x0 < xb ? lo : hi), inside the map.  A partner pixel of a pair, a
//    clamped duplicate or a zero-padded tap that leaks into the blend turns a finite result into NaN (or moves it) and is caught.
//  * Its user: the mask-only flow_check verdict of a pixel in both forms (psfm_flow_check_px<false, PAIRS>), with forward flows that
//    put the sample on, just inside, just outside and two pixels outside every border, and non-finite border pixels in B.
// Exit status 0 = all equal; prints the number of comparisons.  Built and run by tests/test_tap_pairs_host.py.  Test infrastructure.
#include <stdio.h>
#include <vector>

#include "psfm_chain.h"

static unsigned bits(float v) { unsigned u; memcpy(&u, &v, 4); return u; }

int main()
{
    const float fr[] = {0.0f, 0.25f, 0.5f, 0.8125f, 0.99999994f};
    const float poison[] = {0.0f /* none */, NAN, INFINITY, -INFINITY};
    long n = 0, bad = 0;
    for (int W = 2; W <= 6; ++W)
        for (int H = 2; H <= 3; ++H) {
            // one element of slack on both sides: an out-of-bounds read of either sampler would show as a sentinel in the result
            std::vector<float2> store(H * W + 2);
            float2* map = store.data() + 1;
            for (int pz = 0; pz < 4; ++pz)
                for (int pp = (pz == 0 ? H * W - 1 : 0); pp < H * W; ++pp) {      // which pixel is non-finite (pz == 0: none, one pass)
                    for (int i = -1; i <= H * W; ++i) { map[i].x = 1.0f + 3.0f * (float)i; map[i].y = -2.0f - 7.0f * (float)i; }
                    if (pz != 0) { map[pp].x = poison[pz]; map[pp].y = poison[pz]; }
                    for (int y0 = -3; y0 <= H + 2; ++y0)
                        for (int x0 = -3; x0 <= W + 2; ++x0)
                            for (float fw : fr)
                                for (float fn : fr) {
                                    PsfmTaps t = psfm_weights(fw, fn);
                                    t.x0 = x0; t.y0 = y0;
                                    const float2 a = psfm_sample_flow(map, H, W, t);
                                    const float2 b = psfm_sample_flow_pairs(map, H, W, t);
                                    const PsfmPairIdx k = psfm_pair_idx(H, W, t);
                                    const int xb = min(max(x0, 0), W - 2);
                                    const bool rule = (k.whi == (x0 > xb)) & (k.elo == (x0 < xb)) & (k.n % W == xb) & (k.s % W == xb) &
                                                      (k.n >= 0) & (k.n + 1 < H * W) & (k.s >= 0) & (k.s + 1 < H * W);
                                    ++n;
                                    if (bits(a.x) != bits(b.x) || bits(a.y) != bits(b.y) || !rule) {
                                        if (++bad <= 10)
                                            printf("MISMATCH W=%d H=%d x0=%d y0=%d fw=%g fn=%g poison=%d@%d: flow %08x %08x vs %08x %08x rule=%d\n",
                                                   W, H, x0, y0, fw, fn, pz, pp, bits(a.x), bits(a.y), bits(b.x), bits(b.y), (int)rule);
                                    }
                                }
                }
        }
    // ---- the flow_check verdict built on the pairs ----
    for (int W = 2; W <= 6; ++W)
        for (int H = 2; H <= 6; H += (H == 3 ? 3 : 1)) {
            std::vector<float2> back(H * W);
            for (int pz = 0; pz < 4; ++pz) {
                for (int i = 0; i < H * W; ++i)
                    back[i] = make_float2(-0.37f * (float)((i * 7) % 5 - 2) + 0.4f * (float)(i % 3 - 1), 0.29f * (float)((i * 3) % 7 - 3));
                if (pz != 0)      // non-finite values in the first / last two columns and rows
                    for (int y = 0; y < H; ++y)
                        for (int x = 0; x < W; ++x)
                            if (((x < 2) | (x >= W - 2) | (y < 2) | (y >= H - 2)) && ((x * 3 + y * 5 + pz) % 4 == 0)) {
                                back[y * W + x].x = poison[pz]; back[y * W + x].y = poison[(pz % 3) + 1];
                            }
                PsfmFcParams q;
                q.H = H; q.W = W; q.cw = (float)((W - 1) / 2.0); q.ch = (float)((H - 1) / 2.0);
                q.rcw = psfm_rcp_host(q.cw); q.rch = psfm_rcp_host(q.ch); q.thres = 1.0f; q.t2 = psfm_sq_threshold(1.0f);
                const double offs[] = {-2.0, -1.0, -0.999, -0.5, -1e-6, 0.0, 1e-6, 0.5, 0.999};
                // every pixel, forward flows that carry it to an offset from the map's first / last column and row
                for (double fy : offs)
                    for (double fx : offs)
                        for (int sgn = -1; sgn <= 1; sgn += 2)
                            for (int yy = 0; yy < H; ++yy)
                                for (int xx = 0; xx < W; ++xx) {
                                    const float2 f = make_float2((float)(sgn * fx) + (sgn > 0 ? (float)(W - 1 - xx) : (float)-xx),
                                                                 (float)(sgn * fy) + (sgn > 0 ? (float)(H - 1 - yy) : (float)-yy));
                                    float e;
                                    const uint8_t o0 = psfm_flow_check_px<false, false>(back.data(), xx, yy, f, q, &e);
                                    const uint8_t o1 = psfm_flow_check_px<false, true>(back.data(), xx, yy, f, q, &e);
                                    ++n;
                                    if (o0 != o1 && ++bad <= 10) printf("FLOW_CHECK MISMATCH W=%d H=%d px=(%d,%d) f=(%g,%g) poison=%d\n", W, H, xx, yy, f.x, f.y, pz);
                                }
            }
        }
    printf("%ld comparisons, %ld mismatches\n", n, bad);
    return bad == 0 ? 0 : 1;
}
