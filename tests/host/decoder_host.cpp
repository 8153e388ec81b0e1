// HOST driver of particle-sfm_amd/csrc/psfm_decoder.h for tests/test_decoder_host.py: the whole of psfm_traj_decode (the
// classifier's OANet decoder, motion_seg/core/network/oanet.py:13-206) compiled through tests/host/shim.  It walks the header's own
// plan step by step, block by block, with the header's folds, softmaxes and reduction orders; where the kernels issue the fp32
// matrix instruction it writes the k-ordered fmaf chain that the instruction equals.  Built with -ffp-contract=off.  Test
// infrastructure.  With -DPSFM_DECODER_HOST_MAIN it is a program of its own (for a sanitizer build):
//   decoder_host <weights.f32> <encoding.f32> <k> <logits-out.f32>
#include "psfm_decoder.h"

#include <stdio.h>
#include <stdlib.h>
#include <vector>

extern "C" int psfm_host_decoder_weight_count(void) { return PSFM_DEC_WEIGHTS; }

extern "C" size_t psfm_host_decoder_workspace_bytes(long k) { return psfm_dec_workspace(k).total; }

// The header's tables for the test: 7 section offsets of the packed weights + the total, then the 11 workspace offsets, the total,
// nb and nb2 for `k`.
extern "C" void psfm_host_decoder_tables(long k, long* weights8, long* ws14)
{
    const long w[8] = {PSFM_DEC_W_CONV1, PSFM_DEC_W_DOWN1, PSFM_DEC_W_UP1, PSFM_DEC_W_L1_1, PSFM_DEC_W_L1_2, PSFM_DEC_W_L2, PSFM_DEC_W_OUT,
                       PSFM_DEC_WEIGHTS};
    for (int i = 0; i < 8; i++) weights8[i] = w[i];
    const PsfmDecWs L = psfm_dec_workspace(k);
    const size_t o[14] = {L.a, L.t, L.x1, L.xup, L.emb, L.stat_part, L.stat_fin, L.sm_part, L.sm_fin, L.pool_part, L.x2, L.total,
                          (size_t)L.nb, (size_t)L.nb2};
    for (int i = 0; i < 14; i++) ws14[i] = (long)o[i];
}

static void run_layer(const PsfmDecLayer& Y, long k, int nb)
{
    std::vector<float> fm(3 * PSFM_DEC_C), fs(3 * PSFM_DEC_C), ft(3 * PSFM_DEC_C);
    for (int si = 0; si < Y.nseg; si++) {
        const PsfmDecSeg& S = Y.seg[si];
        if (S.stat)
            for (int c = 0; c < S.cin; c++)
                psfm_dec_fold(S.stat[c], S.stat[PSFM_DEC_C + c], S.bn, S.bn_n, S.bn_c0 + c, fm[si * PSFM_DEC_C + c], fs[si * PSFM_DEC_C + c],
                              ft[si * PSFM_DEC_C + c]);
    }
    std::vector<float> xin(3 * PSFM_DEC_C), img(PSFM_DEC_TILE * PSFM_DEC_LDX);
    for (int b = 0; b < nb; b++) {
        const long p0 = (long)b * PSFM_DEC_TILE;
        const int np = (int)(k - p0 < PSFM_DEC_TILE ? k - p0 : PSFM_DEC_TILE);
        for (int i = 0; i < PSFM_DEC_TILE * PSFM_DEC_LDX; i++) img[i] = NAN;          // (LDS starts out undefined)
        for (int pc = 0; pc < np; pc++) {
            const long p = p0 + pc;
            for (int si = 0; si < Y.nseg; si++) {
                const PsfmDecSeg& S = Y.seg[si];
                for (int c = 0; c < S.cin; c++) {
                    float v = S.src[(long)c * k + p];
                    if (S.stat) v = psfm_dec_norm_relu(v, fm[si * PSFM_DEC_C + c], fs[si * PSFM_DEC_C + c], ft[si * PSFM_DEC_C + c]);
                    xin[si * PSFM_DEC_C + c] = v;
                }
            }
            float* col = &img[pc * PSFM_DEC_LDX];
            float acc[PSFM_DEC_C];
            for (int row = 0; row < PSFM_DEC_C; row++) {
                float a = row < Y.cout ? Y.bias[row] : 0.0f;
                if (row < Y.cout)
                    for (int si = 0; si < Y.nseg; si++) {
                        const PsfmDecSeg& S = Y.seg[si];
                        for (int c = 0; c < S.cin; c++) a = fmaf(S.w[(long)row * S.ldw + c], xin[si * PSFM_DEC_C + c], a);
                    }
                acc[row] = a;
            }
            if (Y.mode == PSFM_DEC_UNPOOL) {
                float e[PSFM_DEC_C];
                for (int j = 0; j < PSFM_DEC_C; j++) e[j] = acc[j];
                psfm_dec_softmax_clusters(e);
                for (int row = 0; row < PSFM_DEC_C; row++) {
                    float a = 0.0f;
                    for (int j = 0; j < PSFM_DEC_CL; j++) a = fmaf(Y.x2[row * PSFM_DEC_CL + j], e[j], a);
                    acc[row] = a;
                }
            }
            for (int row = 0; row < PSFM_DEC_C; row++) {
                float v = acc[row];
                const bool live = Y.mode == PSFM_DEC_UNPOOL || row < Y.cout;
                if (Y.mode != PSFM_DEC_UNPOOL && Y.bias2 && row < Y.cout) v += Y.bias2[row];
                if (live && Y.residual) v += Y.residual[(long)row * k + p];
                if (live && Y.mode != PSFM_DEC_FINAL) Y.out[(long)row * k + p] = v;
                col[row] = v;
            }
            if (Y.mode == PSFM_DEC_FINAL) {
                float logit, prob;
                uint8_t pred;
                psfm_dec_verdict(col, Y.wout, logit, prob, pred);
                if (Y.logits) Y.logits[p] = logit;
                if (Y.prob) Y.prob[p] = prob;
                if (Y.pred) Y.pred[p] = pred;
            }
        }
        if (Y.mode == PSFM_DEC_FINAL) continue;
        const int n0 = np < 32 ? np : 32, n1 = np - n0;
        const int rows = Y.mode == PSFM_DEC_EMBED_DOWN ? PSFM_DEC_CL : PSFM_DEC_C;
        for (int c = 0; c < rows; c++) {
            const float *x0 = &img[c], *x1 = &img[32 * PSFM_DEC_LDX + c];
            double* dst = Y.part + ((size_t)b * rows + c) * 2;
            if (Y.mode == PSFM_DEC_EMBED_DOWN) {
                const float m = fmaxf(psfm_dec_max(x0, PSFM_DEC_LDX, n0), psfm_dec_max(x1, PSFM_DEC_LDX, n1));
                double s0, s1;
                psfm_dec_softmax_part(x0, PSFM_DEC_LDX, n0, m, s0);
                psfm_dec_softmax_part(x1, PSFM_DEC_LDX, n1, m, s1);
                dst[0] = (double)m;
                dst[1] = s0 + s1;
            } else {
                double s[2] = {0.0, 0.0}, q[2] = {0.0, 0.0};
                for (int i = 0; i < np; i++) {
                    const double v = (double)img[i * PSFM_DEC_LDX + c];
                    s[i >> 5] += v;
                    q[i >> 5] += v * v;
                }
                dst[0] = s[0] + s[1];
                dst[1] = q[0] + q[1];
            }
        }
    }
}

// nb per-block values at stride `stride` from p, combined in the header's order by `threads` emulated threads
static double combine(const double* p, size_t stride, int nb, bool is_max, const double* scale_m, double M)
{
    double a[PSFM_DEC_THREADS];
    for (int t = 0; t < PSFM_DEC_THREADS; t++) {
        double s = is_max ? -INFINITY : 0.0;
        for (int i = t; i < nb; i += PSFM_DEC_THREADS) {
            const double v = p[(size_t)i * stride];
            if (is_max) s = fmax(s, v);
            else s += scale_m ? v * exp(scale_m[(size_t)i * stride] - M) : v;
        }
        a[t] = s;
    }
    for (int st = PSFM_DEC_THREADS / 2; st > 0; st >>= 1)
        for (int t = 0; t < PSFM_DEC_THREADS; t++) {
            if (is_max) psfm_dec_tree_max(a, t, st);
            else psfm_dec_tree_add(a, t, st);
        }
    return a[0];
}

static void run_l2(const float* part, int nb2, const float* w, float* x2)
{
    const int C = PSFM_DEC_C, J = PSFM_DEC_CL;
    std::vector<float> x(C * J), a(C * J), b(C * J), y(C * J);
    for (int c = 0; c < C; c++)
        for (int j = 0; j < J; j++) {
            float s = 0.0f;
            for (int i = 0; i < nb2; i++) s += part[((size_t)i * C + c) * J + j];
            x[c * J + j] = s;
        }
    auto norm = [&](const std::vector<float>& v, const float* bn) {          // y = relu(bn(in(v))) over the clusters per channel
        for (int c = 0; c < C; c++) {
            double s[2] = {0.0, 0.0}, q[2] = {0.0, 0.0};
            for (int j = 0; j < J; j++) {
                const double u = (double)v[c * J + j];
                s[j / (J / 2)] += u;
                q[j / (J / 2)] += u * u;
            }
            double mean, inv;
            float m, sc, sh;
            psfm_dec_stat_finish(s[0] + s[1], q[0] + q[1], (double)J, mean, inv);
            psfm_dec_fold(mean, inv, bn, C, c, m, sc, sh);
            for (int j = 0; j < J; j++) y[c * J + j] = psfm_dec_norm_relu(v[c * J + j], m, sc, sh);
        }
    };
    auto conv = [&](const float* W, const float* bias, std::vector<float>& out) {      // out = W y + bias over the channels
        for (int c = 0; c < C; c++)
            for (int j = 0; j < J; j++) {
                float acc = bias[c];
                for (int cc = 0; cc < C; cc++) acc = fmaf(W[c * C + cc], y[cc * J + j], acc);
                out[c * J + j] = acc;
            }
    };
    for (int f = 0; f < 4; f++) {
        const float* p = w + f * PSFM_DEC_OA_SIZE;
        norm(x, p);
        conv(p + PSFM_DEC_OA_W1, p + PSFM_DEC_OA_B1, a);
        for (int j = 0; j < J; j++) {
            float s2, t2;
            psfm_dec_fold_bn(p + PSFM_DEC_OA_BN2, J, j, s2, t2);
            for (int c = 0; c < C; c++) y[c * J + j] = psfm_dec_norm_relu(a[c * J + j], 0.0f, s2, t2);
        }
        for (int c = 0; c < C; c++)
            for (int jo = 0; jo < J; jo++) {
                float acc = p[PSFM_DEC_OA_B2 + jo];
                for (int j = 0; j < J; j++) acc = fmaf(y[c * J + j], p[PSFM_DEC_OA_W2 + jo * J + j], acc);
                b[c * J + jo] = acc;
            }
        for (int i = 0; i < C * J; i++) a[i] += b[i];
        norm(a, p + PSFM_DEC_OA_BN3);
        conv(p + PSFM_DEC_OA_W3, p + PSFM_DEC_OA_B3, b);
        for (int i = 0; i < C * J; i++) x[i] = b[i] + x[i];
    }
    for (int i = 0; i < C * J; i++) x2[i] = x[i];
}

// psfm_traj_decode on the host.  Returns the number of steps of the plan (0 for k = 0), -1 for an argument the entry point refuses.
extern "C" int psfm_host_traj_decode(const float* encoding, const float* weights, long k, void* workspace, size_t workspace_bytes,
                                     float* logits, float* prob, uint8_t* pred)
{
    if (k < 0 || k == 1 || k > PSFM_DEC_MAX_K) return -1;
    if (k == 0) return 0;
    if (!encoding || !weights || !workspace || workspace_bytes < psfm_dec_workspace(k).total) return -1;
    static PsfmDecPlan P;
    psfm_dec_plan(P, encoding, weights, k, workspace, logits, prob, pred);
    for (int i = 0; i < P.nsteps; i++) {
        const PsfmDecStep& S = P.step[i];
        if (S.kind == PSFM_DEC_STEP_LAYER) run_layer(S.layer, k, P.nb);
        else if (S.kind == PSFM_DEC_STEP_STATS) {
            for (int c = 0; c < PSFM_DEC_C; c++) {
                const double s = combine(P.stat_part + (size_t)c * 2, (size_t)PSFM_DEC_C * 2, P.nb, false, 0, 0.0);
                const double q = combine(P.stat_part + (size_t)c * 2 + 1, (size_t)PSFM_DEC_C * 2, P.nb, false, 0, 0.0);
                psfm_dec_stat_finish(s, q, (double)k, S.fin[c], S.fin[PSFM_DEC_C + c]);
            }
        } else if (S.kind == PSFM_DEC_STEP_SOFTMAX) {
            for (int j = 0; j < PSFM_DEC_CL; j++) {
                const double* p = P.sm_part + (size_t)j * 2;
                const double M = combine(p, (size_t)PSFM_DEC_CL * 2, P.nb, true, 0, 0.0);
                const double sum = combine(p + 1, (size_t)PSFM_DEC_CL * 2, P.nb, false, p, M);
                P.sm_fin[2 * j] = (float)M;
                P.sm_fin[2 * j + 1] = (float)(1.0 / sum);
            }
        } else if (S.kind == PSFM_DEC_STEP_POOL) {
            std::vector<float> sw((size_t)PSFM_DEC_CL * PSFM_DEC_SLICE);
            for (int b = 0; b < P.nb2; b++) {
                const long base = (long)b * PSFM_DEC_SLICE;
                const int n = (int)(k - base < PSFM_DEC_SLICE ? k - base : PSFM_DEC_SLICE);
                for (int j = 0; j < PSFM_DEC_CL; j++)
                    for (int i = 0; i < n; i++)
                        sw[(size_t)j * PSFM_DEC_SLICE + i] = psfm_dec_pool_weight(P.emb[(long)j * k + base + i], P.sm_fin[2 * j], P.sm_fin[2 * j + 1]);
                for (int c = 0; c < PSFM_DEC_C; c++)
                    for (int j = 0; j < PSFM_DEC_CL; j++) {
                        float acc = 0.0f;
                        for (int i = 0; i < n; i++) acc = fmaf(P.x1[(long)c * k + base + i], sw[(size_t)j * PSFM_DEC_SLICE + i], acc);
                        P.pool_part[((size_t)b * PSFM_DEC_C + c) * PSFM_DEC_CL + j] = acc;
                    }
            }
        } else run_l2(P.pool_part, P.nb2, weights + PSFM_DEC_W_L2, P.x2);
    }
    return P.nsteps;
}

#ifdef PSFM_DECODER_HOST_MAIN
static std::vector<float> read_floats(const char* path, size_t n)
{
    std::vector<float> v(n);
    FILE* f = fopen(path, "rb");
    if (!f || fread(v.data(), sizeof(float), n, f) != n) { fprintf(stderr, "cannot read %zu floats from %s\n", n, path); exit(2); }
    fclose(f);
    return v;
}

int main(int argc, char** argv)
{
    if (argc != 5) { fprintf(stderr, "usage: %s weights.f32 encoding.f32 k logits-out.f32\n", argv[0]); return 2; }
    const long k = atol(argv[3]);
    const std::vector<float> w = read_floats(argv[1], PSFM_DEC_WEIGHTS), x = read_floats(argv[2], (size_t)PSFM_DEC_IN * k);
    const size_t bytes = psfm_host_decoder_workspace_bytes(k);
    std::vector<char> ws(bytes);                    // exactly the stated size: the sanitizer guards both ends
    std::vector<float> logits(k), prob(k);
    std::vector<uint8_t> pred(k);
    const int steps = psfm_host_traj_decode(x.data(), w.data(), k, ws.data(), bytes, logits.data(), prob.data(), pred.data());
    if (steps <= 0) { fprintf(stderr, "refused\n"); return 1; }
    FILE* f = fopen(argv[4], "wb");
    if (!f || fwrite(logits.data(), sizeof(float), k, f) != (size_t)k) return 2;
    fclose(f);
    long dyn = 0;
    for (long i = 0; i < k; i++) dyn += pred[i];
    printf("steps %d  k %ld  dynamic %ld\n", steps, k, dyn);
    return 0;
}
#endif
