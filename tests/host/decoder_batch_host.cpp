// HOST driver of particle-sfm_amd/csrc/psfm_decoder_batch.h for tests/test_decoder_batch_host.py: the batch plan of
// psfm_traj_decode_batch -- the table of windows, the flattened tile and slice maps, the lookup a block performs, the plan by
// section names and its resolution per window -- compiled through tests/host/shim.  The arithmetic is decoder_host.cpp's, included
// as it stands: the batch walks the SAME run_layer / combine / run_l2 with the addresses a block of the batch kernels would form.
// Test infrastructure.
#include "decoder_host.cpp"
#include "psfm_decoder_batch.h"

#include <string.h>

extern "C" int psfm_host_decoder_batch_max(void) { return PSFM_DEC_BATCH_MAX; }
extern "C" size_t psfm_host_decoder_batch_arg_bytes(void) { return sizeof(PsfmDecBatch) + sizeof(PsfmDecLayer); }

// The layout for k[0 .. n_win): the four columns (64 entries each), {n_win, tiles, slices, bad}, the workspace bytes.  Returns the
// header's status (0 = planned).
extern "C" int psfm_host_decoder_batch_layout(const long* k, int n_win, long* k_out, long* ws_off, long* tile0, long* slice0, long* info4,
                                              size_t* total)
{
    static PsfmDecBatch B;
    std::vector<int64_t> kk(k, k + (n_win > 0 ? n_win : 0));
    int bad;
    const int rc = psfm_dec_batch_layout(B, kk.data(), n_win, *total, bad);
    info4[3] = bad;
    if (rc != PSFM_DEC_BATCH_OK) return rc;
    for (int b = 0; b < PSFM_DEC_BATCH_MAX; b++) { k_out[b] = B.k[b]; ws_off[b] = (long)B.ws_off[b]; tile0[b] = B.tile0[b]; slice0[b] = B.slice0[b]; }
    info4[0] = B.n_win; info4[1] = B.tiles; info4[2] = B.slices;
    return rc;
}

// The lookup of a block: first[64] as the layout wrote it.
extern "C" int psfm_host_decoder_batch_find(const long* first, int blk)
{
    int f[PSFM_DEC_BATCH_MAX];
    for (int i = 0; i < PSFM_DEC_BATCH_MAX; i++) f[i] = (int)first[i];
    return psfm_dec_batch_find(f, blk);
}

// A layer of the plan by names, as a block of window W sees it.
static PsfmDecLayer resolved(const PsfmDecLayer& N, const PsfmDecWin& W, const PsfmDecBatch& B, int b)
{
    PsfmDecLayer Y = N;
    for (int i = 0; i < 3; i++) { Y.seg[i].src = psfm_dec_resolve(N.seg[i].src, W); Y.seg[i].stat = psfm_dec_resolve(N.seg[i].stat, W); }
    Y.residual = psfm_dec_resolve(N.residual, W);
    Y.out = psfm_dec_resolve(N.out, W);
    Y.part = psfm_dec_resolve(N.part, W);
    Y.x2 = psfm_dec_resolve(N.x2, W);
    Y.logits = B.logits[b]; Y.prob = B.prob[b]; Y.pred = B.pred[b];
    return Y;
}

// For every window: the plan by names, resolved in the window, against psfm_dec_plan for that window alone at the window's workspace.
// Returns the number of fields that differ (0 = the two plans are the same), -1 when the layout refuses the batch.
extern "C" long psfm_host_decoder_batch_plan_mismatches(const long* k, int n_win)
{
    static PsfmDecBatch B;
    static PsfmDecPlan N, P;
    std::vector<int64_t> kk(k, k + (n_win > 0 ? n_win : 0));
    size_t total;
    int bad;
    if (psfm_dec_batch_layout(B, kk.data(), n_win, total, bad) != PSFM_DEC_BATCH_OK) return -1;
    char* const ws = (char*)0x7f0000000000;                 // (nothing is dereferenced)
    const float* const w = (const float*)0x100000;
    B.ws = ws;
    long diff = 0;
    psfm_dec_plan_names(N, w);
    for (int b = 0; b < n_win; b++) {
        if (kk[b] == 0) continue;
        B.enc[b] = (const float*)(0x200000 + 0x1000 * (size_t)b);
        B.logits[b] = (float*)(0x300000 + 0x1000 * (size_t)b); B.prob[b] = (float*)(0x400000 + 0x1000 * (size_t)b);
        B.pred[b] = (uint8_t*)(0x500000 + 0x1000 * (size_t)b);
        const PsfmDecWin W = psfm_dec_batch_window(B, b);
        psfm_dec_plan(P, B.enc[b], w, kk[b], ws + B.ws_off[b], B.logits[b], B.prob[b], B.pred[b]);
        diff += N.nsteps != P.nsteps;
        diff += W.L.nb != P.nb || W.L.nb2 != P.nb2 || W.k != P.k;
        diff += (float*)(W.base + W.L.x1) != P.x1 || (float*)(W.base + W.L.emb) != P.emb || (float*)(W.base + W.L.sm_fin) != P.sm_fin;
        diff += (float*)(W.base + W.L.pool_part) != P.pool_part || (float*)(W.base + W.L.x2) != P.x2;
        diff += (double*)(W.base + W.L.stat_part) != P.stat_part || (double*)(W.base + W.L.sm_part) != P.sm_part;
        for (int i = 0; i < N.nsteps && i < P.nsteps; i++) {
            const PsfmDecStep &A = N.step[i], &S = P.step[i];
            diff += A.kind != S.kind;
            diff += psfm_dec_resolve(A.fin, W) != S.fin;
            if (A.kind != PSFM_DEC_STEP_LAYER) continue;
            const PsfmDecLayer Y = resolved(A.layer, W, B, b);
            const PsfmDecLayer& Z = S.layer;
            for (int j = 0; j < 3; j++) {
                const PsfmDecSeg &u = Y.seg[j], &v = Z.seg[j];
                diff += u.src != v.src || u.w != v.w || u.stat != v.stat || u.bn != v.bn || u.cin != v.cin || u.ldw != v.ldw || u.bn_n != v.bn_n ||
                        u.bn_c0 != v.bn_c0;
            }
            diff += Y.nseg != Z.nseg || Y.mode != Z.mode || Y.cout != Z.cout || Y.bias != Z.bias || Y.bias2 != Z.bias2 || Y.residual != Z.residual;
            diff += Y.out != Z.out || Y.part != Z.part || Y.x2 != Z.x2 || Y.wout != Z.wout || Y.logits != Z.logits || Y.prob != Z.prob || Y.pred != Z.pred;
        }
    }
    return diff;
}

// psfm_traj_decode_batch on the host: ONE walk over the plan by names; per step every block of the batch's grid finds its window as
// the kernels do and works there.  Returns the number of steps (0: nothing to launch), -1 for what the entry point refuses.
extern "C" int psfm_host_traj_decode_batch(int n_win, const float* const* encoding, const long* k, const float* weights, void* workspace,
                                           size_t workspace_bytes, float* const* logits, float* const* prob, uint8_t* const* pred)
{
    static PsfmDecBatch B;
    static PsfmDecPlan N;
    if (n_win < 0 || n_win > PSFM_DEC_BATCH_MAX) return -1;
    std::vector<int64_t> kk(k, k + n_win);
    size_t need;
    int bad;
    if (psfm_dec_batch_layout(B, kk.data(), n_win, need, bad) != PSFM_DEC_BATCH_OK) return -1;
    if (B.tiles == 0) return 0;
    if (!encoding || !weights || !workspace || workspace_bytes < need) return -1;
    for (int b = 0; b < n_win; b++) {
        if (kk[b] > 0 && !encoding[b]) return -1;
        B.enc[b] = encoding[b];
        B.logits[b] = logits ? logits[b] : 0; B.prob[b] = prob ? prob[b] : 0; B.pred[b] = pred ? pred[b] : 0;
    }
    B.ws = (char*)workspace;
    psfm_dec_plan_names(N, weights);
    for (int i = 0; i < N.nsteps; i++) {
        const PsfmDecStep& S = N.step[i];
        if (S.kind == PSFM_DEC_STEP_LAYER || S.kind == PSFM_DEC_STEP_POOL) {
            // the flattened grids: block -> (window, block inside the window); run_layer and the pool loop take a whole window, so a
            // window runs when its first block comes by, and every block must land in the window whose range holds it
            const bool layer = S.kind == PSFM_DEC_STEP_LAYER;
            const int* first = layer ? B.tile0 : B.slice0;
            const int grid = layer ? B.tiles : B.slices;
            for (int blk = 0; blk < grid; blk++) {
                const int b = psfm_dec_batch_find(first, blk);
                const PsfmDecWin W = psfm_dec_batch_window(B, b);
                const int rel = blk - first[b];
                if (b >= n_win || rel < 0 || rel >= (layer ? W.L.nb : W.L.nb2)) return -2;
                if (rel != 0) continue;
                if (layer) run_layer(resolved(S.layer, W, B, b), W.k, W.L.nb);
                else {
                    // (decoder_host.cpp's pool step on this window's sections)
                    const float *x1 = (const float*)(W.base + W.L.x1), *emb = (const float*)(W.base + W.L.emb), *fin = (const float*)(W.base + W.L.sm_fin);
                    float* part = (float*)(W.base + W.L.pool_part);
                    std::vector<float> sw((size_t)PSFM_DEC_CL * PSFM_DEC_SLICE);
                    for (int s = 0; s < W.L.nb2; s++) {
                        const long base = (long)s * PSFM_DEC_SLICE;
                        const int n = (int)(W.k - base < PSFM_DEC_SLICE ? W.k - base : PSFM_DEC_SLICE);
                        for (int j = 0; j < PSFM_DEC_CL; j++)
                            for (int p = 0; p < n; p++)
                                sw[(size_t)j * PSFM_DEC_SLICE + p] = psfm_dec_pool_weight(emb[(long)j * W.k + base + p], fin[2 * j], fin[2 * j + 1]);
                        for (int c = 0; c < PSFM_DEC_C; c++)
                            for (int j = 0; j < PSFM_DEC_CL; j++) {
                                float acc = 0.0f;
                                for (int p = 0; p < n; p++) acc = fmaf(x1[(long)c * W.k + base + p], sw[(size_t)j * PSFM_DEC_SLICE + p], acc);
                                part[((size_t)s * PSFM_DEC_C + c) * PSFM_DEC_CL + j] = acc;
                            }
                    }
                }
            }
            continue;
        }
        for (int b = 0; b < n_win; b++) {                   // the per-window grids
            if (B.k[b] == 0) continue;
            const PsfmDecWin W = psfm_dec_batch_window(B, b);
            if (S.kind == PSFM_DEC_STEP_STATS) {
                const double* sp = (const double*)(W.base + W.L.stat_part);
                double* fin = psfm_dec_resolve(S.fin, W);
                for (int c = 0; c < PSFM_DEC_C; c++) {
                    const double s = combine(sp + (size_t)c * 2, (size_t)PSFM_DEC_C * 2, W.L.nb, false, 0, 0.0);
                    const double q = combine(sp + (size_t)c * 2 + 1, (size_t)PSFM_DEC_C * 2, W.L.nb, false, 0, 0.0);
                    psfm_dec_stat_finish(s, q, (double)W.k, fin[c], fin[PSFM_DEC_C + c]);
                }
            } else if (S.kind == PSFM_DEC_STEP_SOFTMAX) {
                float* fin = (float*)(W.base + W.L.sm_fin);
                for (int j = 0; j < PSFM_DEC_CL; j++) {
                    const double* p = (const double*)(W.base + W.L.sm_part) + (size_t)j * 2;
                    const double M = combine(p, (size_t)PSFM_DEC_CL * 2, W.L.nb, true, 0, 0.0);
                    const double sum = combine(p + 1, (size_t)PSFM_DEC_CL * 2, W.L.nb, false, p, M);
                    fin[2 * j] = (float)M;
                    fin[2 * j + 1] = (float)(1.0 / sum);
                }
            } else run_l2((const float*)(W.base + W.L.pool_part), W.L.nb2, weights + PSFM_DEC_W_L2, (float*)(W.base + W.L.x2));
        }
    }
    return N.nsteps;
}
