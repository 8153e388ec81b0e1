// psfm_decoder.h -- the motion classifier's OANet decoder without the matrix instruction: the packed-weight offset table, the
// workspace layout, the plan (which launch reads and writes what), the InstanceNorm / BatchNorm fold, the statistics combine, the
// two softmaxes and the reduction orders, shared by the kernels (psfm_decoder.hip) and the host build of the CPU suite
// (tests/host/decoder_host.cpp through tests/host/shim).
// psfm_decoder_batch.h adds the window dimension of psfm_traj_decode_batch on top of this file.
//
// Reference: traj_oa_depth.decoder = OANBlock(128, 16, depth 8, clusters 100), eval mode (motion_seg/core/network/oanet.py:13-206),
// then torch.sigmoid (traj_oa_depth.py:124) and `> 0.5` (main_motion_segmentation.py:80).  N = k trajectories are the points, B = 1.
//   - InstanceNorm2d(eps 1e-3) has no affine and no running statistics: the BIASED variance over the k points of this call;
//   - BatchNorm2d in eval is the affine of running_mean / running_var (eps 1e-5) / weight / bias;
//   - down1's softmax runs over the k points per cluster, x_down = x1_1 S^T uses the RAW x1_1; up1's softmax runs over the 100
//     clusters per point and has its own BatchNorm and convolution; down1, up1 and the first 128 channels of l1_2.0 normalise the
//     same x1_1 with ONE set of instance statistics and differ in their BatchNorm only.
// Every activation is [channel][k] fp32.  Every product is a k-ordered fmaf chain in ascending input index that starts from the
// bias: what __builtin_amdgcn_mfma_f32_32x32x2f32 evaluates bit for bit, and what the host build writes as a loop.
// STATISTICS: a layer's blocks write per channel the f64 sum and f64 sum of squares of their (at most 64) stored fp32 outputs;
// psfm_dec_stats_kernel adds the blocks' partials in f64 in a fixed order (thread t takes blocks t, t + 256, ..., then a binary tree)
// and forms mean and 1 / sqrt(var + 1e-3) in f64.  The square of an fp32 value is exact in f64 and a sum of 10^5 of them loses
// nothing that matters, so var = E[x^2] - mean^2 in f64 keeps about 9 digits even where the mean is 10^3 standard deviations: no
// fp32 E[x^2] - E[x]^2 anywhere.  No floating-point atomics; two identical calls give identical bits.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#define PSFM_DEC_C 128          // net_channels
#define PSFM_DEC_IN 16          // the encoder's features
#define PSFM_DEC_CL 100         // clusters
#define PSFM_DEC_TILE 64        // points per block of the layer kernel
#define PSFM_DEC_SLICE 512      // points per block of the pool product
#define PSFM_DEC_KC 32          // input channels per staged weight chunk
#define PSFM_DEC_LDW 33         // floats per row of a staged chunk (odd: consecutive rows start on different banks)
#define PSFM_DEC_LDX 129        // floats per row of a staged [point][channel] tile
#define PSFM_DEC_THREADS 256
#define PSFM_DEC_IN_EPS 1e-3
#define PSFM_DEC_BN_EPS 1e-5
#define PSFM_DEC_MAX_K ((int64_t)(INT32_MAX / PSFM_DEC_C))     // 32-bit indices in the kernels: an activation index below 128 k

// Packed weights (include/psfm.h documents the order: the module's state_dict order, every tensor row-major [out][in]).
#define PSFM_DEC_W_CONV1 0              // conv1.weight [128][16], .bias [128]
#define PSFM_DEC_W_DOWN1 2176           // down1: a pool block
#define PSFM_DEC_W_UP1 15588            // up1: a pool block
#define PSFM_DEC_W_L1_1 29000           // l1_1.{0..3}: PointCN(128)
#define PSFM_DEC_W_L1_2 165192          // l1_2.0: PointCN(256,128); l1_2.{1..3}: PointCN(128) from PSFM_DEC_W_L1_2 + PSFM_DEC_PW_SIZE
#define PSFM_DEC_W_L2 351176            // l2.{0..3}: OAFilter(128,100)
#define PSFM_DEC_W_OUT 529368           // output.weight [128], .bias [1]
#define PSFM_DEC_WEIGHTS 529497
// a BatchNorm over n channels: weight [n], bias [n], running_mean [n], running_var [n]
// a pool block: BatchNorm(128), conv [100][128], bias [100]
#define PSFM_DEC_PL_W 512
#define PSFM_DEC_PL_B 13312
#define PSFM_DEC_PL_SIZE 13412
// PointCN(128): BatchNorm(128), conv a [128][128], bias, BatchNorm(128), conv b [128][128], bias
#define PSFM_DEC_PC_WA 512
#define PSFM_DEC_PC_BA 16896
#define PSFM_DEC_PC_BN2 17024
#define PSFM_DEC_PC_WB 17536
#define PSFM_DEC_PC_BB 33920
#define PSFM_DEC_PC_SIZE 34048
// PointCN(256,128): shot_cut [128][256], bias, BatchNorm(256), conv a [128][256], bias, BatchNorm(128), conv b [128][128], bias
#define PSFM_DEC_PW_SCB 32768
#define PSFM_DEC_PW_BN1 32896
#define PSFM_DEC_PW_WA 33920
#define PSFM_DEC_PW_BA 66688
#define PSFM_DEC_PW_BN2 66816
#define PSFM_DEC_PW_WB 67328
#define PSFM_DEC_PW_BB 83712
#define PSFM_DEC_PW_SIZE 83840
// OAFilter(128,100): BatchNorm(128), conv1 [128][128], bias, BatchNorm(100), conv2 [100][100], bias [100], BatchNorm(128), conv3 [128][128], bias
#define PSFM_DEC_OA_W1 512
#define PSFM_DEC_OA_B1 16896
#define PSFM_DEC_OA_BN2 17024
#define PSFM_DEC_OA_W2 17424
#define PSFM_DEC_OA_B2 27424
#define PSFM_DEC_OA_BN3 27524
#define PSFM_DEC_OA_W3 28036
#define PSFM_DEC_OA_B3 44420
#define PSFM_DEC_OA_SIZE 44548

#define PSFM_DEC_SLOTS 24               // reduced statistics: one slot of (mean[128], inv[128]) f64 per normalised tensor
#define PSFM_DEC_MAX_STEPS 64

// ---- workspace ------------------------------------------------------------------------------------------------------------
struct PsfmDecWs {
    size_t a, t, x1, xup, emb;          // [128][k] x 4, [100][k]: the activations that must survive and the two ping-pong buffers
    size_t stat_part, stat_fin;         // f64 [nb][128][2]; f64 [PSFM_DEC_SLOTS][2][128]
    size_t sm_part, sm_fin;             // f64 [nb][100][2] (max, sum of exponentials); f32 [100][2] (max, 1 / sum)
    size_t pool_part, x2;               // f32 [nb2][128][100]; f32 [128][100]
    size_t total;
    int nb, nb2;                        // blocks of the layer kernel, of the pool product
};

__host__ __device__ __forceinline__ size_t psfm_dec_align(size_t v) { return (v + 255) & ~(size_t)255; }

__host__ __device__ inline PsfmDecWs psfm_dec_workspace(int64_t k)
{
    PsfmDecWs w;
    const size_t n = (size_t)(k > 0 ? k : 0);
    w.nb = (int)((n + PSFM_DEC_TILE - 1) / PSFM_DEC_TILE);
    w.nb2 = (int)((n + PSFM_DEC_SLICE - 1) / PSFM_DEC_SLICE);
    size_t o = 0;
    w.a = o;         o = psfm_dec_align(o + n * PSFM_DEC_C * sizeof(float));
    w.t = o;         o = psfm_dec_align(o + n * PSFM_DEC_C * sizeof(float));
    w.x1 = o;        o = psfm_dec_align(o + n * PSFM_DEC_C * sizeof(float));
    w.xup = o;       o = psfm_dec_align(o + n * PSFM_DEC_C * sizeof(float));
    w.emb = o;       o = psfm_dec_align(o + n * PSFM_DEC_CL * sizeof(float));
    w.stat_part = o; o = psfm_dec_align(o + (size_t)w.nb * PSFM_DEC_C * 2 * sizeof(double));
    w.stat_fin = o;  o = psfm_dec_align(o + (size_t)PSFM_DEC_SLOTS * 2 * PSFM_DEC_C * sizeof(double));
    w.sm_part = o;   o = psfm_dec_align(o + (size_t)w.nb * PSFM_DEC_CL * 2 * sizeof(double));
    w.sm_fin = o;    o = psfm_dec_align(o + (size_t)PSFM_DEC_CL * 2 * sizeof(float));
    w.pool_part = o; o = psfm_dec_align(o + (size_t)w.nb2 * PSFM_DEC_C * PSFM_DEC_CL * sizeof(float));
    w.x2 = o;        o = psfm_dec_align(o + (size_t)PSFM_DEC_C * PSFM_DEC_CL * sizeof(float));
    w.total = o;
    return w;
}

// ---- the plan ---------------------------------------------------------------------------------------------------------------
// One input of a layer: `cin` channels of src [cin][k] against columns of w (row stride ldw).  stat != NULL: the channels are
// normalised on the way in -- InstanceNorm from stat (mean[128], inv[128]), BatchNorm channels bn_c0 .. of a BatchNorm over bn_n
// channels at bn -- and passed through ReLU; stat == NULL: taken raw.
struct PsfmDecSeg { const float* src; const float* w; const double* stat; const float* bn; int cin, ldw, bn_n, bn_c0; };

enum { PSFM_DEC_PLAIN = 0,      // out = sum of the segments + bias (+ bias2) (+ residual); per-block channel statistics of out
       PSFM_DEC_EMBED_DOWN = 1, // 100 rows: out = the embedding; per-block softmax partials over the points
       PSFM_DEC_UNPOOL = 2,     // 100 rows: softmax over the clusters per point, then out = x2 S; per-block statistics of out
       PSFM_DEC_FINAL = 3 };    // as PLAIN, then the `output` convolution, the sigmoid and the threshold; nothing else is stored

struct PsfmDecLayer {
    PsfmDecSeg seg[3];
    int nseg, mode, cout;
    const float *bias, *bias2, *residual;
    float* out;
    double* part;                       // PLAIN, UNPOOL: stat_part; EMBED_DOWN: sm_part
    const float* x2;                    // UNPOOL
    const float* wout;                  // FINAL: output.weight [128], .bias
    float *logits, *prob;               // FINAL, each may be NULL
    uint8_t* pred;
};

enum { PSFM_DEC_STEP_LAYER = 0, PSFM_DEC_STEP_STATS = 1, PSFM_DEC_STEP_SOFTMAX = 2, PSFM_DEC_STEP_POOL = 3, PSFM_DEC_STEP_L2 = 4 };

struct PsfmDecStep { int kind; PsfmDecLayer layer; double* fin; /* STATS: where the reduced statistics go */ };

struct PsfmDecPlan {
    PsfmDecStep step[PSFM_DEC_MAX_STEPS];
    int nsteps, nb, nb2;
    int64_t k;
    const float* w;
    float *x1, *emb, *sm_fin, *pool_part, *x2;
    double *stat_part, *sm_part;
};

// Where the eleven sections of a workspace begin, in the order of PsfmDecWs.
struct PsfmDecBufs { char *a, *t, *x1, *xup, *emb, *stat_part, *stat_fin, *sm_part, *sm_fin, *pool_part, *x2; };

// The fixed sequence of launches on the sections B for input enc; `w` is the packed weights.  Nothing is dereferenced here, and
// nothing depends on k: psfm_decoder_batch.h plans once with section NAMES in place of addresses and resolves them per window.
inline void psfm_dec_plan_at(PsfmDecPlan& P, const float* enc, const float* w, const PsfmDecBufs& B, float* logits, float* prob, uint8_t* pred)
{
    float *A = (float*)B.a, *T = (float*)B.t, *X1 = (float*)B.x1, *XUP = (float*)B.xup;
    double* fin = (double*)B.stat_fin;
    P.nsteps = 0; P.w = w;
    P.x1 = X1; P.emb = (float*)B.emb; P.sm_fin = (float*)B.sm_fin; P.pool_part = (float*)B.pool_part;
    P.x2 = (float*)B.x2; P.stat_part = (double*)B.stat_part; P.sm_part = (double*)B.sm_part;
    int slot = 0;
    const PsfmDecSeg none = {0, 0, 0, 0, 0, 0, 0, 0};
    // a layer step, followed by the reduction of its statistics into a fresh slot (returned) unless it stores none
    auto layer = [&](int mode, int cout, int nseg, PsfmDecSeg s0, PsfmDecSeg s1, PsfmDecSeg s2, const float* bias, const float* bias2,
                     const float* residual, float* out) -> double* {
        PsfmDecStep& S = P.step[P.nsteps++];
        S.kind = PSFM_DEC_STEP_LAYER; S.fin = 0;
        PsfmDecLayer& Y = S.layer;
        Y.seg[0] = s0; Y.seg[1] = s1; Y.seg[2] = s2; Y.nseg = nseg; Y.mode = mode; Y.cout = cout;
        Y.bias = bias; Y.bias2 = bias2; Y.residual = residual; Y.out = out;
        Y.part = mode == PSFM_DEC_EMBED_DOWN ? P.sm_part : P.stat_part;
        Y.x2 = P.x2; Y.wout = w + PSFM_DEC_W_OUT; Y.logits = logits; Y.prob = prob; Y.pred = pred;
        if (mode == PSFM_DEC_EMBED_DOWN || mode == PSFM_DEC_FINAL) return 0;
        PsfmDecStep& R = P.step[P.nsteps++];
        R.kind = PSFM_DEC_STEP_STATS; R.layer = Y; R.fin = fin + (size_t)(slot++) * 2 * PSFM_DEC_C;
        return R.fin;
    };
    auto simple = [&](int kind) { PsfmDecStep& S = P.step[P.nsteps++]; S.kind = kind; S.fin = 0; S.layer = P.step[0].layer; };
    auto seg = [&](const float* src, const float* wm, int cin, int ldw, const double* stat, const float* bn, int bn_n, int bn_c0) {
        PsfmDecSeg s = {src, wm, stat, bn, cin, ldw, bn_n, bn_c0};
        return s;
    };
    // PointCN(128) at weights p on `in` (statistics st): T = conv a; out = conv b + in.  Returns out's statistics.
    auto point_cn = [&](const float* p, const float* in, const double* st, float* out, bool last) -> double* {
        double* st_t = layer(PSFM_DEC_PLAIN, PSFM_DEC_C, 1, seg(in, p + PSFM_DEC_PC_WA, 128, 128, st, p, 128, 0), none, none,
                             p + PSFM_DEC_PC_BA, 0, 0, T);
        return layer(last ? PSFM_DEC_FINAL : PSFM_DEC_PLAIN, PSFM_DEC_C, 1, seg(T, p + PSFM_DEC_PC_WB, 128, 128, st_t, p + PSFM_DEC_PC_BN2, 128, 0),
                     none, none, p + PSFM_DEC_PC_BB, 0, in, out);
    };
    // conv1, l1_1: x1_1 ends in X1
    double* st = layer(PSFM_DEC_PLAIN, PSFM_DEC_C, 1, seg(enc, w + PSFM_DEC_W_CONV1, PSFM_DEC_IN, PSFM_DEC_IN, 0, 0, 0, 0), none, none,
                       w + PSFM_DEC_W_CONV1 + PSFM_DEC_C * PSFM_DEC_IN, 0, 0, A);
    for (int i = 0; i < 4; i++) st = point_cn(w + PSFM_DEC_W_L1_1 + i * PSFM_DEC_PC_SIZE, A, st, i == 3 ? X1 : A, false);
    double* st_x1 = st;
    // down1: the embedding and its softmax over the points, the pooled product, l2
    const float* pd = w + PSFM_DEC_W_DOWN1;
    layer(PSFM_DEC_EMBED_DOWN, PSFM_DEC_CL, 1, seg(X1, pd + PSFM_DEC_PL_W, 128, 128, st_x1, pd, 128, 0), none, none, pd + PSFM_DEC_PL_B, 0, 0, P.emb);
    simple(PSFM_DEC_STEP_SOFTMAX);
    simple(PSFM_DEC_STEP_POOL);
    simple(PSFM_DEC_STEP_L2);
    // up1: x_up = x2 softmax_clusters(embedding)
    const float* pu = w + PSFM_DEC_W_UP1;
    double* st_up = layer(PSFM_DEC_UNPOOL, PSFM_DEC_CL, 1, seg(X1, pu + PSFM_DEC_PL_W, 128, 128, st_x1, pu, 128, 0), none, none, pu + PSFM_DEC_PL_B,
                          0, 0, XUP);
    // l1_2.0 = PointCN(256,128) on cat(x1_1, x_up)
    const float* pw = w + PSFM_DEC_W_L1_2;
    double* st_t = layer(PSFM_DEC_PLAIN, PSFM_DEC_C, 2, seg(X1, pw + PSFM_DEC_PW_WA, 128, 256, st_x1, pw + PSFM_DEC_PW_BN1, 256, 0),
                         seg(XUP, pw + PSFM_DEC_PW_WA + 128, 128, 256, st_up, pw + PSFM_DEC_PW_BN1, 256, 128), none, pw + PSFM_DEC_PW_BA, 0, 0, T);
    st = layer(PSFM_DEC_PLAIN, PSFM_DEC_C, 3, seg(T, pw + PSFM_DEC_PW_WB, 128, 128, st_t, pw + PSFM_DEC_PW_BN2, 128, 0),
               seg(X1, pw, 128, 256, 0, 0, 0, 0), seg(XUP, pw + 128, 128, 256, 0, 0, 0, 0), pw + PSFM_DEC_PW_BB, pw + PSFM_DEC_PW_SCB, 0, A);
    for (int i = 0; i < 3; i++) st = point_cn(w + PSFM_DEC_W_L1_2 + PSFM_DEC_PW_SIZE + i * PSFM_DEC_PC_SIZE, A, st, A, i == 2);
}

// The plan for k points in the workspace at `ws`.
inline void psfm_dec_plan(PsfmDecPlan& P, const float* enc, const float* w, int64_t k, void* ws, float* logits, float* prob, uint8_t* pred)
{
    const PsfmDecWs L = psfm_dec_workspace(k);
    char* base = (char*)ws;
    const PsfmDecBufs B = {base + L.a, base + L.t, base + L.x1, base + L.xup, base + L.emb, base + L.stat_part, base + L.stat_fin,
                           base + L.sm_part, base + L.sm_fin, base + L.pool_part, base + L.x2};
    psfm_dec_plan_at(P, enc, w, B, logits, prob, pred);
    P.nb = L.nb; P.nb2 = L.nb2; P.k = k;
}

// ---- arithmetic -------------------------------------------------------------------------------------------------------------
// InstanceNorm (mean, inv = 1 / sqrt(var + 1e-3)) and BatchNorm channel c of bn (weight, bias, running_mean, running_var, n each)
// as y = fma(x - m, s, t), s and t formed in f64 and rounded once.  The mean is subtracted first, as the reference does: where a
// channel's spread is far below its mean (down to identical points) x s + t' would leave the rounding of mean s in every value.
__host__ __device__ __forceinline__ void psfm_dec_fold(double mean, double inv, const float* bn, int n, int c, float& m, float& s, float& t)
{
    const double g = (double)bn[c] / sqrt((double)bn[3 * n + c] + PSFM_DEC_BN_EPS);
    m = (float)mean;
    s = (float)(inv * g);
    t = (float)((double)bn[n + c] - (double)bn[2 * n + c] * g);
}

// BatchNorm alone (OAFilter.conv2 over the 100 point-channels)
__host__ __device__ __forceinline__ void psfm_dec_fold_bn(const float* bn, int n, int c, float& s, float& t)
{
    float m;
    psfm_dec_fold(0.0, 1.0, bn, n, c, m, s, t);
}

__host__ __device__ __forceinline__ float psfm_dec_norm_relu(float x, float m, float s, float t) { return fmaxf(__fmaf_rn(__fsub_rn(x, m), s, t), 0.0f); }

// sum and sum of squares over n values -> mean and 1 / sqrt(biased variance + eps)
__host__ __device__ __forceinline__ void psfm_dec_stat_finish(double sum, double sq, double n, double& mean, double& inv)
{
    mean = sum / n;
    double var = sq / n - mean * mean;
    var = var > 0.0 ? var : 0.0;
    inv = 1.0 / sqrt(var + PSFM_DEC_IN_EPS);
}

// The fixed order in which PSFM_DEC_THREADS threads add nb per-block values: thread t takes t, t + 256, ...; then this tree.
// a[256]; on the device one call per thread and level with a barrier between levels, on the host a loop over t per level.
__host__ __device__ __forceinline__ void psfm_dec_tree_add(double* a, int t, int s) { if (t < s) a[t] += a[t + s]; }
__host__ __device__ __forceinline__ void psfm_dec_tree_max(double* a, int t, int s) { if (t < s) a[t] = fmax(a[t], a[t + s]); }

// down1: a block's share of one cluster's softmax over the points: (max m, sum of exp(e - m)) over its n values at stride ld
__host__ __device__ __forceinline__ void psfm_dec_softmax_part(const float* e, int ld, int n, float m, double& s)
{
    s = 0.0;
    for (int i = 0; i < n; i++) s += (double)expf(e[i * ld] - m);
}
__host__ __device__ __forceinline__ float psfm_dec_max(const float* e, int ld, int n)
{
    float m = -INFINITY;
    for (int i = 0; i < n; i++) m = fmaxf(m, e[i * ld]);
    return m;
}
// ... and one entry of S once the blocks are combined to (M, 1 / sum)
__host__ __device__ __forceinline__ float psfm_dec_pool_weight(float e, float M, float inv_sum) { return __fmul_rn(expf(e - M), inv_sum); }

// up1: softmax over the 100 clusters of one point, in place
__host__ __device__ __forceinline__ void psfm_dec_softmax_clusters(float* e)
{
    float m = e[0];
    for (int j = 1; j < PSFM_DEC_CL; j++) m = fmaxf(m, e[j]);
    float s = 0.0f;
    for (int j = 0; j < PSFM_DEC_CL; j++) { e[j] = expf(e[j] - m); s += e[j]; }
    for (int j = 0; j < PSFM_DEC_CL; j++) e[j] = __fdiv_rn(e[j], s);
}

// the `output` convolution on one point's 128 channels (stride 1), the sigmoid, the threshold on the fp32 probability
__host__ __device__ __forceinline__ void psfm_dec_verdict(const float* x, const float* wout, float& logit, float& prob, uint8_t& pred)
{
    float a = wout[PSFM_DEC_C];
    for (int c = 0; c < PSFM_DEC_C; c++) a = __fmaf_rn(wout[c], x[c], a);
    logit = a;
    prob = __fdiv_rn(1.0f, 1.0f + expf(-a));
    pred = prob > 0.5f ? 1 : 0;
}
