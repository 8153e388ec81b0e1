// psfm_decoder.hip -- the motion classifier's OANet decoder, the sigmoid and the threshold as a fixed sequence of launches behind
// psfm_traj_encode.
//
// Reference: traj_oa_depth.decoder = OANBlock(128, 16, depth 8, clusters 100), eval mode (motion_seg/core/network/oanet.py:13-206).
// torch runs it as about 150 launches per window that stream every [128][k] activation through HBM once per operator; here one
// launch per convolution normalises its input while it stages it, forms the product on the exact fp32 matrix instruction
// (v_mfma_f32_32x32x2_f32: bit for bit the k-ordered fmaf chain of psfm_decoder.h) and leaves its output's channel statistics as
// per-block f64 partials.  What is not the matrix instruction -- the plan, the folds, the softmaxes, the orders -- is psfm_decoder.h.
// The five kernel bodies are __device__ functions; psfm_traj_decode's kernels call them with the block's own index, the kernels of
// psfm_traj_decode_batch (the windows of a sequence in ONE sequence of launches, psfm_decoder_batch.h) after they found their window.
#include "psfm_decoder_batch.h"
#include "psfm_internal.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

// The row of a 32x32 accumulator tile that register r of this lane holds (the column is lane & 31).
__device__ __forceinline__ int pd_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// acc[t] += A (32 rows x kc) B_t^T (32 rows x kc), t < NT: both operands are LDS images [row][k], A at row stride lda, tile t of B
// 32 rows further at row stride ldb.  Lane l feeds A[l & 31][kk + (l >> 5)] and B[l & 31][kk + (l >> 5)] of step kk: ascending k.
template <int NT>
__device__ __forceinline__ void pd_mma(f32x16 (&acc)[NT], const float* A, int lda, const float* B, int ldb, int kc, int lane)
{
    const int i = lane & 31, h = lane >> 5;
    const float* a = A + i * lda + h;
    const float* b = B + i * ldb + h;
    for (int kk = 0; kk < kc; kk += 2) {
        const float av = a[kk];
#pragma unroll
        for (int t = 0; t < NT; t++) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b[t * 32 * ldb + kk], acc[t], 0, 0, 0);
    }
}

// acc[t] (rows = this wave's 32 rows of the weights, columns = tile t of the image) += W[rows][0 .. cin) image[.][0 .. cin):
// W (global, `wrows` valid rows of stride ldw) goes through ldsW in chunks of PSFM_DEC_KC input channels; `img` is the LDS image
// [column][k] at stride ldi.  SWAP: the image gives the rows (this wave's 32) and W the column tiles instead.
// Begins with a barrier (the image is complete, ldsW is free) and ends after the last product.
template <int NT, bool SWAP>
__device__ __forceinline__ void pd_gemm(f32x16 (&acc)[NT], const float* __restrict__ w, int ldw, int cin, int wrows, float* ldsW,
                                        const float* img, int ldi, int tid)
{
    const int wave = tid >> 6, lane = tid & 63;
    for (int k0 = 0; k0 < cin; k0 += PSFM_DEC_KC) {
        const int kc = min(PSFM_DEC_KC, cin - k0);
        __syncthreads();
        for (int idx = tid; idx < PSFM_DEC_C * kc; idx += PSFM_DEC_THREADS) {
            const int o = idx / kc, kk = idx - o * kc;
            ldsW[o * PSFM_DEC_LDW + kk] = o < wrows ? w[o * ldw + k0 + kk] : 0.0f;
        }
        __syncthreads();
        if (SWAP) pd_mma<NT>(acc, img + wave * 32 * ldi + k0, ldi, ldsW, PSFM_DEC_LDW, kc, lane);
        else pd_mma<NT>(acc, ldsW + wave * 32 * PSFM_DEC_LDW, PSFM_DEC_LDW, img + k0, ldi, kc, lane);
    }
}

// Where a block's addresses come from.  PdOne: the plan holds them (psfm_traj_decode).  PdWin: the plan holds section names and the
// block resolves them in its window of the batch (psfm_decoder_batch.h); the three outputs come from the table.
struct PdOne {
    template <class T> __device__ __forceinline__ T* operator()(T* p) const { return p; }
    __device__ __forceinline__ float* logits(const PsfmDecLayer& Y) const { return Y.logits; }
    __device__ __forceinline__ float* prob(const PsfmDecLayer& Y) const { return Y.prob; }
    __device__ __forceinline__ uint8_t* pred(const PsfmDecLayer& Y) const { return Y.pred; }
};
struct PdWin {
    PsfmDecWin W;
    float *lo, *pr;
    uint8_t* pd;
    template <class T> __device__ __forceinline__ T* operator()(T* name) const { return psfm_dec_resolve(name, W); }
    __device__ __forceinline__ float* logits(const PsfmDecLayer&) const { return lo; }
    __device__ __forceinline__ float* prob(const PsfmDecLayer&) const { return pr; }
    __device__ __forceinline__ uint8_t* pred(const PsfmDecLayer&) const { return pd; }
};

// One convolution over the points (psfm_decoder.h: PsfmDecLayer), block `blk` of the k points.  A block owns PSFM_DEC_TILE points and
// all output channels: wave w holds rows 32 w .. 32 w + 31 of both 32-point tiles in 2 x 16 accumulator registers.
template <class R>
__device__ __forceinline__ void pd_layer(const PsfmDecLayer& Y, const R& at, int k, int blk)
{
    __shared__ float ldsX[PSFM_DEC_TILE * PSFM_DEC_LDX];
    __shared__ float ldsW[PSFM_DEC_C * PSFM_DEC_LDW];
    __shared__ float fm[PSFM_DEC_C], fs[PSFM_DEC_C], ft[PSFM_DEC_C];
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 31;
    const int p0 = blk * PSFM_DEC_TILE, np = min(PSFM_DEC_TILE, k - p0);
    f32x16 acc[2];
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int row = wave * 32 + pd_row(r, lane);
        acc[0][r] = acc[1][r] = row < Y.cout ? Y.bias[row] : 0.0f;
    }
    for (int si = 0; si < Y.nseg; si++) {
        const PsfmDecSeg& S = Y.seg[si];
        const float* src = at(S.src);
        const double* stat = at(S.stat);
        __syncthreads();                                    // the products of the segment before have read ldsX
        if (stat)
            for (int c = tid; c < S.cin; c += PSFM_DEC_THREADS) psfm_dec_fold(stat[c], stat[PSFM_DEC_C + c], S.bn, S.bn_n, S.bn_c0 + c, fm[c], fs[c], ft[c]);
        __syncthreads();
        for (int idx = tid; idx < S.cin * PSFM_DEC_TILE; idx += PSFM_DEC_THREADS) {
            const int c = idx >> 6, p = idx & 63;
            float v = 0.0f;
            if (p < np) {
                v = src[c * k + p0 + p];
                if (stat) v = psfm_dec_norm_relu(v, fm[c], fs[c], ft[c]);
            }
            ldsX[p * PSFM_DEC_LDX + c] = v;
        }
        pd_gemm<2, false>(acc, S.w, S.ldw, S.cin, Y.cout, ldsW, ldsX, PSFM_DEC_LDX, tid);
    }
    __syncthreads();                                        // every wave is done with ldsX as an operand

    if (Y.mode == PSFM_DEC_UNPOOL) {
        // the embedding as the image [point][cluster], its softmax over the clusters, then x2 [128][100] against it
#pragma unroll
        for (int t = 0; t < 2; t++)
#pragma unroll
            for (int r = 0; r < 16; r++) ldsX[(t * 32 + col) * PSFM_DEC_LDX + wave * 32 + pd_row(r, lane)] = acc[t][r];
        __syncthreads();
        if (tid < PSFM_DEC_TILE) psfm_dec_softmax_clusters(ldsX + tid * PSFM_DEC_LDX);
#pragma unroll
        for (int r = 0; r < 16; r++) acc[0][r] = acc[1][r] = 0.0f;
        pd_gemm<2, false>(acc, at(Y.x2), PSFM_DEC_CL, PSFM_DEC_CL, PSFM_DEC_C, ldsW, ldsX, PSFM_DEC_LDX, tid);
        __syncthreads();
    }

    // the block's output tile: to memory, and as the image [point][channel] for what is reduced over it
    const float* residual = at(Y.residual);
    float* out = at(Y.out);
#pragma unroll
    for (int t = 0; t < 2; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int row = wave * 32 + pd_row(r, lane), pc = t * 32 + col;
            float v = acc[t][r];
            if (Y.mode != PSFM_DEC_UNPOOL && Y.bias2 && row < Y.cout) v += Y.bias2[row];
            const bool live = pc < np && (Y.mode == PSFM_DEC_UNPOOL || row < Y.cout);
            if (live && residual) v += residual[row * k + p0 + pc];
            if (live && Y.mode != PSFM_DEC_FINAL) out[row * k + p0 + pc] = v;
            ldsX[pc * PSFM_DEC_LDX + row] = v;
        }
    __syncthreads();

    if (Y.mode == PSFM_DEC_FINAL) {
        if (tid < np) {
            float logit, prob;
            uint8_t pred;
            psfm_dec_verdict(ldsX + tid * PSFM_DEC_LDX, Y.wout, logit, prob, pred);
            if (at.logits(Y)) at.logits(Y)[p0 + tid] = logit;
            if (at.prob(Y)) at.prob(Y)[p0 + tid] = prob;
            if (at.pred(Y)) at.pred(Y)[p0 + tid] = pred;
        }
        return;
    }
    // two threads per channel, 32 points each, combined in the same order in both
    const int c = tid >> 1, half = tid & 1, first = half * 32, n = max(0, min(32, np - first));
    const float* x = ldsX + first * PSFM_DEC_LDX + c;
    if (Y.mode == PSFM_DEC_EMBED_DOWN) {
        float m = psfm_dec_max(x, PSFM_DEC_LDX, n);
        m = fmaxf(m, __shfl_xor(m, 1));
        double s;
        psfm_dec_softmax_part(x, PSFM_DEC_LDX, n, m, s);
        const double o = __shfl_xor(s, 1);
        s = half ? o + s : s + o;
        if (!half && c < PSFM_DEC_CL) {
            double* dst = at(Y.part) + ((size_t)blk * PSFM_DEC_CL + c) * 2;
            dst[0] = (double)m;
            dst[1] = s;
        }
    } else {
        double s = 0.0, q = 0.0;
        for (int i = 0; i < n; i++) {
            const double v = (double)x[i * PSFM_DEC_LDX];
            s += v;
            q += v * v;
        }
        const double so = __shfl_xor(s, 1), qo = __shfl_xor(q, 1);
        s = half ? so + s : s + so;
        q = half ? qo + q : q + qo;
        if (!half) {
            double* dst = at(Y.part) + ((size_t)blk * PSFM_DEC_C + c) * 2;
            dst[0] = s;
            dst[1] = q;
        }
    }
}

// The blocks' partial sums of channel blockIdx.x in the fixed order of psfm_decoder.h -> fin[c] = mean, fin[128 + c] = inv.
__device__ __forceinline__ void pd_stats(const double* __restrict__ part, int nb, int k, double* __restrict__ fin)
{
    __shared__ double a[PSFM_DEC_THREADS], b[PSFM_DEC_THREADS];
    const int tid = (int)threadIdx.x, c = (int)blockIdx.x;
    double s = 0.0, q = 0.0;
    for (int i = tid; i < nb; i += PSFM_DEC_THREADS) {
        s += part[((size_t)i * PSFM_DEC_C + c) * 2];
        q += part[((size_t)i * PSFM_DEC_C + c) * 2 + 1];
    }
    a[tid] = s;
    b[tid] = q;
    for (int st = PSFM_DEC_THREADS / 2; st > 0; st >>= 1) {
        __syncthreads();
        psfm_dec_tree_add(a, tid, st);
        psfm_dec_tree_add(b, tid, st);
    }
    if (tid == 0) psfm_dec_stat_finish(a[0], b[0], (double)k, fin[c], fin[PSFM_DEC_C + c]);
}

// down1: the blocks' (max, sum of exponentials) of cluster blockIdx.x -> sm_fin[2 j] = M, [2 j + 1] = 1 / sum.
__device__ __forceinline__ void pd_softmax(const double* __restrict__ part, int nb, float* __restrict__ sm_fin)
{
    __shared__ double a[PSFM_DEC_THREADS];
    const int tid = (int)threadIdx.x, j = (int)blockIdx.x;
    double m = -INFINITY;
    for (int i = tid; i < nb; i += PSFM_DEC_THREADS) m = fmax(m, part[((size_t)i * PSFM_DEC_CL + j) * 2]);
    a[tid] = m;
    for (int st = PSFM_DEC_THREADS / 2; st > 0; st >>= 1) {
        __syncthreads();
        psfm_dec_tree_max(a, tid, st);
    }
    __syncthreads();
    const double M = a[0];
    __syncthreads();
    double s = 0.0;
    for (int i = tid; i < nb; i += PSFM_DEC_THREADS) {
        const double* p = part + ((size_t)i * PSFM_DEC_CL + j) * 2;
        s += p[1] * exp(p[0] - M);
    }
    a[tid] = s;
    for (int st = PSFM_DEC_THREADS / 2; st > 0; st >>= 1) {
        __syncthreads();
        psfm_dec_tree_add(a, tid, st);
    }
    if (tid == 0) {
        sm_fin[2 * j] = (float)M;
        sm_fin[2 * j + 1] = (float)(1.0 / a[0]);
    }
}

// down1: x1_1 S^T over the PSFM_DEC_SLICE points of slice `blk` as a partial [128][100]; wave w holds channels 32 w .. against all
// clusters.
__device__ __forceinline__ void pd_pool(const float* __restrict__ x1, const float* __restrict__ emb, const float* __restrict__ sm_fin, int k,
                                        float* __restrict__ part, int blk)
{
    __shared__ float ldsA[PSFM_DEC_C * PSFM_DEC_LDW], ldsB[PSFM_DEC_C * PSFM_DEC_LDW];
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int base = blk * PSFM_DEC_SLICE;
    f32x16 acc[4];
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[t][r] = 0.0f;
    for (int q0 = 0; q0 < PSFM_DEC_SLICE && base + q0 < k; q0 += PSFM_DEC_KC) {
        __syncthreads();
        for (int idx = tid; idx < PSFM_DEC_C * PSFM_DEC_KC; idx += PSFM_DEC_THREADS) {
            const int c = idx >> 5, p = base + q0 + (idx & 31);
            const bool in = p < k;
            ldsA[c * PSFM_DEC_LDW + (idx & 31)] = in ? x1[c * k + p] : 0.0f;
            ldsB[c * PSFM_DEC_LDW + (idx & 31)] = in && c < PSFM_DEC_CL ? psfm_dec_pool_weight(emb[c * k + p], sm_fin[2 * c], sm_fin[2 * c + 1]) : 0.0f;
        }
        __syncthreads();
        pd_mma<4>(acc, ldsA + wave * 32 * PSFM_DEC_LDW, PSFM_DEC_LDW, ldsB, PSFM_DEC_LDW, PSFM_DEC_KC, lane);
    }
    float* dst = part + (size_t)blk * PSFM_DEC_C * PSFM_DEC_CL;
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int j = t * 32 + (lane & 31);
            if (j < PSFM_DEC_CL) dst[(wave * 32 + pd_row(r, lane)) * PSFM_DEC_CL + j] = acc[t][r];
        }
}

// l2: the pool partials added in block order, then the four OAFilters on the [128][100] tensor, in one block.  A lane keeps its 64
// elements (channel = its wave's rows, cluster = its column of each of the four tiles) in registers from filter to filter; the
// images that the products and the statistics read are built in LDS.
#define PD_L2_LDS ((PSFM_DEC_C * PSFM_DEC_LDX + PSFM_DEC_C * PSFM_DEC_LDW + 3 * PSFM_DEC_C) * sizeof(float))

__device__ __forceinline__ void pd_l2_norm(const f32x16 (&v)[4], const float* bn, float* img, float* fm, float* fs, float* ft, int tid)
{
    // v -> img as [cluster][channel], normalised over the 100 clusters per channel (InstanceNorm), BatchNorm bn, ReLU
    const int wave = tid >> 6, lane = tid & 63, col = lane & 31;
    __syncthreads();                                        // img is free
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) img[(wave * 32 + pd_row(r, lane)) * PSFM_DEC_LDX + t * 32 + col] = v[t][r];
    __syncthreads();
    const int c = tid >> 1, half = tid & 1;
    double s = 0.0, q = 0.0;
    for (int i = 0; i < PSFM_DEC_CL / 2; i++) {
        const double x = (double)img[c * PSFM_DEC_LDX + half * (PSFM_DEC_CL / 2) + i];
        s += x;
        q += x * x;
    }
    const double so = __shfl_xor(s, 1), qo = __shfl_xor(q, 1);
    s = half ? so + s : s + so;
    q = half ? qo + q : q + qo;
    if (!half) {
        double mean, inv;
        psfm_dec_stat_finish(s, q, (double)PSFM_DEC_CL, mean, inv);
        psfm_dec_fold(mean, inv, bn, PSFM_DEC_C, c, fm[c], fs[c], ft[c]);
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int row = wave * 32 + pd_row(r, lane), j = t * 32 + col;
            img[j * PSFM_DEC_LDX + row] = j < PSFM_DEC_CL ? psfm_dec_norm_relu(v[t][r], fm[row], fs[row], ft[row]) : 0.0f;
        }
}

__device__ __forceinline__ void pd_l2(const float* __restrict__ part, int nb2, const float* __restrict__ w, float* __restrict__ x2)
{
    extern __shared__ float smem[];
    float* img = smem;
    float* ldsW = img + PSFM_DEC_C * PSFM_DEC_LDX;
    float* fm = ldsW + PSFM_DEC_C * PSFM_DEC_LDW;
    float* fs = fm + PSFM_DEC_C;
    float* ft = fs + PSFM_DEC_C;
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 31;
    f32x16 x[4], a[4], b[4];
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int row = wave * 32 + pd_row(r, lane), j = t * 32 + col;
            float s = 0.0f;
            if (j < PSFM_DEC_CL)
                for (int i = 0; i < nb2; i++) s += part[((size_t)i * PSFM_DEC_C + row) * PSFM_DEC_CL + j];
            x[t][r] = s;
        }
    for (int f = 0; f < 4; f++) {
        const float* p = w + f * PSFM_DEC_OA_SIZE;
        // conv1: a = W1 relu(bn1(in(x))) + b1
        pd_l2_norm(x, p, img, fm, fs, ft, tid);
#pragma unroll
        for (int t = 0; t < 4; t++)
#pragma unroll
            for (int r = 0; r < 16; r++) a[t][r] = p[PSFM_DEC_OA_B1 + wave * 32 + pd_row(r, lane)];
        pd_gemm<4, false>(a, p + PSFM_DEC_OA_W1, PSFM_DEC_C, PSFM_DEC_C, PSFM_DEC_C, ldsW, img, PSFM_DEC_LDX, tid);
        // conv2 across the clusters: a += W2 relu(bn2(a)) + b2, the image is [channel][cluster] and gives the rows
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int j = t * 32 + col;
            float s2 = 0.0f, t2 = 0.0f;
            if (j < PSFM_DEC_CL) psfm_dec_fold_bn(p + PSFM_DEC_OA_BN2, PSFM_DEC_CL, j, s2, t2);
#pragma unroll
            for (int r = 0; r < 16; r++) {
                img[(wave * 32 + pd_row(r, lane)) * PSFM_DEC_LDX + j] = j < PSFM_DEC_CL ? psfm_dec_norm_relu(a[t][r], 0.0f, s2, t2) : 0.0f;
                b[t][r] = j < PSFM_DEC_CL ? p[PSFM_DEC_OA_B2 + j] : 0.0f;
            }
        }
        pd_gemm<4, true>(b, p + PSFM_DEC_OA_W2, PSFM_DEC_CL, PSFM_DEC_CL, PSFM_DEC_CL, ldsW, img, PSFM_DEC_LDX, tid);
#pragma unroll
        for (int t = 0; t < 4; t++)
#pragma unroll
            for (int r = 0; r < 16; r++) a[t][r] += b[t][r];
        // conv3: x = W3 relu(bn3(in(a))) + b3 + x
        pd_l2_norm(a, p + PSFM_DEC_OA_BN3, img, fm, fs, ft, tid);
#pragma unroll
        for (int t = 0; t < 4; t++)
#pragma unroll
            for (int r = 0; r < 16; r++) b[t][r] = p[PSFM_DEC_OA_B3 + wave * 32 + pd_row(r, lane)];
        pd_gemm<4, false>(b, p + PSFM_DEC_OA_W3, PSFM_DEC_C, PSFM_DEC_C, PSFM_DEC_C, ldsW, img, PSFM_DEC_LDX, tid);
#pragma unroll
        for (int t = 0; t < 4; t++)
#pragma unroll
            for (int r = 0; r < 16; r++) x[t][r] = t * 32 + col < PSFM_DEC_CL ? b[t][r] + x[t][r] : 0.0f;
    }
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int j = t * 32 + col;
            if (j < PSFM_DEC_CL) x2[(wave * 32 + pd_row(r, lane)) * PSFM_DEC_CL + j] = x[t][r];
        }
}

// ---- the kernels: one window (psfm_traj_decode) ------------------------------------------------------------------------------
__global__ __launch_bounds__(PSFM_DEC_THREADS) void psfm_dec_layer_kernel(const PsfmDecLayer Y, int k) { pd_layer(Y, PdOne(), k, (int)blockIdx.x); }

__global__ __launch_bounds__(PSFM_DEC_THREADS) void psfm_dec_stats_kernel(const double* __restrict__ part, int nb, int k, double* __restrict__ fin)
{
    pd_stats(part, nb, k, fin);
}

__global__ __launch_bounds__(PSFM_DEC_THREADS) void psfm_dec_softmax_kernel(const double* __restrict__ part, int nb, float* __restrict__ sm_fin)
{
    pd_softmax(part, nb, sm_fin);
}

__global__ __launch_bounds__(PSFM_DEC_THREADS) void psfm_dec_pool_kernel(const float* __restrict__ x1, const float* __restrict__ emb,
                                                                       const float* __restrict__ sm_fin, int k, float* __restrict__ part)
{
    pd_pool(x1, emb, sm_fin, k, part, (int)blockIdx.x);
}

__global__ __launch_bounds__(PSFM_DEC_THREADS) void psfm_dec_l2_kernel(const float* __restrict__ part, int nb2, const float* __restrict__ w,
                                                                     float* __restrict__ x2)
{
    pd_l2(part, nb2, w, x2);
}

// ---- the kernels: a batch of windows (psfm_traj_decode_batch, psfm_decoder_batch.h) -------------------------------------------
// The same bodies; a block first finds its window in the table B and then works on that window's k, sections and partial-sum rows.
// Y and fin hold section names.
__global__ __launch_bounds__(PSFM_DEC_THREADS) void psfm_dec_layer_batch_kernel(const PsfmDecLayer Y, const PsfmDecBatch B)
{
    const int b = psfm_dec_batch_find(B.tile0, (int)blockIdx.x);
    const PdWin at = {psfm_dec_batch_window(B, b), B.logits[b], B.prob[b], B.pred[b]};
    pd_layer(Y, at, at.W.k, (int)blockIdx.x - B.tile0[b]);
}

__global__ __launch_bounds__(PSFM_DEC_THREADS) void psfm_dec_stats_batch_kernel(const PsfmDecBatch B, double* fin)
{
    const int b = (int)blockIdx.y;
    if (B.k[b] == 0) return;
    const PsfmDecWin W = psfm_dec_batch_window(B, b);
    pd_stats((const double*)(W.base + W.L.stat_part), W.L.nb, W.k, psfm_dec_resolve(fin, W));
}

__global__ __launch_bounds__(PSFM_DEC_THREADS) void psfm_dec_softmax_batch_kernel(const PsfmDecBatch B)
{
    const int b = (int)blockIdx.y;
    if (B.k[b] == 0) return;
    const PsfmDecWin W = psfm_dec_batch_window(B, b);
    pd_softmax((const double*)(W.base + W.L.sm_part), W.L.nb, (float*)(W.base + W.L.sm_fin));
}

__global__ __launch_bounds__(PSFM_DEC_THREADS) void psfm_dec_pool_batch_kernel(const PsfmDecBatch B)
{
    const int b = psfm_dec_batch_find(B.slice0, (int)blockIdx.x);
    const PsfmDecWin W = psfm_dec_batch_window(B, b);
    pd_pool((const float*)(W.base + W.L.x1), (const float*)(W.base + W.L.emb), (const float*)(W.base + W.L.sm_fin), W.k,
            (float*)(W.base + W.L.pool_part), (int)blockIdx.x - B.slice0[b]);
}

__global__ __launch_bounds__(PSFM_DEC_THREADS) void psfm_dec_l2_batch_kernel(const PsfmDecBatch B, const float* __restrict__ w)
{
    const int b = (int)blockIdx.x;
    if (B.k[b] == 0) return;
    const PsfmDecWin W = psfm_dec_batch_window(B, b);
    pd_l2((const float*)(W.base + W.L.pool_part), W.L.nb2, w, (float*)(W.base + W.L.x2));
}

extern "C" int psfm_traj_decode_weight_count(void) { return PSFM_DEC_WEIGHTS; }

extern "C" size_t psfm_traj_decode_workspace_bytes(int64_t k) { return k > 0 && k <= PSFM_DEC_MAX_K ? psfm_dec_workspace(k).total : 0; }

extern "C" psfm_status psfm_traj_decode(psfm_ctx* c, const float* encoding, const float* weights, int64_t k, void* workspace,
                                        size_t workspace_bytes, float* logits, float* prob, uint8_t* pred, void* stream)
{
    if (!c) { psfm_set_error("ctx is NULL"); return PSFM_ERR_ARG; }
    if (k < 0 || k > PSFM_DEC_MAX_K) {
        psfm_set_error("psfm_traj_decode: bad argument (k=%lld, supported is 0 or 2 <= k <= %lld)", (long long)k, (long long)PSFM_DEC_MAX_K);
        return PSFM_ERR_ARG;
    }
    if (k == 0) return PSFM_OK;
    if (k == 1) {
        psfm_set_error("psfm_traj_decode: k=1: InstanceNorm2d needs more than one point (the reference raises here)");
        return PSFM_ERR_ARG;
    }
    if (!encoding || !weights || !workspace) { psfm_set_error("psfm_traj_decode: NULL argument"); return PSFM_ERR_ARG; }
    const size_t need = psfm_dec_workspace(k).total;
    if (workspace_bytes < need) {
        psfm_set_error("psfm_traj_decode: workspace_bytes=%zu, k=%lld needs %zu (psfm_traj_decode_workspace_bytes)", workspace_bytes, (long long)k, need);
        return PSFM_ERR_ARG;
    }
    PSFM_HIP(hipSetDevice(c->device));
    PSFM_HIP(hipFuncSetAttribute((const void*)psfm_dec_l2_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PD_L2_LDS));
    PsfmGate gate(c->device, 0);
    static thread_local PsfmDecPlan P;
    psfm_dec_plan(P, encoding, weights, k, workspace, logits, prob, pred);
    hipStream_t s = (hipStream_t)stream;
    for (int i = 0; i < P.nsteps; i++) {
        const PsfmDecStep& S = P.step[i];
        switch (S.kind) {
        case PSFM_DEC_STEP_LAYER:
            hipLaunchKernelGGL(psfm_dec_layer_kernel, dim3((unsigned)P.nb), dim3(PSFM_DEC_THREADS), 0, s, S.layer, (int)k);
            break;
        case PSFM_DEC_STEP_STATS:
            hipLaunchKernelGGL(psfm_dec_stats_kernel, dim3(PSFM_DEC_C), dim3(PSFM_DEC_THREADS), 0, s, (const double*)P.stat_part, P.nb, (int)k, S.fin);
            break;
        case PSFM_DEC_STEP_SOFTMAX:
            hipLaunchKernelGGL(psfm_dec_softmax_kernel, dim3(PSFM_DEC_CL), dim3(PSFM_DEC_THREADS), 0, s, (const double*)P.sm_part, P.nb, P.sm_fin);
            break;
        case PSFM_DEC_STEP_POOL:
            hipLaunchKernelGGL(psfm_dec_pool_kernel, dim3((unsigned)P.nb2), dim3(PSFM_DEC_THREADS), 0, s, (const float*)P.x1, (const float*)P.emb,
                               (const float*)P.sm_fin, (int)k, P.pool_part);
            break;
        case PSFM_DEC_STEP_L2:
            hipLaunchKernelGGL(psfm_dec_l2_kernel, dim3(1), dim3(PSFM_DEC_THREADS), PD_L2_LDS, s, (const float*)P.pool_part, P.nb2,
                               weights + PSFM_DEC_W_L2, P.x2);
            break;
        }
    }
    PSFM_HIP(hipGetLastError());
    return PSFM_OK;
}

extern "C" size_t psfm_traj_decode_batch_workspace_bytes(const int64_t* k, int n_win)
{
    static thread_local PsfmDecBatch B;
    size_t total;
    int bad;
    if (n_win < 0 || n_win > PSFM_DEC_BATCH_MAX || (n_win > 0 && !k)) return 0;
    return psfm_dec_batch_layout(B, k, n_win, total, bad) == PSFM_DEC_BATCH_OK ? total : 0;
}

extern "C" psfm_status psfm_traj_decode_batch(psfm_ctx* c, int n_win, const float* const* encoding, const int64_t* k, const float* weights,
                                              void* workspace, size_t workspace_bytes, float* const* logits, float* const* prob,
                                              uint8_t* const* pred, void* stream)
{
    if (!c) { psfm_set_error("ctx is NULL"); return PSFM_ERR_ARG; }
    if (n_win < 0 || n_win > PSFM_DEC_BATCH_MAX) {
        psfm_set_error("psfm_traj_decode_batch: bad argument (n_win=%d, supported is 0 <= n_win <= %d)", n_win, PSFM_DEC_BATCH_MAX);
        return PSFM_ERR_ARG;
    }
    if (n_win == 0) return PSFM_OK;
    if (!k) { psfm_set_error("psfm_traj_decode_batch: k is NULL"); return PSFM_ERR_ARG; }
    static thread_local PsfmDecBatch B;
    size_t need;
    int bad;
    if (psfm_dec_batch_layout(B, k, n_win, need, bad) != PSFM_DEC_BATCH_OK) {
        if (k[bad] == 1)
            psfm_set_error("psfm_traj_decode_batch: window %d: k=1: InstanceNorm2d needs more than one point (the reference raises here)", bad);
        else
            psfm_set_error("psfm_traj_decode_batch: window %d: bad argument (k=%lld, supported is 0 or 2 <= k <= %lld)", bad, (long long)k[bad],
                           (long long)PSFM_DEC_MAX_K);
        return PSFM_ERR_ARG;
    }
    if (B.tiles == 0) return PSFM_OK;                       // every window is empty
    if (!encoding || !weights || !workspace) { psfm_set_error("psfm_traj_decode_batch: NULL argument"); return PSFM_ERR_ARG; }
    for (int b = 0; b < n_win; b++)
        if (k[b] > 0 && !encoding[b]) { psfm_set_error("psfm_traj_decode_batch: window %d: encoding is NULL (k=%lld)", b, (long long)k[b]); return PSFM_ERR_ARG; }
    if (workspace_bytes < need) {
        psfm_set_error("psfm_traj_decode_batch: workspace_bytes=%zu, these %d windows need %zu (psfm_traj_decode_batch_workspace_bytes)",
                       workspace_bytes, n_win, need);
        return PSFM_ERR_ARG;
    }
    for (int b = 0; b < n_win; b++) {
        B.enc[b] = encoding[b];
        B.logits[b] = logits ? logits[b] : 0;
        B.prob[b] = prob ? prob[b] : 0;
        B.pred[b] = pred ? pred[b] : 0;
    }
    B.ws = (char*)workspace;
    PSFM_HIP(hipSetDevice(c->device));
    PSFM_HIP(hipFuncSetAttribute((const void*)psfm_dec_l2_batch_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PD_L2_LDS));
    PsfmGate gate(c->device, 0);
    static thread_local PsfmDecPlan P;
    psfm_dec_plan_names(P, weights);
    hipStream_t s = (hipStream_t)stream;
    const dim3 threads(PSFM_DEC_THREADS);
    for (int i = 0; i < P.nsteps; i++) {
        const PsfmDecStep& S = P.step[i];
        switch (S.kind) {
        case PSFM_DEC_STEP_LAYER:
            hipLaunchKernelGGL(psfm_dec_layer_batch_kernel, dim3((unsigned)B.tiles), threads, 0, s, S.layer, B);
            break;
        case PSFM_DEC_STEP_STATS:
            hipLaunchKernelGGL(psfm_dec_stats_batch_kernel, dim3(PSFM_DEC_C, (unsigned)n_win), threads, 0, s, B, S.fin);
            break;
        case PSFM_DEC_STEP_SOFTMAX:
            hipLaunchKernelGGL(psfm_dec_softmax_batch_kernel, dim3(PSFM_DEC_CL, (unsigned)n_win), threads, 0, s, B);
            break;
        case PSFM_DEC_STEP_POOL:
            hipLaunchKernelGGL(psfm_dec_pool_batch_kernel, dim3((unsigned)B.slices), threads, 0, s, B);
            break;
        case PSFM_DEC_STEP_L2:
            hipLaunchKernelGGL(psfm_dec_l2_batch_kernel, dim3((unsigned)n_win), threads, PD_L2_LDS, s, B, weights + PSFM_DEC_W_L2);
            break;
        }
    }
    PSFM_HIP(hipGetLastError());
    return PSFM_OK;
}
