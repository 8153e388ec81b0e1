// psfm_encoder.h -- the per-token arithmetic of the motion classifier's trajectory transformer, shared by the kernel
// (psfm_encoder.hip) and the host build of the CPU suite (tests/host/encoder_host.cpp through tests/host/shim).
//
// Reference: pt_transformer.forward in eval mode (motion_seg/core/network/traj_oa_depth.py:25-60): project (two 1x1 convolutions
// 10 -> 16 -> 16 with ReLU), nn.Transformer(d_model 16, 4 heads, 2 encoder + 2 decoder layers, feed-forward 64, post-norm, ReLU)
// over each trajectory's L tokens with the SAME tensor as src and tgt, then the max over the tokens.  What the reference's call
// (:48) means, and this keeps:
//   - keys at padded positions get -inf in every SELF-attention (src_key_padding_mask, tgt_key_padding_mask); queries at padded
//     positions are computed like any other;
//   - memory_key_padding_mask is None: CROSS-attention attends to all L memory positions, padded ones included;
//   - the final max (:51) runs over all L tokens, padded ones included; no position is ever zeroed (batch_first=False takes no
//     nested-tensor path).
// A trajectory is independent of every other.  One TOKEN is the unit of work here: its 16-vector stays with its owner (a lane in
// the kernel), and tokens of a trajectory meet only in the seven exchanges of a 32-float row each -- K and V of the attention that
// follows, at last the decoder's output for the max.  Between two exchanges a token runs one psfm_enc_phase.
// fp32 throughout; every dot product is an explicit fmaf chain in ascending index order starting from the bias (the translation
// units are built with -ffp-contract=off), so the host build and the kernel evaluate the same operations; they differ in expf only.
// The softmax is normalised after the weighted sum (4 divisions per token and attention, not 4 L).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#define PSFM_ENC_IN 10          // input channels (psfm_traj_augment's planes)
#define PSFM_ENC_D 16           // d_model
#define PSFM_ENC_FF 64          // dim_feedforward
#define PSFM_ENC_MAX_L 64       // one trajectory inside one wave
#define PSFM_ENC_PHASES 7
#define PSFM_ENC_ROW 33         // floats per exchanged row: K[16], V[16] + 1, so that the rows of consecutive lanes start on different banks

// Packed weights (include/psfm.h documents the order: the module's state_dict order, every tensor row-major [out][in]).
#define PSFM_ENC_W_FC1 0        // input_fc1.weight [16][10], .bias [16]
#define PSFM_ENC_W_FC2 176      // fc2.weight [16][16], .bias [16]
#define PSFM_ENC_W_ENC 448      // encoder.layers.{0,1}
#define PSFM_ENC_W_ENC_NORM 7008
#define PSFM_ENC_W_DEC 7040     // decoder.layers.{0,1}
#define PSFM_ENC_W_DEC_NORM 15840
#define PSFM_ENC_WEIGHTS 15872
// an attention block: in_proj_weight [48][16] (q, k, v), in_proj_bias [48], out_proj.weight [16][16], out_proj.bias [16]
#define PSFM_ENC_AT_INB 768
#define PSFM_ENC_AT_OUTW 816
#define PSFM_ENC_AT_OUTB 1072
#define PSFM_ENC_AT_SIZE 1088
// a feed-forward block: linear1.weight [64][16], .bias [64], linear2.weight [16][64], .bias [16]
#define PSFM_ENC_FF_B1 1024
#define PSFM_ENC_FF_W2 1088
#define PSFM_ENC_FF_B2 2112
#define PSFM_ENC_FF_SIZE 2128
// an encoder layer: self_attn, feed-forward, norm1, norm2 (weight [16], bias [16] each)
#define PSFM_ENC_EL_FF 1088
#define PSFM_ENC_EL_N1 3216
#define PSFM_ENC_EL_N2 3248
#define PSFM_ENC_EL_SIZE 3280
// a decoder layer: self_attn, multihead_attn, feed-forward, norm1, norm2, norm3
#define PSFM_ENC_DL_CA 1088
#define PSFM_ENC_DL_FF 2176
#define PSFM_ENC_DL_N1 4304
#define PSFM_ENC_DL_N2 4336
#define PSFM_ENC_DL_N3 4368
#define PSFM_ENC_DL_SIZE 4400

// what a token carries from phase to phase: x = project(f), cur = the running h / d, mem = the encoder's output, q = its query of
// the attention under way, pub = the row it hands to the exchange
struct PsfmEncTok { float x[PSFM_ENC_D], cur[PSFM_ENC_D], mem[PSFM_ENC_D], q[PSFM_ENC_D], pub[2 * PSFM_ENC_D]; };

// out = W in + b, W [OUT][IN] row-major: out[o] = fma(W[o][IN-1], in[IN-1], ... fma(W[o][0], in[0], b[o]))
template <int OUT, int IN>
__device__ __forceinline__ void psfm_enc_linear(const float* __restrict__ W, const float* __restrict__ b, const float (&in)[IN], float (&out)[OUT])
{
#pragma unroll
    for (int o = 0; o < OUT; o++) {
        float a = b[o];
#pragma unroll
        for (int i = 0; i < IN; i++) a = __fmaf_rn(W[o * IN + i], in[i], a);
        out[o] = a;
    }
}

// LayerNorm over the 16 features: biased variance, eps 1e-5, the parameters' own gain and bias (g[16], then b[16]); sums as a
// fixed binary tree
__device__ __forceinline__ void psfm_enc_ln(float (&v)[PSFM_ENC_D], const float* __restrict__ gb)
{
    float t[PSFM_ENC_D];
#pragma unroll
    for (int i = 0; i < 16; i++) t[i] = v[i];
#pragma unroll
    for (int n = 8; n >= 1; n >>= 1)
#pragma unroll
        for (int i = 0; i < n; i++) t[i] = t[i] + t[i + n];
    const float mu = t[0] * 0.0625f;
    float d[PSFM_ENC_D];
#pragma unroll
    for (int i = 0; i < 16; i++) { d[i] = v[i] - mu; t[i] = d[i] * d[i]; }
#pragma unroll
    for (int n = 8; n >= 1; n >>= 1)
#pragma unroll
        for (int i = 0; i < n; i++) t[i] = t[i] + t[i + n];
    const float r = 1.0f / sqrtf(t[0] * 0.0625f + 1e-5f);
#pragma unroll
    for (int i = 0; i < 16; i++) v[i] = __fmaf_rn(d[i] * r, gb[i], gb[16 + i]);
}

// one head's score of key row r: q is already scaled by 1/sqrt(4)
__device__ __forceinline__ float psfm_enc_score(const float (&q)[PSFM_ENC_D], const float* r, int h)
{
    float s = q[4 * h] * r[4 * h];
#pragma unroll
    for (int c = 1; c < 4; c++) s = __fmaf_rn(q[4 * h + c], r[4 * h + c], s);
    return s;
}

// 4 heads of width 4 over the L rows (K in [0,16), V in [16,32)) of the token's trajectory; bit j of `pad` = key j is masked.
// Two passes over the rows (the maximum, then the sums), scores recomputed: no per-key state.  Every key masked (a trajectory
// without a valid token, which load_cut_seq never produces): NaN, in this trajectory only.
__device__ __forceinline__ void psfm_enc_attend(const float (&q)[PSFM_ENC_D], const float* rows, int L, uint64_t pad,
                                                float (&o)[PSFM_ENC_D])
{
    float m[4], sum[4];
#pragma unroll
    for (int h = 0; h < 4; h++) { m[h] = -INFINITY; sum[h] = 0.0f; }
#pragma unroll 1
    for (int j = 0; j < L; j++) {
        const float* r = rows + j * PSFM_ENC_ROW;
        const bool masked = (pad >> j) & 1;
#pragma unroll
        for (int h = 0; h < 4; h++) {
            const float s = psfm_enc_score(q, r, h);
            m[h] = masked ? m[h] : fmaxf(m[h], s);
        }
    }
#pragma unroll
    for (int i = 0; i < 16; i++) o[i] = 0.0f;
#pragma unroll 1
    for (int j = 0; j < L; j++) {
        const float* r = rows + j * PSFM_ENC_ROW;
        const bool masked = (pad >> j) & 1;
#pragma unroll
        for (int h = 0; h < 4; h++) {
            const float e = masked ? 0.0f : expf(psfm_enc_score(q, r, h) - m[h]);
            sum[h] = sum[h] + e;
#pragma unroll
            for (int c = 0; c < 4; c++) o[4 * h + c] = __fmaf_rn(e, r[16 + 4 * h + c], o[4 * h + c]);
        }
    }
#pragma unroll
    for (int h = 0; h < 4; h++) {
        const float inv = 1.0f / sum[h];
#pragma unroll
        for (int c = 0; c < 4; c++) o[4 * h + c] = o[4 * h + c] * inv;
    }
}

// the in-projection of the attention block at w: q from q_src (scaled by 1/sqrt(head width) = 0.5, exact), the row K | V from kv_src
__device__ __forceinline__ void psfm_enc_qkv(const float* __restrict__ w, const float (&q_src)[PSFM_ENC_D], const float (&kv_src)[PSFM_ENC_D],
                                             float (&q)[PSFM_ENC_D], float (&row)[2 * PSFM_ENC_D])
{
    psfm_enc_linear<16, 16>(w, w + PSFM_ENC_AT_INB, q_src, q);
#pragma unroll
    for (int i = 0; i < 16; i++) q[i] = q[i] * 0.5f;
    psfm_enc_linear<32, 16>(w + 256, w + PSFM_ENC_AT_INB + 16, kv_src, row);
}

// W_b relu(W_a h + b_a) + b_b of the feed-forward block at w, 8 hidden units at a time: out[o] still accumulates over the hidden
// units in ascending order
__device__ __forceinline__ void psfm_enc_ffn(const float* __restrict__ w, const float (&h)[PSFM_ENC_D], float (&out)[PSFM_ENC_D])
{
#pragma unroll
    for (int o = 0; o < 16; o++) out[o] = w[PSFM_ENC_FF_B2 + o];
#pragma unroll 1
    for (int j0 = 0; j0 < PSFM_ENC_FF; j0 += 8) {
        float t[8];
        psfm_enc_linear<8, 16>(w + j0 * 16, w + PSFM_ENC_FF_B1 + j0, h, t);
#pragma unroll
        for (int j = 0; j < 8; j++) t[j] = fmaxf(t[j], 0.0f);
#pragma unroll
        for (int o = 0; o < 16; o++)
#pragma unroll
            for (int j = 0; j < 8; j++) out[o] = __fmaf_rn(w[PSFM_ENC_FF_W2 + o * PSFM_ENC_FF + j0 + j], t[j], out[o]);
    }
}

// where phase p finds its weights: the attention it finishes (fin, its LayerNorm fin_ln), the feed-forward block behind it (ffn,
// ffn_ln; -1: none) and the attention it starts (start; -1: none)
struct PsfmEncPlan { int fin, fin_ln, ffn, ffn_ln, start; };

__device__ __forceinline__ PsfmEncPlan psfm_enc_plan(int p)
{
    PsfmEncPlan n = {-1, -1, -1, -1, -1};
    if (p == 0) {
        n.start = PSFM_ENC_W_ENC;
    } else if (p <= 2) {                                     // encoder layer p - 1
        const int b = PSFM_ENC_W_ENC + (p - 1) * PSFM_ENC_EL_SIZE;
        n.fin = b; n.fin_ln = b + PSFM_ENC_EL_N1; n.ffn = b + PSFM_ENC_EL_FF; n.ffn_ln = b + PSFM_ENC_EL_N2;
        n.start = p == 1 ? b + PSFM_ENC_EL_SIZE : PSFM_ENC_W_DEC;
    } else {                                                 // decoder layer (p - 3) / 2: self-attention (odd p), then cross-attention
        const int b = PSFM_ENC_W_DEC + ((p - 3) >> 1) * PSFM_ENC_DL_SIZE;
        if (p & 1) {
            n.fin = b; n.fin_ln = b + PSFM_ENC_DL_N1; n.start = b + PSFM_ENC_DL_CA;
        } else {
            n.fin = b + PSFM_ENC_DL_CA; n.fin_ln = b + PSFM_ENC_DL_N2; n.ffn = b + PSFM_ENC_DL_FF; n.ffn_ln = b + PSFM_ENC_DL_N3;
            n.start = p == 4 ? b + PSFM_ENC_DL_SIZE : -1;
        }
    }
    return n;
}

// Phase p of one token, p = 0 .. 6.  `rows`: the L rows its trajectory exchanged behind phase p - 1 (unused at p = 0); f: its ten
// input channels (used at p = 0); pad: bit j = position j of the trajectory is padded.  Leaves the row to exchange in s.pub.
//   0  x = project(f); encoder layer 0's self-attention starts from x
//   1  encoder layer 0 finishes (attention, LN1, feed-forward, LN2); layer 1 starts
//   2  encoder layer 1 finishes; mem = encoder.norm; the decoder starts again from x: layer 0's self-attention
//   3  decoder layer 0's self-attention finishes (LN1); its cross-attention starts: q from d, K | V from mem
//   4  that cross-attention finishes, UNMASKED (LN2), feed-forward (LN3); layer 1's self-attention starts
//   5, 6  the same for decoder layer 1; then decoder.norm, and pub[0,16) = the token's output for the max over the tokens
__device__ __forceinline__ void psfm_enc_phase(int p, PsfmEncTok& s, const float* __restrict__ w, const float (&f)[PSFM_ENC_IN],
                                               const float* rows, int L, uint64_t pad)
{
    const PsfmEncPlan n = psfm_enc_plan(p);
    if (p == 0) {
        float t[PSFM_ENC_D];
        psfm_enc_linear<16, 10>(w + PSFM_ENC_W_FC1, w + PSFM_ENC_W_FC1 + 160, f, t);
#pragma unroll
        for (int i = 0; i < 16; i++) t[i] = fmaxf(t[i], 0.0f);
        psfm_enc_linear<16, 16>(w + PSFM_ENC_W_FC2, w + PSFM_ENC_W_FC2 + 256, t, s.x);
#pragma unroll
        for (int i = 0; i < 16; i++) { s.x[i] = fmaxf(s.x[i], 0.0f); s.cur[i] = s.x[i]; }
    } else {
        float a[PSFM_ENC_D], o[PSFM_ENC_D];
        const bool cross = p == 4 || p == 6;
        psfm_enc_attend(s.q, rows, L, cross ? 0 : pad, a);
        psfm_enc_linear<16, 16>(w + n.fin + PSFM_ENC_AT_OUTW, w + n.fin + PSFM_ENC_AT_OUTB, a, o);
#pragma unroll
        for (int i = 0; i < 16; i++) s.cur[i] = s.cur[i] + o[i];
        psfm_enc_ln(s.cur, w + n.fin_ln);
        if (n.ffn >= 0) {
            psfm_enc_ffn(w + n.ffn, s.cur, o);
#pragma unroll
            for (int i = 0; i < 16; i++) s.cur[i] = s.cur[i] + o[i];
            psfm_enc_ln(s.cur, w + n.ffn_ln);
        }
        if (p == 2) {
#pragma unroll
            for (int i = 0; i < 16; i++) s.mem[i] = s.cur[i];
            psfm_enc_ln(s.mem, w + PSFM_ENC_W_ENC_NORM);
#pragma unroll
            for (int i = 0; i < 16; i++) s.cur[i] = s.x[i];
        }
        if (p == PSFM_ENC_PHASES - 1) psfm_enc_ln(s.cur, w + PSFM_ENC_W_DEC_NORM);
    }
    // the row to exchange: the K | V of the attention that starts here, or (last phase) the token's output in [0,16).  Written in ONE
    // place: two places leave the compiler two floats of pub in scratch (it merges their last stores through a selected address)
    const bool last = p == PSFM_ENC_PHASES - 1;
    const bool from_mem = p == 3 || p == 5;
    float row[2 * PSFM_ENC_D];
#pragma unroll
    for (int i = 0; i < 2 * PSFM_ENC_D; i++) row[i] = i < PSFM_ENC_D ? s.cur[i] : s.pub[i];
    if (!last) {
        float kv[PSFM_ENC_D];
#pragma unroll
        for (int i = 0; i < 16; i++) kv[i] = from_mem ? s.mem[i] : s.cur[i];
        psfm_enc_qkv(w + n.start, s.cur, kv, s.q, row);
    }
#pragma unroll
    for (int i = 0; i < 2 * PSFM_ENC_D; i++) s.pub[i] = row[i];
}

// feature c of a trajectory from the rows exchanged behind the last phase: the max over ALL L tokens
__device__ __forceinline__ float psfm_enc_max(const float* rows, int L, int c)
{
    float m = rows[c];
    for (int j = 1; j < L; j++) m = fmaxf(m, rows[j * PSFM_ENC_ROW + c]);
    return m;
}

// position (k, l) is padded: extract_feature's (pad_mask > 0.5) on the .float() of the mask (:47)
__device__ __forceinline__ bool psfm_enc_padded(const double* __restrict__ mask_absent, int e) { return (float)mask_absent[e] > 0.5f; }

// Where thread `thread` of block `block` (waves of 64 lanes, `waves` per block) works: one lane per token, per_wave = 64 / L whole
// trajectories per wave, so a trajectory never leaves its wave.  Rows are counted in the block's slab of 64 * waves rows: my_row is
// the lane's own, row0 the first of its trajectory's L.  A lane without a token (the wave's tail, a trajectory past k) is inactive:
// it runs token 0 of trajectory 0 on the rows of its wave's first trajectory -- all of them inside the wave's 64 rows -- and writes
// nothing.  shift: where the trajectory's L padding bits start in the wave's 64-bit ballot.
struct PsfmEncLane { bool active; int traj, tok, my_row, row0, shift; };

__device__ __forceinline__ PsfmEncLane psfm_enc_lane(int thread, int64_t block, int waves, int L, int per_wave, int64_t k)
{
    const int lane = thread & 63, wave = thread >> 6, t = lane / L;
    const int64_t traj = (block * waves + wave) * per_wave + t;
    PsfmEncLane m;
    m.active = t < per_wave && traj < k;
    m.traj = m.active ? (int)traj : 0;
    m.tok = m.active ? lane - t * L : 0;
    m.my_row = wave * 64 + lane;
    m.shift = m.active ? t * L : 0;
    m.row0 = wave * 64 + m.shift;
    return m;
}

// the trajectory's padding bits out of its wave's ballot of "this lane's position is padded"
__device__ __forceinline__ uint64_t psfm_enc_pad_bits(uint64_t ballot, const PsfmEncLane& m, int L)
{
    return m.active ? (ballot >> m.shift) & (L == 64 ? ~(uint64_t)0 : ((uint64_t)1 << L) - 1) : 0;
}

