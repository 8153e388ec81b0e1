// psfm_motion_boundary.hip -- gfx950 kernels of the motion-boundary option (psfm_ctx_set_motion_boundary):
//   the mask of trajectory.py:39-43 over a whole flow stack, alone (psfm_motion_boundary) or folded with the occlusion maps into the
//   KILL MAP the chain step samples (bit 0 occlusion, bit 1 motion boundary), and the chain step with the second verdict
//   (psfm_chain_step_body<.., MB = true>: trajectory.py:51-53 and the kill rule of :60); and what psfm_connect_batch launches with the
//   option on: the kill maps of a batch of stacks, frame range by frame range (psfm_kill_map_batch), and the batched chain step.
// The per-pixel rule lives in psfm_motion_boundary.h; the host build of the CPU suite compiles the same text.
#include "psfm_device.h"
#include <hip/hip_ext.h>
#include <stdlib.h>
#include <string.h>

#include "psfm_internal.h"
#include "psfm_motion_boundary.h"
#include "psfm_chain_step.h"
#include "psfm_batch_shapes.h"

#define PSFM_MB_BLOCK 256
#define PSFM_MB_PPL 4             // pixels per lane: 32 bytes of flow = two 16-byte loads, 4 result bytes = one 32-bit store

// ------------------------------------------------------------------------------------------------
// The mask as a stream.  Algorithmic bytes per pixel: 8 (flow) [+ 1 (occlusion byte)] + 1 (result); the south neighbours are the
// row the same XCD streams W / 4 lanes later, the east neighbour of a lane's last pixel is the next lane's first.
//
// The stack is ONE run of N = n H W pixels and lane g owns pixels 4g .. 4g + 3 of it, wherever rows and frames end: the lane's own
// pixels are always 32 aligned bytes (flows 16-byte aligned: the launcher checks), the results 4 aligned bytes.  A launch has
// blockIdx.y = frame f and covers the lanes whose FIRST pixel lies in frame f -- [ceil(f P / 4), ceil((f + 1) P / 4)) -- so a
// lane's position inside its frame is 32-bit arithmetic; its last pixels may belong to frame f + 1 (P not a multiple of 4).
//   own pixels     2 x 16 bytes
//   row below      2 x 16 bytes at + W pixels when W is even (the address is then 16-byte aligned), 4 x 8 bytes otherwise; a pixel
//                  of a frame's last row has dy = 0 and the loaded value is never used (the unguarded forms read the next frame's
//                  first row there; the last lanes of the stack, which have nothing behind them, take guarded 8-byte loads)
//   east           pixel j + 1 of the lane; for the last one 8 bytes more (the next lane's first pixel)
// blockIdx.x -> chunk of 256 lanes through the XCD banding of flow_check (psfm_track.hip): blocks go to the eight XCDs round-robin,
// so each XCD takes one contiguous band of rows and finds the row below in its own L2.
// ------------------------------------------------------------------------------------------------
struct PsfmMbArgs {
    const float2* flows; const uint8_t* occ; uint8_t* out;
    int H, W, P;                  // P = H W < 2^29 (psfm_frame_ok)
    int n, frame0;                // frames of the stack; frame of blockIdx.y == 0
    float thres;
    int chunks, xcd_per;          // 256-lane chunks per frame (ceil((P / 4 + 1) / 256)); > 0: chunks per XCD band
    int out_al4;                  // out (and occ) 4-byte aligned: results leave as one 32-bit store
    PsfmFastDiv wdiv;
};

// One lane's four pixels from q0 on (r0: the first one's index in its frame).  FAST (decided per block, from uniform values): every
// lane of the block has its four pixels, the pixel behind them and the four pixels one row below inside the stack, and the byte
// buffers are 4-byte aligned -- nothing is guarded, so all loads are issued back to back behind one wait.  Otherwise (the last block
// of a frame's lanes, the tail of the stack, unaligned byte buffers) every access is checked.
template <bool HAS_OCC, bool WEVEN, bool FAST>
__device__ __forceinline__ void psfm_mb_lane(const PsfmMbArgs& a, int64_t q0, int r0, int64_t N)
{
    const float2* __restrict__ Fq = a.flows + q0;
    const bool whole = FAST || q0 + PSFM_MB_PPL <= N;       // all four pixels exist
    const bool words = FAST || (whole & (a.out_al4 != 0));  // the four bytes travel as one 32-bit word
    const float2 z2 = make_float2(0.0f, 0.0f);

    // ---- position of every pixel in its frame ----
    int x[PSFM_MB_PPL], y[PSFM_MB_PPL];
    y[0] = (int)psfm_fastdiv((unsigned)r0, a.wdiv); x[0] = r0 - y[0] * a.W;
#pragma unroll
    for (int j = 1; j < PSFM_MB_PPL; ++j) {
        x[j] = x[j - 1] + 1; y[j] = y[j - 1];
        if (x[j] == a.W) { x[j] = 0; ++y[j]; }
        if (y[j] == a.H) y[j] = 0;                           // first row of the next frame
    }

    // ---- loads ----
    float2 own[PSFM_MB_PPL + 1], below[PSFM_MB_PPL];
    if (whole) {
        const float4 lo = *(const float4*)Fq, hi = *(const float4*)(Fq + 2);
        own[0] = make_float2(lo.x, lo.y); own[1] = make_float2(lo.z, lo.w);
        own[2] = make_float2(hi.x, hi.y); own[3] = make_float2(hi.z, hi.w);
    } else {
#pragma unroll
        for (int j = 0; j < PSFM_MB_PPL; ++j) own[j] = q0 + j < N ? Fq[j] : z2;
    }
    own[PSFM_MB_PPL] = (FAST || q0 + PSFM_MB_PPL < N) ? Fq[PSFM_MB_PPL] : z2;
    if (WEVEN && (FAST || q0 + a.W + PSFM_MB_PPL <= N)) {
        const float4 lo = *(const float4*)(Fq + a.W), hi = *(const float4*)(Fq + a.W + 2);
        below[0] = make_float2(lo.x, lo.y); below[1] = make_float2(lo.z, lo.w);
        below[2] = make_float2(hi.x, hi.y); below[3] = make_float2(hi.z, hi.w);
    } else {
#pragma unroll
        for (int j = 0; j < PSFM_MB_PPL; ++j)      // (y + 1 < H: the pixel below is in the stack)
            below[j] = (FAST || ((q0 + j < N) & (y[j] + 1 < a.H))) ? Fq[a.W + j] : z2;
    }
    unsigned ob = 0;                                         // the lane's four occlusion bytes
    if (HAS_OCC) {
        if (words) ob = *(const unsigned*)(a.occ + q0);
        else {
#pragma unroll
            for (int j = 0; j < PSFM_MB_PPL; ++j) if (q0 + j < N) ob |= (unsigned)a.occ[q0 + j] << (8 * j);
        }
    }

    // ---- verdicts ----
    unsigned res = 0;
#pragma unroll
    for (int j = 0; j < PSFM_MB_PPL; ++j) {
        unsigned v = psfm_mb_px(own[j], own[j + 1], x[j] + 1 < a.W, below[j], y[j] + 1 < a.H, a.thres);
        if (HAS_OCC) v = (((ob >> (8 * j)) & 0xffu) != 0 ? PSFM_KILL_OCC : 0u) | (v ? PSFM_KILL_MB : 0u);
        res |= v << (8 * j);
    }
    if (words) *(unsigned*)(a.out + q0) = res;
    else {
#pragma unroll
        for (int j = 0; j < PSFM_MB_PPL; ++j) if (q0 + j < N) a.out[q0 + j] = (uint8_t)(res >> (8 * j));
    }
}

template <bool HAS_OCC, bool WEVEN>
__global__ __launch_bounds__(PSFM_MB_BLOCK) void psfm_mb_kernel(PsfmMbArgs a)
{
    const int bx = (int)blockIdx.x;
    const int chunk = a.xcd_per > 0 ? (bx & 7) * a.xcd_per + (bx >> 3) : bx;
    if (chunk >= a.chunks) return;
    const int f = a.frame0 + (int)blockIdx.y;
    const int64_t N = (int64_t)a.n * a.P;
    const int64_t F0 = (int64_t)f * a.P;
    const int64_t g_lo = (F0 + 3) >> 2, g_hi = (F0 + a.P + 3) >> 2;
    const int64_t g_blk = g_lo + (int64_t)chunk * PSFM_MB_BLOCK;          // the block's first lane
    const int64_t g = g_blk + threadIdx.x;
    const int64_t q0 = g * PSFM_MB_PPL;                                   // < N when g < g_hi: g_hi <= ceil(N / 4)
    const int r0 = (int)(q0 - F0);                                        // in [0, P) when g < g_hi
    // (block-uniform) the block's last lane is a lane of the frame, and the furthest byte it touches -- pixel q0 + W + 3 -- exists
    const int64_t g_last = g_blk + PSFM_MB_BLOCK - 1;
    const bool fast = (a.out_al4 != 0) & (g_last < g_hi) & (g_last * PSFM_MB_PPL + a.W + 2 * PSFM_MB_PPL <= N);
    if (fast) {
        psfm_mb_lane<HAS_OCC, WEVEN, true>(a, q0, r0, N);
    } else {
        if (g >= g_hi) return;
        psfm_mb_lane<HAS_OCC, WEVEN, false>(a, q0, r0, N);
    }
}

// one pixel per thread, for a flow stack that is not 16-byte aligned (no caller of the package has one)
template <bool HAS_OCC>
__global__ __launch_bounds__(PSFM_MB_BLOCK) void psfm_mb_px_kernel(PsfmMbArgs a)
{
    const int p = (int)blockIdx.x * PSFM_MB_BLOCK + (int)threadIdx.x;
    if (p >= a.P) return;
    const int64_t base = (int64_t)(a.frame0 + (int)blockIdx.y) * a.P;
    const int y = (int)psfm_fastdiv((unsigned)p, a.wdiv), x = p - y * a.W;
    unsigned v = psfm_mb_at(a.flows + base, x, y, a.H, a.W, a.thres);
    if (HAS_OCC) v = (a.occ[base + p] != 0 ? PSFM_KILL_OCC : 0u) | (v ? PSFM_KILL_MB : 0u);
    a.out[base + p] = (uint8_t)v;
}

psfm_status psfm_launch_motion_boundary(const float* flows, const uint8_t* occ, int n, int h, int w, float thres, uint8_t* out, hipStream_t s)
{
    if (n <= 0) return PSFM_OK;
    PsfmMbArgs a;
    a.flows = (const float2*)flows; a.occ = occ; a.out = out;
    a.H = h; a.W = w; a.P = h * w; a.n = n; a.thres = thres;
    a.wdiv = psfm_fastdiv_make((unsigned)w);
    a.out_al4 = (((uintptr_t)out % 4) == 0 && (!occ || ((uintptr_t)occ % 4) == 0)) ? 1 : 0;
    const bool vec = ((uintptr_t)flows % 16) == 0;
    const int lanes = a.P / PSFM_MB_PPL + 1;                 // of one frame, at most
    a.chunks = vec ? (lanes + PSFM_MB_BLOCK - 1) / PSFM_MB_BLOCK : (a.P + PSFM_MB_BLOCK - 1) / PSFM_MB_BLOCK;
    a.xcd_per = (vec && a.chunks >= 64) ? (a.chunks + 7) / 8 : 0;
    const unsigned gx = (unsigned)(a.xcd_per > 0 ? 8 * a.xcd_per : a.chunks);
    for (int f0 = 0; f0 < n; f0 += 32768) {                  // (gridDim.y < 65536)
        a.frame0 = f0;
        const dim3 grid(gx, (unsigned)(n - f0 < 32768 ? n - f0 : 32768)), block(PSFM_MB_BLOCK);
        if (vec) {
            const bool weven = (w & 1) == 0;
            if (occ && weven) hipLaunchKernelGGL((psfm_mb_kernel<true, true>), grid, block, 0, s, a);
            else if (occ) hipLaunchKernelGGL((psfm_mb_kernel<true, false>), grid, block, 0, s, a);
            else if (weven) hipLaunchKernelGGL((psfm_mb_kernel<false, true>), grid, block, 0, s, a);
            else hipLaunchKernelGGL((psfm_mb_kernel<false, false>), grid, block, 0, s, a);
        } else {
            if (occ) hipLaunchKernelGGL(psfm_mb_px_kernel<true>, grid, block, 0, s, a);
            else hipLaunchKernelGGL(psfm_mb_px_kernel<false>, grid, block, 0, s, a);
        }
    }
    PSFM_HIP(hipGetLastError());
    return PSFM_OK;
}

extern "C" psfm_status psfm_motion_boundary(psfm_ctx* c, const float* flows, int n, int h, int w, float thres, uint8_t* mb_out, void* stream)
{
    if (!c) { psfm_set_error("ctx is NULL"); return PSFM_ERR_ARG; }
    PSFM_HIP(hipSetDevice(c->device));
    PsfmGate gate(c->device, 0);
    if (n < 0 || !psfm_frame_ok(h, w) || (n > 0 && (!flows || !mb_out))) {
        psfm_set_error("psfm_motion_boundary: bad argument (n=%d h=%d w=%d)", n, h, w);
        return PSFM_ERR_ARG;
    }
    return psfm_launch_motion_boundary(flows, nullptr, n, h, w, thres, mb_out, (hipStream_t)stream);
}

extern "C" psfm_status psfm_kill_map(psfm_ctx* c, const float* flows, const uint8_t* occ, int n, int h, int w, float thres, uint8_t* kill_out,
                                     void* stream)
{
    if (!c) { psfm_set_error("ctx is NULL"); return PSFM_ERR_ARG; }
    PSFM_HIP(hipSetDevice(c->device));
    PsfmGate gate(c->device, 0);
    if (n < 0 || !psfm_frame_ok(h, w) || (n > 0 && (!flows || !occ || !kill_out))) {
        psfm_set_error("psfm_kill_map: bad argument (n=%d h=%d w=%d)", n, h, w);
        return PSFM_ERR_ARG;
    }
    return psfm_launch_motion_boundary(flows, occ, n, h, w, thres, kill_out, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------
// The kill maps of a BATCH of same-shape stacks (psfm_connect_batch with the option on; psfm_kill_map_batch): ONE launch for frames
// [pair0, pair0 + n_pairs) of every stack -- blockIdx.y = frame pair0 + y, blockIdx.z = stack, a table row per stack in device memory
// (as PsfmFcSeq is for psfm_flow_check_x2v_batch_kernel), every row with its own threshold.
//
// Inside the batch the maps are built chunk by chunk behind flow_check on the side stream: the occlusion bytes of frame f + 1 may not
// exist yet when frame f is done.  So here a FRAME is the run of pixels and lane l of a frame owns its pixels 4 l .. 4 l + 3 -- no lane
// straddles a frame end (the single launch above lets one, which is why it cannot serve a range).  What the launch touches:
//   occlusion bytes, kill bytes   of the frames of the range only, each frame's own P bytes
//   flows                         of the same frames; the unguarded blocks also LOAD the pixel behind a lane's four and the four one
//                                 row below without looking where the frame ends (last row: dy = 0, the value is never used) -- such a
//                                 block is only unguarded when those loads stay inside the stack
// P even (the launcher checks; else one pixel per thread): a frame's flows start on a 16-byte boundary when the stack does.  The byte
// buffers of a frame are 4-byte aligned or not, frame by frame (P = 2 mod 4): a frame whose bytes are not takes the guarded form, whose
// bytes travel one by one.  Guarded too: the last block of a frame's lanes (P is no multiple of 1024 pixels), and the blocks of a
// stack's last frame that would load beyond it.  Everything else -- the interior -- checks nothing and issues its loads back to back
// behind one wait, as the single launch does.
// ------------------------------------------------------------------------------------------------
struct PsfmKmArgs {
    int H, W, P;                  // P = H W, even
    int pair0;                    // frame of blockIdx.y == 0
    int chunks, xcd_per;          // 256-lane chunks per frame (ceil(ceil(P / 4) / 256)); > 0: chunks per XCD band
    PsfmFastDiv wdiv;
};

// One lane's four pixels r0 .. r0 + 3 of ITS frame (F / occ / out: the frame's own).  FAST: all four exist, the bytes are 4-byte
// aligned and every load below stays inside the stack.  Otherwise nothing outside the frame is touched.
template <bool WEVEN, bool FAST>
__device__ __forceinline__ void psfm_km_lane(const float2* __restrict__ F, const uint8_t* __restrict__ occ, uint8_t* __restrict__ out,
                                             const PsfmKmArgs& a, int r0, float thres, bool bytes_al4)
{
    const float2* __restrict__ Fq = F + r0;
    const bool whole = FAST || r0 + PSFM_MB_PPL <= a.P;     // all four pixels exist
    const bool words = FAST || (whole & bytes_al4);         // the four bytes travel as one 32-bit word
    const float2 z2 = make_float2(0.0f, 0.0f);

    int x[PSFM_MB_PPL], y[PSFM_MB_PPL];
    y[0] = (int)psfm_fastdiv((unsigned)r0, a.wdiv); x[0] = r0 - y[0] * a.W;
#pragma unroll
    for (int j = 1; j < PSFM_MB_PPL; ++j) {
        x[j] = x[j - 1] + 1; y[j] = y[j - 1];
        if (x[j] == a.W) { x[j] = 0; ++y[j]; }              // (y == H: a pixel behind the frame, never stored)
    }

    float2 own[PSFM_MB_PPL + 1], below[PSFM_MB_PPL];
    if (whole) {
        const float4 lo = *(const float4*)Fq, hi = *(const float4*)(Fq + 2);
        own[0] = make_float2(lo.x, lo.y); own[1] = make_float2(lo.z, lo.w);
        own[2] = make_float2(hi.x, hi.y); own[3] = make_float2(hi.z, hi.w);
    } else {
#pragma unroll
        for (int j = 0; j < PSFM_MB_PPL; ++j) own[j] = r0 + j < a.P ? Fq[j] : z2;
    }
    own[PSFM_MB_PPL] = (FAST || r0 + PSFM_MB_PPL < a.P) ? Fq[PSFM_MB_PPL] : z2;
    if (WEVEN && (FAST || r0 + a.W + PSFM_MB_PPL <= a.P)) {
        const float4 lo = *(const float4*)(Fq + a.W), hi = *(const float4*)(Fq + a.W + 2);
        below[0] = make_float2(lo.x, lo.y); below[1] = make_float2(lo.z, lo.w);
        below[2] = make_float2(hi.x, hi.y); below[3] = make_float2(hi.z, hi.w);
    } else {
#pragma unroll
        for (int j = 0; j < PSFM_MB_PPL; ++j)      // (y + 1 < H: the pixel below is in the frame)
            below[j] = (FAST || ((r0 + j < a.P) & (y[j] + 1 < a.H))) ? Fq[a.W + j] : z2;
    }
    unsigned ob = 0;
    if (words) ob = *(const unsigned*)(occ + r0);
    else {
#pragma unroll
        for (int j = 0; j < PSFM_MB_PPL; ++j) if (r0 + j < a.P) ob |= (unsigned)occ[r0 + j] << (8 * j);
    }

    unsigned res = 0;
#pragma unroll
    for (int j = 0; j < PSFM_MB_PPL; ++j) {
        const unsigned v = psfm_mb_px(own[j], own[j + 1], x[j] + 1 < a.W, below[j], y[j] + 1 < a.H, thres);
        res |= ((((ob >> (8 * j)) & 0xffu) != 0 ? PSFM_KILL_OCC : 0u) | (v ? PSFM_KILL_MB : 0u)) << (8 * j);
    }
    if (words) *(unsigned*)(out + r0) = res;
    else {
#pragma unroll
        for (int j = 0; j < PSFM_MB_PPL; ++j) if (r0 + j < a.P) out[r0 + j] = (uint8_t)(res >> (8 * j));
    }
}

template <bool WEVEN>
__global__ __launch_bounds__(PSFM_MB_BLOCK) void psfm_kill_map_batch_kernel(const PsfmKmSeq* __restrict__ T, PsfmKmArgs a)
{
    const int bx = (int)blockIdx.x;
    const int chunk = a.xcd_per > 0 ? (bx & 7) * a.xcd_per + (bx >> 3) : bx;
    if (chunk >= a.chunks) return;
    const PsfmKmSeq& t = T[blockIdx.z];
    const int f = a.pair0 + (int)blockIdx.y;
    if (f >= t.n) return;                                                  // a stack is touched only where it has frames
    const int64_t F0 = (int64_t)f * a.P;
    const float2* F = (const float2*)t.flows + F0;
    const uint8_t* occ = t.occ + F0;
    uint8_t* out = t.out + F0;
    const int r_blk = chunk * (PSFM_MB_BLOCK * PSFM_MB_PPL);               // the block's first pixel in the frame
    const int r0 = r_blk + (int)threadIdx.x * PSFM_MB_PPL;
    // (block-uniform) the block's last lane has its four pixels in the frame, and the furthest flow it loads -- the pixel W + 3 behind
    // its first -- exists in the stack
    const int r_last = r_blk + (PSFM_MB_BLOCK - 1) * PSFM_MB_PPL;
    const bool al4 = ((((uintptr_t)occ) | ((uintptr_t)out)) & 3) == 0;
    const bool fast = al4 & (r_last + PSFM_MB_PPL <= a.P) & (F0 + r_last + a.W + PSFM_MB_PPL <= (int64_t)t.n * a.P);
    if (fast) {
        psfm_km_lane<WEVEN, true>(F, occ, out, a, r0, t.thres, true);
    } else {
        if (r0 >= a.P) return;
        psfm_km_lane<WEVEN, false>(F, occ, out, a, r0, t.thres, al4);
    }
}

// one pixel per thread: P odd (every second frame's flows are off their 16-byte alignment) or a flow stack that is not aligned
__global__ __launch_bounds__(PSFM_MB_BLOCK) void psfm_kill_map_batch_px_kernel(const PsfmKmSeq* __restrict__ T, PsfmKmArgs a)
{
    const int p = (int)blockIdx.x * PSFM_MB_BLOCK + (int)threadIdx.x;
    const PsfmKmSeq& t = T[blockIdx.z];
    const int f = a.pair0 + (int)blockIdx.y;
    if (p >= a.P || f >= t.n) return;
    const int64_t base = (int64_t)f * a.P;
    const int y = (int)psfm_fastdiv((unsigned)p, a.wdiv), x = p - y * a.W;
    const unsigned v = psfm_mb_at((const float2*)t.flows + base, x, y, a.H, a.W, t.thres);
    t.out[base + p] = (uint8_t)((t.occ[base + p] != 0 ? PSFM_KILL_OCC : 0u) | (v ? PSFM_KILL_MB : 0u));
}

// ... and for stacks of DIFFERENT frame sizes (psfm_connect_batch with h = w = 0): blockIdx.x runs over the blocks of all stacks
// (psfm_batch_shapes.h), blockIdx.y = frame pair0 + y.  The frame, the band rule and the form are the row's -- four pixels per lane
// with W even or odd, or one pixel per thread -- and the switch between them is block-uniform; inside a form the block does what the
// block of the launch above does for the same chunk of the same frame (the same fast / guarded decision from the row's P, W and n).
static_assert(PSFM_BS_KM_LANES == PSFM_MB_BLOCK && PSFM_BS_KM_PPL == PSFM_MB_PPL, "psfm_batch_shapes.h counts the chunks of these kernels");
template <bool WEVEN>
__device__ __forceinline__ void psfm_km_shapes_lanes(const PsfmKmShapeRow& t, const PsfmKmArgs& a, int chunk, int f)
{
    const int64_t F0 = (int64_t)f * a.P;
    const float2* F = (const float2*)t.flows + F0;
    const uint8_t* occ = t.occ + F0;
    uint8_t* out = t.out + F0;
    const int r_blk = chunk * (PSFM_MB_BLOCK * PSFM_MB_PPL);
    const int r0 = r_blk + (int)threadIdx.x * PSFM_MB_PPL;
    const int r_last = r_blk + (PSFM_MB_BLOCK - 1) * PSFM_MB_PPL;
    const bool al4 = ((((uintptr_t)occ) | ((uintptr_t)out)) & 3) == 0;
    const bool fast = al4 & (r_last + PSFM_MB_PPL <= a.P) & (F0 + r_last + a.W + PSFM_MB_PPL <= (int64_t)t.n * a.P);
    if (fast) {
        psfm_km_lane<WEVEN, true>(F, occ, out, a, r0, t.thres, true);
    } else {
        if (r0 >= a.P) return;
        psfm_km_lane<WEVEN, false>(F, occ, out, a, r0, t.thres, al4);
    }
}

__global__ __launch_bounds__(PSFM_MB_BLOCK) void psfm_kill_map_shapes_kernel(const PsfmKmShapeRow* __restrict__ T, const int* __restrict__ blk_end,
                                                                          int pair0)
{
    const int b = __builtin_amdgcn_readfirstlane(psfm_bs_find(blk_end, (int)blockIdx.x));
    const PsfmKmShapeRow& t = T[b];
    const int f = pair0 + (int)blockIdx.y;
    if (f >= t.n) return;                                                  // a stack is touched only where it has frames
    const int chunk = psfm_bs_chunk((int)blockIdx.x - t.blk0, t.chunks, t.xcd_per);
    if (chunk < 0) return;                                                 // (a spare block: the stack's count is rounded up to 8)
    PsfmKmArgs a;
    a.H = t.H; a.W = t.W; a.P = t.P; a.pair0 = pair0; a.chunks = t.chunks; a.xcd_per = t.xcd_per; a.wdiv = t.wdiv;
    const int form = t.form;
    if (form == PSFM_BS_KM_LANE_WEVEN) psfm_km_shapes_lanes<true>(t, a, chunk, f);
    else if (form == PSFM_BS_KM_LANE_WODD) psfm_km_shapes_lanes<false>(t, a, chunk, f);
    else {
        const int p = chunk * PSFM_MB_BLOCK + (int)threadIdx.x;
        if (p >= a.P) return;
        const int64_t base = (int64_t)f * a.P;
        const int y = (int)psfm_fastdiv((unsigned)p, a.wdiv), x = p - y * a.W;
        const unsigned v = psfm_mb_at((const float2*)t.flows + base, x, y, a.H, a.W, t.thres);
        t.out[base + p] = (uint8_t)((t.occ[base + p] != 0 ? PSFM_KILL_OCC : 0u) | (v ? PSFM_KILL_MB : 0u));
    }
}

// the table of a psfm_kill_map_batch call travels in this kernel's arguments (read when the launch is enqueued: the caller's arrays may
// go away as soon as the call returns) and is stored where the launch behind it finds it
struct PsfmKmTab { PsfmKmSeq row[PSFM_BATCH_MAX]; };
__global__ __launch_bounds__(PSFM_BATCH_MAX) void psfm_km_table_kernel(PsfmKmTab t, int n_seq, PsfmKmSeq* __restrict__ dst)
{
    if ((int)threadIdx.x < n_seq) dst[threadIdx.x] = t.row[threadIdx.x];
}

bool psfm_kill_map_batch_vec_ok(int h, int w, const void* flows) { return (((int64_t)h * w) % 2) == 0 && ((uintptr_t)flows % 16) == 0; }

psfm_status psfm_launch_kill_map_batch(const PsfmKmSeq* tab_dev, int n_seq, int pair0, int n_pairs, int h, int w, bool vec, hipStream_t s)
{
    if (n_pairs <= 0 || n_seq <= 0) return PSFM_OK;
    PsfmKmArgs a;
    a.H = h; a.W = w; a.P = h * w;
    a.wdiv = psfm_fastdiv_make((unsigned)w);
    const int lanes = (a.P + PSFM_MB_PPL - 1) / PSFM_MB_PPL;
    a.chunks = vec ? (lanes + PSFM_MB_BLOCK - 1) / PSFM_MB_BLOCK : (a.P + PSFM_MB_BLOCK - 1) / PSFM_MB_BLOCK;
    a.xcd_per = (vec && a.chunks >= 64) ? (a.chunks + 7) / 8 : 0;
    const unsigned gx = (unsigned)(a.xcd_per > 0 ? 8 * a.xcd_per : a.chunks);
    for (int f0 = 0; f0 < n_pairs; f0 += 32768) {            // (gridDim.y < 65536)
        a.pair0 = pair0 + f0;
        const dim3 grid(gx, (unsigned)(n_pairs - f0 < 32768 ? n_pairs - f0 : 32768), (unsigned)n_seq), block(PSFM_MB_BLOCK);
        if (!vec) hipLaunchKernelGGL(psfm_kill_map_batch_px_kernel, grid, block, 0, s, tab_dev, a);
        else if ((w & 1) == 0) hipLaunchKernelGGL(psfm_kill_map_batch_kernel<true>, grid, block, 0, s, tab_dev, a);
        else hipLaunchKernelGGL(psfm_kill_map_batch_kernel<false>, grid, block, 0, s, tab_dev, a);
    }
    PSFM_HIP(hipGetLastError());
    return PSFM_OK;
}

// stacks of different frame sizes: a stack's row (its place in the flattened grid apart: psfm_bs_km_prefix) and the launch
void psfm_km_shape_row(const PsfmKmSeq& q, int h, int w, PsfmKmShapeRow* row)
{
    memset(row, 0, sizeof(*row));
    row->flows = q.flows; row->occ = q.occ; row->out = q.out; row->n = q.n; row->thres = q.thres;
    row->H = h; row->W = w; row->P = h * w;
    row->wdiv = psfm_fastdiv_make((unsigned)w);
    row->form = psfm_bs_km_form(row->P, w, ((uintptr_t)q.flows % 16) == 0);
    row->chunks = psfm_bs_km_chunks(row->P, row->form);
    row->xcd_per = row->form == PSFM_BS_KM_PX ? 0 : psfm_bs_xcd_per(row->chunks);
}

psfm_status psfm_launch_kill_map_shapes(const PsfmKmShapeRow* tab_dev, const int* blk_end_dev, int blocks, int pair0, int n_pairs, hipStream_t s)
{
    if (n_pairs <= 0 || blocks <= 0) return PSFM_OK;
    for (int f0 = 0; f0 < n_pairs; f0 += 32768) {            // (gridDim.y < 65536)
        const dim3 grid((unsigned)blocks, (unsigned)(n_pairs - f0 < 32768 ? n_pairs - f0 : 32768)), block(PSFM_MB_BLOCK);
        hipLaunchKernelGGL(psfm_kill_map_shapes_kernel, grid, block, 0, s, tab_dev, blk_end_dev, pair0 + f0);
    }
    PSFM_HIP(hipGetLastError());
    return PSFM_OK;
}

extern "C" psfm_status psfm_kill_map_batch(psfm_ctx* c, const float* const* flows, const uint8_t* const* occ, const int* n_flows, int n_seq, int h,
                                           int w, const float* thres, int pair0, int n_pairs, uint8_t* const* kill_out, void* stream)
{
    if (!c) { psfm_set_error("ctx is NULL"); return PSFM_ERR_ARG; }
    bool ok = flows && occ && n_flows && thres && kill_out && n_seq >= 1 && n_seq <= PSFM_BATCH_MAX && psfm_frame_ok(h, w) && pair0 >= 0 && n_pairs >= 0;
    for (int i = 0; ok && i < n_seq; ++i)
        ok = flows[i] && occ[i] && kill_out[i] && n_flows[i] >= 0 && thres[i] >= 0.0f && thres[i] != INFINITY;      // (NaN fails the comparison)
    if (!ok) {
        psfm_set_error("psfm_kill_map_batch: bad argument (n_seq=%d of 1..%d, h=%d w=%d pair0=%d n_pairs=%d; no NULL pointer, every threshold "
                       "finite and >= 0)", n_seq, PSFM_BATCH_MAX, h, w, pair0, n_pairs);
        return PSFM_ERR_ARG;
    }
    PSFM_HIP(hipSetDevice(c->device));
    PsfmGate gate(c->device, 0);
    if (n_pairs == 0) return PSFM_OK;
    PsfmKmTab tab;
    memset(&tab, 0, sizeof(tab));
    bool vec = true;
    int n_max = 0;
    for (int i = 0; i < n_seq; ++i) {
        tab.row[i].flows = flows[i]; tab.row[i].occ = occ[i]; tab.row[i].out = kill_out[i]; tab.row[i].n = n_flows[i]; tab.row[i].thres = thres[i];
        vec = vec && psfm_kill_map_batch_vec_ok(h, w, flows[i]);
        n_max = n_flows[i] > n_max ? n_flows[i] : n_max;
    }
    if (pair0 >= n_max) return PSFM_OK;
    if (n_pairs > n_max - pair0) n_pairs = n_max - pair0;
    psfm_status st;
    if ((st = c->batch_km.ensure(sizeof(tab))) != PSFM_OK) return st;
    hipLaunchKernelGGL(psfm_km_table_kernel, dim3(1), dim3(PSFM_BATCH_MAX), 0, (hipStream_t)stream, tab, n_seq, c->batch_km.as<PsfmKmSeq>());
    return psfm_launch_kill_map_batch(c->batch_km.as<PsfmKmSeq>(), n_seq, pair0, n_pairs, h, w, vec, (hipStream_t)stream);
}

extern "C" psfm_status psfm_ctx_set_motion_boundary(psfm_ctx* c, int enable, float thres)
{
    if (!c) { psfm_set_error("ctx is NULL"); return PSFM_ERR_ARG; }
    if (!(thres >= 0.0f) || thres == INFINITY) {             // (NaN fails the first comparison)
        psfm_set_error("psfm_ctx_set_motion_boundary: thres must be finite and >= 0");
        return PSFM_ERR_ARG;
    }
    c->mb_enable = enable != 0;
    c->mb_thres = thres;
    return PSFM_OK;
}

// ------------------------------------------------------------------------------------------------
// The chain step with the motion-boundary verdict: psfm_chain_step_kernel's body with MB = true, `a.occ` = the frame's kill map.
// The instantiations live here, under a name of their own: the register census of tests/test_persist_resources.py reads every kernel
// of psfm_track.hip by (name, template arguments), and that translation unit compiles to what it was.
// ------------------------------------------------------------------------------------------------
template <int R, bool OPT>
__global__ __launch_bounds__(PSFM_CHAIN_BLOCK) PSFM_CHAIN_WAVES void psfm_chain_step_mb_kernel(PsfmChainArgs a)
{
    PsfmChainOut o;
    (void)psfm_chain_step_body<R, OPT, false, true>(a, o);
}

psfm_status psfm_launch_chain_step_mb(psfm_ctx* c, const PsfmTrackDims& d, const float* flow, const uint8_t* kill, int frame, bool optimize,
                                      hipStream_t s)
{
    PsfmChainArgs a;
    psfm_fill_chain_args(c, d, flow, kill, frame, a, s);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    c->prof.kernel_span(PSFM_PROF_CHAIN, &e0, &e1);
    const dim3 grid((unsigned)((d.cap + PSFM_CHAIN_TILE - 1) / PSFM_CHAIN_TILE)), block(PSFM_CHAIN_BLOCK);
    if (optimize) {
        switch (d.ratio) {
            case 1: hipExtLaunchKernelGGL((psfm_chain_step_mb_kernel<1, true>), grid, block, 0, s, e0, e1, 0, a); break;
            case 2: hipExtLaunchKernelGGL((psfm_chain_step_mb_kernel<2, true>), grid, block, 0, s, e0, e1, 0, a); break;
            case 4: hipExtLaunchKernelGGL((psfm_chain_step_mb_kernel<4, true>), grid, block, 0, s, e0, e1, 0, a); break;
            default: hipExtLaunchKernelGGL((psfm_chain_step_mb_kernel<0, true>), grid, block, 0, s, e0, e1, 0, a); break;
        }
    } else {
        switch (d.ratio) {
            case 1: hipExtLaunchKernelGGL((psfm_chain_step_mb_kernel<1, false>), grid, block, 0, s, e0, e1, 0, a); break;
            case 2: hipExtLaunchKernelGGL((psfm_chain_step_mb_kernel<2, false>), grid, block, 0, s, e0, e1, 0, a); break;
            case 4: hipExtLaunchKernelGGL((psfm_chain_step_mb_kernel<4, false>), grid, block, 0, s, e0, e1, 0, a); break;
            default: hipExtLaunchKernelGGL((psfm_chain_step_mb_kernel<0, false>), grid, block, 0, s, e0, e1, 0, a); break;
        }
    }
    PSFM_HIP(hipGetLastError());
    return PSFM_OK;
}

// ... and its batched form (psfm_connect_batch with the option on in every context): psfm_chain_step_batch_kernel of psfm_track.hip
// with MB = true, the rows' `a.occ` = the sequences' kill maps.  The third template argument exists here only; the MB = false forms are
// the two-argument template of psfm_track.hip, which compiles to what it was.
template <int R, bool OPT, bool MB>
__global__ __launch_bounds__(PSFM_CHAIN_BLOCK) PSFM_CHAIN_WAVES void psfm_chain_step_batch_kernel(const PsfmBatchSeq* __restrict__ seqs, int frame)
{
    static_assert(MB, "the MB = false form is psfm_chain_step_batch_kernel<R, OPT> of psfm_track.hip");
    const PsfmBatchSeq& q = seqs[blockIdx.y];
    if (frame >= q.n_flows) return;
    PsfmChainArgs a = q.a;
    // (as in psfm_track.hip: a launch that covers fewer lanes than the sequence has in use says so)
    if (blockIdx.x == 0 && threadIdx.x == 0 && a.ctr->n_lanes > (int)(gridDim.x * PSFM_CHAIN_TILE)) atomicOr(&a.ctr->overflow, 16);
    psfm_chain_args_rebase(a, q.st, frame);
    PsfmChainOut o;
    (void)psfm_chain_step_body<R, OPT, false, MB>(a, o);
}

psfm_status psfm_launch_chain_step_batch_mb(psfm_ctx* owner, const PsfmBatchSeq* tab_dev, int n_seq, int ratio, int64_t cap_max, int frame,
                                            bool optimize, hipStream_t s)
{
    hipEvent_t e0 = nullptr, e1 = nullptr;
    owner->prof.kernel_span(PSFM_PROF_CHAIN, &e0, &e1);
    const unsigned gx = (unsigned)(((cap_max + PSFM_CHAIN_TILE - 1) / PSFM_CHAIN_TILE + 7) / 8 * 8);
    const dim3 grid(gx, (unsigned)n_seq), block(PSFM_CHAIN_BLOCK);
    if (optimize) {
        switch (ratio) {
            case 1: hipExtLaunchKernelGGL((psfm_chain_step_batch_kernel<1, true, true>), grid, block, 0, s, e0, e1, 0, tab_dev, frame); break;
            case 2: hipExtLaunchKernelGGL((psfm_chain_step_batch_kernel<2, true, true>), grid, block, 0, s, e0, e1, 0, tab_dev, frame); break;
            case 4: hipExtLaunchKernelGGL((psfm_chain_step_batch_kernel<4, true, true>), grid, block, 0, s, e0, e1, 0, tab_dev, frame); break;
            default: hipExtLaunchKernelGGL((psfm_chain_step_batch_kernel<0, true, true>), grid, block, 0, s, e0, e1, 0, tab_dev, frame); break;
        }
    } else {
        switch (ratio) {
            case 1: hipExtLaunchKernelGGL((psfm_chain_step_batch_kernel<1, false, true>), grid, block, 0, s, e0, e1, 0, tab_dev, frame); break;
            case 2: hipExtLaunchKernelGGL((psfm_chain_step_batch_kernel<2, false, true>), grid, block, 0, s, e0, e1, 0, tab_dev, frame); break;
            case 4: hipExtLaunchKernelGGL((psfm_chain_step_batch_kernel<4, false, true>), grid, block, 0, s, e0, e1, 0, tab_dev, frame); break;
            default: hipExtLaunchKernelGGL((psfm_chain_step_batch_kernel<0, false, true>), grid, block, 0, s, e0, e1, 0, tab_dev, frame); break;
        }
    }
    PSFM_HIP(hipGetLastError());
    return PSFM_OK;
}
