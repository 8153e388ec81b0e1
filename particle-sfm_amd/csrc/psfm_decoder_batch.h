// psfm_decoder_batch.h -- the windows of a sequence through ONE sequence of decoder launches (psfm_traj_decode_batch): the table of
// windows that travels by value in the kernel arguments, the flattened tile and slice maps, the lookup a block performs, and the
// plan with section NAMES in place of addresses that a block resolves for its window.  Shared by the kernels (psfm_decoder.hip)
// and the host build of the CPU suite (tests/host/decoder_batch_host.cpp through tests/host/shim).
//
// InstanceNorm and both softmaxes run over the k points of ONE window, so windows cannot be concatenated: every window keeps its own
// k, its own workspace (the layout of psfm_dec_workspace(k[b]), one after another on 256-byte boundaries), its own tiles (64 points,
// numbered from 0 inside the window) and its own partial-sum rows.  What a block computes, and in which order, is what the same
// block of psfm_traj_decode on that window alone computes: the results are bit-identical.
//   layer, pool    a 1-D grid over the tiles (slices) of all windows, window-major; block -> (window, tile in the window) by
//                  psfm_dec_batch_find over the table's first-tile (first-slice) column
//   statistics     grid (128, n_win);  softmax: grid (100, n_win);  l2: grid (n_win): blockIdx.y (blockIdx.x) is the window
// A window with k = 0 owns no tile and no slice; its blocks of the per-window grids return at once.
#pragma once
#include "psfm_decoder.h"

#define PSFM_DEC_BATCH_MAX 64           // windows per call (the bound of psfm_connect_batch); the Python layer splits longer lists

// The table of windows: columns, so that a block scans one of them with wide scalar loads.  Entries at and above n_win: k = 0,
// first tile = first slice = INT32_MAX (the lookup never lands there), pointers NULL.
struct PsfmDecBatch {
    const float* enc[PSFM_DEC_BATCH_MAX];       // [16][k] f32
    float* logits[PSFM_DEC_BATCH_MAX];          // each may be NULL
    float* prob[PSFM_DEC_BATCH_MAX];
    uint8_t* pred[PSFM_DEC_BATCH_MAX];
    size_t ws_off[PSFM_DEC_BATCH_MAX];          // the window's workspace inside `ws`, a multiple of 256
    int k[PSFM_DEC_BATCH_MAX];
    int tile0[PSFM_DEC_BATCH_MAX];              // tiles of the windows before this one
    int slice0[PSFM_DEC_BATCH_MAX];             // slices of the windows before this one
    int n_win, tiles, slices;                   // tiles, slices: of all windows = the two 1-D grids
    char* ws;
};
static_assert(sizeof(PsfmDecBatch) + sizeof(PsfmDecLayer) <= 4096, "the table and a layer must fit the kernel arguments");

enum { PSFM_DEC_BATCH_OK = 0, PSFM_DEC_BATCH_BAD_N = 1, PSFM_DEC_BATCH_BAD_K = 2 };

// k[0 .. n_win) -> the table's k, ws_off, tile0, slice0, n_win, tiles, slices (pointers cleared; the caller fills them) and the
// workspace bytes of the whole batch.  PSFM_DEC_BATCH_BAD_N: n_win outside [0, 64]; PSFM_DEC_BATCH_BAD_K: window `bad` is the first
// with k < 0, k == 1 or k above PSFM_DEC_MAX_K.  On refusal `total` is 0.
inline int psfm_dec_batch_layout(PsfmDecBatch& B, const int64_t* k, int n_win, size_t& total, int& bad)
{
    total = 0; bad = -1;
    if (n_win < 0 || n_win > PSFM_DEC_BATCH_MAX) return PSFM_DEC_BATCH_BAD_N;
    for (int b = 0; b < n_win; b++)
        if (k[b] < 0 || k[b] == 1 || k[b] > PSFM_DEC_MAX_K) { bad = b; return PSFM_DEC_BATCH_BAD_K; }
    size_t off = 0;
    int tiles = 0, slices = 0;
    for (int b = 0; b < PSFM_DEC_BATCH_MAX; b++) {
        const bool in = b < n_win;
        const PsfmDecWs L = psfm_dec_workspace(in ? k[b] : 0);
        B.enc[b] = 0; B.logits[b] = 0; B.prob[b] = 0; B.pred[b] = 0;
        B.k[b] = in ? (int)k[b] : 0;
        B.ws_off[b] = off;
        B.tile0[b] = in ? tiles : INT32_MAX;
        B.slice0[b] = in ? slices : INT32_MAX;
        if (in && k[b] > 0) { off += L.total; tiles += L.nb; slices += L.nb2; }         // (L.total is a multiple of 256)
    }
    B.n_win = n_win; B.tiles = tiles; B.slices = slices; B.ws = 0;
    total = off;
    return PSFM_DEC_BATCH_OK;
}

// The window of block `blk` of a flattened grid: the LAST entry of `first` (tile0 or slice0, all 64 entries) that is <= blk.  The
// column never decreases (the padding is INT32_MAX), so that is the number of entries <= blk, less one.  An empty window repeats its
// successor's entry, so the last of a run of equal entries is the window that owns the block.  `blk` is the same in every lane of a
// block (blockIdx.x) and `first` lies in the kernel arguments: 64 scalar compares, no divergence.
__host__ __device__ __forceinline__ int psfm_dec_batch_find(const int* first, int blk)
{
    int n = 0;
#pragma unroll
    for (int i = 0; i < PSFM_DEC_BATCH_MAX; i++) n += first[i] <= blk ? 1 : 0;
    return n - 1;
}

// ---- the plan by section names ------------------------------------------------------------------------------------------------
// psfm_dec_plan_at is given, in place of the address of a workspace section (or of the encoding), its NAME: the section's number
// shifted above every offset that the plan adds to it (the widest is a statistics slot inside stat_fin).  A block turns a name back
// into the address in its own window with psfm_dec_resolve.  NULL stays NULL (a segment without statistics, no residual).  The
// weights are shared by all windows and stay addresses.
enum { PSFM_DEC_SEC_A = 1, PSFM_DEC_SEC_T, PSFM_DEC_SEC_X1, PSFM_DEC_SEC_XUP, PSFM_DEC_SEC_EMB, PSFM_DEC_SEC_STAT_PART, PSFM_DEC_SEC_STAT_FIN,
       PSFM_DEC_SEC_SM_PART, PSFM_DEC_SEC_SM_FIN, PSFM_DEC_SEC_POOL_PART, PSFM_DEC_SEC_X2, PSFM_DEC_SEC_ENC };
#define PSFM_DEC_SEC_SHIFT 40

__host__ __device__ __forceinline__ char* psfm_dec_name(int sec) { return (char*)((uintptr_t)sec << PSFM_DEC_SEC_SHIFT); }

inline void psfm_dec_plan_names(PsfmDecPlan& P, const float* w)
{
    const PsfmDecBufs B = {psfm_dec_name(PSFM_DEC_SEC_A), psfm_dec_name(PSFM_DEC_SEC_T), psfm_dec_name(PSFM_DEC_SEC_X1),
                           psfm_dec_name(PSFM_DEC_SEC_XUP), psfm_dec_name(PSFM_DEC_SEC_EMB), psfm_dec_name(PSFM_DEC_SEC_STAT_PART),
                           psfm_dec_name(PSFM_DEC_SEC_STAT_FIN), psfm_dec_name(PSFM_DEC_SEC_SM_PART), psfm_dec_name(PSFM_DEC_SEC_SM_FIN),
                           psfm_dec_name(PSFM_DEC_SEC_POOL_PART), psfm_dec_name(PSFM_DEC_SEC_X2)};
    psfm_dec_plan_at(P, (const float*)psfm_dec_name(PSFM_DEC_SEC_ENC), w, B, 0, 0, 0);
    P.nb = P.nb2 = 0; P.k = 0;
}

// One window as a block sees it: its k, its layout, where its workspace and its encoding begin.
struct PsfmDecWin {
    int k;
    PsfmDecWs L;
    char* base;
    const float* enc;
};

__host__ __device__ __forceinline__ PsfmDecWin psfm_dec_batch_window(const PsfmDecBatch& B, int b)
{
    PsfmDecWin W;
    W.k = B.k[b];
    W.L = psfm_dec_workspace(W.k);
    W.base = B.ws + B.ws_off[b];
    W.enc = B.enc[b];
    return W;
}

template <class T>
__host__ __device__ __forceinline__ T* psfm_dec_resolve(T* name, const PsfmDecWin& W)
{
    const uintptr_t v = (uintptr_t)name;
    if (!v) return 0;
    const int sec = (int)(v >> PSFM_DEC_SEC_SHIFT);
    const size_t delta = (size_t)(v & (((uintptr_t)1 << PSFM_DEC_SEC_SHIFT) - 1));
    if (sec == PSFM_DEC_SEC_ENC) return (T*)((char*)W.enc + delta);
    const PsfmDecWs& L = W.L;
    const size_t off = sec == PSFM_DEC_SEC_A ? L.a : sec == PSFM_DEC_SEC_T ? L.t : sec == PSFM_DEC_SEC_X1 ? L.x1 : sec == PSFM_DEC_SEC_XUP ? L.xup
                     : sec == PSFM_DEC_SEC_EMB ? L.emb : sec == PSFM_DEC_SEC_STAT_PART ? L.stat_part : sec == PSFM_DEC_SEC_STAT_FIN ? L.stat_fin
                     : sec == PSFM_DEC_SEC_SM_PART ? L.sm_part : sec == PSFM_DEC_SEC_SM_FIN ? L.sm_fin : sec == PSFM_DEC_SEC_POOL_PART ? L.pool_part
                     : L.x2;
    return (T*)(W.base + off + delta);
}
