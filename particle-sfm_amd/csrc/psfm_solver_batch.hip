// psfm_solver_batch.hip -- the batched forms of the device-paced sequence (psfm_connect_batch, psfm_batch.hip): kernels over a table
// of sequences (PsfmBatchSeqOpt, psfm_pc_params.h) and their launchers.  A block does for its sequence what psfm_seq_kernel
// (psfm_solver_fused.hip) does for its only one: psfm_seq_body, psfm_pc_fused.h.
#include <string.h>
#include <hip/hip_ext.h>

#include "psfm_pc_fused.h"
#include "psfm_solver_internal.h"

// ------------------------------------------------------------------------------------------------
// B sequences per launch, of one frame size or each of its own -- a row holds its sequence's -- (psfm_connect_batch; run_particlesfm.py:168-176 walks a directory of sequences): a frame of a
// DAVIS / Sintel / ScanNet-sized sequence is a few hundred blocks -- 10-40 % of the device's block slots -- for one dependent chain
// of round trips.  blockIdx.y = sequence: every sequence keeps its own context (lanes, log, counters, tickets, control block), its
// own device-side program counter and K, so the sequences advance independently -- one may be continuing a solve while its
// neighbours take their next frame, a stalled or finished one turns its blocks into no-ops -- and the launches fill the machine.
// gridDim.x is a multiple of 8: block (x, y) sits on XCD x % 8, as psfm_xcd_tile assumes.
// ------------------------------------------------------------------------------------------------
template <int R, int WAVES>
__global__ __launch_bounds__(PC_BLOCK) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES)))
void psfm_seq_batch_kernel(const PsfmBatchSeqOpt* __restrict__ seqs, int launch_id)
{
    const PsfmBatchSeqOpt& q = seqs[blockIdx.y];
    // (the launch may cover fewer lanes than the table has: say so if it is not enough -- psfm_batch.hip runs the batch again then)
    if (blockIdx.x == 0 && threadIdx.x == 0 && q.a.ctr->n_lanes > (int)(gridDim.x * PC_BLOCK)) atomicOr(&q.a.ctr->overflow, 16);
    psfm_seq_body<R>(q.a, q.P, q.st, q.occ2_stride, q.n_flows, launch_id);
}

// behind the last solve of every sequence of a batch (what psfm_solve_flush does for one): the accepted iterate into the log
__global__ __launch_bounds__(PC_BLOCK) void psfm_pc_flush_batch_kernel(const PsfmBatchSeqOpt* __restrict__ seqs, int clear_sel)
{
    const PsfmBatchSeqOpt& q = seqs[blockIdx.y];
    if (q.n_flows < 2) return;
    PcParams P = q.P;
    pc_params_rebase(P, q.st, q.occ2_stride, q.n_flows - 1);
    if (*P.stall) return;
    if (clear_sel) { if (blockIdx.x == 0 && threadIdx.x == 0) *P.sel = 0; return; }
    const int m = *P.sel;
    if (m == 0) return;
    const int n = P.n_lanes_ptr ? min(*P.n_lanes_ptr, P.n_rows) : P.n_rows;
    for (int i = blockIdx.x * PC_BLOCK + threadIdx.x; i < n; i += gridDim.x * PC_BLOCK) {
        if (pc_participates(P, i, n)) {
            P.x1a[i] = pc_buf1(P, m)[i];
            P.x2a[i] = pc_buf2(P, m)[i];
        }
    }
}

// per-sequence device-side program counters of a batch, set by the host at a checkpoint (a redone solve, an adapted K):
// v[i] = {pc_frame, pc_phase, pc_owner, solve_K}; pc_frame -1 = leave sequence i alone, -2 = its K only (the device may be inside a
// solve of that sequence: continuation launches do not read K)
struct PsfmBatchPc { int v[PSFM_BATCH_MAX][4]; };
__global__ void psfm_batch_set_pc_kernel(const PsfmBatchSeqOpt* __restrict__ seqs, PsfmBatchPc pc, int n_seq)
{
    const int i = threadIdx.x;
    if (i >= n_seq || pc.v[i][0] == -1) return;
    PsfmCounters* ctr = seqs[i].a.ctr;
    if (pc.v[i][0] == -2) { ctr->solve_K = pc.v[i][3]; return; }
    ctr->pc_frame = pc.v[i][0]; ctr->pc_phase = pc.v[i][1]; ctr->pc_owner = pc.v[i][2]; ctr->solve_K = pc.v[i][3];
}

// a checkpoint of the batch in ONE device-to-host copy: every sequence's counters and the statistics of the solves of frames
// [lo[i], lo[i] + win) packed into out[i * row_bytes ..]
struct PsfmBatchWin { int lo[PSFM_BATCH_MAX]; };
__global__ __launch_bounds__(64) void psfm_batch_pack_kernel(const PsfmBatchSeqOpt* __restrict__ seqs, PsfmBatchWin w, int win, int row_bytes,
                                                            char* __restrict__ out)
{
    const PsfmBatchSeqOpt& q = seqs[blockIdx.x];
    char* dst = out + (size_t)blockIdx.x * row_bytes;
    const int* src = (const int*)q.a.ctr;
    for (int k = threadIdx.x; k < (int)(sizeof(PsfmCounters) / 4); k += 64) ((int*)dst)[k] = src[k];
    const int lo = w.lo[blockIdx.x];
    const int n = min(win, q.n_flows + 1 - lo);
    if (!q.P.stats_dev || n <= 0) return;
    const int* ssrc = (const int*)(q.P.stats_dev + lo);
    int* sdst = (int*)(dst + sizeof(PsfmCounters));
    for (int k = threadIdx.x; k < n * (int)(sizeof(psfm_solve_stats) / 4); k += 64) sdst[k] = ssrc[k];
}

// ---- batch (psfm_batch.hip): rows of the table, the batched launches ----
size_t psfm_batch_seq_opt_bytes(void) { return sizeof(PsfmBatchSeqOpt); }
psfm_status psfm_batch_fill_seq_opt(psfm_ctx* c, const PsfmTrackDims& d, const float* flows, const uint8_t* occ, int64_t occ_pitch,
                                    const float* flows_f2, const uint8_t* occ_s2, void* row_host, hipStream_t s)
{
    PsfmBatchSeqOpt* q = (PsfmBatchSeqOpt*)row_host;
    memset(q, 0, sizeof(*q));
    psfm_status rc = pc_seq_args(c, d, flows, occ, occ_pitch, flows_f2, occ_s2, q->P, q->a, q->st, s);
    if (rc != PSFM_OK) return rc;
    q->occ2_stride = (int64_t)d.H * d.W;
    q->n_flows = d.n_flows;
    return PSFM_OK;
}

psfm_status psfm_launch_seq_batch(psfm_ctx* owner, const void* tab_dev, int n_seq, int ratio, int64_t cap_max, int n_launches, int launch_id0,
                                  bool mb, hipStream_t s)
{
    if (mb) return psfm_launch_seq_batch_mb(owner, tab_dev, n_seq, ratio, cap_max, n_launches, launch_id0, s);      // (kernels of psfm_solver_batch_mb.hip)
    const unsigned gx = (unsigned)(((cap_max + PC_BLOCK - 1) / PC_BLOCK + 7) / 8 * 8);
    const dim3 grid(gx, (unsigned)n_seq), block(PC_BLOCK);
    const PsfmBatchSeqOpt* tab = (const PsfmBatchSeqOpt*)tab_dev;
    for (int k = 0; k < n_launches; ++k) {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        owner->prof.kernel_span(PSFM_PROF_SOLVER, &e0, &e1, true);
        const int id = launch_id0 + k;
#define PSFM_SEQ_BATCH_LAUNCH(R_) hipExtLaunchKernelGGL((psfm_seq_batch_kernel<R_, PSFM_SEQ_WAVES_DEFAULT>), grid, block, 0, s, e0, e1, 0, tab, id)
        PSFM_RATIO_DISPATCH(ratio, PSFM_SEQ_BATCH_LAUNCH)
#undef PSFM_SEQ_BATCH_LAUNCH
    }
    PSFM_HIP(hipGetLastError());
    return PSFM_OK;
}

psfm_status psfm_launch_flush_batch(const void* tab_dev, int n_seq, int64_t cap_max, hipStream_t s)
{
    int64_t nb = (cap_max + PC_BLOCK - 1) / PC_BLOCK;
    if (nb > 2048) nb = 2048;
    hipLaunchKernelGGL(psfm_pc_flush_batch_kernel, dim3((unsigned)nb, (unsigned)n_seq), dim3(PC_BLOCK), 0, s, (const PsfmBatchSeqOpt*)tab_dev, 0);
    hipLaunchKernelGGL(psfm_pc_flush_batch_kernel, dim3(1, (unsigned)n_seq), dim3(PC_BLOCK), 0, s, (const PsfmBatchSeqOpt*)tab_dev, 1);
    PSFM_HIP(hipGetLastError());
    return PSFM_OK;
}

psfm_status psfm_launch_batch_set_pc(const void* tab_dev, const int (*v)[4], int n_seq, hipStream_t s)
{
    PsfmBatchPc pc;
    memset(&pc, 0, sizeof(pc));
    for (int i = 0; i < PSFM_BATCH_MAX; ++i) pc.v[i][0] = -1;
    for (int i = 0; i < n_seq; ++i) for (int k = 0; k < 4; ++k) pc.v[i][k] = v[i][k];
    hipLaunchKernelGGL(psfm_batch_set_pc_kernel, dim3(1), dim3(PSFM_BATCH_MAX), 0, s, (const PsfmBatchSeqOpt*)tab_dev, pc, n_seq);
    PSFM_HIP(hipGetLastError());
    return PSFM_OK;
}

size_t psfm_batch_pack_row_bytes(int win) { return sizeof(PsfmCounters) + sizeof(psfm_solve_stats) * (size_t)win; }
psfm_status psfm_launch_batch_pack(const void* tab_dev, const int* lo, int n_seq, int win, char* out_dev, hipStream_t s)
{
    PsfmBatchWin w;
    memset(&w, 0, sizeof(w));
    for (int i = 0; i < n_seq; ++i) w.lo[i] = lo[i];
    hipLaunchKernelGGL(psfm_batch_pack_kernel, dim3((unsigned)n_seq), dim3(64), 0, s, (const PsfmBatchSeqOpt*)tab_dev, w, win,
                       (int)psfm_batch_pack_row_bytes(win), out_dev);
    PSFM_HIP(hipGetLastError());
    return PSFM_OK;
}
