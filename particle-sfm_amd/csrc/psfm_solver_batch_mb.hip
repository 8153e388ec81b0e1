// psfm_solver_batch_mb.hip -- the batched device-paced sequence (psfm_solver_batch.hip) with the motion-boundary verdict in its chain
// step: psfm_seq_batch_kernel<R, WAVES, MB = true>, what psfm_connect_batch launches when every context of the batch has
// psfm_ctx_set_motion_boundary on.  The row's `a.occ` is then the sequence's KILL MAP (psfm_motion_boundary.h: bit 0 occlusion, bit 1
// motion boundary); the solve reads only the stride-2 occlusion maps, which stay 0/1.
// This form reads the device-side program counter into scalars and replays Ceres' control flow on ONE copy of the control block in LDS
// (psfm_seq_body<R, true>, pc_fused_replay_lds: psfm_pc_fused.h): no scratch at four waves per SIMD, a quarter of the twin's LDS.
// A translation unit of its own: psfm_solver_batch.hip keeps the kernels it had, byte for byte (tests/test_solver_resources.py counts
// them), and the MB = false template there keeps its two arguments.
#include <hip/hip_ext.h>

#include "psfm_pc_fused.h"
#include "psfm_solver_internal.h"

template <int R, int WAVES, bool MB>
__global__ __launch_bounds__(PC_BLOCK) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES)))
void psfm_seq_batch_kernel(const PsfmBatchSeqOpt* __restrict__ seqs, int launch_id)
{
    static_assert(MB, "the MB = false form is psfm_seq_batch_kernel<R, WAVES> of psfm_solver_batch.hip");
    const PsfmBatchSeqOpt& q = seqs[blockIdx.y];
    // (as in psfm_solver_batch.hip: a launch that covers fewer lanes than the sequence has in use says so)
    if (blockIdx.x == 0 && threadIdx.x == 0 && q.a.ctr->n_lanes > (int)(gridDim.x * PC_BLOCK)) atomicOr(&q.a.ctr->overflow, 16);
    psfm_seq_body<R, MB>(q.a, q.P, q.st, q.occ2_stride, q.n_flows, launch_id);
}

psfm_status psfm_launch_seq_batch_mb(psfm_ctx* owner, const void* tab_dev, int n_seq, int ratio, int64_t cap_max, int n_launches, int launch_id0,
                                     hipStream_t s)
{
    const unsigned gx = (unsigned)(((cap_max + PC_BLOCK - 1) / PC_BLOCK + 7) / 8 * 8);
    const dim3 grid(gx, (unsigned)n_seq), block(PC_BLOCK);
    const PsfmBatchSeqOpt* tab = (const PsfmBatchSeqOpt*)tab_dev;
    for (int k = 0; k < n_launches; ++k) {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        owner->prof.kernel_span(PSFM_PROF_SOLVER, &e0, &e1, true);
        const int id = launch_id0 + k;
#define PSFM_SEQ_BATCH_MB_LAUNCH(R_) hipExtLaunchKernelGGL((psfm_seq_batch_kernel<R_, PSFM_SEQ_WAVES_DEFAULT, true>), grid, block, 0, s, e0, e1, 0, tab, id)
        PSFM_RATIO_DISPATCH(ratio, PSFM_SEQ_BATCH_MB_LAUNCH)
#undef PSFM_SEQ_BATCH_MB_LAUNCH
    }
    PSFM_HIP(hipGetLastError());
    return PSFM_OK;
}
