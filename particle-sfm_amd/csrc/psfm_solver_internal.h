// psfm_solver_internal.h -- host-side declarations the units of the path-consistency solver share.  A kernel is launched only by the
// unit that defines it; the other units call its launcher.  (What other drivers call: psfm_internal.h.)
#pragma once
#include "psfm_pc_params.h"

// ---- psfm_solver.hip: the launch chain, the resident solve, the host driver of a solve ----
psfm_status pc_workspace(psfm_ctx* c, int64_t rows, int n_buf);
psfm_status pc_frame_params(psfm_ctx* c, const PsfmTrackDims& d, const float* flow01, const float* flow12,
                            const float* flow02, const uint8_t* occ02, int frame, PcParams& P, hipStream_t s);

// ---- psfm_solver_fused.hip ----
psfm_status pc_fused_workspace(psfm_ctx* c, const PsfmTrackDims& d, PcParams& P, int K, hipStream_t s, bool zero_tickets = false);
psfm_status pc_launch_fused_export(psfm_ctx* c, const PsfmTrackDims& d, PcParams& P, int K, hipStream_t s);
psfm_status pc_seq_args(psfm_ctx* c, const PsfmTrackDims& d, const float* flows, const uint8_t* occ, int64_t occ_pitch,
                        const float* flows_f2, const uint8_t* occ_s2, PcParams& P, PsfmChainArgs& a, PsfmSeqStride& st, hipStream_t s);

// LAUNCH_(R) with the kernel instantiation of the sample ratio: R = 1, 2, 4 for those ratios, 0 (the generic form) for any other
#define PSFM_RATIO_DISPATCH(ratio_, LAUNCH_) \
    switch (ratio_) { case 1: LAUNCH_(1); break; case 2: LAUNCH_(2); break; case 4: LAUNCH_(4); break; default: LAUNCH_(0); break; }
