// HOST driver of particle-sfm_amd/csrc/psfm_augment.h for tests/test_augment_host.py: the arithmetic of psfm_traj_augment_kernel
// (the classifier's 10-channel input, traj_oa_depth.py:72-114) compiled through tests/host/shim, with a plain loop where the
// kernel has threads.  Built with -ffp-contract=off: every *_rn intrinsic is the IEEE operation it names.  Test infrastructure.
#include "psfm_augment.h"

extern "C" void psfm_host_traj_augment(const double* xy_norm, const double* mask_absent, const float* depth, long k, int n_frames, int h, int w,
                                       const float* kinv, float* out)
{
    PsfmAugKinv K;
    for (int i = 0; i < 9; i++) K.m[i] = kinv[i];
    const int total = (int)(k * n_frames);
    for (int e = 0; e < total; e++) {
        float v[PSFM_AUG_PLANES];
        psfm_aug_element(xy_norm, mask_absent, depth, e, e % n_frames, n_frames, h, w, K, v);
        for (int p = 0; p < PSFM_AUG_PLANES; p++) out[(int64_t)p * total + e] = v[p];
    }
}
