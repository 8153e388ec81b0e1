// HOST driver of particle-sfm_amd/csrc/psfm_ground_truth.h for tests/test_ground_truth_host.py: the arithmetic of pg_eval_kernel and
// pg_vote_kernel (eval_traj_iou.py:53-108, prepare_flyingthings3d.py:89-108) compiled through tests/host/shim, with plain loops
// where the kernels have threads.  Built with -ffp-contract=off: every *_rn intrinsic is the IEEE operation it names.  Test
// infrastructure.
#include "psfm_ground_truth.h"

extern "C" void psfm_host_traj_eval_counts(const int* frame_ids, const double* xy, const uint8_t* labels, long n_points, const uint8_t* masks,
                                           const float* table, int n_frames, int h, int w, int64_t* counts)
{
    const float cw = (float)((w - 1) / 2.0), ch = (float)((h - 1) / 2.0);
    for (long i = 0; i < (long)n_frames * PSFM_GT_CLASSES; i++) counts[i] = 0;
    for (long p = 0; p < n_points; p++) {
        const int f = frame_ids[p];
        if (f < 0 || f >= n_frames) continue;
        const float v = psfm_gt_sample(masks + (int64_t)f * h * w, table, xy[2 * p], xy[2 * p + 1], cw, ch, h, w);
        counts[(int64_t)f * PSFM_GT_CLASSES + psfm_gt_class(labels[p], v)] += 1;
    }
}

// the sample itself (the exact-0.5 case is checked on the value, not only on the class)
extern "C" void psfm_host_gt_sample(const double* xy, long n, const uint8_t* mask, const float* table, int h, int w, float* out)
{
    const float cw = (float)((w - 1) / 2.0), ch = (float)((h - 1) / 2.0);
    for (long p = 0; p < n; p++) out[p] = psfm_gt_sample(mask, table, xy[2 * p], xy[2 * p + 1], cw, ch, h, w);
}

// returns 1 when a present point could not be read
extern "C" int psfm_host_traj_vote_labels(const double* xy, const double* mask_absent, const uint8_t* gts, long k, int n_frames, int h, int w,
                                          uint8_t* labels)
{
    bool bad = false;
    for (long i = 0; i < k; i++) labels[i] = psfm_gt_vote_row(xy + 2 * i * n_frames, mask_absent + i * n_frames, gts, n_frames, h, w, &bad);
    return bad ? 1 : 0;
}
