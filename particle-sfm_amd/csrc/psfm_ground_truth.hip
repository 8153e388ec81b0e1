// psfm_ground_truth.hip -- trajectories against ground-truth masks, on the device.
//
//   psfm_traj_eval_counts   motion_seg/eval_traj_iou.py:79-115 (per_img_traj_metrics): the reference regroups every labelled point by
//                           frame in a Python loop, bilinearly samples the frame's mask at the frame's points and hands two boolean
//                           arrays to sklearn.  All four metrics are functions of the per-frame counts tp, fp, fn, tn; this is ONE
//                           launch over the labelled CSR that leaves those counts, as integers, in HBM.
//   psfm_traj_vote_labels   scripts/prepare_flyingthings3d.py:89-108 (find_traj_label): a trajectory's training label by majority
//                           vote of the mask at its rounded pixels -- a triple Python loop in the reference, one lane per row here.
// The arithmetic of both is psfm_ground_truth.h.
#include "psfm_ground_truth.h"
#include "psfm_internal.h"

#define PG_BLOCK 256
#define PG_ITEMS 16                  // points per thread: a block takes PG_BLOCK * PG_ITEMS consecutive points of the CSR
#define PG_TILE 256                  // frames of a block's LDS histogram, one per thread at the flush

struct PsfmGtTable { float v[256]; };

// One lane per point, in CSR order: adjacent lanes are consecutive frames of one trajectory, so the 4 + 16 + 1 input bytes per point
// are consecutive across a wave and a wave gathers from about as many masks as a trajectory has frames.  The counts are integers, so
// the order of accumulation cannot matter: a point adds 1 to its (frame, class) counter of the block's LDS histogram (the PG_TILE
// frames around the block's first point: the CSR lists trajectories by the window that brought them in, so a block's frames lie
// close together), and the block adds its non-zero counters to global memory with 64-bit integer atomics at the end.  A frame
// outside the tile (only when n_frames > PG_TILE) goes to global memory directly.
__global__ __launch_bounds__(PG_BLOCK) void pg_eval_kernel(const int* __restrict__ frame_ids, const double2* __restrict__ xy,
                                                          const uint8_t* __restrict__ labels, int64_t n_points,
                                                          const uint8_t* __restrict__ masks, PsfmGtTable table, int n_frames, int H, int W,
                                                          float cw, float ch, unsigned long long* __restrict__ counts)
{
    __shared__ float s_table[256];
    __shared__ unsigned s_hist[PG_TILE * PSFM_GT_CLASSES];
    const int tid = threadIdx.x;
    s_table[tid] = table.v[tid];
#pragma unroll
    for (int c = 0; c < PSFM_GT_CLASSES; c++) s_hist[c * PG_TILE + tid] = 0u;
    const int64_t p0 = (int64_t)blockIdx.x * (PG_BLOCK * PG_ITEMS);
    int tile0 = 0;
    if (n_frames > PG_TILE) {        // (uniform over the block; p0 < n_points by the size of the grid)
        tile0 = frame_ids[p0] - PG_TILE / 2;
        tile0 = min(max(tile0, 0), n_frames - PG_TILE);
    }
    __syncthreads();
    const int64_t hw = (int64_t)H * W;
    for (int it = 0; it < PG_ITEMS; it++) {
        const int64_t p = p0 + it * PG_BLOCK + tid;
        if (p >= n_points) break;
        const int f = frame_ids[p];
        if (f < 0 || f >= n_frames) continue;                 // a point of no frame: ignored, nothing read
        const double2 q = xy[p];
        const float v = psfm_gt_sample(masks + f * hw, s_table, q.x, q.y, cw, ch, H, W);
        const int cls = psfm_gt_class(labels[p], v);
        const unsigned r = (unsigned)(f - tile0);
        if (r < (unsigned)PG_TILE) atomicAdd(&s_hist[cls * PG_TILE + r], 1u);
        else atomicAdd(&counts[(int64_t)f * PSFM_GT_CLASSES + cls], 1ull);
    }
    __syncthreads();
    const int f = tile0 + tid;
    if (f < n_frames) {
#pragma unroll
        for (int c = 0; c < PSFM_GT_CLASSES; c++) {
            const unsigned n = s_hist[c * PG_TILE + tid];
            if (n) atomicAdd(&counts[(int64_t)f * PSFM_GT_CLASSES + c], (unsigned long long)n);
        }
    }
}

// One lane per trajectory: its row of the window tensors, column by column.
__global__ __launch_bounds__(PG_BLOCK) void pg_vote_kernel(const double* __restrict__ xy, const double* __restrict__ mask_absent,
                                                          const uint8_t* __restrict__ gts, int64_t k, int L, int H, int W,
                                                          uint8_t* __restrict__ labels, int* __restrict__ flag)
{
    const int64_t i = (int64_t)blockIdx.x * PG_BLOCK + threadIdx.x;
    if (i >= k) return;
    bool bad = false;
    labels[i] = psfm_gt_vote_row(xy + 2 * i * L, mask_absent + i * L, gts, L, H, W, &bad);
    if (bad) *flag = 1;              // a present point outside the image: reported by the host after the launch
}

extern "C" psfm_status psfm_traj_eval_counts(psfm_ctx* c, const int32_t* frame_ids, const double* xy, const uint8_t* labels, int64_t n_points,
                                             const uint8_t* masks_u8, const float* table_host, int n_frames, int h, int w, int64_t* counts_out,
                                             void* stream)
{
    if (!c) { psfm_set_error("ctx is NULL"); return PSFM_ERR_ARG; }
    const int given = (frame_ids != nullptr) + (xy != nullptr) + (labels != nullptr);
    if (given == 0) {                // the labelled set of psfm_labels_finish
        if (!c->lb_finished) { psfm_set_error("psfm_traj_eval_counts: no labelled set in the context (psfm_labels_finish)"); return PSFM_ERR_ARG; }
        frame_ids = c->lb_frames.as<int32_t>(); xy = c->lb_xy.as<double>(); labels = c->lb_labels.as<uint8_t>();
        n_points = c->lb_n_points;
    } else if (given != 3) {
        psfm_set_error("psfm_traj_eval_counts: frame_ids, xy and labels must be given together (or all NULL: the context's labelled set)");
        return PSFM_ERR_ARG;
    }
    // h, w >= 2: the sampler divides by (w-1)/2; a mask is reached as base + a 32-bit byte offset (psfm_frame_ok)
    if (n_points < 0 || n_frames < 1 || !psfm_frame_ok(h, w) || n_points > (int64_t)INT32_MAX * (PG_BLOCK * PG_ITEMS)) {
        psfm_set_error("psfm_traj_eval_counts: bad argument (n_points=%lld n_frames=%d h=%d w=%d)", (long long)n_points, n_frames, h, w);
        return PSFM_ERR_ARG;
    }
    if (!masks_u8 || !table_host || !counts_out) { psfm_set_error("psfm_traj_eval_counts: NULL argument"); return PSFM_ERR_ARG; }
    PSFM_HIP(hipSetDevice(c->device));
    PsfmGate gate(c->device, 0);
    hipStream_t s = (hipStream_t)stream;
    PSFM_HIP(hipMemsetAsync(counts_out, 0, sizeof(int64_t) * PSFM_GT_CLASSES * (size_t)n_frames, s));
    if (n_points == 0) return PSFM_OK;
    PsfmGtTable table;
    for (int i = 0; i < 256; i++) table.v[i] = table_host[i];
    const int64_t per_block = PG_BLOCK * PG_ITEMS;
    hipLaunchKernelGGL(pg_eval_kernel, dim3((unsigned)((n_points + per_block - 1) / per_block)), dim3(PG_BLOCK), 0, s, (const int*)frame_ids,
                       (const double2*)xy, labels, n_points, masks_u8, table, n_frames, h, w, (float)((w - 1) / 2.0), (float)((h - 1) / 2.0),
                       (unsigned long long*)counts_out);
    PSFM_HIP(hipGetLastError());
    return PSFM_OK;
}

extern "C" psfm_status psfm_traj_vote_labels(psfm_ctx* c, const double* xy, const double* mask_absent, const uint8_t* gts_u8, int64_t k,
                                             int n_frames, int h, int w, uint8_t* labels_out, void* stream)
{
    if (!c) { psfm_set_error("ctx is NULL"); return PSFM_ERR_ARG; }
    // 32-bit indices in the kernel: a pixel index below h*w; the grid
    if (k < 0 || n_frames < 1 || h < 1 || w < 1 || (int64_t)h * w > INT32_MAX || k > (int64_t)INT32_MAX * PG_BLOCK) {
        psfm_set_error("psfm_traj_vote_labels: bad argument (k=%lld n_frames=%d h=%d w=%d)", (long long)k, n_frames, h, w);
        return PSFM_ERR_ARG;
    }
    if (k == 0) return PSFM_OK;
    if (!xy || !mask_absent || !gts_u8 || !labels_out) { psfm_set_error("psfm_traj_vote_labels: NULL argument"); return PSFM_ERR_ARG; }
    PSFM_HIP(hipSetDevice(c->device));
    PsfmGate gate(c->device, 0);
    hipStream_t s = (hipStream_t)stream;
    psfm_status st;
    if ((st = c->gt_flag.ensure(256)) != PSFM_OK) return st;
    PSFM_HIP(hipMemsetAsync(c->gt_flag.p, 0, 4, s));
    hipLaunchKernelGGL(pg_vote_kernel, dim3((unsigned)((k + PG_BLOCK - 1) / PG_BLOCK)), dim3(PG_BLOCK), 0, s, xy, mask_absent, gts_u8, k, n_frames,
                       h, w, labels_out, c->gt_flag.as<int>());
    PSFM_HIP(hipGetLastError());
    int* flag_host = (int*)((char*)c->host_pinned + 352);      // (a free word of the pinned staging block)
    *flag_host = 0;
    PSFM_HIP(hipMemcpyAsync(flag_host, c->gt_flag.p, 4, hipMemcpyDeviceToHost, s));
    PSFM_HIP(hipStreamSynchronize(s));
    if (*flag_host != 0) {
        psfm_set_error("psfm_traj_vote_labels: a present point lies outside the %d x %d map (or is not finite); labels_out is unspecified", h, w);
        return PSFM_ERR_ARG;
    }
    return PSFM_OK;
}
