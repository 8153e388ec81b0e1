/*
 * psfm.h -- C ABI of libpsfm_hip.so: the MI355X (gfx950) implementation of
 * ParticleSfM's point-trajectory hot path.
 *
 * This is the drop-in boundary.  Every entry point replaces one interface of the
 * reference (paths relative to the reference root, bytedance/particle-sfm):
 *
 *   psfm_load_flo_stack     point_trajectory/utils.py:26-56         load_flows() / read_flo()
 *   psfm_flow_check         point_trajectory/utils.py:94-105        flow_check()
 *   psfm_grid_sample        point_trajectory/trajectory.py:25-37    grid_sample()
 *   psfm_optimize_location  point_trajectory/optimize/src/trajectory_optimize.cpp:30-96
 *                           (pybind entry: optimize/src/bindings.cc:31)
 *   psfm_track              point_trajectory/track.py:24-50          track()
 *                           point_trajectory/track_optimize.py:24-53 track_optimize()
 *                           (+ the IncrementalTrajectorySet / Trajectory bookkeeping they
 *                           drive: trajectory.py:98-194, optimize/src/trajectory_base.cpp:21-93)
 *   psfm_connect            point_trajectory/main_connect_point_trajectories.py:36-53 (flow_check + track[_optimize])
 *   psfm_connect_batch      the same for a batch of sequences: the loop of run_particlesfm.py:168-176
 *   psfm_result_*           the list of Trajectory objects those functions return and the
 *                           id / min-length rule of main_connect_point_trajectories.py:56-60
 *   psfm_result_set         the files the reference's stages hand over (np.load(track.npy) in motion_seg/load_cut_seq.py:46,
 *   psfm_load_track_npy     sfm/matches_from_flow.py:56): a trajectory set from elsewhere as the context's result
 *   psfm_traj_augment       motion_seg/core/network/traj_oa_depth.py:72-114 augment_traj() (the classifier's 10-channel input)
 *   psfm_traj_encode        motion_seg/core/network/traj_oa_depth.py:25-60 pt_transformer.forward() (joint_encoder, eval mode)
 *   psfm_traj_decode        motion_seg/core/network/oanet.py:13-206 OANBlock.forward() (traj_oa_depth.decoder, eval mode),
 *                           traj_oa_depth.py:124 torch.sigmoid, main_motion_segmentation.py:80 `> 0.5`
 *   psfm_labels_*           motion_seg/main_motion_segmentation.py:89-129 (per-window predictions -> labelled track.npy)
 *   psfm_traj_eval_counts   motion_seg/eval_traj_iou.py:53-115 per_img_traj_metrics() (labelled points against ground-truth masks)
 *   psfm_traj_vote_labels   scripts/prepare_flyingthings3d.py:89-108 find_traj_label() (a trajectory's training label)
 *
 * Conventions
 *   - plain C, no C++/torch types.  Every data pointer is a DEVICE pointer
 *     (HBM of the context's GPU) unless the name ends in `_host`.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  Kernels are
 *     enqueued on it; calls that must learn a data-dependent size (psfm_track) synchronise
 *     that stream before returning.
 *   - every function returns a psfm_status; on failure psfm_last_error() (thread local)
 *     describes it.  Nothing throws across this boundary and there is no CPU fallback:
 *     without a GPU every compute entry point fails with PSFM_ERR_HIP.
 *   - a psfm_ctx owns the device workspace (trajectory log, lane tables, results); it is
 *     not thread-safe, use one per host thread / stream.  The library keeps ONE piece of
 *     process-wide state: a shared/exclusive gate per device -- every entry point that launches
 *     work holds it shared, the persistent frame loop (psfm_ctx_set_chain_mode) holds it
 *     exclusively for its few milliseconds, because all of its blocks must be resident at once.
 *     Contexts on different devices never interact; last-error text is thread local.
 */
#ifndef PSFM_H_
#define PSFM_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PSFM_VERSION 141   /* round 5: psfm_connect_batch.  Not moved by later exports (psfm_ctx_set_batch_redo and psfm_connect_batch_census
                              among them): tests/test_abi_and_host.py pins the number, and callers find an export by its symbol */

typedef enum psfm_status {
    PSFM_OK = 0,
    PSFM_ERR_ARG = 1,       /* bad argument */
    PSFM_ERR_HIP = 2,       /* HIP runtime error (no device, OOM, launch failure) */
    PSFM_ERR_CAPACITY = 3,  /* lane / trajectory tables too small: raise psfm_ctx_set_capacity and retry */
    PSFM_ERR_SOLVER = 4     /* the trust-region loop did not terminate (a solve Ceres would end in FAILURE is NOT an error: like the reference, the parameters stay as they came in and psfm_solve_stats.termination says 5) */
} psfm_status;

typedef struct psfm_ctx psfm_ctx;

/* Termination codes of the path-consistency solve (Ceres 2.0.0 TerminationType detail). */
enum {
    PSFM_TERM_FUNCTION_TOL = 0,
    PSFM_TERM_PARAMETER_TOL = 1,
    PSFM_TERM_GRADIENT_TOL = 2,
    PSFM_TERM_MAX_ITER = 3,
    PSFM_TERM_MIN_RADIUS = 4,
    PSFM_TERM_FAILURE = 5
};

typedef struct psfm_solve_stats {
    int32_t iterations;        /* trust-region iterations (excluding iteration 0) */
    int32_t successful_steps;
    int32_t termination;       /* PSFM_TERM_* */
    int32_t dogleg_nonGN;      /* iterations whose step was not the pure Gauss-Newton step */
    double initial_cost;
    double final_cost;
} psfm_solve_stats;

typedef struct psfm_track_info {
    int64_t n_traj;            /* all trajectories, index == id (full_trajs order) */
    int64_t n_points;          /* sum of their lengths */
    int64_t n_lanes_peak;      /* peak number of lanes used (<= lane capacity): the high-water mark of the lane allocator, whose blocks
                                  take and return lanes concurrently inside one launch -- it may differ by a few lanes between two
                                  identical calls; no id, length or position depends on the lane a track sat in */
    int64_t lane_capacity;
    int64_t solver_iterations; /* total trust-region iterations over all frames (track_optimize) */
    int32_t n_solves;
    int32_t chain_mode;        /* how the frame recurrence ran: 1 one launch per frame, 2 one persistent launch, 3 one launch per
                                  frame for a whole batch of sequences (psfm_connect_batch), 4 one launch per direction over
                                  caller-given query points (psfm_track_queries), 5 one loop of launches over frames for query points
                                  with the path-consistency solve (psfm_track_queries_optimize), 6 one launch per direction over the
                                  query points of a whole batch of sequences (psfm_track_queries_batch), 7 one loop of launches over
                                  the steps of a whole batch of sequences with the multi-problem path-consistency solve
                                  (psfm_track_queries_optimize_batch), 8 one chain step per frame for the sequences that left a batch,
                                  their solves as the frame-mode multi-problem launch chain (psfm_connect_batch with
                                  psfm_ctx_set_batch_redo(ctxs[0], 1)) */
} psfm_track_info;

const char* psfm_last_error(void);
int psfm_version(void);

/* Number of visible HIP devices (0 when there is no GPU); never fails. */
int psfm_device_count(void);

psfm_status psfm_ctx_create(int device, psfm_ctx** out);
psfm_status psfm_ctx_destroy(psfm_ctx* ctx);

/* Lane table = lane_factor * (grid points); finished-trajectory table = max(traj_factor, n_flows/8) * (grid points).
 * Defaults 2.0 / 8.0.  psfm_track returns PSFM_ERR_CAPACITY when either overflows. */
psfm_status psfm_ctx_set_capacity(psfm_ctx* ctx, double lane_factor, double traj_factor);

/* How psfm_track / psfm_connect run the frame recurrence in track mode (flows_f2 == NULL):
 *   0 (default) by shape: ONE persistent launch for the whole sequence where that is the faster way on an MI355X
 *     (sample_ratio >= 2 and >= 100 k grid points; psfm_connect, which then also checks flow consistency inside that
 *     launch, additionally wants >= 400 k grid points and <= 6 pixels per grid point, e.g. 1080p at sample_ratio 2),
 *     one launch per frame elsewhere.  The persistent loop needs every lane of the stride-r grid resident at once
 *     (grid points <= 256 x resident blocks) and the device to itself; it hands over to per-frame launches by itself
 *     when it runs out of lanes or of patience at a barrier;
 *   1 one launch per frame always;  2 the persistent loop wherever it can run (waits for the device), per-frame elsewhere.
 * Results are identical in every mode.  track_optimize always uses one launch per frame (the solves sit in between). */
psfm_status psfm_ctx_set_chain_mode(psfm_ctx* ctx, int mode);

/* Motion-boundary termination of trajectories (trajectory.py:39-43,51-53 and the commented kill rule of :60, "for some in-the-wilds,
 * we use motion boundary"): enable != 0 makes psfm_track / psfm_connect on this context kill a track when
 * !valid | occ_cond | mb_cond, with mb_cond a second bilinear verdict (> 0.1) over motion_boundary(flow, thres) of the frame's own
 * flow.  Default off: nothing differs from the shipped rule.  thres must be finite and >= 0 (PSFM_ERR_ARG otherwise).
 * With the option on
 *   - both entry points run the recurrence with one launch per frame whatever psfm_ctx_set_chain_mode says (info->chain_mode == 1);
 *     the occlusion and motion-boundary masks travel as one byte per pixel in a stack owned by the context, built by one launch
 *     from the flows and the COMPLETE occlusion maps -- `occ` of the caller stays 0/1;
 *   - track_optimize runs a frame as two launches (chain step, then the solve in any of its forms);
 *   - psfm_connect_batch takes a batch whose contexts ALL have the option on (each context's own thres is honoured; its frame launches
 *     carry the second verdict, info->chain_mode == 3) and refuses one whose contexts disagree (PSFM_ERR_ARG);
 *   - psfm_shard_begin refuses the context (PSFM_ERR_ARG). */
psfm_status psfm_ctx_set_motion_boundary(psfm_ctx* ctx, int enable, float thres);

/* trajectory.py:39-43 for a stack of flow maps: mb_out[f,y,x] = 1 where the flow gradient of pixel (x, y) of map f exceeds
 * thres x the flow's norm, else 0 (the rule, operation by operation: csrc/psfm_motion_boundary.h).
 *   flows (n,H,W,2) f32      mb_out (n,H,W) u8
 * Asynchronous on `stream`; identical calls give identical bytes. */
psfm_status psfm_motion_boundary(psfm_ctx* ctx, const float* flows, int n, int h, int w, float thres, uint8_t* mb_out, void* stream);

/* The kill maps psfm_track / psfm_connect sample with the option on, from the same launch that builds them there:
 * kill_out[f,y,x] = (occ[f,y,x] != 0) | motion boundary << 1.  occ (n,H,W) u8 is read only; kill_out must not alias it.
 * Asynchronous on `stream`. */
psfm_status psfm_kill_map(psfm_ctx* ctx, const float* flows, const uint8_t* occ, int n, int h, int w, float thres, uint8_t* kill_out,
                          void* stream);

/* psfm_kill_map for n_seq (1..64) stacks of the SAME frame size in ONE launch, restricted to frames [pair0, pair0 + n_pairs) of every
 * stack: what psfm_connect_batch enqueues behind each chunk of flow_check when its contexts have the option on.
 *   flows[i] (n_flows[i],H,W,2) f32, occ[i] / kill_out[i] (n_flows[i],H,W) u8, thres[i]: stack i's own threshold
 * A stack with fewer frames than pair0 + n_pairs is touched only where it has frames.  Every byte written equals psfm_kill_map's on
 * that stack alone.  The range is a contract: the call reads the occlusion bytes of the frames of the range only and writes the kill
 * bytes of exactly those frames; the flows it uses are those frames' (it may LOAD flow values of the following frame of the same
 * stack that it never uses, never anything outside the stack).  The frames outside the range may therefore be unwritten or in
 * production while the call runs.  PSFM_ERR_ARG, with nothing written: a NULL pointer (an array or one of its entries), n_seq outside
 * 1..64, a bad frame size, a negative n_flows[i], a negative or non-finite threshold, pair0 < 0 or n_pairs < 0.
 * `ctx` keeps the table of stacks.  Asynchronous on `stream`. */
psfm_status psfm_kill_map_batch(psfm_ctx* ctx, const float* const* flows, const uint8_t* const* occ, const int* n_flows, int n_seq, int h,
                                int w, const float* thres, int pair0, int n_pairs, uint8_t* const* kill_out, void* stream);

/* How psfm_track / psfm_connect run the path-consistency solve of a frame (track_optimize.py:49-50 ->
 * trajectory_optimize.cpp:74-82) -- the results do not depend on it:
 *   mode 0 (default) adaptive: the FUSED solve -- one launch per frame (the frame's chain step included) that speculates k
 *     trust-region iterations taking the Gauss-Newton step and being accepted, and replays Ceres' control flow over their
 *     sums; a solve that is not over after k accepted iterations gets a continuation launch (decided on the device) --
 *     while the solves of a sequence go that way; the launch CHAIN (one launch per trust-region iteration, any dogleg case,
 *     rejections) for windows of frames whose solves do not; a fused solve that meets a rejection / a dogleg interpolation /
 *     an invalid step is redone by the chain;
 *   mode 1 the chain always;  mode 2 the fused solve always (+ redo).
 *   k: iterations per fused launch, 0 = follow what the sequence needs (accepted steps + 1), at most 8. */
psfm_status psfm_ctx_set_solver(psfm_ctx* ctx, int mode, int k);
/* Solves of the last psfm_track / psfm_connect by how they ran: fused and done in one launch, fused then redone by
 * the chain, chain.  k_now: the adaptive iterations per fused launch after that sequence.  Any pointer may be NULL. */
psfm_status psfm_solver_counters(psfm_ctx* ctx, int64_t* fused, int64_t* fused_redone, int64_t* chain, int32_t* k_now);

/* Solves that reject steps run their whole trust-region loop as ONE resident launch whose blocks must all be on the device at once
 * (two 256-thread blocks per CU: psfm_resident_capacity, 512 on an MI355X).  By default a call only does that when it has the device
 * to itself (the exclusive gate): sequences processed concurrently by several host threads fall back to one launch per trust-region
 * iteration, 3-5x slower on such flows.  psfm_ctx_set_resident_budget(ctx, n) with n > 0 lets this context's resident solves use at
 * most n blocks while OTHER contexts run theirs -- the caller guarantees that the budgets of all contexts in flight on the device add
 * up to at most the capacity (e.g. 4 worker threads x 128).  A launch that does not become co-resident after all (other work holding
 * the block slots) gives up at its spin limit and is redone with launches.  n = 0: the default policy.
 * What a budget may change: a budget below the solve's own block count (lane capacity / 256) makes the solver's launches smaller, and
 * the f64 sums over the tracks (cost, step norms, the dogleg's inner products) are then added in another grouping.  Every DECISION of
 * the trust-region loop has been the same with and without a budget on all tests (iterations, accepted steps, terminations: tested
 * against the unbudgeted run and the oracle, tests/test_gpu_solver.py::test_budget_below_the_solves_block_count); positions agree to
 * rounding (<= 1e-9 px), not bit for bit.  Ids and lengths never depend on it. */
psfm_status psfm_ctx_set_resident_budget(psfm_ctx* ctx, int blocks);
psfm_status psfm_resident_capacity(psfm_ctx* ctx, int32_t* blocks);

/* Launches of the last psfm_track / psfm_connect / psfm_optimize_location on the context for the solves that did NOT go as the fused
 * solve speculates: resident launches (one per solve: the trust-region loop with the tracks' state on chip -- needs the device to
 * itself), how many of them gave up their hand-off, launches of ONE trust-region iteration each (the launch chain).  Which kernel a
 * measured solver time belongs to.  Any pointer may be NULL. */
psfm_status psfm_solver_launches(psfm_ctx* ctx, int64_t* resident, int64_t* giveups, int64_t* iterations);

/* utils.py:94-105.  flows_f, flows_b: (n_pairs,H,W,2) f32 stacks in the .flo-native interleaved
 * layout.  occ_out: (n_pairs,H,W) u8 0/1.  err_out: (n_pairs,H,W) f32 or NULL (the reference
 * pipeline never consumes it).  Bit-exact with the reference's torch-CPU arithmetic. */
psfm_status psfm_flow_check(psfm_ctx* ctx, const float* flows_f, const float* flows_b, int n_pairs, int h,
                            int w, float thres, uint8_t* occ_out, float* err_out, void* stream);

/* utils.py:26-56 (load_flows / read_flo) for a whole stack, straight into HBM: the n Middlebury .flo files `paths_host` (12-byte header
 * {f32 202021.25, i32 w, i32 h} + h*w interleaved (u,v) f32 -- the layout the kernels read), all of frame size w x h, into
 * dst (n,H,W,2) f32 on the device.  n_threads reader threads -> a ring of pinned staging buffers owned by the context -> asynchronous
 * H2D copies; returns when the last copy has completed (`stream` is only used to order the copies behind what the caller enqueued).
 * A missing / foreign / truncated file or a frame of another size is PSFM_ERR_ARG with the file named in psfm_last_error(). */
psfm_status psfm_load_flo_stack(psfm_ctx* ctx, const char* const* paths_host, int n, int h, int w, float* dst, int n_threads, void* stream);

/* trajectory.py:25-37 on an (H,W,C) f32 map, C in {1,2}; xy: (n,2) f64; out: (n,C) f32. */
psfm_status psfm_grid_sample(psfm_ctx* ctx, const float* map_hwc, int c, int h, int w, const double* xy,
                             int64_t n, float* out, void* stream);

/* trajectory_optimize.cpp:30-96.  uv12 (n,4), ref1 (n,2), ref2 (n,2), scale (n), out (n,4): f64;
 * flow12: (H,W,2) f32 (the f64 force-cast of the reference is exact).  stats_host may be NULL.
 * Synchronises `stream` (the iteration count is data dependent). */
psfm_status psfm_optimize_location(psfm_ctx* ctx, const double* uv12, const double* ref1, const double* ref2,
                                   const double* scale, const float* flow12, int64_t n, int w, int h,
                                   double* out, psfm_solve_stats* stats_host, void* stream);

/* optimize/src/path_consistency_cost.h:42-59 + linear_interpolation.h:97-123 (over ceres::Grid2D's clamp-to-edge GetValue): what
 * ceres::AutoDiffCostFunction<PathConsistencyError, 6, 4>::Evaluate returns for each of the n residual blocks of
 * trajectory_optimize.cpp:56-65 at uv12 -- residuals (n,6) and jacobians (n,6,4) row-major, f64; either may be NULL.  The arithmetic is
 * the one the solver kernels run (csrc/psfm_pc_core.h); exported so that it can be checked without a solve around it.  Asynchronous on
 * `stream`. */
psfm_status psfm_path_consistency_eval(psfm_ctx* ctx, const double* uv12, const double* ref1, const double* ref2,
                                       const double* scale, const float* flow12, int64_t n, int w, int h,
                                       double* residuals, double* jacobians, void* stream);

/* The record sort of the id assignment (the reference's trajectory ids are the rank of a track by (death step, birth
 * frame, birth grid index), the order trajectory.py:129-158 appends to full_trajs in): n (key, value) pairs on the device, keys sorted
 * ascending by their bits [0, end_bit), 1 <= end_bit <= 32, STABLE; in place.  The kernels are the ones psfm_track / psfm_connect run
 * on their records (csrc/psfm_sort.hip); exported so that the sort can be checked on its own.  n < 2^31.  Asynchronous on `stream`. */
psfm_status psfm_sort_records(psfm_ctx* ctx, uint32_t* keys, int32_t* values, int64_t n, int end_bit, void* stream);

/* The same for keys of up to 64 bits, 1 <= end_bit <= 64 (the 8-byte instances of the same kernels: what the id assignment runs for
 * long or dense sequences and for batches whose sequence number does not fit beside a 32-bit key): ceil(end_bit / 8) passes, the bits
 * at and above end_bit order nothing and the keys leave whole.  STABLE; in place; n < 2^31.  Asynchronous on `stream`. */
psfm_status psfm_sort_records64(psfm_ctx* ctx, uint64_t* keys, int32_t* values, int64_t n, int end_bit, void* stream);

/* Which forms the LAST id assignment of this context ran (psfm_track / psfm_connect; for psfm_connect_batch: the context that owns the
 * batch, ctxs[0]) -- they give the same bytes, so nothing else tells them apart.
 *   sort_form     0 none yet, 1 this library's sort on 32-bit keys, 2 this library's sort on 64-bit keys, 3 rocPRIM's device sort
 *   offsets_form  0 none yet, 1 one-block group plan, 3 decode + scan over the trajectories (more than 16 384 (death, birth) groups:
 *                 n_flows > 178); 2 is kept for a chunked group plan, which was measured slower than 3 and is not built in
 * Reads host-side state only; either pointer may be NULL. */
psfm_status psfm_ctx_get_finalize_forms(psfm_ctx* ctx, int* sort_form, int* offsets_form);

/* Whether the LAST id assignment of this context ran the placed form: after the persistent frame loop, with 32-bit sort keys and
 * n_flows + 1 <= 256, the records are placed by birth order (which the loop knows) and sorted in ONE pass on the last valid time
 * instead of being compacted and sorted in four (csrc/psfm_place.h; PSFM_FIN_PLACE=0 in the environment keeps the four passes).
 * sort_form above reports 1 either way; the bytes of the result are the same.  *placed: 0 / 1.  Reads host-side state only. */
psfm_status psfm_ctx_get_finalize_placed(psfm_ctx* ctx, int* placed);

/* How the LAST id assignment of this context turned the persistent loop's flow log into positions.  *gather: 0 no flow log (the
 * per-frame kernels log positions), 1 one thread per trajectory adds the flows in the loop's order, 2 the lanes that store a
 * trajectory's 32 positions sum them as a prefix sum, and redo in the loop's order the chunks in which an addition could round
 * (csrc/psfm_gather_exact.h; frames up to 3840 pixels a side; PSFM_FIN_GATHER=0 in the environment keeps 1).  The bytes of the
 * result are the same.  Reads host-side state only. */
psfm_status psfm_ctx_get_finalize_gather(psfm_ctx* ctx, int* gather);

/* track.py:24-50 when flows_f2 == NULL, track_optimize.py:24-53 otherwise.
 *   flows    (n_flows,H,W,2) f32      occ     (n_flows,H,W) u8
 *   flows_f2 (n_flows-1,H,W,2) f32    occ_s2  (n_flows-1,H,W) u8        (stride-2 stacks)
 * Runs the whole frame recurrence and the id assignment on the device; the result stays in the
 * context (HBM) until the next psfm_track on it.  info_host may be NULL.  Synchronises `stream`. */
psfm_status psfm_track(psfm_ctx* ctx, const float* flows, const uint8_t* occ, const float* flows_f2,
                       const uint8_t* occ_s2, int n_flows, int h, int w, int sample_ratio,
                       psfm_track_info* info_host, void* stream);

/* The compute part of the stage entry main_connect_point_trajectories.py:36-53 in one call: flow_check of the
 * stride-1 stacks (and of the stride-2 stacks when flows_f2 != NULL) followed by track / track_optimize.
 *   - track mode with the device to itself (see psfm_ctx_set_chain_mode): ONE persistent launch that computes the
 *     occlusion maps and runs the recurrence -- the blocks check flow consistency in the time they would otherwise wait
 *     at the frame barriers (a caller-provided `occ` takes part when H*W is a multiple of 128, else the stand-alone
 *     kernel fills it first);
 *   - otherwise the maps are produced on an internal side stream while the frame loop consumes them.
 *   flows_f, flows_b   (n_flows,H,W,2) f32      flows_f2, flows_b2  (n_flows-1,H,W,2) f32 or NULL
 *   occ, occ_s2        optional outputs (n_flows,H,W) / (n_flows-1,H,W) u8; NULL = kept in the context
 * Result access as for psfm_track.  Synchronises `stream`.
 * Reproducibility: in track mode two identical calls give identical bytes.  With the stride-2 solve (flows_f2 != NULL; psfm_track
 * and psfm_connect_batch likewise) they give identical ids, births, lengths and solver decisions, but no promise is made for the
 * last bits: a solve's final_cost has been observed to differ by one unit in the last place between two identical calls (the
 * adaptive policy of psfm_ctx_set_solver carries over from call to call; and with the form forced, in psfm_connect_batch), and
 * positions are held to 1e-9 px between two runs, as between the batched and the single form. */
psfm_status psfm_connect(psfm_ctx* ctx, const float* flows_f, const float* flows_b, const float* flows_f2,
                         const float* flows_b2, int n_flows, int h, int w, float thres, int sample_ratio,
                         uint8_t* occ, uint8_t* occ_s2, psfm_track_info* info_host, void* stream);

/* Caller-given QUERY POINTS tracked through a flow stack: for every query q -- a position q_xy[q] at frame q_t[q],
 * 0 <= q_t[q] <= n_flows -- the body of track.py:37-47 for that one position: flow_sample = grid_sample(flows[f], p)
 * (trajectory.py:25-37), next, alive = step_forward(p, flow_sample, occ[f], mb) (trajectory.py:45-62), at f = t, t+1, ...; the track
 * ends at the first step that is not alive, or at frame n_flows.  No grid, no respawn, no id assignment: a query interacts with no
 * other track.  The kill rule is the shipped one (trajectory.py:61), or the motion-boundary form (:60) when the context has
 * psfm_ctx_set_motion_boundary on; the kill maps are then built from the stack being sampled.
 *   flows_f (n_flows,H,W,2) f32, occ_f (n_flows,H,W) u8   the forward stack and its occlusion maps, or both NULL
 *   flows_b, occ_b   the BACKWARD stack -- flows_b[f] is the flow from frame f+1 to frame f -- and ITS occlusion maps, that is
 *                    flow_check(flows_b, flows_f), or both NULL.  A query at frame t samples map t-1 and moves to frame t-1, down to 0
 *   q_xy (n_q,2) f64, q_t (n_q) i32   on the DEVICE
 * At least one stack must be given; maps are densely packed.  With both stacks a query is tracked both ways and the two halves are one
 * trajectory: points in ascending time, the query point once, birth = t - (len_b - 1), len = len_b + len_f - 1.
 * Queries outside the image are legal (all taps out of bounds, flow 0, next position invalid: length 1).  Refused with PSFM_ERR_ARG,
 * BEFORE anything is tracked and with the previous result intact: a query with a non-finite coordinate or a frame outside
 * [0, n_flows] -- psfm_last_error() names the first such index -- no stack or a stack without its maps, n_q outside [0, 2^28)
 * (a frame row of the position slab, 16 bytes per query, stays below 4 GB; checked before any allocation).
 * The result REPLACES the context's result set as psfm_track does -- trajectory i is query i, len >= 1; info->n_traj = n_q,
 * info->chain_mode = 4 -- and every consumer of a result works on it unchanged (psfm_result_device / _copy, psfm_result_filter /
 * _filtered_copy, psfm_window_sample, psfm_traj_to_matches, the label merge), except psfm_result_keys, whose key needs a birth grid
 * index: it refuses a query result (PSFM_ERR_ARG).  Identical calls give identical bytes.  Synchronises `stream`.
 * Out of scope: tracking through occlusion.  (Path consistency: psfm_track_queries_optimize; several sequences per call:
 * psfm_track_queries_batch.) */
psfm_status psfm_track_queries(psfm_ctx* ctx, const float* flows_f, const uint8_t* occ_f, const float* flows_b, const uint8_t* occ_b,
                               int n_flows, int h, int w, const double* q_xy, const int32_t* q_t, int64_t n_q,
                               psfm_track_info* info_host, void* stream);

/* psfm_track_queries WITH the stride-2 path-consistency solve every grid trajectory of track_optimize gets (track_optimize.py:49-50):
 * the reference's IncrementalTrajectorySet(buffer_size=3) fed with the queries of every frame (new_traj_all takes any points), then
 * the body of track_optimize.py:37-50.  Forward, for f = 0 .. n_flows-1:
 *   1. the queries with q_t == f become active (a query with q_t == n_flows never steps: length 1);
 *   2. every active query steps from its tail p_f exactly as in psfm_track_queries (motion-boundary form included); one that is not
 *      alive ends at its last position, one that is alive gets p_{f+1};
 *   3. if f >= 1, the active queries that now hold three positions p_{f-1}, p_f, p_{f+1} (alive, f + 1 - q_t >= 2) are the rows of ONE
 *      joint solve, built as optimize_buffer does (trajectory.py:161-194): flow01 = grid_sample(flows[f-1], p0),
 *      flow02 = grid_sample(flows_f2[f-1], p0), occ02 = grid_sample(occ_f2[f-1], p0), scale = (1 - occ02) * (|flow02| < 20) in fp32,
 *      ref1 = p0 + flow01, ref2 = p0 + flow02, uv12 = (p1, p2), cost map flows[f].  The result overwrites p_f and p_{f+1}; the next
 *      step starts from the optimised p_{f+1};
 *   4. at the end of the stack every active query ends.
 * The solve of a frame is JOINT over the call's queries -- Ceres' trust-region loop is global, as it is over the reference's active
 * set -- so a query's positions depend on its companions exactly as a grid track's do; rows are in query order.  A frame with no row
 * runs no solve (the reference's np.stack([]) raises there: the one deviation, on input the reference cannot handle).  The query point
 * itself (p0 of its first solve) is never moved.
 * Backward: the same engine on the time-reversed sequence -- the stride-1 stack is flows_b with ITS maps occ_b = flow_check(flows_b,
 * flows_f); the stride-2 stack is flows_b2 (flows_b2[f]: frame f+2 -> f) with ITS maps occ_b2 = flow_check(flows_b2, flows_f2).
 * Both: the halves are solved independently and joined as psfm_track_queries joins them.
 *   flows_f, occ_f, flows_f2 (n_flows-1,H,W,2), occ_f2 (n_flows-1,H,W)   the forward direction: all four, or none
 *   flows_b, occ_b, flows_b2, occ_b2                                      the backward direction: all four, or none
 * With n_flows == 1 no solve can happen and the stride-2 pointers may be NULL.  Refusals as psfm_track_queries (PSFM_ERR_ARG before
 * anything is tracked, the previous result intact, psfm_last_error() names the first bad query), and a direction whose stride-1
 * stack comes without its stride-2 stack while n_flows >= 2.  The result replaces the context's result set as psfm_track_queries'
 * does (trajectory i is query i, info->n_traj = n_q, a live label merge is void, psfm_result_keys refuses it); info->chain_mode = 5.
 * psfm_result_solve_stats: one entry per solve that ran, forward frames ascending, then backward frames in the order they ran
 * (descending).  The solve is the one psfm_optimize_location runs and honours psfm_ctx_set_solver / psfm_ctx_set_resident_budget as
 * it does.  One small device-to-host copy per frame (the row count).  Synchronises `stream`.  No promise of identical bytes from
 * identical calls is made here (psfm_track_queries_optimize_batch makes one for its launch-chain form): decisions are the same,
 * positions are held to 1e-9 px between two runs. */
psfm_status psfm_track_queries_optimize(psfm_ctx* ctx, const float* flows_f, const uint8_t* occ_f, const float* flows_f2,
                                        const uint8_t* occ_f2, const float* flows_b, const uint8_t* occ_b, const float* flows_b2,
                                        const uint8_t* occ_b2, int n_flows, int h, int w, const double* q_xy, const int32_t* q_t,
                                        int64_t n_q, psfm_track_info* info_host, void* stream);

/* psfm_track_queries for n_seq sequences in ONE call: sequence i -- its stacks, its frame size h[i] x w[i], its n_flows[i] maps, its
 * n_q[i] queries -- is tracked into ctxs[i], and there is NO new rule: afterwards context i holds byte for byte what
 * psfm_track_queries(ctxs[i], ... sequence i ...) would have left (birth, len, off, xy, the sizes; the result is marked as a query
 * result, so psfm_result_keys refuses it; a live label merge is void; the solve statistics are cleared and an unfinished sharded run
 * is abandoned), and every consumer runs unchanged, context by context (psfm_result_*, psfm_result_filter(_batch),
 * psfm_window_sample(_batch), psfm_traj_to_matches(_batch), the label merge).  infos_host[i].chain_mode = 6.
 *   ctxs[i]      one context per sequence, 1 <= n_seq <= 64, distinct, non-NULL, all on one device; ctxs[0] also owns the call's
 *                shared workspace
 *   flows_f, occ_f   both NULL, or both arrays of n_seq non-NULL pointers: a direction is given for the WHOLE batch.  The same for
 *                flows_b, occ_b (flows_b[i][f]: frame f+1 -> f, with ITS maps).  At least one direction
 *   n_flows[i] >= 1, h[i], w[i]   may differ from sequence to sequence
 *   q_xy[i] (n_q[i],2) f64, q_t[i] (n_q[i]) i32   on the DEVICE; n_q[i] == 0 is legal (that context gets the empty result, the others
 *                go on); all sequences together have fewer than 2^28 queries
 *   infos_host   n_seq entries or NULL
 * Motion boundary (psfm_ctx_set_motion_boundary): on in EVERY context of the batch, each with its own threshold, or in none.  With it
 * on the kill maps of each stack being sampled are built from that stack's own flows and maps into its context, one launch per stack,
 * before the tracking launch.
 * Refused with PSFM_ERR_ARG, BEFORE anything is tracked and with EVERY context untouched: n_seq out of range; a NULL, repeated or
 * foreign-device context; no direction, or a stack without its maps; a NULL entry in a given array; n_flows[i] < 1 or a bad frame
 * size; n_q[i] < 0, or n_q[i] > 0 with a NULL q_xy[i] or q_t[i]; 2^28 or more queries; contexts that disagree about the motion
 * boundary; a query with a non-finite coordinate or a frame outside [0, n_flows[i]] -- psfm_last_error() names the lowest such
 * sequence and the lowest such query inside it.
 * Three host synchronisations, as the single call: behind the validation, behind the per-sequence point totals, at the end (a batch
 * without any query has nothing to validate or track: two synchronisations around the table's copy, one launch for the empty results and the totals' copy).  Apart
 * from the kill maps the number of launches and copies does not depend on n_seq; psfm_query_batch_census reports both figures for
 * the last call that had `ctx` as ctxs[0] (the kill maps' launches are not counted).  Integer sums in a fixed order: identical calls
 * give identical bytes.  Synchronises `stream`.
 * (Path consistency for a batch of sequences: psfm_track_queries_optimize_batch.) */
psfm_status psfm_track_queries_batch(psfm_ctx* const* ctxs, int n_seq, const float* const* flows_f, const uint8_t* const* occ_f,
                                     const float* const* flows_b, const uint8_t* const* occ_b, const int* n_flows, const int* h,
                                     const int* w, const double* const* q_xy, const int32_t* const* q_t, const int64_t* n_q,
                                     psfm_track_info* infos_host, void* stream);
psfm_status psfm_query_batch_census(psfm_ctx* ctx, int32_t* launches, int32_t* host_syncs);

/* psfm_track_queries_optimize for n_seq sequences in ONE call: the query points of every sequence tracked with the stride-2
 * path-consistency solve after every step (track_optimize.py:49-50), with one set of launches per step for the whole batch.  The
 * arguments are psfm_track_queries_batch's plus the four stride-2 arrays:
 *   flows_f2[i] (n_flows[i]-1,H_i,W_i,2), occ_f2[i] (n_flows[i]-1,H_i,W_i)   with the forward direction
 *   flows_b2[i], occ_b2[i]                                                   with the backward direction (flows_b2[i][f]: frame f+2 -> f)
 * each an array of n_seq pointers or NULL for the whole batch, as the stride-1 arrays are; a sequence with n_flows[i] == 1 may have
 * NULL entries (no solve can happen in it).  Up to 64 sequences, each with its own frame size, length and query count (zero
 * included); one context per sequence, ctxs[0] owns the batch's shared workspace; the gate and the motion-boundary rule (on every
 * context or on none, each with its own threshold, one kill-map launch per stack) are psfm_track_queries_batch's.
 * Per direction and step k = 0 .. max(n_flows) - 1: one step launch over all sequences (the per-lane step of
 * psfm_track_queries_optimize; a sequence with n_flows[i] <= k does nothing), and from k = 1 on one scan launch (one block per
 * sequence) that leaves every sequence's row count in device memory, one rows launch that writes the solves' inputs in place, the
 * launch chain of the solver over the table of all sequences' problems -- iteration 0 and the trust-region iterations as one grid
 * (blocks, problems) per launch, a problem's block count computed on the device from its row count, every sum in the single solve's
 * order --, one poll (a small launch that packs every control block into pinned memory) with ONE synchronisation, further chunks of
 * iteration launches while any problem is left undone, then the write-back and the scatter.  The host never reads a row count.  At
 * the end one length scan and one CSR gather for all contexts.
 * Context i ends up with what psfm_track_queries_optimize(ctxs[i], ... sequence i ...) leaves: the result set (trajectory q is query
 * q, psfm_result_keys refuses it) and psfm_result_solve_stats -- one entry per solve that had rows, forward frames ascending, then
 * backward frames in the order they ran; the solves run as launches (no resident form), whose iterates are the resident form's bit
 * for bit.  infos_host[i].chain_mode = 7; n_solves and solver_iterations are sequence i's.
 * Refusals (PSFM_ERR_ARG before anything is tracked, every context untouched): those of psfm_track_queries_batch -- the lowest bad
 * sequence and its lowest bad query are named -- and those of psfm_track_queries_optimize: a stride-2 array without its occlusion
 * array or without the direction's stride-1 arrays; a sequence whose stride-2 stack comes without its maps; a direction whose
 * stride-1 stack lacks its stride-2 stack in a sequence with n_flows >= 2 (the sequence is named).
 * psfm_query_pc_batch_census: the last call that had `ctx` as ctxs[0] -- launches_fixed (kernels and copies that do not depend on
 * how the solves went nor on n_seq; the kill maps apart), launches_iter (trust-region iteration launches, each over all problems),
 * host_syncs (validation, one per poll, the point totals, the end).  Identical calls give identical bytes.  Synchronises `stream`.
 * Out of scope: the resident and fused solver forms for a batch; a device-paced frame loop (one synchronisation per step remains). */
psfm_status psfm_track_queries_optimize_batch(psfm_ctx* const* ctxs, int n_seq, const float* const* flows_f, const uint8_t* const* occ_f,
                                              const float* const* flows_f2, const uint8_t* const* occ_f2, const float* const* flows_b,
                                              const uint8_t* const* occ_b, const float* const* flows_b2, const uint8_t* const* occ_b2,
                                              const int* n_flows, const int* h, const int* w, const double* const* q_xy,
                                              const int32_t* const* q_t, const int64_t* n_q, psfm_track_info* infos_host, void* stream);
psfm_status psfm_query_pc_batch_census(psfm_ctx* ctx, int32_t* launches_fixed, int32_t* launches_iter, int32_t* host_syncs);

/* The loop of the reference's driver over a directory of sequences (run_particlesfm.py:168-176 -> connect_point_trajectory ->
 * main_connect_point_trajectories.py:36-53 per sequence) for n_seq sequences of one sample ratio (any lengths; one frame size h x w,
 * or with h = w = 0 a frame size per sequence, see below) in ONE call: psfm_connect for every one of them, with every frame launch covering the whole batch (block (x, y) = tile
 * x of sequence y).  A frame of a small sequence -- DAVIS, Sintel, ScanNet sizes -- is one dependent chain of memory round trips on
 * a few hundred of the device's block slots; a batch fills them.  One host synchronisation per window of 16 frames and one
 * segmented finalize (one sort) for all sequences.
 *   ctxs[i]      one context per sequence, all on one device, each given once; afterwards context i holds sequence i's result
 *                exactly as after psfm_connect (psfm_result_*, psfm_result_filter, psfm_traj_to_matches, psfm_window_sample work
 *                on it); ctxs[0] also owns the batch's shared workspace
 *   flows_f[i], flows_b[i]    (n_flows[i],H,W,2) f32      n_flows[i] >= 1
 *   flows_f2, flows_b2        NULL (track) or arrays of n_seq pointers to (n_flows[i]-1,H,W,2) stacks (track_optimize, every sequence)
 *   infos_host   n_seq entries or NULL
 * track_optimize: a sequence whose solves reject steps has them redone by the launch chain at the checkpoint, like psfm_track; when
 * a whole window of it is like that (or its context is set to the launch chain, psfm_ctx_set_solver mode 1) it leaves the batch
 * and is run alone by psfm_connect behind it.  Ids, lengths and every solver decision do not depend on the batching; track-mode positions are bit-identical, path-consistency
 * positions agree to rounding (<= 1e-9 px: a sequence that leaves the batch solves on a share of the block slots, see
 * psfm_ctx_set_resident_budget).  n_seq <= 64.  Synchronises `stream`.
 * Motion boundary (psfm_ctx_set_motion_boundary): on in EVERY context of the batch, each with its own threshold, or in none; contexts
 * that disagree are PSFM_ERR_ARG.  With it on every frame launch forms the second verdict from the sequences' kill maps, which are
 * built for all sequences together (psfm_kill_map_batch's launch) behind each chunk of flow_check; results are those of psfm_connect
 * with the option on, sequence by sequence, and info->chain_mode is 3 for a sequence that stayed in the batch.
 * Sequences that leave the batch, together (psfm_ctx_set_batch_redo(ctxs[0], 1); default 0: alone, as above): they are run again from
 * frame 0 through ONE set of launches -- the batched chain step of every frame and, behind it, the frame's solves of all of them
 * as the frame-mode multi-problem launch chain: one init launch, iteration launches paced by one poll and ONE host synchronisation
 * for all sequences, one write-back launch -- and one segmented finalize; launches only, the device is never taken exclusively.  With
 * the option on a context pinned to the launch chain (psfm_ctx_set_solver mode 1) goes there directly.  info->chain_mode is 8 for a
 * sequence that ran this way.  Against what psfm_connect leaves for that sequence alone on a context pinned to the launch chain
 * (psfm_ctx_set_solver(ctx, 1, 0)) with no resident budget, the same lane capacity and the same motion-boundary setting, it holds:
 * ids, births, lengths, offsets and every solve's iterations, successful steps, termination and non-Gauss-Newton count are EXACT.
 * Positions and the two costs of a solve are what psfm_track promises between two runs of one sequence, no more: the block count,
 * the list plan, the order of the block sums and the control step are the single chain's, so they are byte-equal where the lanes
 * were handed out alike (a solve's sums run in lane order, and lanes are handed out by blocks that race inside a chain step), and
 * positions agree to <= 1e-9 px otherwise.  Observed on an MI355X: all bytes equal on sequences of up to 6 000 grid points with few
 * respawns; the last bit of a cost on 12 288 dense points; positions to 1e-13 px on realistic flows of 25 000 to 307 000 points.
 * Where the capacities differ, the same <= 1e-9 px holds.  Sequences that stayed in the batch are untouched by the option.
 * psfm_connect_batch_census: the last call that had `ctx0` as ctxs[0] -- n_left (sequences that left the fused batch), n_together
 * (those that went through the joint redo), and of that redo launches_fixed (the table copy, the lane-table init, one chain step
 * per frame, per frame with a solve the init launch, the polls and the write-back launch), launches_iter (trust-region iteration
 * launches, each over all sequences) and host_syncs (one per poll, one behind the finalize): per frame the fixed launches are
 * three (chain step, init, write-back) whatever n_together is; polls, iteration launches and synchronisations are set by the
 * SLOWEST solve of the frame in the table -- they do not grow with the number of sequences beyond that solve's need, but a further
 * sequence whose solve is the slowest of a frame adds a chunk of iteration launches and a poll there.
 * The joint redo files its solves in each context's adaptive policy (psfm_ctx_set_solver mode 0: launch chain or fused solve next,
 * iterations per fused launch), as the checkpoints of psfm_connect do for a sequence redone alone, over the whole sequence instead
 * of its last window: what a context starts its next call with may differ between the two routes.
 * Sequences of different frame sizes: h = w = 0, and every ctxs[i] carries the frame size of sequence i (psfm_ctx_set_frame_size):
 * flows_f[i] is (n_flows[i],H_i,W_i,2) and so on.  One sample_ratio, one thres, stride-2 stacks for all or none, as above; every
 * result, info->chain_mode and the census are what the call gives the sequences grouped by size (track mode: the same bytes; path
 * consistency: as between two runs).  Exactly one of h, w being 0 is PSFM_ERR_ARG, and so is a context without a frame size (the
 * lowest such sequence is named).  With h > 0 and w > 0 the contexts' stored sizes are ignored; with h = w = 0 and all stored sizes
 * equal the call is the one with that h, w.  The frame launches read every dimension from the sequence's row and keep blockIdx.y =
 * sequence (a block beyond a small sequence's lanes leaves at once); flow_check and the kill maps run over a grid flattened over the
 * sequences; the segmented finalize sorts with the key fields of the widest grid and the longest sequence, which leaves every
 * sequence's order -- its ids -- what it is alone.  When one stack cannot take the 16-byte-load flow_check (fewer than 1024 pixels, an
 * odd pixel count, a misaligned stack) the maps of all stacks are made up front, stack by stack. */
psfm_status psfm_connect_batch(psfm_ctx* const* ctxs, int n_seq, const float* const* flows_f, const float* const* flows_b,
                               const float* const* flows_f2, const float* const* flows_b2, const int* n_flows, int h, int w,
                               float thres, int sample_ratio, psfm_track_info* infos_host, void* stream);
/* mode 0: sequences that leave the fused batch run alone through psfm_connect (default); 1: together (see above).  Read from ctxs[0]
 * of a psfm_connect_batch call.  Any other value: PSFM_ERR_ARG. */
psfm_status psfm_ctx_set_batch_redo(psfm_ctx* ctx, int mode);
/* The frame size of the sequence this context holds in a psfm_connect_batch call with h = w = 0.  (0, 0) clears it; anything else must
 * be a frame size the entry points take (h, w >= 2, h w < 2^29), else PSFM_ERR_ARG and the stored size stays.  No other entry point
 * reads it. */
psfm_status psfm_ctx_set_frame_size(psfm_ctx* ctx, int h, int w);
psfm_status psfm_connect_batch_census(psfm_ctx* ctx0, int32_t* n_left, int32_t* n_together, int32_t* launches_fixed,
                                      int32_t* launches_iter, int32_t* host_syncs);

/* Device-resident result of the last psfm_track: CSR over trajectories in id order.
 *   birth (n_traj) i32 first frame; len (n_traj) i32; off (n_traj+1) i64; xy (n_points,2) f64.
 * Trajectory i has times birth[i] .. birth[i]+len[i]-1 and points xy[off[i] .. off[i+1]). */
psfm_status psfm_result_device(psfm_ctx* ctx, const int32_t** birth, const int32_t** len,
                               const int64_t** off, const double** xy);

/* Copy the result into caller-provided HOST buffers (any may be NULL to skip). */
psfm_status psfm_result_copy(psfm_ctx* ctx, int32_t* birth_host, int32_t* len_host, int64_t* off_host,
                             double* xy_host, void* stream);

/* Per-solve statistics of the last psfm_track (track_optimize mode): up to `max_n` entries. */
psfm_status psfm_result_solve_stats(psfm_ctx* ctx, psfm_solve_stats* stats_host, int32_t max_n,
                                    int32_t* n_out);

/* The saved trajectory set of main_connect_point_trajectories.py:56-61 -- trajectories of length >= traj_min_len, ids =
 * their indices in the full list -- compacted in HBM from the result of the last psfm_track / psfm_connect, so that only
 * what is kept crosses PCIe (the host-side filter is a boolean gather over every point).
 *   psfm_result_filter        builds the filtered CSR in the context, returns its sizes; synchronises `stream`
 *   psfm_result_filtered_copy copies it to HOST buffers: ids (k) i32, birth (k) i32, len (k) i32, off (k+1) i64,
 *                             xy (n_points,2) f64; any may be NULL */
psfm_status psfm_result_filter(psfm_ctx* ctx, int traj_min_len, int64_t* n_traj_host, int64_t* n_points_host, void* stream);
psfm_status psfm_result_filtered_copy(psfm_ctx* ctx, int32_t* ids_host, int32_t* birth_host, int32_t* len_host,
                                      int64_t* off_host, double* xy_host, void* stream);

/* A trajectory set from elsewhere -- yesterday's track.npy, the reference's CPU stage, another tracker -- becomes the context's
 * result, so that every consumer of a result (the filter, the window samplers, the label merge, the match tables, the database
 * rows, ground-truth scoring) runs on it as on a tracker's.  The arrays are a saved set as psfm_result_filtered_copy returns it,
 * without `off` (derived from len): trajectory i has id ids[i], frames birth[i] .. birth[i] + len[i] - 1 and its points in xy in
 * that order; each pointer HOST or DEVICE (the direction follows from the pointer).
 * The result is a CSR in which index == id, so the set is expanded to *n_result_host = ids[n_traj - 1] + 1 entries: an id the set
 * does not hold becomes an entry with len = 0, birth = 0 and no points (the file does not say what it was, only that it was not
 * saved); xy is taken as it is.  psfm_result_filter(ctx, 1) then reproduces the given set byte for byte, psfm_result_filter(ctx, m)
 * its trajectories of length >= m.  On such a result psfm_result_filter(_batch) and psfm_window_sample(_batch) refuse
 * traj_min_len < 1 (PSFM_ERR_ARG) and psfm_result_keys refuses it (no birth grid index); a live label merge and a sampler plan are
 * void.  The next tracker call replaces it like any result.
 * PSFM_ERR_ARG, with the lowest bad trajectory index named in psfm_last_error() and the previous result and saved set intact:
 * negative sizes, a NULL array that is not empty, ids not strictly ascending or outside [0, 2^28), len < 1, birth < 0,
 * birth + len > 2^30, sum(len) != n_points.  n_traj == 0 is legal and leaves an empty result.  Coordinates are not looked at.
 * Synchronises `stream`; two host synchronisations (the verdict, the point total). */
psfm_status psfm_result_set(psfm_ctx* ctx, int64_t n_traj, int64_t n_points, const int32_t* ids, const int32_t* birth,
                            const int32_t* len, const double* xy, int64_t* n_result_host, void* stream);

/* psfm_result_set for a track.npy that save_track_npy(layout="reference") of this package wrote, straight from the file: the
 * 64-byte footer behind the pickle names the raw f64 point bytes and the fixed-size records (one per trajectory); the records go
 * through the context's ring of pinned buffers (psfm_load_flo_stack's) into a device workspace and are decoded there, the set is
 * validated and expanded as by psfm_result_set, and only then the point bytes are streamed into the result.  The pickle is never
 * interpreted: rec_template (rec_size bytes, 63 as the writer stands and at most 68: the record with zeroed fields) and field_at (offsets of the six 4-byte fields
 * id, b, b + n, s, e, n) come from the writer's own definition.  n_threads reader threads (1 .. 32).
 * PSFM_ERR_ARG with the context untouched: a missing, short or foreign file, a footer that fails a check, a record that differs
 * from the template or whose fields disagree (the lowest such trajectory is named), a set psfm_result_set would refuse.  A read
 * error while the points stream leaves an EMPTY result (the previous one is gone by then; the message says so). */
psfm_status psfm_load_track_npy(psfm_ctx* ctx, const char* path, const uint8_t* rec_template, int rec_size, const int32_t* field_at,
                                int n_threads, int64_t* n_traj_host, int64_t* n_points_host, int64_t* n_result_host, void* stream);

/* The motion-segmentation window tensors (motion_seg/load_cut_seq.py:60-89) from the device-resident result of the last
 * psfm_track / psfm_connect -- TrajectorySet::sample_inside_window (optimize/src/trajectory_base.cpp:127-185) for the
 * contiguous window [frame0, frame0 + n_frames) plus the resize / normalise of motion_seg/core/dataset/data_utils.py:74-89:
 *   trajectories of length >= traj_min_len (the saved set, main_connect_point_trajectories.py:56-61) with >= min_length
 *   observations inside the window, ascending id; more than max_num_tracks -> a random subset in shuffled order
 *   (seeded; the reference shuffles unseeded).
 * Outputs, all DEVICE pointers, any may be NULL (all NULL = count only); `capacity` = rows the buffers can hold:
 *   ids_out (K) i32   xy_raw (K,n_frames,2) f64 zero-padded   mask_absent (K,n_frames) f64, 1.0 where the trajectory
 *   has no point (load_cut_seq's `1 - masks`)   xy_norm (K,n_frames,2) f64 = clip(xy / (raw/in) / in, 0, 1)
 * *k_host = K.  Synchronises `stream`. */
psfm_status psfm_window_sample(psfm_ctx* ctx, int frame0, int n_frames, int traj_min_len, int min_length,
                               int64_t max_num_tracks, uint64_t seed, int raw_h, int raw_w, int in_h, int in_w,
                               int64_t capacity, int32_t* ids_out, double* xy_raw, double* xy_norm, double* mask_absent,
                               int64_t* k_host, void* stream);

/* The motion classifier's input step -- traj_oa_depth.augment_traj with image_grid, depth_project and gather_point
 * (motion_seg/core/network/traj_oa_depth.py:72-114) behind the host glue of motion_seg/main_motion_segmentation.py:71-78 -- from
 * exactly what psfm_window_sample wrote: xy_norm (k,n_frames,2) f64, mask_absent (k,n_frames) f64, plus the depth maps at the
 * network input size, depth (n_frames,h,w) f32.  out is the reference's [1,10,k,n_frames] fp32 tensor, contiguous; planes:
 *   0-1 the coordinates cast to f32 (.float())   2-3 their frame-to-frame motion   4-6 the back-projected point
 *   depth * (Kinv @ (px,py,1)) of the pixel under the trajectory   7-9 its motion.
 * Bit-equal to the reference: every operation is an individually rounded fp32 operation in the reference's order (no FMA), and
 * the point cloud of every pixel ([B,3,H,W,L] in the reference) is never materialised.  Kept quirks of gather_point (:97-98):
 *   - pixel index = (int)(y*h) * w + (int)(x*w), truncating, clamped to [0, h*w-1]: x == 1.0 gives column w, the first pixel of
 *     the NEXT row; y == 1.0 leaves the image and is clamped to the last pixel;
 *   - a padded slot has coordinates 0, gathers pixel 0 of its frame and carries that 3-D point, not zero;
 *   - motion at frame l < n_frames-1 is (v[l+1] - v[l]) * (1 - mask_absent[l+1]) (:109-112): only the LATER frame's mask gates
 *     it, so a padded slot followed by a present one has non-zero motion; the last frame's motion is 0.
 * Non-finite coordinates (finite flows produce none) give unspecified values; every access stays in bounds.
 * kinv_host: 9 floats on the HOST, row-major K^-1 (image_grid: fx = fy = (h+w)/2, cx = w/2, cy = h/2, inverted in f64, cast to
 * f32).  ASYNCHRONOUS: one launch on `stream`, no allocation, no host synchronisation.  k = 0 is a no-op.  PSFM_ERR_ARG: a NULL
 * pointer with k > 0, k < 0, n_frames < 1, h or w < 1, h*w or 10*k*n_frames above 2^31 - 1 (the kernel's 32-bit indices). */
psfm_status psfm_traj_augment(psfm_ctx* ctx, const double* xy_norm, const double* mask_absent, const float* depth, int64_t k,
                              int n_frames, int h, int w, const float* kinv_host, float* out, void* stream);

/* The motion classifier's trajectory transformer -- traj_oa_depth.joint_encoder(aug_trajs, masks) = pt_transformer.forward in eval
 * mode (motion_seg/core/network/traj_oa_depth.py:25-60) -- from exactly what psfm_traj_augment and psfm_window_sample wrote:
 * features [10][k][n_frames] f32, mask_absent (k,n_frames) f64 (padded where its .float() > 0.5).  out is the reference's [1,16,k]
 * fp32 tensor (what it hands to the OANet decoder as feat.unsqueeze(-1)): psfm_traj_decode's input.
 * Per trajectory, tokens l = 0 .. n_frames-1, fp32, dropout off:
 *   x = relu(fc2(relu(input_fc1(f))))                                        two 1x1 convolutions, 10 -> 16 -> 16
 *   encoder layer x 2 (post-norm): h = LN1(h + SA(h)); h = LN2(h + linear2(relu(linear1(h)))); memory = encoder.norm(h)
 *   decoder layer x 2, starting again from x (the reference passes the same tensor as src and tgt):
 *     d = LN1(d + SA(d)); d = LN2(d + CA(d, memory)); d = LN3(d + FFN(d));  out = max over ALL tokens of decoder.norm(d)
 *   attention: 4 heads of width 4, q scaled by 1/2.  Keys at padded positions are masked in both SELF-attentions; queries at padded
 *   positions are computed like any other; CROSS-attention attends to all memory positions, padded ones included (the reference
 *   passes no memory_key_padding_mask); the max includes the padded tokens; no position is zeroed.  LayerNorm: biased variance,
 *   eps 1e-5.
 * Same formula, another summation order and another expf than torch's: results agree with the module's f64 evaluation as closely
 * as the module's own fp32 run does (tests/golden/make_encoder_golden.py measures that error and derives the tests' bound from it).
 * No result depends on k or on a trajectory's place among the k.  A trajectory whose positions are ALL padded (psfm_window_sample
 * emits none) gets 16 unspecified values (NaN); every access stays in bounds and no other trajectory is affected.
 * weights: psfm_traj_encode_weight_count() = 15872 floats on the DEVICE, the module's 68 parameters in its own state_dict order,
 * every tensor row-major as stored ([out][in]):
 *   input_fc1.weight [16][10], .bias [16]; fc2.weight [16][16], .bias [16];
 *   transformer_model.encoder.layers.{0,1}: self_attn.in_proj_weight [48][16] (q, k, v), .in_proj_bias [48], self_attn.out_proj.weight
 *     [16][16], .bias [16], linear1.weight [64][16], .bias [64], linear2.weight [16][64], .bias [16], norm1.weight, .bias, norm2.weight,
 *     .bias [16] each                                                                                            (3280 per layer);
 *   transformer_model.encoder.norm.weight, .bias;
 *   transformer_model.decoder.layers.{0,1}: self_attn (as above), multihead_attn (the same four), linear1, linear2, norm1, norm2, norm3
 *                                                                                                                (4400 per layer);
 *   transformer_model.decoder.norm.weight, .bias.
 * ASYNCHRONOUS: one launch on `stream`, no allocation, no host synchronisation.  k = 0 is a no-op.  PSFM_ERR_ARG, nothing launched:
 * n_frames < 1 or n_frames > 64 (a trajectory lives inside one 64-lane wave), k < 0, 10*k*n_frames above 2^31 - 1 (the kernel's
 * 32-bit indices), a NULL pointer with k > 0. */
int psfm_traj_encode_weight_count(void);
psfm_status psfm_traj_encode(psfm_ctx* ctx, const float* features, const double* mask_absent, const float* weights, int64_t k,
                             int n_frames, float* out, void* stream);

/* motion_seg/core/network/oanet.py:13-206: traj_oa_depth.decoder = OANBlock(net_channels 128, input_channel 16, depth 8, clusters 100)
 * in eval mode on psfm_traj_encode's output, then torch.sigmoid (traj_oa_depth.py:124) and the `> 0.5` of
 * main_motion_segmentation.py:80.  encoding [16][k] f32; logits, prob [k] f32 and pred [k] u8 (1 = dynamic: what
 * psfm_labels_merge_window takes) may each be NULL.  The k trajectories are the points, B = 1, fp32 throughout:
 *   x1_1 = l1_1(conv1(encoding)): conv 16 -> 128, then 4 x PointCN(128) = IN, BN, ReLU, conv, IN, BN, ReLU, conv, plus the input
 *   down1: S = softmax over the k POINTS per cluster of conv 128 -> 100 of IN/BN/ReLU(x1_1); x_down [128][100] = x1_1 S^T (raw x1_1)
 *   l2: 4 x OAFilter(128, 100): IN/BN/ReLU/conv 128 -> 128; across the clusters out + conv 100 -> 100 of BN/ReLU(out); IN/BN/ReLU/conv
 *       128 -> 128, plus the input
 *   up1: S = softmax over the 100 CLUSTERS per point of conv 128 -> 100 of IN/BN/ReLU(x1_1) (its own BN and conv); x_up = x2 S
 *   l1_2: PointCN(256, 128) on cat(x1_1, x_up) (with its shot_cut conv 256 -> 128 of the raw input), 3 x PointCN(128)
 *   logit = output conv 128 -> 1; prob = sigmoid(logit); pred = prob > 0.5 on the fp32 probability
 * IN = InstanceNorm2d(eps 1e-3), no affine, no running statistics: the BIASED variance over the k points of this call, in eval mode
 * too (so a row's result depends on all rows).  BN = BatchNorm2d in eval: running_mean / running_var (eps 1e-5) / weight / bias.
 * Every product runs on the exact fp32 matrix instruction; channel statistics are f64 sums of the stored fp32 values, added across
 * blocks in a fixed order: no floating-point atomics, two identical calls give identical bits.  Results agree with the module's f64
 * evaluation as closely as the module's own fp32 run does (tests/golden/make_decoder_golden.py measures that error per case).
 * weights: psfm_traj_decode_weight_count() = 529497 floats on the DEVICE: the decoder's 186 float tensors (521785 parameters, 7712
 * running statistics) in the module's own state_dict order without the 30 num_batches_tracked, every tensor row-major as stored:
 *   conv1.weight [128][16], .bias; down1, up1: conv.1 (BN: weight, bias, running_mean, running_var), conv.3.weight [100][128], .bias;
 *   l1_1.{0..3}: conv.1 (BN), conv.3 [128][128], conv.5 (BN), conv.7 [128][128];
 *   l1_2.0: shot_cut [128][256], conv.1 (BN 256), conv.3 [128][256], conv.5 (BN), conv.7; l1_2.{1..3} as l1_1;
 *   l2.{0..3}: conv1.1 (BN), conv1.3 [128][128], conv2.0 (BN 100), conv2.2 [100][100], conv3.2 (BN), conv3.4 [128][128];
 *   output.weight [128], .bias [1].  The kernels fold the BatchNorms: a checkpoint's tensors are passed as they are.
 * workspace: psfm_traj_decode_workspace_bytes(k) bytes on the DEVICE, the caller's (about 2.6 KB per trajectory: four [128][k]
 * activations, the [100][k] embedding, per-block partials); its contents before the call do not matter and are unspecified after.
 * ASYNCHRONOUS: a fixed sequence of launches on `stream` whose number does not depend on the data, no allocation, no host
 * synchronisation.  k = 0 is a no-op.  PSFM_ERR_ARG, nothing launched: k < 0; k == 1 (InstanceNorm2d needs more than one point: the
 * reference raises); 128 k above 2^31 - 1 (the kernels' 32-bit indices); a NULL encoding, weights or workspace with k > 0;
 * workspace_bytes too small (the message names the needed size; psfm_traj_decode_workspace_bytes returns 0 for a k it refuses). */
int psfm_traj_decode_weight_count(void);
size_t psfm_traj_decode_workspace_bytes(int64_t k);
psfm_status psfm_traj_decode(psfm_ctx* ctx, const float* encoding, const float* weights, int64_t k, void* workspace,
                             size_t workspace_bytes, float* logits, float* prob, uint8_t* pred, void* stream);

/* psfm_traj_decode for n_win windows (the windows of main_motion_segmentation.py:69-112, of one sequence or of several) in ONE
 * sequence of launches: as many launches as ONE psfm_traj_decode, whatever n_win, the k[b] and the data are.  No new rule: for every
 * window b, logits[b], prob[b] and pred[b] are BIT-IDENTICAL to psfm_traj_decode(encoding[b], k[b]) on that window alone -- the same
 * 64-point tiles numbered inside the window, the same per-block partial sums added in the same fixed order, InstanceNorm and both
 * softmaxes over the k[b] points of that window only.  No floating-point atomics; identical calls give identical bytes.
 *   encoding  HOST array of n_win DEVICE pointers, encoding[b] = [16][k[b]] f32 (may be NULL where k[b] == 0)
 *   k         HOST array of n_win counts; 0 (the window is skipped, its outputs are not touched) or 2 <= k[b] <= the single call's
 *             cap (128 k[b] <= 2^31 - 1: the kernels' 32-bit indices are relative to a window's own buffers)
 *   logits, prob, pred   HOST arrays of n_win DEVICE pointers ([k[b]] f32, f32, u8); an array, or a single entry, may be NULL
 *   workspace psfm_traj_decode_batch_workspace_bytes(k, n_win) bytes on the DEVICE: the windows' psfm_traj_decode workspaces one
 *             after another, each on a 256-byte boundary (the sum of psfm_traj_decode_workspace_bytes(k[b])); contents before
 *             the call do not matter and are unspecified after.  Returns 0 for a batch the call refuses.
 * The host arrays are read before the call returns; the per-window table (k, workspace offset, input, outputs, first tile, first
 * slice) travels by value in the kernel arguments: nothing is uploaded, no staging buffer outlives the call.  The convolutions and
 * the pooled product run over the tiles (slices) of all windows in one grid, the statistics and the softmax over the points on a
 * (channel, window) grid, the OAFilter stack on [128][100] with one block per window.  ASYNCHRONOUS on `stream`: no allocation, no
 * host synchronisation.  n_win == 0 or every k[b] == 0: PSFM_OK, nothing launched.  PSFM_ERR_ARG, nothing launched: n_win outside
 * [0, 64] (callers split longer lists); a k[b] < 0, == 1 or above the cap (the message names the first such window); a NULL
 * encoding[b] with k[b] > 0; NULL weights or workspace while any k[b] > 0; workspace_bytes too small (the message names the needed
 * size). */
size_t psfm_traj_decode_batch_workspace_bytes(const int64_t* k, int n_win);
psfm_status psfm_traj_decode_batch(psfm_ctx* ctx, int n_win, const float* const* encoding, const int64_t* k, const float* weights,
                                   void* workspace, size_t workspace_bytes, float* const* logits, float* const* prob,
                                   uint8_t* const* pred, void* stream);

/* The front end of the motion classifier for n_win windows in one pass each: what psfm_traj_decode_batch is to psfm_traj_decode,
 * the three calls below are to psfm_window_sample, psfm_traj_augment and psfm_traj_encode.  No new rule: every window's tensors are
 * BIT-IDENTICAL to the single call on that window alone.  Conventions of psfm_traj_decode_batch: HOST arrays of per-window values
 * and DEVICE pointers, read before the call returns; the per-window table travels by value in the kernel arguments; 0 <= n_win <= 64
 * (callers split longer lists); PSFM_ERR_ARG with nothing launched on a bad argument, the message names the first offending window.
 * No floating-point atomics; identical calls give identical bytes.
 *
 * psfm_window_sample_batch   psfm_window_sample(frame0[b], n_frames, ..., seed[b]) for every window b of ONE context, on the result
 *   of its last psfm_track / psfm_connect.  Windows share n_frames; they may overlap; one outside the sequence has k = 0; k = 1 is
 *   legal.  Window b occupies rows [sum of k[a] for a < b, + k[b]) of each output, so its block is a contiguous (k[b], n_frames, .)
 *   tensor: the same ids in the same order (ascending at or below max_num_tracks; above it the max_num_tracks smallest splitmix64
 *   keys of (seed[b], id) in key order, equal keys in ascending id order), the same xy_raw, xy_norm and mask_absent, byte for byte.
 *   `capacity` = rows the outputs can hold over all windows; k_host[b] = the window's rows.
 *     PLAN   all four outputs NULL: the selection is made for all windows in one pass over the trajectories -- per-(window, block)
 *            counts by ballots, one fixed-order integer scan, one compaction; per window above the cap one hash and one stable 64-bit
 *            sort -- and KEPT in workspace the context owns.  Synchronises `stream` ONCE, for all windows together.
 *     FILL   any output given, and a plan is kept for the same n_win, frame0[], n_frames, traj_min_len, min_length, max_num_tracks
 *            and seed[] on the same result: ONE gather launch over the rows of all windows.  ASYNCHRONOUS on `stream` (the stream of
 *            the plan call, or one ordered behind it): no synchronisation, no allocation.  capacity below the sum of k:
 *            PSFM_ERR_CAPACITY, nothing written.
 *            Without a matching plan the call makes the plan itself (one synchronisation), then gathers.  A stale plan is never
 *            used: psfm_track, psfm_connect, psfm_connect_batch, psfm_track_queries, psfm_track_queries_optimize,
 *            psfm_track_queries_batch and psfm_result_filter on the context void it, as does any differing argument.
 *   PSFM_ERR_ARG: n_win outside [0, 64], n_frames < 1, max_num_tracks < 0, capacity < 0, a NULL host array with n_win > 0, sizes < 1
 *   with xy_norm given, a window whose frame0 + n_frames leaves the 32-bit range.
 *
 * psfm_traj_augment_batch    psfm_traj_augment for n_win windows of n_frames frames and one (h, w, kinv) in ONE launch.  xy_norm[b]
 *   (k[b],n_frames,2) f64, mask_absent[b] (k[b],n_frames) f64, depth[b] (n_frames,h,w) f32, out[b] [10][k[b]][n_frames] f32: views
 *   of psfm_window_sample_batch's outputs, or any other buffers.  Blocks of 256 elements are numbered inside a window.  k[b] == 0
 *   skips the window (its pointers may be NULL, nothing of it is touched).  The single call's limits hold per window (h*w and
 *   10*k[b]*n_frames at most 2^31 - 1).  ASYNCHRONOUS, no allocation.  n_win == 0 or every k[b] == 0: PSFM_OK, nothing launched.
 *   PSFM_ERR_ARG: n_win outside [0, 64], n_frames, h or w < 1, a k[b] < 0 or above the limit, a NULL entry with k[b] > 0.
 *
 * psfm_traj_encode_batch     psfm_traj_encode for n_win windows of n_frames frames with one set of weights in ONE launch.
 *   features[b] [10][k[b]][n_frames] f32, mask_absent[b] (k[b],n_frames) f64, out[b] [16][k[b]] f32 (what psfm_traj_decode_batch
 *   takes as encoding[b]).  Blocks are numbered inside a window, so the packing of trajectories into waves is the single call's; the
 *   kernel has the vector registers and the LDS of the single one, the window costs scalar registers only.  1 <= n_frames <= 64.
 *   ASYNCHRONOUS, no allocation.  k[b] == 0 skips the window; n_win == 0 or every k[b] == 0: PSFM_OK, nothing launched.
 *   PSFM_ERR_ARG: n_win outside [0, 64], n_frames outside [1, 64], a k[b] < 0 or above the single call's limit, a NULL entry with
 *   k[b] > 0, NULL weights. */
psfm_status psfm_window_sample_batch(psfm_ctx* ctx, int n_win, const int* frame0, int n_frames, int traj_min_len, int min_length,
                                     int64_t max_num_tracks, const uint64_t* seed, int raw_h, int raw_w, int in_h, int in_w,
                                     int64_t capacity, int32_t* ids_out, double* xy_raw, double* xy_norm, double* mask_absent,
                                     int64_t* k_host, void* stream);
psfm_status psfm_traj_augment_batch(psfm_ctx* ctx, int n_win, const double* const* xy_norm, const double* const* mask_absent,
                                    const float* const* depth, const int64_t* k, int n_frames, int h, int w, const float* kinv_host,
                                    float* const* out, void* stream);
psfm_status psfm_traj_encode_batch(psfm_ctx* ctx, int n_win, const float* const* features, const double* const* mask_absent,
                                   const float* weights, const int64_t* k, int n_frames, float* const* out, void* stream);

/* sfm/matches_from_flow.py:51-118 (traj_to_matches) from the saved set that psfm_result_filter left in HBM -- the
 * reference's per-trajectory Python loops as index arithmetic on the device (no track.npy round trip):
 *   keypoints  image i lists the kept points observed in frame i in trajectory (id) order (:67-81); labels_dev: optional
 *              (n_points of the saved set) u8 DEVICE array, 1 = dynamic point, dropped (remove_dynamic, :71-74), NULL = keep all
 *   matches    point j of a trajectory with n kept points pairs with every other point when n <= sample_k (20 in the
 *              reference, :52), else with the points at k * (n / sample_k), itself skipped (:83-101); a match is the row
 *              [keypoint index of j, keypoint index of the target] under the image pair (frame of j, frame of the target)
 * n_img = number of images (every frame index must be < n_img).  Returns the table sizes; synchronises `stream`.
 * psfm_matches_copy copies the tables to HOST buffers (any may be NULL):
 *   kp_off (n_img+1) i64, kp_xy (n_kp,2) f64 -- keypoints of image i = kp_xy[kp_off[i] .. kp_off[i+1])
 *   pair_key (n_pairs) i64 = src_image * n_img + tgt_image, ascending;  pair_off (n_pairs+1) i64 into rows;
 *   pair_first (n_pairs) i64 = position of the pair's first match in the reference's loop order (its dict order);
 *   rows (n_matches,2) i32, inside a pair in the reference's loop order. */
psfm_status psfm_traj_to_matches(psfm_ctx* ctx, int n_img, int sample_k, const uint8_t* labels_dev, int64_t* n_kp_host,
                                 int64_t* n_matches_host, int64_t* n_pairs_host, void* stream);
psfm_status psfm_matches_copy(psfm_ctx* ctx, int64_t* kp_off_host, double* kp_xy_host, int64_t* pair_key_host,
                              int64_t* pair_off_host, int64_t* pair_first_host, int32_t* rows_host, void* stream);

/* motion_seg/main_motion_segmentation.py:89-129: the network's per-window, per-trajectory predictions merged into the labelled
 * trajectory set that sfm/matches_from_flow.py consumes -- the dict loop of :92-112 and the saved dict of :122-129 -- over the saved
 * set that psfm_result_filter left in HBM, without a track.npy round trip.  What the reference's loop produces, and this reproduces:
 *   - a trajectory enters with the first row that names it and has a point inside that row's window (:100-103); the set lists the
 *     trajectories in that order of first appearance (window, then row), NOT by ascending id;
 *   - a point carries the prediction of the FIRST window that covered it; a later window only adds the frames the trajectory does
 *     not hold yet (:105-112), so a trajectory can carry both labels;
 *   - only points inside windows where the trajectory was sampled enter: a trajectory that psfm_window_sample left out of a middle
 *     window (max_num_tracks) has a GAP in its frames, one with fewer than min_length observations in every window never enters.
 *     The labelled set therefore carries explicit per-point frames and is not the saved set with a label array on top.
 * psfm_labels_begin         needs a non-empty saved set in the context (else PSFM_ERR_ARG); clears the merge state and ties it to
 *                           that saved set: a later psfm_result_filter / psfm_track / psfm_connect / psfm_connect_batch on the
 *                           context voids it, and psfm_labels_merge_window / psfm_labels_finish then return PSFM_ERR_ARG.
 *                           ASYNCHRONOUS: three memsets on `stream`, no host synchronisation (the merge state is allocated by the
 *                           first call for a saved set of that size and grows with it).
 * psfm_labels_merge_window  one window, in stream order: row i says trajectory ids_dev[i] (i32, an id of the saved set) is dynamic
 *                           (pred_dev[i] != 0) or static on frames [frame0, frame0 + n_frames).  ASYNCHRONOUS: one launch, no host
 *                           synchronisation, no allocation -- it can be enqueued right behind the network's output tensor.  k = 0 is
 *                           a no-op.  Preconditions: ids are unique within a call (psfm_window_sample guarantees it; the result for
 *                           duplicates is unspecified, every access stays in bounds); fewer than 2^32 - 1 rows over all windows.  A
 *                           row whose trajectory has no point in the window is ignored (the reference would file an empty entry,
 *                           which changes no match; psfm_window_sample never emits such a row).  An id that is not in the saved
 *                           set raises a device-side flag: the call stays asynchronous, psfm_labels_finish reports PSFM_ERR_ARG.
 * psfm_labels_finish        builds the labelled set in the context and returns its sizes; synchronises `stream`.  CSR in order of
 *                           first appearance, a trajectory's points in time order:
 *                             ids (n_traj) i32, off (n_traj+1) i64, frame_ids (n_points) i32, xy (n_points,2) f64,
 *                             labels (n_points) u8 (1 = dynamic)
 *                           No window merged: the empty set (n_traj = 0).  More windows may be merged and finish called again.
 * psfm_labels_device        the DEVICE pointers of that CSR (any argument may be NULL); psfm_labels_copy copies it into caller-provided
 *                           buffers, HOST or DEVICE (the direction follows from the pointer), any may be NULL, and synchronises
 *                           `stream`.  The labelled set is a copy of its own: it stays valid when the saved set changes.
 * psfm_labels_to_matches    sfm/matches_from_flow.py:51-118 over the labelled set: the tables of psfm_traj_to_matches (same
 *                           pipeline, same context tables -- read them with psfm_matches_copy), with the trajectories in the
 *                           set's order (the dict order :67 iterates in), a point's frame from frame_ids, and the kept points =
 *                           labels == 0 when remove_dynamic != 0 (:71-74), all points otherwise.  A frame outside [0, n_img) is
 *                           PSFM_ERR_ARG.  Synchronises `stream`.
 * psfm_labels_set           a labelled set from elsewhere (a labelled track.npy, another classifier): the caller's CSR -- the five
 *                           arrays of psfm_labels_finish, HOST or DEVICE (the direction follows from the pointer) -- is copied into
 *                           the context and becomes its labelled set, exactly as if psfm_labels_finish had built it; a merge in
 *                           progress ends (psfm_labels_begin starts a new one).  The trajectories keep the given order; a
 *                           trajectory's frames may come in any order and have gaps.  PSFM_ERR_ARG: negative sizes, a NULL array
 *                           that is not empty, or an off that does not run from 0 to n_points without stepping back (checked on
 *                           the device: the context then holds no labelled set).  Synchronises `stream`. */
psfm_status psfm_labels_set(psfm_ctx* ctx, int64_t n_traj, int64_t n_points, const int32_t* ids, const int64_t* off,
                            const int32_t* frame_ids, const double* xy, const uint8_t* labels, void* stream);
psfm_status psfm_labels_begin(psfm_ctx* ctx, void* stream);
psfm_status psfm_labels_merge_window(psfm_ctx* ctx, int frame0, int n_frames, const int32_t* ids_dev, const uint8_t* pred_dev,
                                     int64_t k, void* stream);
psfm_status psfm_labels_finish(psfm_ctx* ctx, int64_t* n_traj_host, int64_t* n_points_host, void* stream);
psfm_status psfm_labels_device(psfm_ctx* ctx, const int32_t** ids, const int64_t** off, const int32_t** frame_ids, const double** xy,
                               const uint8_t** labels);
psfm_status psfm_labels_copy(psfm_ctx* ctx, int32_t* ids_out, int64_t* off_out, int32_t* frame_ids_out, double* xy_out,
                             uint8_t* labels_out, void* stream);
psfm_status psfm_labels_to_matches(psfm_ctx* ctx, int n_img, int sample_k, int remove_dynamic, int64_t* n_kp_host,
                                   int64_t* n_matches_host, int64_t* n_pairs_host, void* stream);
/* the sizes of the labelled set in the context (PSFM_ERR_ARG: none); either may be NULL.  No device work. */
psfm_status psfm_labels_sizes(psfm_ctx* ctx, int64_t* n_traj, int64_t* n_points);

/* The saved sets and the match tables of n_seq = 1 .. 64 sequences in ONE pass each: psfm_result_filter, psfm_traj_to_matches and
 * psfm_labels_to_matches for every context of a batch (psfm_connect_batch / label_sequences_batched leave one context per
 * sequence), with a number of host synchronisations (at most 2 for the filter, at most 4 for the tables: the single calls') and of
 * launches that does not depend on n_seq.  No new rule: afterwards context b is in exactly the state the single call
 * (ctxs[b], ..., n_img[b], labels_dev[b]) leaves -- the saved set / the tables byte for byte, the counts, res_gen -- so
 * psfm_result_filtered_copy, psfm_matches_copy, psfm_matches_to_database and everything behind them run unchanged, context by
 * context.  The contexts are distinct, non-NULL and on one device; ctxs[0] owns the call's shared workspace (the intermediates of
 * all sequences live once, there).  All *_host arguments are arrays of n_seq entries.
 *   psfm_result_filter_batch      n_traj_host / n_points_host [n_seq]
 *   psfm_traj_to_matches_batch    over the saved sets; n_img [n_seq] may differ per sequence and exceed the frames present;
 *                                 labels_dev: NULL, or [n_seq] DEVICE arrays as in psfm_traj_to_matches, NULL entries allowed
 *   psfm_labels_to_matches_batch  over the labelled sets (every context needs one: psfm_labels_finish / psfm_labels_set)
 * A sequence that turns out empty gets its empty state (the zero-filled kp_off of n_img[b] + 1 entries included); the others go on.
 * PSFM_ERR_ARG before anything is launched, with every context untouched (tables of an earlier call still copy out) and
 * psfm_last_error() naming the first offending sequence: n_seq out of range; a NULL, repeated or foreign-device context;
 * n_img[b] < 1; sample_k < 1; no labelled set; 2^32 - 1 or more points (2^31 - 1 or more trajectories for the filter) over all
 * sequences; a sort key (sequence, src * n_img + tgt) that does not fit 64 bits.  PSFM_ERR_ARG found on the device: a frame outside
 * [0, n_img[b]) -- never used as an index -- names the lowest such sequence and leaves EVERY context of the call with empty tables
 * (all counts 0).  Two identical calls give identical bytes.
 *   psfm_matches_batch_census     for the last of these calls that ctx0 owned: its host synchronisations and the library's own
 *                                 launches, copies and memsets (not what rocPRIM launches inside a sort or a scan). */
psfm_status psfm_result_filter_batch(psfm_ctx* const* ctxs, int n_seq, int traj_min_len, int64_t* n_traj_host, int64_t* n_points_host,
                                     void* stream);
psfm_status psfm_traj_to_matches_batch(psfm_ctx* const* ctxs, int n_seq, const int* n_img, int sample_k, const uint8_t* const* labels_dev,
                                       int64_t* n_kp_host, int64_t* n_matches_host, int64_t* n_pairs_host, void* stream);
psfm_status psfm_labels_to_matches_batch(psfm_ctx* const* ctxs, int n_seq, const int* n_img, int sample_k, int remove_dynamic,
                                         int64_t* n_kp_host, int64_t* n_matches_host, int64_t* n_pairs_host, void* stream);
psfm_status psfm_matches_batch_census(psfm_ctx* ctx0, int32_t* host_syncs, int32_t* launches);

/* sfm/import_feature_matches.py:76-104 (import_keypoints_matches) writing through sfm/colmap_utils/database.py:181-225: the match
 * tables that the last psfm_traj_to_matches / psfm_labels_to_matches left in the context become the blobs of the COLMAP database's
 * keypoints, matches and two_view_geometries rows (csrc/psfm_database.hip; the per-element rules are csrc/psfm_database.h).
 * psfm_matches_to_database   db_id_host, db_pos_host (n_img) i32 on the HOST, indexed by image = frame index: the image's COLMAP
 *                            image_id, and its position in the order the reference iterates its image_ids mapping in (the order of
 *                            the SELECT that built it: neither name order nor id order).
 *                              keypoints  float32(xy + 0.5): the add in f64, one rounding to f32 (:82-84, database.py:185); same
 *                                         kp_off as the match tables
 *                              pairs      directed pair (s, t) is written unless the reverse pair (t, s) is in the table and
 *                                         pos[t] < pos[s] -- what the reference's `matched` set amounts to (:88-99); a self pair is
 *                                         written.  With more than sample_k kept points in a trajectory the two directions hold
 *                                         different matches: the reference drops data here, and so does this.
 *                              rows       pair_id = min(id_s, id_t) * (2^31 - 1) + max(id_s, id_t) i64; rows u32, the two columns
 *                                         swapped when id_s > id_t (database.py:196-207); the kept pairs in ascending pair_key
 *                                         order, their rows contiguous and in the match table's order
 *                            Returns the number of kept pairs and of their rows; synchronises `stream`.  Integers in a fixed order:
 *                            two calls on the same tables give identical bytes.  PSFM_ERR_ARG (the context stays usable, earlier
 *                            database tables are kept): no match tables in the context; n_img differs from the one they were built
 *                            with; an id outside [1, 2^31 - 2]; an id given twice; db_pos not a permutation of 0..n_img-1; a NULL
 *                            argument.
 * psfm_database_copy         copies the tables into caller-provided buffers, HOST or DEVICE (the direction follows from the pointer),
 *                            any may be NULL; synchronises `stream`:
 *                              kp_f32 (n_kp,2) f32 -- keypoints of image i = rows kp_off[i] .. kp_off[i+1] (psfm_matches_copy)
 *                              pair_id (n_pairs_kept) i64;  pair_key (n_pairs_kept) i64 = src * n_img + tgt of the kept pairs,
 *                              ascending;  pair_off (n_pairs_kept+1) i64 into rows;  rows (n_rows_kept,2) u32
 *                            The database tables are a copy of their own: they stay valid when the match tables are rebuilt.
 *                            PSFM_ERR_ARG before the first successful psfm_matches_to_database.
 * psfm_database_chunk_rows   output rows per block of the row compaction (the tests place pair boundaries around it).
 * psfm_database_compact_again  for measurement: the row-compaction launch of the last psfm_matches_to_database once more, same
 *                            input, same output bytes.  ASYNCHRONOUS: one launch on `stream`.  PSFM_ERR_ARG when the match tables
 *                            were rebuilt since (or no database tables exist). */
psfm_status psfm_matches_to_database(psfm_ctx* ctx, int n_img, const int32_t* db_id_host, const int32_t* db_pos_host,
                                     int64_t* n_pairs_kept_host, int64_t* n_rows_kept_host, void* stream);
psfm_status psfm_database_copy(psfm_ctx* ctx, float* kp_f32, int64_t* pair_id, int64_t* pair_key, int64_t* pair_off, uint32_t* rows,
                               void* stream);
int psfm_database_chunk_rows(void);
psfm_status psfm_database_compact_again(psfm_ctx* ctx, void* stream);

/* sfm/convert.py:43-104 (save_depth_pose): the sparse depth maps of the registered images of a COLMAP model (csrc/psfm_sparse_depth.hip;
 * the per-element rules are csrc/psfm_sparse_depth.h).
 * psfm_sparse_depth          obs_xy (n_obs,2) f64, obs_id (n_obs) i64: the concatenated point lists of the model's images (xys,
 *                            point3D_ids), DEVICE.  img_desc_host: n_img descriptors on the HOST, 64 bytes each:
 *                              i64 obs_begin, obs_end   the image's observations, in list order
 *                              f64 r20, r21, r22, t2    row 2 of R = qvec2rotmat(qvec) (read_write_model.py:459-469, evaluated by the
 *                                                       caller so that R is the reference's) and tvec[2]
 *                              i32 w, h                 the image's camera
 *                              i64 out_off              first element of its (h, w) map in depth_out: the maps of a call follow each
 *                                                       other without gaps, the first at 0 -- cameras of different sizes share a call
 *                            pt_id_sorted (n_pts) i64 ascending, pt_row (n_pts) i32 = the row of pt_xyz that holds that id (equal
 *                            ids in file order: the last one is used, as a dict built in file order would), pt_xyz (n_pts,3) f64:
 *                            DEVICE.  depth_out: DEVICE, sum of h * w f64.
 *                              pixel   clip(int32(round-half-even(x)), 0, w - 1), y with h (:88-90), from xys, not from the projection
 *                              depth   ((r20 X + r21 Y) + r22 Z) + t2, each operation rounded once (:86-87 is this sum in BLAS's
 *                                      order: within 4 * 2^-53 * (|r20 X| + |r21 Y| + |r22 Z| + |t2|) of it)
 *                              id -1   skipped (:77); a pixel that several observations round into holds the LAST one's depth (:91),
 *                                      found as an integer maximum of list positions: no floating-point atomics, identical bytes
 *                                      from identical calls; a pixel nobody rounds into holds 0.0
 *                            Synchronises `stream`.  PSFM_ERR_ARG (the context stays usable; depth_out is then unspecified): an
 *                            observation whose id names no point -- *missing_id_host (may be NULL) = the smallest such id, -1
 *                            otherwise; a coordinate of a counted observation that is not finite or whose rounded value int32 does
 *                            not hold (|v| >= 2^31, or rint(v) = 2^31: the reference's cast is platform-defined there); a pt_row
 *                            outside [0, n_pts); descriptors that leave [0, n_obs), overlap or leave gaps in depth_out, w or h < 1,
 *                            2^32 - 1 or more observations in one image; NaN in a pose; n_pts >= 2^31.  The winner map (u32 per
 *                            pixel) and the rows found for the observations live in the context's workspace.
 * psfm_sparse_depth_sort_ids pt_id (n_pts) i64 DEVICE, every id in [0, 2^32) -> pt_id_sorted, pt_row through the record sort of the
 *                            finalize (stable).  PSFM_ERR_ARG on an id outside that range: sort those on the host (stable argsort).
 * psfm_ctx_set_sparse_depth  budget_bytes: what callers that split a model into several psfm_sparse_depth calls (psfm_sfm.convert)
 *                            let the maps + winner maps of one call take, 12 bytes per pixel; one image always goes through; 0 = no
 *                            limit; default 2^30.  timing != 0: events around the zero fill, the winner pass and the store pass of
 *                            every call, read by psfm_sparse_depth_last_ms (ms3[0..2], milliseconds).
 * psfm_colmap_points3d_count / _scan   HOST code, no GPU is touched: the walk over a points3D.bin image in memory
 *                            (read_write_model.py:336-363): u64 count, per point 43 bytes (u64 id, 3 f64 xyz, 3 u8 rgb, f64 error), a
 *                            u64 track length L and 8 L bytes.  count -> *n; scan -> ids_out (n) u64, xyz_out (n,3) f64, err_out (n)
 *                            f64, track_len_out (n) u64, any may be NULL.  Every read is checked against nbytes first.  The buffer
 *                            must hold exactly the announced records: a buffer cut at ANY byte, record boundaries included, and one
 *                            with trailing bytes are PSFM_ERR_ARG with the record index in psfm_last_error(); scan then writes
 *                            nothing. */
psfm_status psfm_sparse_depth(psfm_ctx* ctx, const double* obs_xy, const int64_t* obs_id, int64_t n_obs, const void* img_desc_host,
                              int n_img, const int64_t* pt_id_sorted, const int32_t* pt_row, const double* pt_xyz, int64_t n_pts,
                              double* depth_out, int64_t* missing_id_host, void* stream);
psfm_status psfm_sparse_depth_sort_ids(psfm_ctx* ctx, const int64_t* pt_id, int64_t n_pts, int64_t* pt_id_sorted, int32_t* pt_row,
                                       void* stream);
psfm_status psfm_ctx_set_sparse_depth(psfm_ctx* ctx, int64_t budget_bytes, int timing);
psfm_status psfm_ctx_get_sparse_depth_budget(psfm_ctx* ctx, int64_t* budget_bytes);
psfm_status psfm_sparse_depth_last_ms(psfm_ctx* ctx, double* ms3);
psfm_status psfm_colmap_points3d_count(const void* buf, uint64_t nbytes, uint64_t* n);
psfm_status psfm_colmap_points3d_scan(const void* buf, uint64_t nbytes, uint64_t* ids_out, double* xyz_out, double* err_out,
                                      uint64_t* track_len_out);

/* sfm/convert.py:26-41 and :95 (normalize_depth_for_display, gray2rgb, plt.imsave's byte conversion): the display images of the sparse
 * depth maps of one psfm_sparse_depth call (csrc/psfm_depth_display.hip; the per-element rules are csrc/psfm_depth_display.h).
 * psfm_depth_display         depth: DEVICE, what psfm_sparse_depth wrote (sum of h * w f64, 16-byte aligned).  img_desc_host: the
 *                            SAME 64-byte descriptors on the HOST (no smaller one is defined: a caller has them already); only w, h
 *                            and out_off are read, the maps follow each other without gaps, the first at 0.  pc in [0, 100] (the
 *                            reference: 98).  table_host 256 x 4 u8 and bad_rgba_host 4 u8 on the HOST: the colour map at 0..255
 *                            and at NaN as RGBA bytes (data: matplotlib's map times 255, truncated, alpha 255).  rgba_out: DEVICE,
 *                            16-byte aligned, 4 bytes per pixel at the same element offsets as depth.  Per image:
 *                              valid   d > 0, n of them; n = 0: no image, its part of rgba_out is left untouched
 *                              inv     1.0 / (d + 1.0) for every pixel: one f64 add, one IEEE division (d = -1 gives +inf)
 *                              z1, z2  np.percentile (method 'linear') of the valid inv at pc and at 100 - pc: vi = (n - 1) * (q / 100),
 *                                      j = floor(vi), g = vi - j, a = s[j], b = s[min(j + 1, n - 1)], a + (b - a) * g, and where
 *                                      g >= 0.5: b - (b - a) * (1 - g); every operation rounded once.  The order statistics come
 *                                      from an MSB-first 8-bit radix select over the bit patterns (integer atomics only: identical
 *                                      bytes from identical calls)
 *                              pixel   v = (inv - z2) / (z1 - z2) clamped to [0, 1] (NaN stays NaN), v32 = (float)v, xa = v32 * 256.0f,
 *                                      index 255 where xa == 256 else xa truncated; bytes = table[index], NaN: the bad entry
 *                            n_valid_out (n_img) i64 and z_out (n_img, 2) f64 (z1, z2; 0.0 for n = 0): HOST, either may be NULL.
 *                            Synchronises `stream` (once in the middle too: the counts size the workspace).  19 launches whatever
 *                            n_img.  PSFM_ERR_ARG, nothing launched, the context stays usable: a NULL argument, n_img < 1, w or
 *                            h < 1, an image of 2^31 pixels or more, descriptors that overlap or leave gaps, pc not finite or outside
 *                            [0, 100], a pointer that is not 16-byte aligned.  depth must not change during the call.
 * psfm_ctx_set_depth_display timing != 0: events around the count, compact, select and colour passes of every call, read by
 *                            psfm_depth_display_last_ms (ms4[0..3], milliseconds).
 * psfm_depth_display_chunk   valid pixels one block of the compaction covers at most (tests place maps around it). */
psfm_status psfm_depth_display(psfm_ctx* ctx, const double* depth, const void* img_desc_host, int n_img, double pc,
                               const uint8_t* table_host, const uint8_t* bad_rgba_host, uint8_t* rgba_out, int64_t* n_valid_out,
                               double* z_out, void* stream);
psfm_status psfm_ctx_set_depth_display(psfm_ctx* ctx, int timing);
psfm_status psfm_depth_display_last_ms(psfm_ctx* ctx, double* ms4);
int psfm_depth_display_chunk(void);

/* Trajectories against ground-truth masks (csrc/psfm_ground_truth.hip; the two per-element rules are csrc/psfm_ground_truth.h).
 * psfm_traj_eval_counts     motion_seg/eval_traj_iou.py:79-115 (per_img_traj_metrics) reduced to what its four metrics are functions
 *                           of: per frame, the counts tp, fp, fn, tn over the labelled points of that frame.  A point (x, y) f64 is
 *                           rounded to fp32 and sampled by the sampler of psfm_grid_sample (:53-65: true division by (size-1)/2,
 *                           bilinear, zeros padding, align_corners) from its frame's mask; gt = sample > 0.5f, pred = label != 0
 *                           (:70).  The mask is a u8 map seen through a 256-entry fp32 table: tap value = table_host[byte], a tap
 *                           outside the image = 0.  (The reference's mask is 1.0 - png[:,:,0] / 255.0 in f64 (:49) cast to fp32
 *                           (:107), i.e. table[b] = (float)(1.0 - b / 255.0); a caller with 0/1 masks passes another table.)
 *                             frame_ids (n_points) i32, xy (n_points,2) f64, labels (n_points) u8: DEVICE arrays, e.g. the CSR of
 *                               psfm_labels_device.  All three NULL = the labelled set that psfm_labels_finish left in the context
 *                               (n_points is then ignored; no such set: PSFM_ERR_ARG).  One or two NULL: PSFM_ERR_ARG.
 *                             masks_u8 (n_frames,h,w) u8 DEVICE; table_host 256 fp32 on the HOST (read before the call returns)
 *                             counts_out (n_frames,4) i64 DEVICE: tp, fp, fn, tn of frame f over the points with frame id f.  A
 *                               point whose frame id is outside [0, n_frames) is ignored (nothing is read for it).
 *                           ASYNCHRONOUS: a memset and one launch on `stream`, no allocation, no host synchronisation.  n_points = 0
 *                           (with non-NULL arrays) gives zeros.  The counts are integers accumulated with integer atomics: two calls
 *                           on the same input give identical counts.  PSFM_ERR_ARG, nothing launched: n_points < 0, n_frames < 1,
 *                           h or w < 2 (the sampler divides by (w-1)/2), 8*h*w >= 2^32 (the 32-bit byte offsets of every entry
 *                           point that takes h, w), a NULL masks_u8 / table_host / counts_out.
 * psfm_traj_vote_labels     scripts/prepare_flyingthings3d.py:89-108 (find_traj_label) from exactly what psfm_window_sample wrote
 *                           for a window that covers the sequence: xy (k,n_frames,2) f64 raw positions, mask_absent (k,n_frames) f64
 *                           (nonzero = padded), plus gts_u8 (n_frames,h,w) u8; labels_out (k) u8.  Per row: over the present
 *                           columns j, label_num += gts[j][rint(y)][rint(x)] -- rint rounds half to even like Python's round() on a
 *                           numpy.float64; the sum is an integer that cannot wrap (NumPy 1.21's behaviour; a u8 sum would wrap at
 *                           256) -- and label = label_num > total_num / 2 with integer division, total_num = the number of present
 *                           columns; a row without one gets 0.  Deviation: a present point whose pixel is outside [0,h) x [0,w), or
 *                           that is not finite, is never read; the call then returns PSFM_ERR_ARG and labels_out is unspecified
 *                           (every access stayed in bounds).  The reference wraps a negative index and raises on one >= h.
 *                           Synchronises `stream`.  k = 0 is a no-op.  PSFM_ERR_ARG, nothing launched: k < 0, n_frames < 1, h or
 *                           w < 1, h*w above 2^31 - 1, a NULL pointer with k > 0. */
psfm_status psfm_traj_eval_counts(psfm_ctx* ctx, const int32_t* frame_ids, const double* xy, const uint8_t* labels, int64_t n_points,
                                  const uint8_t* masks_u8, const float* table_host, int n_frames, int h, int w, int64_t* counts_out,
                                  void* stream);
psfm_status psfm_traj_vote_labels(psfm_ctx* ctx, const double* xy, const double* mask_absent, const uint8_t* gts_u8, int64_t k,
                                  int n_frames, int h, int w, uint8_t* labels_out, void* stream);

/* ONE sequence over several processes / GPUs, exactly (psfm_dist.connect_sharded drives these).
 * The tracks are split by the row band of the stride-r grid they are born on: this process owns the births on grid points
 * [g0, g1) and runs every frame for its tracks.  `maps`: caller-owned DEVICE buffer of 2 x map_pitch bytes (map_pitch >=
 * G + 1); after psfm_shard_step(frame) the slab (frame & 1) holds, stamped, the grid points within distance sample_ratio of
 * one of this process's surviving tracks (+ byte G: a track survived) -- the caller all-reduces (max) those G + 1 bytes over
 * the ranks before the next step reads them.  The solve of a frame runs as export (this process's sums: kind 0 the fused
 * solve with k iterations -> k x 13 doubles, 1 / 2 the launch chain's first / next iteration -> 13) -> the caller combines the
 * ranks' sums in rank order -> control on the totals (same numbers, same decision on every rank; synchronises and
 * reports done / redo / statistics).  redo: a fused solve met something it did not speculate -> restore, then the chain
 * (export 1, control, export 2, control, ... until done, write-back).  psfm_shard_finish leaves the own trajectories as the
 * usual result (psfm_result_copy), sorted by (last valid time, birth frame, birth grid index); ids over all ranks follow
 * from those keys.  No collective is issued by the library. */
psfm_status psfm_shard_begin(psfm_ctx* ctx, int n_flows, int h, int w, int sample_ratio, int64_t g0, int64_t g1, int optimize,
                             uint8_t* maps, int64_t map_pitch, void* stream);
psfm_status psfm_shard_step(psfm_ctx* ctx, const float* flow, const uint8_t* occ, int frame, void* stream);
psfm_status psfm_shard_solve_export(psfm_ctx* ctx, const float* flow01, const float* flow12, const float* flow02,
                                    const uint8_t* occ02, int frame, int kind, int k, double* sums_out, void* stream);
/* psfm_shard_step(frame) + psfm_shard_solve_export(frame, kind 0, k) as ONE launch (track_optimize.py:31-50 for the own tracks:
 * the chain step of the frame and the fused solve of its tracks, sums exported); frame >= 1, flow12 = the frame's own forward
 * flow, occ = its occlusion map.  The frame's marks are exchanged behind it like psfm_shard_step's.  sums_out NULL (a shard that is
 * the whole sequence only, see psfm_shard_solve_local): nothing is exported, the launch runs the control step on its own totals
 * and no psfm_shard_solve_control* call follows; a solve that did not go as speculated raises the device-side stall flag, which
 * reaches psfm_shard_peek_stall with every 8th frame (and psfm_shard_window_state at once). */
psfm_status psfm_shard_frame(psfm_ctx* ctx, const float* flow01, const float* flow12, const float* flow02, const uint8_t* occ,
                             const uint8_t* occ02, int frame, int k, double* sums_out, void* stream);
psfm_status psfm_shard_solve_control(psfm_ctx* ctx, int frame, int kind, int k, const double* totals, int32_t* done_host,
                                     int32_t* redo_host, psfm_solve_stats* stats_host, void* stream);
/* The fused path without a host round trip per solve: psfm_shard_solve_control_async runs the control step of a fused export
 * (kind 0, k iterations) and returns; psfm_shard_window_state synchronises once for a whole window of frames -- the stalled
 * frame (a solve that did not go as speculated; every later launch of the context has been a no-op since) or -1, and the
 * statistics of the window's solves.  The caller then redoes the stalled solve (restore + the per-iteration protocol) and
 * re-runs the frames behind it. */
psfm_status psfm_shard_solve_control_async(psfm_ctx* ctx, int frame, int k, const double* totals, void* stream);
psfm_status psfm_shard_window_state(psfm_ctx* ctx, int f_lo, int f_hi, psfm_solve_stats* stats_host, int32_t* stalled_frame,
                                    void* stream);
/* The redo of a stalled solve without a host round trip per trust-region iteration: psfm_shard_solve_control_chain_async enqueues the
 * control step behind an export of kind 1 / 2 and returns; the caller enqueues a batch of rounds (export 2 -> exchange -> control)
 * ahead and asks once per batch with psfm_shard_solve_poll (synchronises).  Rounds behind the one that ended the solve are no-ops. */
psfm_status psfm_shard_solve_control_chain_async(psfm_ctx* ctx, int frame, int kind, const double* totals, void* stream);
psfm_status psfm_shard_solve_poll(psfm_ctx* ctx, int32_t* done_host, psfm_solve_stats* stats_host, void* stream);
/* A shard that is the WHOLE sequence (g0 = 0, g1 = every grid point: ONE rank, the windowed engine for one long sequence on one GPU;
 * PSFM_ERR_ARG for a band): its solves need no exchange, so solves whose steps get rejected run like psfm_connect's
 * (track_optimize.py:49-50 -> trajectory_optimize.cpp:74-82) instead of export -> exchange -> control once per trust-region
 * iteration.  psfm_shard_solve_local ENQUEUES the solve of `frame` behind psfm_shard_step(frame): the resident solve -- ONE launch per
 * solve, inside the context's resident budget (psfm_ctx_set_resident_budget; without one: `unroll` launches of one iteration each);
 * a solve that is not done behind its launches raises the device-side stall flag (psfm_shard_window_state).
 * psfm_shard_solve_redo_local redoes a stalled solve to termination and writes it back (synchronises; chain_stalled: the solve had
 * been enqueued by psfm_shard_solve_local, not by a fused export).  Same sums in the same order as the exchange form: same positions. */
psfm_status psfm_shard_solve_local(psfm_ctx* ctx, const float* flow01, const float* flow12, const float* flow02, const uint8_t* occ02,
                                   int frame, int unroll, void* stream);
psfm_status psfm_shard_solve_redo_local(psfm_ctx* ctx, const float* flow01, const float* flow12, const float* flow02,
                                        const uint8_t* occ02, int frame, int chain_stalled, psfm_solve_stats* stats_host, void* stream);
/* ONE solve over several ranks with no host and no collective library in its loop (csrc/psfm_shard.hip, csrc/psfm_solver.hip: PcPeers):
 * every rank runs the resident solve of trajectory_optimize.cpp:74-82 on its own tracks, and the second hop of the launch's all-reduce
 * writes each leader's sums into EVERY rank's granule area through peer-mapped pointers (IPC handles between processes -- P2P over
 * xGMI between GPUs -- plain pointers between host threads of one process).  Set-up once per context: psfm_shard_peer_area (this rank's
 * area + its 64-byte IPC handle), psfm_shard_peer_open (another process's area), psfm_shard_peer_connect (world <= 8, rank, every rank's
 * area as this process addresses it, every rank's launch size from psfm_shard_solve_blocks; 0 blocks anywhere = PSFM_ERR_ARG: keep the
 * exchange form).  Per frame psfm_shard_solve_peer(frame, epoch) ENQUEUES this rank's launch; all ranks pass the same epoch (a counter
 * they advance together, 1 .. 2^20 - 1, never reused on an area: psfm_shard_peer_epoch).  REQUIRED between two psfm_shard_solve_peer calls: a
 * cross-rank collective (or any point every rank reaches only behind its launch of the solve before) -- consecutive solves reuse the two
 * sets of leader rows, and a rank that ran ahead into the next solve would overwrite rows another rank's blocks still poll (spurious
 * give-ups).  psfm_dist.py has the all-reduce of the step marks there.  A launch that gives up (a rank missing, not co-resident) raises the stall flag on every rank --
 * psfm_shard_window_state reports it and the caller redoes that solve with psfm_shard_solve_export / _control. */
psfm_status psfm_shard_peer_area(psfm_ctx* ctx, void** area_dev, void* ipc_handle_64, void* stream);
psfm_status psfm_shard_peer_open(psfm_ctx* ctx, const void* ipc_handle_64, int peer_rank, void** mapped);
/* The last epoch a launch of this context tagged its area's granules with.  A driver starts a run from the maximum over the ranks (an
 * area outlives the engine object that drove it: starting over would let stale granules match) and resets every rank's area
 * (reset != 0, between two collectives) before the 20-bit count wraps. */
psfm_status psfm_shard_peer_epoch(psfm_ctx* ctx, uint32_t* last_epoch, int reset, void* stream);
psfm_status psfm_shard_peer_connect(psfm_ctx* ctx, int world, int rank, void* const* areas, const int32_t* n_blocks);
psfm_status psfm_shard_solve_blocks(psfm_ctx* ctx, int32_t* n_blocks);
psfm_status psfm_shard_solve_peer(psfm_ctx* ctx, const float* flow01, const float* flow12, const float* flow02, const uint8_t* occ02,
                                  int frame, uint32_t epoch, void* stream);

/* the stall flag as of the last control step the device has completed, without synchronising (-1: none) */
psfm_status psfm_shard_peek_stall(psfm_ctx* ctx, int32_t* stalled_frame);
psfm_status psfm_shard_solve_restore(psfm_ctx* ctx, int frame, void* stream);
psfm_status psfm_shard_solve_writeback(psfm_ctx* ctx, int frame, const psfm_solve_stats* stats, void* stream);
psfm_status psfm_shard_solve_record(psfm_ctx* ctx, const psfm_solve_stats* stats);
psfm_status psfm_shard_finish(psfm_ctx* ctx, psfm_track_info* info_host, void* stream);
/* keys_dev (n_traj) i64 DEVICE: (last valid time << 47) | (birth frame << 31) | birth grid index of every trajectory of the
 * result, ascending -- the order key of full_trajs (SURVEY a-17); a trajectory's id over all ranks = its key's rank. */
psfm_status psfm_result_keys(psfm_ctx* ctx, int sample_ratio, int w, int64_t* keys_dev, void* stream);

/* Per-kernel device time of the last psfm_track / psfm_flow_check when profiling is enabled with
 * psfm_ctx_set_profiling(ctx, 1): HIP events recorded on the launch stream around every launch of
 * the named kernel family (enable = N > 1: only every N-th per-frame chain_step launch is timed, which keeps the
 * event overhead out of a throughput measurement; a persistent launch is always timed and counts as ONE launch).
 * kind: 0 flow_check, 1 chain_step, 2 respawn, 3 solver, 4 finalize.
 * Returns the accumulated milliseconds and the number of launches. */
psfm_status psfm_ctx_set_profiling(psfm_ctx* ctx, int enable);
psfm_status psfm_profile_get(psfm_ctx* ctx, int kind, double* total_ms, int64_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* PSFM_H_ */
