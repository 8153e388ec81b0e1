// psfm_internal.h -- host-side context and launcher prototypes (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <functional>
#include <shared_mutex>
#include <string>
#include <vector>

#include "../../include/psfm.h"

#define PSFM_MAX_PEERS 8      // ranks of one solve (psfm_shard_peer_*): the GPUs of one node

void psfm_set_error(const char* fmt, ...);

#define PSFM_HIP(expr)                                                                          \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess) {                                                                 \
            psfm_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return PSFM_ERR_HIP;                                                                \
        }                                                                                       \
    } while (0)

// A frame size every kernel can address: the samplers reach a map as base + a 32-bit BYTE offset (psfm_device.h: "every map / table
// here is < 4 GB"), so the largest per-frame map -- (H,W,2) f32 = 8 H W bytes -- must stay below 2^32 (H W < 2^29: 23170 x 23170;
// a 1080p frame is 2^21).  Every entry point that takes h, w checks this first (PSFM_ERR_ARG), none wraps silently.
static inline bool psfm_frame_ok(int h, int w) { return h >= 2 && w >= 2 && (int64_t)h * (int64_t)w * 8 < ((int64_t)1 << 32); }

// Per device and process: every entry point that launches kernels or copies holds this gate SHARED; the persistent frame
// loop needs it EXCLUSIVE.  All blocks of that kernel must be resident at once, and with another queue feeding the device
// they may never be (measured: a second host thread running psfm_connect alongside stalls the loop until its spin limit)
// -- so it only runs when no other psfm call of this process is in flight on the device, and calls that arrive meanwhile
// wait for it (<= a few ms).  A call that finds the device busy uses per-frame launches, which overlap well with other
// sequences.  (Other PROCESSES on the device are not covered: there the loop's bounded spin and its hand-over to
// per-frame launches are the safety net.)
std::shared_mutex& psfm_device_gate(int device);
int psfm_gate_waiters(int device);             // psfm calls of this process currently blocked behind an exclusive holder on the device
void psfm_gate_waiters_add(int device, int d);
struct PsfmGate {
    std::shared_mutex& m;
    int device;
    bool exclusive = false;
    PsfmGate(int dev, int want_exclusive /* 0 no, 1 if free, 2 wait for it */) : m(psfm_device_gate(dev)), device(dev)
    {
        if (want_exclusive == 2) { m.lock(); exclusive = true; }
        else if (want_exclusive == 1 && m.try_lock()) exclusive = true;
        else if (!m.try_lock_shared()) {
            // somebody holds the device exclusively (a persistent launch, or a track_optimize sequence running its solves as
            // resident launches): say so -- a sequence gives the device up at its next checkpoint (yield_exclusive) -- and wait
            psfm_gate_waiters_add(device, 1);
            m.lock_shared();
            psfm_gate_waiters_add(device, -1);
        }
    }
    // An exclusive holder whose work can go on with plain launches lets the waiting calls in (call with nothing of this call in
    // flight on the device: behind a stream synchronisation).  Returns true when it gave the device up.
    bool yield_exclusive()
    {
        if (!exclusive || psfm_gate_waiters(device) <= 0) return false;
        m.unlock();
        exclusive = false;
        m.lock_shared();
        return true;
    }
    ~PsfmGate() { if (exclusive) m.unlock(); else m.unlock_shared(); }
    PsfmGate(const PsfmGate&) = delete;
    PsfmGate& operator=(const PsfmGate&) = delete;
};

// grow-only device buffer
struct PsfmBuf {
    void* p = nullptr;
    size_t bytes = 0;
    psfm_status ensure(size_t need);
    void release();
    template <class T> T* as() const { return (T*)p; }
};

// Device-side counters of the frame recurrence (one cache line, zeroed at init).
struct PsfmCounters {
    int n_lanes;      // lanes ever handed out (high-water mark); chain_step scans [0, n_lanes)
    int overflow;     // bit0: lane table / free stack full, bit1: trajectory table full, bit2: more tracks than resident
                      // lanes (persistent loop), bit3: barrier spin limit hit (persistent loop), bit4: a batched frame launch
                      // covered fewer lanes than the sequence had in use (psfm_batch.hip runs the batch again, untrimmed)
    int stall;        // != 0: solve of frame stall-1 ran out of unrolled iterations; later launches are no-ops
    int abort;        // persistent frame loop: a block gave up (spin limit); every block leaves at its next barrier
    int spill_cnt;    // persistent frame loop: records written to the shared tail behind the private segments
    int sel;          // track_optimize: iterate buffer that holds the accepted positions (times f, f+1) of the last fused
                      // solve; 0 = they are in the log.  The next chain step copies them on its way (psfm_chain_step.h)
    int n_lanes_snap[2]; // n_lanes as the launch in front of frame f left it, in entry f & 1 (set by track_init, by the control
                      // thread of the frame kernel of f-1 and by the solver's write-back): the tile bound every block of the frame
                      // kernel of f agrees on -- n_lanes itself grows while that launch runs, and nothing it reads changes under it
    // device-paced sequence (psfm_seq_kernel): which frame the next launch works on (pc_phase 0: its chain step + fused solve,
    // 1: more iterations of its solve), which launch that is (a block of an earlier launch that starts after its control thread
    // has moved on must not pick the new work up), iterations per fused launch
    int pc_frame, pc_phase, pc_owner, solve_K;
    int pad[4];
};

// Death records and free lanes are published through PSFM_NSHARD independent tables so that the
// per-block atomics land on different words (a single word saturates at ~88 atomics/us on MI355X).
#define PSFM_NSHARD 64
struct PsfmShard {
    int fin_cnt;      // trajectory records written into this shard's slice
    unsigned points;  // trajectory points written through this shard's blocks (set 0 only)
    int pad0[30];
    int free_top;     // top of this shard's free-lane stack
    int pad1[31];
};

enum { PSFM_PROF_FLOW_CHECK = 0, PSFM_PROF_CHAIN = 1, PSFM_PROF_RESPAWN = 2, PSFM_PROF_SOLVER = 3,
       PSFM_PROF_FINALIZE = 4, PSFM_PROF_KINDS = 5 };

struct PsfmProfiler {
    bool enabled = false;
    int stride = 1;          // kernel_span() hands out events for every `stride`-th call only
    int64_t calls = 0;
    struct Span { int kind; hipEvent_t a, b; };
    std::vector<Span> spans;
    std::vector<hipEvent_t> pool;
    double total_ms[PSFM_PROF_KINDS] = {0};
    int64_t launches[PSFM_PROF_KINDS] = {0};
    hipEvent_t get();
    void begin(int kind, hipStream_t s);
    void kernel_span(int kind, hipEvent_t* a, hipEvent_t* b, bool always = false);  // events for hipExtLaunchKernelGGL (exact kernel begin/end)
    void end(hipStream_t s);
    void collect();  // after a stream sync: fold spans into totals
    void reset();
    void destroy();
};

// Device control block of the path-consistency solver (written by the last block of each kernel).
struct PsfmSolveCtrl;

struct PsfmTrackDims;

struct psfm_ctx {
    int device = 0;
    double lane_factor = 2.0, traj_factor = 8.0;
    // frame recurrence workspace
    PsfmBuf log;          // (n_flows+1) x cap double2
    PsfmBuf birth_frame;  // cap i32, -1 = free lane
    PsfmBuf birth_idx;    // cap i32
    PsfmBuf free_stack;   // 2 sets x PSFM_NSHARD x free_cap i32 (double-buffered by frame parity)
    PsfmBuf fin_keys;     // traj_cap u64
    PsfmBuf fin_lanes;    // traj_cap i32
    PsfmBuf occupied;     // 2 x G u8: frame-stamped grid-resolution `blocked` maps
    PsfmBuf counters;     // PsfmCounters
    PsfmBuf shards;       // 2 x PSFM_NSHARD x PsfmShard
    PsfmBuf survivors;    // (n_flows+1) i32
    // persistent frame loop (psfm_persist.hip)
    PsfmBuf handoff;      // cap x 3 u64: newborn handed to the owner of a popped lane
    PsfmBuf seg_info;     // per block: records in its private segment, trajectory points it wrote
    PsfmBuf seg_table;    // finalize: (src start, count, dst start) per record segment
    PsfmBuf persist_bar;  // barrier: 64 arrival counters, 1 top counter, 64 release flags (128 B apart)
    PsfmBuf place_tab;    // birth masks per (frame, 64 grid points) as the loop leaves them | births of the virtual blocks as starts inside the frame | births per frame (psfm_place.h)
    int persist_max_blocks = -1;   // resident 256-thread blocks on this device (-1: not queried yet)
    int chain_mode = 0;            // 0 auto, 1 per-frame launches only, 2 persistent loop required
    bool mb_enable = false;        // psfm_ctx_set_motion_boundary: tracks also die on motion boundaries (per-frame launches; psfm_connect_batch
                                   // when every context of the batch has it on)
    float mb_thres = 0.02f;
    PsfmBuf kill;                  // ... the kill maps of the sequence: (n_flows,H,W) u8, bit 0 occlusion, bit 1 motion boundary
    void* host_seg = nullptr;      // pinned staging for seg_info / seg_table
    size_t host_seg_bytes = 0;
    // finalize workspace + result
    PsfmBuf sort_keys, sort_lanes, sort_tmp, scan_tmp;
    PsfmBuf fin_marks;            // finalize: first sorted record of every (last, birth) group; all -1 between two calls (fin_marks_clean)
    bool fin_marks_clean = false;
    int fin_sort_form = 0, fin_offsets_form = 0;   // what the last finalize ran: sort_form / offsets_form of its plan (psfm_fin_form,
                                                   // psfm_finalize_plan.h), 0 until that step was reached (psfm_ctx_get_finalize_forms)
    int fin_placed = 0;                            // ... and whether its records were placed by birth order and sorted in one pass (psfm_place.h)
    int fin_gather = 0;                            // ... and its gather from the flow log: 0 none (position log), 1 serial sums, 2 blocked sums (psfm_gather_exact.h)
    PsfmBuf res_birth, res_len, res_off, res_xy;
    int64_t res_n_traj = 0, res_n_points = 0;
    int res_n_flows = 0;           // flows of the sequence the result came from (psfm_result_keys checks its packed key)
    bool res_is_query = false;     // the result is psfm_track_queries': trajectory i is query i, no birth grid index (psfm_result_keys
                                   // refuses it); cleared by every other entry point that replaces the result
    bool res_is_set = false;       // the result is psfm_result_set's / psfm_load_track_npy's: a set from elsewhere expanded to index == id,
                                   // ids it does not hold as entries with len = 0 -- no birth grid index (psfm_result_keys refuses it), and
                                   // the filter and the samplers refuse traj_min_len < 1 on it; cleared like res_is_query
    PsfmBuf rs_ws, rs_rec;         // psfm_result_set.hip: verdict block | the staged ids, births, lengths, record slices; a file's records
    PsfmBuf rs_birth, rs_len, rs_off, rs_xy;   // ... the next result while it is validated: exchanged with res_* behind a clean verdict
    PsfmBuf qr_ws;                 // psfm_track_queries (psfm_query.hip): first refused query | lengths per direction | scan storage
                                   // (psfm_track_queries_optimize, psfm_query_pc.hip: ... | rows per wave | the rows of a frame's solve)
    // psfm_track_queries_batch (psfm_query_batch.hip), this context as the call's owner: the table of sequences | the block prefix |
    // the refusal slots; lengths per direction of all sequences | scan storage | point totals; their pinned staging; the census of
    // the last call (psfm_query_batch_census)
    PsfmBuf qb_tab, qb_ws;
    void* qb_host = nullptr;
    int32_t qb_launches = 0, qb_syncs = 0;
    // psfm_track_queries_optimize_batch (psfm_query_pc_batch.hip), this context as the call's owner: the tables of the frame loop and of
    // the multi-problem solves | rows per wave of all sequences, row counts; the pinned staging of the tables and of the poll; the
    // census of the last call (psfm_query_pc_batch_census).  Every context of a call: the owner (query) of every row of its solve
    PsfmBuf qpb_tab, qpb_ws, qpb_owner;
    void* qpb_host = nullptr;
    int32_t qpb_fixed = 0, qpb_iter = 0, qpb_syncs = 0;
    // solver workspace
    PsfmBuf sol_x, sol_state, sol_partials, sol_ctrl, sol_misc, sol_stats, sol_fused, sol_bar;
    PsfmBuf sol_list;              // launch chain / resident solve: per block, the lanes that take part in the solve (pc_build_list)
    int pc_persist_blocks[4] = {-1, -1, -1, -1};   // co-resident blocks of psfm_pc_resident_kernel<NS> on this device (-1: not queried yet)
    bool pc_persist_ok = false;    // this call has the device to itself (or a resident budget): the launch chain may run as one persistent launch
    int resident_budget = 0;       // psfm_ctx_set_resident_budget: > 0 = resident solves of at most that many blocks under the SHARED gate
    unsigned pc_epoch = 0;         // resident solve: launch counter, part of every granule's tag (stale granules never match)
    // ONE solve over several ranks (psfm_shard_peer_*): this rank's granule area (member rows + the leader rows every rank writes into),
    // the other ranks' leader areas as this process addresses them, every rank's leader count
    PsfmBuf peer_area;
    unsigned peer_epoch = 0;         // the last epoch a launch of this context tagged granules of the area with: a new engine on the same
                                     // context (same area) must go on from here, never start over (stale granules would match)
    int peer_world = 0, peer_rank = 0;
    int peer_L[PSFM_MAX_PEERS] = {0};
    void* peer_lead[PSFM_MAX_PEERS] = {nullptr};
    void* peer_opened[PSFM_MAX_PEERS] = {nullptr};   // mappings this context opened with hipIpcOpenMemHandle (closed with it)
    int pc_giveups = 0;            // resident solves of this call whose hand-off timed out (two of them: launches from there on)
    int solve_K = 4;        // fused solve: trust-region iterations speculated per launch (adapted at checkpoints)
    int solve_mode = 0;     // 0 fused solve (one launch per frame), 1 launch chain (sequences whose solves reject steps)
    int solver_mode = 0, solver_K = 0;   // psfm_ctx_set_solver: 0 adaptive / 1 chain / 2 fused; K 0 = adaptive
    int64_t n_fused_ok = 0, n_fused_redone = 0, n_chain = 0;   // solves of the last psfm_track by how they ran
    int64_t n_resident = 0, n_iter_launches = 0;               // launches of the last call: resident solves, single trust-region iterations
    PsfmTrackDims* shard_dims = nullptr;   // psfm_shard_begin .. psfm_shard_finish
    bool shard_optimize = false;
    int solve_unroll = 6;   // iterations enqueued per frame without polling (adapted at checkpoints)
    PsfmBuf occ_own, occ2_own;           // occlusion maps of psfm_connect when the caller passes none
    PsfmBuf batch_tab, batch_ws, batch_fc;   // psfm_connect_batch (this context as the batch's owner): the table of sequences, packed
                                         // checkpoints, the table of stacks for flow_check (behind it, option on: the one for the kill maps)
    PsfmBuf batch_km;                    // psfm_kill_map_batch: its table of stacks
    void* host_batch = nullptr;          // ... and their pinned staging
    size_t host_batch_bytes = 0;
    void* host_batch2 = nullptr;
    size_t host_batch2_bytes = 0;
    int64_t batch_notrim_shape = 0;      // (h, w, sample_ratio, mode; the largest frame of a batch of several sizes) whose sequences once outgrew launches trimmed to the lanes in use
    int batch_h = 0, batch_w = 0;        // psfm_ctx_set_frame_size: the frame size of the sequence this context holds in a psfm_connect_batch
                                         // call with h = w = 0 (sequences of different frame sizes); 0, 0: none.  Nothing else reads it
    int batch_redo = 0;                  // psfm_ctx_set_batch_redo (read from the batch's owner): sequences that leave the fused batch run
                                         // 0 alone through psfm_connect, 1 together through the frame-mode multi-problem launch chain
    // the census of the last psfm_connect_batch (psfm_connect_batch_census): sequences that left the fused batch, those that went through
    // redo_together, and that run's launches / iteration launches / host synchronisations
    int32_t bt_left = 0, bt_together = 0, bt_fixed = 0, bt_iter = 0, bt_syncs = 0;
    PsfmBuf win_ws;                      // psfm_window_sample / psfm_result_filter workspace
    // psfm_window_sample_batch (psfm_window_batch.hip): the selection of all windows of one call, kept between a plan call and its
    // fill calls.  A buffer of its own: psfm_window_sample and psfm_result_filter may run in between and reuse win_ws.
    PsfmBuf winb_ws;
    void* winb_host = nullptr;           // pinned: the windows' first rows in the pre-cap list (65 int64)
    struct PsfmWinbPlan {
        bool valid = false;
        uint64_t res_gen = 0;
        int n_win = 0, n_frames = 0, traj_min_len = 0, min_length = 0;
        int64_t max_num = 0;
        int frame0[64];                          // (64 = PSFM_WINB_MAX = PSFM_DEC_BATCH_MAX windows per call)
        uint64_t seed[64];
        int64_t k[64];           // rows per window, after the cap
        size_t src[64];          // where the window's ids lie in winb_ws, in bytes
    } winb;
    PsfmBuf flt_ids, flt_birth, flt_len, flt_off, flt_xy;   // psfm_result_filter: the saved set (length >= traj_min_len), CSR
    int64_t flt_n_traj = 0, flt_n_points = 0;
    // psfm_traj_to_matches (psfm_matches.hip): keypoint / match tables of the saved set
    PsfmBuf mt_kp_off, mt_q, mt_pts, mt_kp_ind, mt_kp_xy, mt_moff, mt_keys, mt_rows, mt_gid, mt_pairs;
    int64_t mt_n_kp = 0, mt_n_m = 0, mt_n_pairs = 0;
    int mt_n_img = 0;
    // psfm_result_filter_batch / psfm_*_to_matches_batch (psfm_matches_batch.hip), this context as the call's owner: the table of
    // sequences, the per-sequence sizes and flags a synchronisation reads back, the filter's kept lengths; their pinned staging; the
    // census of the last call (psfm_matches_batch_census)
    PsfmBuf mtb_tab, mtb_sizes, mtb_len;
    void* mtb_host = nullptr;
    int32_t mtb_syncs = 0, mtb_launches = 0;
    // psfm_labels_* (psfm_labels.hip): per-window motion labels merged over the saved set, and the labelled set built from them
    uint64_t res_gen = 0;                // bumped by every entry point that replaces the result or the saved set (psfm_track, psfm_connect,
                                         // psfm_connect_batch, psfm_result_filter): what psfm_labels_begin ties its state to
    uint64_t lb_gen = 0;
    bool lb_active = false, lb_finished = false;
    int64_t lb_rows = 0;                 // rows merged so far (the sequence number of the next window's row 0)
    PsfmBuf lb_state, lb_first, lb_flag; // per saved point u8 (255 unlabelled, 0 static, 1 dynamic); per saved trajectory u32; error flag
    PsfmBuf lb_ws;                       // finish: counts, sort halves
    PsfmBuf lb_ids, lb_off, lb_frames, lb_xy, lb_labels;   // the labelled set, CSR in order of first appearance
    int64_t lb_n_traj = 0, lb_n_points = 0;
    // psfm_matches_to_database (psfm_database.hip): the COLMAP database tables, a copy of their own beside the match tables
    PsfmBuf db_kp, db_pairs, db_rows, db_ws;   // kp f32 (n_kp,2); pair_id | pair_key | pair_off, db_cap entries apart; rows u32; workspace
    int64_t db_n_kp = 0, db_n_pairs = 0, db_n_rows = 0, db_cap = 0;
    int db_n_img = 0;
    bool db_valid = false;
    bool db_src_live = false;            // the match tables are still the ones the database tables were built from (psfm_database_compact_again)
    // psfm_sparse_depth (psfm_sparse_depth.hip): winner map | point rows of the observations | descriptors | flags
    PsfmBuf sd_ws;
    int64_t sd_budget = 1ll << 30;       // bytes of maps + winners (12 per pixel) the callers put into one call; 0: no limit
    bool sd_timing = false;              // record events around the fill, the winner pass and the store pass
    hipEvent_t sd_events[4] = {nullptr, nullptr, nullptr, nullptr};
    double sd_ms[3] = {0.0, 0.0, 0.0};
    // psfm_depth_display (psfm_depth_display.hip): counts | histograms | selection state | descriptors | table; the compacted values
    PsfmBuf dd_ws, dd_comp;
    bool dd_timing = false;              // record events around the count, compact, select and colour passes
    hipEvent_t dd_events[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    double dd_ms[4] = {0.0, 0.0, 0.0, 0.0};
    PsfmBuf gt_flag;                     // psfm_traj_vote_labels (psfm_ground_truth.hip): a present point outside the image
    hipStream_t side_stream = nullptr;   // flow_check of psfm_connect runs here, ahead of the frame loop
    hipStream_t copy_stream = nullptr;   // psfm_load_flo_stack: H2D copies out of the pinned ring
    hipStream_t copy_stream2 = nullptr;  // ... every second slot's copies (two SDMA engines; PSFM_FLO_COPY_STREAMS=1: one)
    std::vector<void*> ingest_slots;     // ... the ring (pinned, ingest_slot_bytes each) and the event behind the last copy out of every slot
    std::vector<hipEvent_t> ingest_events;
    size_t ingest_slot_bytes = 0;
    hipStream_t redo_stream = nullptr;   // psfm_connect_batch: a sequence that left the batch runs here, beside the others that did
    std::vector<psfm_solve_stats> solve_stats;
    PsfmProfiler prof;
    void* host_pinned = nullptr;  // small pinned staging block
    size_t host_pinned_bytes = 0;
};
// ... behind its first 512 bytes (scalar read-backs, each at its user's own offset): finalize's copy of one set of shard tables, then the
// solver's control block
static inline PsfmShard* psfm_host_shards(const psfm_ctx* c) { return (PsfmShard*)((char*)c->host_pinned + 512); }
static inline PsfmSolveCtrl* psfm_host_solve_ctrl(const psfm_ctx* c) { return (PsfmSolveCtrl*)(psfm_host_shards(c) + PSFM_NSHARD); }

// A result that came from psfm_result_set / psfm_load_track_npy holds entries with len = 0 for the ids the set does not name; the
// filter and the samplers skip them with the arithmetic they have as long as traj_min_len >= 1, so they refuse anything below.
static inline bool psfm_set_result_refuses(const psfm_ctx* c, int traj_min_len, const char* who)
{
    if (!c->res_is_set || traj_min_len >= 1) return false;
    psfm_set_error("%s: traj_min_len=%d on a result that psfm_result_set / psfm_load_track_npy put in (ids the set does not hold are "
                   "entries of length 0: traj_min_len must be >= 1)", who, traj_min_len);
    return true;
}

// What a call that runs the frame recurrence (psfm_track / psfm_connect, psfm_connect_batch per sequence) starts from: no solve
// statistics, no result, no solves counted.  pc_persist_ok: the call has the device to itself (or a resident budget).
static inline void psfm_call_begin(psfm_ctx* c, int n_flows, bool pc_persist_ok)
{
    c->solve_stats.clear();
    c->res_n_traj = c->res_n_points = 0;
    c->res_n_flows = n_flows;
    c->res_is_query = false;
    c->res_is_set = false;
    c->pc_persist_ok = pc_persist_ok;
    c->pc_giveups = 0;
    c->n_fused_ok = c->n_fused_redone = c->n_chain = 0;
    c->n_resident = c->n_iter_launches = 0;
}

// ... and what it reports behind its finalize and the stream synchronisation (info may be NULL)
static inline void psfm_fill_track_info(psfm_track_info* info, const psfm_ctx* c, int64_t cap, int64_t total_iters, int chain_mode)
{
    if (!info) return;
    memset(info, 0, sizeof(*info));
    info->n_traj = c->res_n_traj;
    info->n_points = c->res_n_points;
    info->n_lanes_peak = ((const PsfmCounters*)c->host_pinned)->n_lanes;
    info->lane_capacity = cap;
    info->solver_iterations = total_iters;
    info->n_solves = (int32_t)c->solve_stats.size();
    info->chain_mode = chain_mode;
}

// Occlusion maps produced on a side stream while the frame loop consumes them (psfm_connect, psfm_connect_batch): one event per
// chunk of frame pairs; the loop waits for the chunk that contains the pair it is about to read.  The events come from the owner's
// profiler pool and go back there when the call ends, however it ends (the stream is synchronised or the call failed; a recycled
// event is re-recorded before anything waits on it).
struct PsfmOccPipeline {
    psfm_ctx* owner;
    int chunk = 0;                       // frame pairs per chunk (0 = maps already complete)
    hipEvent_t start = nullptr;          // what the side stream waits for: whatever the caller enqueued in front of the call
    std::vector<hipEvent_t> ready;       // stride-1 maps: chunk c covers pairs [c*chunk, (c+1)*chunk)
    std::vector<hipEvent_t> ready_s2;    // stride-2 maps
    int waited = -1, waited_s2 = -1;
    explicit PsfmOccPipeline(psfm_ctx* c) : owner(c) {}
    PsfmOccPipeline(const PsfmOccPipeline&) = delete;
    PsfmOccPipeline& operator=(const PsfmOccPipeline&) = delete;
    ~PsfmOccPipeline()
    {
        if (start) owner->prof.pool.push_back(start);
        for (auto e : ready) owner->prof.pool.push_back(e);
        for (auto e : ready_s2) owner->prof.pool.push_back(e);
    }
    psfm_status need(int pair, bool s2, hipStream_t s)
    {
        if (chunk <= 0) return PSFM_OK;
        std::vector<hipEvent_t>& ev = s2 ? ready_s2 : ready;
        int& w = s2 ? waited_s2 : waited;
        const int cidx = pair / chunk;
        while (w < cidx && w + 1 < (int)ev.size()) {
            ++w;
            PSFM_HIP(hipStreamWaitEvent(s, ev[w], 0));
        }
        return PSFM_OK;
    }
};

// The maps the path-consistency solve of frame f reads (positions at f-1, f, f+1): the stride-1 flows of f-1 and f, the stride-2
// flow and occlusion map of f-1 (P = H W pixels per map)
struct PsfmSolveMaps { const float* flow01; const float* flow12; const float* flow02; const uint8_t* occ02; };
static inline PsfmSolveMaps psfm_solve_maps(const float* flows, const float* flows_f2, const uint8_t* occ_s2, int64_t P, int f)
{
    return {flows + (size_t)(f - 1) * P * 2, flows + (size_t)f * P * 2, flows_f2 + (size_t)(f - 1) * P * 2, occ_s2 + (size_t)(f - 1) * P};
}

// ---- launchers (psfm_track.hip) -------------------------------------------------------------
psfm_status psfm_launch_flow_check(const float* ff, const float* fb, int n_pairs, int h, int w, float thres,
                                   uint8_t* occ, float* err, hipStream_t s);
psfm_status psfm_launch_flow_check_bg(const float* ff, const float* fb, int n_pairs, int h, int w, float thres, uint8_t* occ,
                                      int n_blocks, hipStream_t s);
psfm_status psfm_launch_grid_sample(const float* map, int c, int h, int w, const double* xy, int64_t n,
                                    float* out, hipStream_t s);

struct PsfmTrackDims {
    int H, W, ratio, GW, GH, n_flows;
    int64_t G, cap, traj_cap;
    int shard_cap;          // trajectory records per shard (traj_cap = PSFM_NSHARD * shard_cap)
    int free_cap;           // free-lane stack entries per shard
    int nsh = PSFM_NSHARD;  // free-lane stacks in use (fewer on small grids)
    int shift_b, shift_d;   // key = death<<shift_d | birth<<shift_b | grid index
    float cw, ch;
    int nblk = 0, seg_cap = 0, spill_cap = 0;   // persistent loop: blocks, records per private segment, shared tail
    // track-sharded run (psfm_shard_*): births on grid points [g0, g0 + Gband) only; the two stamped blocked maps (+ the
    // survivor byte at offset G) live in a caller-owned buffer, `shard_pitch` bytes apart, that the ranks all-reduce
    int64_t g0 = 0, Gband = 0, shard_pitch = 0;
    uint8_t* shard_maps = nullptr;
};

psfm_status psfm_track_dims(psfm_ctx* c, int n_flows, int h, int w, int ratio, int64_t g_own, PsfmTrackDims& d);
psfm_status psfm_track_alloc(psfm_ctx* c, const PsfmTrackDims& d);
psfm_status psfm_launch_track_init(psfm_ctx* c, const PsfmTrackDims& d, hipStream_t s);
psfm_status psfm_launch_chain_step(psfm_ctx* c, const PsfmTrackDims& d, const float* flow, const uint8_t* occ,
                                   int frame, bool optimize, hipStream_t s);

// ---- the ingest pipeline (psfm_ingest.hip): reader threads -> the context's ring of pinned buffers -> copies on its copy streams ----
// psfm_ring_stream: item i of n is read by fill(i, slot, &bytes, err) into a slot of `slot_bytes` bytes and copied to dst(i); returns
// when the last copy has completed.  PSFM_ERR_ARG: a fill returned false, its message is in `err` (the caller words the error).  The
// caller holds the device gate.  psfm_ring_stream_file: a byte range of an open file, in 8 MiB chunks.
psfm_status psfm_ring_stream(psfm_ctx* c, const char* who, int64_t n, size_t slot_bytes, int n_threads, hipStream_t s,
                             const std::function<bool(int64_t, char*, size_t*, std::string&)>& fill,
                             const std::function<char*(int64_t)>& dst, std::string& err);
psfm_status psfm_ring_stream_file(psfm_ctx* c, const char* who, int fd, int64_t file_off, size_t nbytes, char* dst_dev, int n_threads,
                                  hipStream_t s, std::string& err);

// ---- motion boundary (psfm_motion_boundary.hip) ----------------------------------------------
// out[f,y,x] = motion-boundary bit of pixel (x, y) of flow map f: 0/1 when occ == NULL, else (occ != 0) | mb << 1 (the kill map)
psfm_status psfm_launch_motion_boundary(const float* flows, const uint8_t* occ, int n, int h, int w, float thres, uint8_t* out, hipStream_t s);
// psfm_launch_chain_step with the motion-boundary verdict: `kill` is the frame's kill map
psfm_status psfm_launch_chain_step_mb(psfm_ctx* c, const PsfmTrackDims& d, const float* flow, const uint8_t* kill, int frame, bool optimize,
                                      hipStream_t s);

// ---- query results (psfm_query.hip), shared by psfm_track_queries and psfm_track_queries_optimize (psfm_query_pc.hip) ----------
// PSFM_ERR_ARG naming the first query with a non-finite coordinate or a frame outside [0, n_flows] (first_bad: 8 bytes on the device)
psfm_status psfm_query_refuse(psfm_ctx* c, const char* who, const double* q_xy, const int32_t* q_t, unsigned Q, int n_flows,
                              unsigned long long* first_bad, hipStream_t s);
// births, lengths, offsets and the CSR of Q > 0 queries from the position slab in c->log and the directions' lengths (NULL: not tracked)
psfm_status psfm_query_finish(psfm_ctx* c, const int32_t* q_t, const int* len_f, const int* len_b, unsigned Q, int n_flows, int64_t* bsum,
                              int64_t* n_points, hipStream_t s);

// ---- psfm_track_queries_batch (psfm_query_batch.hip) as a frame: psfm_qb_run with hooks == NULL is that call; with hooks it is the
// staging, the refusals, the contexts' bookkeeping, the length scan and the CSR gather around ANOTHER tracking loop
// (psfm_track_queries_optimize_batch, psfm_query_pc_batch.hip) ----
struct PsfmQbSeq;         // psfm_query_batch.h
struct PsfmQbRun {
    psfm_ctx* own; psfm_ctx* const* ctxs; int n_seq;
    const PsfmQbSeq* tab_host;                  // the table as it was uploaded (masks: the kill maps under the motion-boundary option)
    const PsfmQbSeq* tab; const int* blk_end;   // ... and on the device, with the inclusive block prefix
    int blocks;                                 // of the flattened grids (> 0)
    bool mb;
    hipStream_t s;
};
struct PsfmQbHooks {
    const char* who;                                            // the entry point's name, for the refusals
    int chain_mode;                                             // what psfm_track_info::chain_mode reports
    psfm_status (*check)(void* user, int seq);                  // further argument checks: seq == -1 once in front, then per sequence
    psfm_status (*track)(void* user, const PsfmQbRun& run);     // the tracking: leaves every slab and the lengths per direction
    void* user;
};
psfm_status psfm_qb_run(psfm_ctx* const* ctxs, int n_seq, const float* const* flows_f, const uint8_t* const* occ_f,
                        const float* const* flows_b, const uint8_t* const* occ_b, const int* n_flows, const int* h, const int* w,
                        const double* const* q_xy, const int32_t* const* q_t, const int64_t* n_q, psfm_track_info* infos_host, void* stream,
                        const PsfmQbHooks* hooks);

// ---- batch: B sequences per launch (psfm_batch.hip; kernels beside their single-sequence forms) -------------------------------
#define PSFM_BATCH_MAX 64
struct PsfmBatchSeq;      // psfm_chain_step.h: one row of the batch table (chain-step arguments of frame 1 + strides)
struct PsfmFcSeq { const float* ff; const float* fb; uint8_t* occ; int n_pairs; int pad; };      // one stack of a batch for flow_check
bool psfm_flow_check_batch_ok(int h, int w, const void* ff, const void* fb, const void* occ);
psfm_status psfm_launch_flow_check_batch(const PsfmFcSeq* tab_dev, int n_seq, int pair0, int n_pairs, int h, int w, float thres, hipStream_t s);
void psfm_batch_fill_seq(psfm_ctx* c, const PsfmTrackDims& d, const float* flows, const uint8_t* occ, int64_t occ_pitch, PsfmBatchSeq* row);
psfm_status psfm_launch_track_init_batch(const PsfmBatchSeq* tab_dev, int n_seq, int64_t cap_max, hipStream_t s);
// mb: the rows' occlusion pointers are the sequences' kill maps and the step forms the motion-boundary verdict (psfm_motion_boundary.hip)
psfm_status psfm_launch_chain_step_batch(psfm_ctx* owner, const PsfmBatchSeq* tab_dev, int n_seq, int ratio, int64_t cap_max, int frame,
                                         bool optimize, bool mb, hipStream_t s);
psfm_status psfm_launch_chain_step_batch_mb(psfm_ctx* owner, const PsfmBatchSeq* tab_dev, int n_seq, int ratio, int64_t cap_max, int frame,
                                            bool optimize, hipStream_t s);
// the kill maps of a batch of stacks (psfm_motion_boundary.hip): one row per stack in device memory, frames [pair0, pair0 + n_pairs) of
// every stack in ONE launch.  vec: P even and every flow stack 16-byte aligned (psfm_kill_map_batch_vec_ok); else one pixel per thread
struct PsfmKmSeq { const float* flows; const uint8_t* occ; uint8_t* out; int n; float thres; };
bool psfm_kill_map_batch_vec_ok(int h, int w, const void* flows);
psfm_status psfm_launch_kill_map_batch(const PsfmKmSeq* tab_dev, int n_seq, int pair0, int n_pairs, int h, int w, bool vec, hipStream_t s);
// ... of stacks of DIFFERENT frame sizes (psfm_connect_batch with h = w = 0; rows, flattened grid and block rule: psfm_batch_shapes.h).
// psfm_*_shape_row fills a row from the stack and its frame size, all but its place in the grid (psfm_bs_fc_prefix / psfm_bs_km_prefix,
// which give `blocks`); the launches cover frames [pair0, pair0 + n_pairs) of every stack, as the two above.  Every stack has passed
// psfm_flow_check_batch_ok for its own frame size.
struct PsfmFcShapeRow;
struct PsfmKmShapeRow;
void psfm_fc_shape_row(const PsfmFcSeq& q, int h, int w, PsfmFcShapeRow* row);
psfm_status psfm_launch_flow_check_shapes(const PsfmFcShapeRow* tab_dev, const int* blk_end_dev, int blocks, int pair0, int n_pairs, float thres,
                                          hipStream_t s);
void psfm_km_shape_row(const PsfmKmSeq& q, int h, int w, PsfmKmShapeRow* row);
psfm_status psfm_launch_kill_map_shapes(const PsfmKmShapeRow* tab_dev, const int* blk_end_dev, int blocks, int pair0, int n_pairs, hipStream_t s);
// track_optimize rows (psfm_solver_batch.hip: chain-step arguments + solver parameters of frame 1 + strides) and their launches
size_t psfm_batch_seq_opt_bytes(void);
psfm_status psfm_batch_fill_seq_opt(psfm_ctx* c, const PsfmTrackDims& d, const float* flows, const uint8_t* occ, int64_t occ_pitch,
                                    const float* flows_f2, const uint8_t* occ_s2, void* row_host, hipStream_t s);
psfm_status psfm_launch_seq_batch(psfm_ctx* owner, const void* tab_dev, int n_seq, int ratio, int64_t cap_max, int n_launches, int launch_id0,
                                  bool mb, hipStream_t s);
psfm_status psfm_launch_seq_batch_mb(psfm_ctx* owner, const void* tab_dev, int n_seq, int ratio, int64_t cap_max, int n_launches, int launch_id0,
                                     hipStream_t s);      // (psfm_solver_batch_mb.hip: the chain step of the rows samples kill maps)
psfm_status psfm_launch_flush_batch(const void* tab_dev, int n_seq, int64_t cap_max, hipStream_t s);
psfm_status psfm_launch_batch_set_pc(const void* tab_dev, const int (*v)[4], int n_seq, hipStream_t s);
size_t psfm_batch_pack_row_bytes(int win);
psfm_status psfm_launch_batch_pack(const void* tab_dev, const int* lo, int n_seq, int win, char* out_dev, hipStream_t s);
// the frame-mode multi-problem launch chain (psfm_solver_multi.hip; index rules psfm_batch_chain.h): the per-frame solves of a table
// of sequences with one grid -- a row from the sequence's track_optimize row, one frame's solves (init launch, paced iteration
// launches and polls into pinned memory, write-back launch; the census counters are the caller's), what the last poll saw
size_t psfm_frame_row_bytes(void);
size_t psfm_frame_poll_bytes(void);
psfm_status psfm_frame_row_fill(psfm_ctx* c, const PsfmTrackDims& d, const void* seq_opt_row_host, void* row_host, int* n_blocks);
psfm_status psfm_frame_solve_batch(const void* rows_dev, int grid_x, int n_problems, int f, void* poll_pinned, int32_t* n_fixed,
                                   int32_t* n_iter, int32_t* n_syncs, hipStream_t s);
void psfm_frame_poll_read(const void* poll_pinned, int i, int* active, psfm_solve_stats* st, int* n_lanes, int* overflow, int* stall);
// one segmented finalize for all sequences of a batch (psfm_finalize.hip): ONE host synchronisation, ONE sort.  dims[i] are the
// sequences' dimensions (same key format); the shared workspace is `own`'s, results land in every context's own res_* buffers
psfm_status psfm_finalize_batch(psfm_ctx* own, psfm_ctx* const* ctxs, const PsfmTrackDims* dims, int n_seq, hipStream_t s);

// ---- match tables (psfm_matches.hip): the pipeline of psfm_traj_to_matches over any CSR of trajectories in HBM ----------------
// A point's frame is birth[t] + (p - off[t]) when `frames` is NULL (the saved set: contiguous frames), frames[p] otherwise (the
// labelled set: explicit frames, gaps allowed).  labels: NULL = keep every point, else points with labels[p] != 0 are dropped.
struct PsfmMatchSrc {
    int64_t k = 0, n_pts = 0;
    const int64_t* off = nullptr; const int* birth = nullptr; const int* frames = nullptr;
    const double2* xy = nullptr; const uint8_t* labels = nullptr;
    const char* who = "psfm_traj_to_matches";
};
psfm_status psfm_match_tables(psfm_ctx* c, const PsfmMatchSrc& src, int n_img, int sample_k, int64_t* n_kp_host, int64_t* n_matches_host,
                              int64_t* n_pairs_host, hipStream_t s);

// ---- persistent frame loop (psfm_persist.hip) ---------------------------------------------------
int psfm_persist_max_blocks(psfm_ctx* c);
int psfm_persist_guests(void);   // LDS-resident extra lanes per block
// flows_b != NULL: the occlusion maps are computed inside the loop (fused flow_check) and written to `occ`
psfm_status psfm_launch_chain_persist(psfm_ctx* c, const PsfmTrackDims& d, const float* flows, const uint8_t* occ,
                                      int64_t occ_pitch, const float* flows_b, float thres, hipStream_t s);

// ---- finalize (psfm_finalize.hip; its decisions and key codec: psfm_finalize_plan.h) ---------
psfm_status psfm_finalize(psfm_ctx* c, const PsfmTrackDims& d, hipStream_t s);
// psfm_sort.hip: stable LSD radix sort of (32-bit key, int) pairs for the finalize (input in half0 when the pass count is even, else half1 -- PsfmFinForm::first_half; result in half0)
int psfm_sort_pairs32_passes(unsigned end_bit);
int psfm_sort_pairs64_passes(unsigned end_bit);
psfm_status psfm_sort_pairs64(psfm_ctx* c, unsigned long long* k_half0, int* v_half0, unsigned long long* k_half1, int* v_half1, int64_t n, unsigned end_bit, hipStream_t s);
psfm_status psfm_sort_pairs32(psfm_ctx* c, unsigned* k_half0, int* v_half0, unsigned* k_half1, int* v_half1, int64_t n, unsigned end_bit, hipStream_t s);
// after psfm_launch_chain_persist; *fallback = true (and PSFM_OK): the loop gave up, rerun with per-frame launches
psfm_status psfm_finalize_persist(psfm_ctx* c, const PsfmTrackDims& d, bool* fallback, hipStream_t s);
// psfm_place.hip: the placed form of that finalize (psfm_place.h).  The loop's birth masks and what the scan makes of them live in
// c->place_tab (psfm_place_table_bytes, allocated in front of the loop's launch); psfm_place_records fills the second halves of
// sort_keys / sort_lanes in birth order, psfm_place_sort is the one stable pass on `last` from the second halves into the first
struct PsfmFinForm;
size_t psfm_place_table_bytes(const PsfmTrackDims& d);
psfm_status psfm_place_records(psfm_ctx* c, const PsfmTrackDims& d, const PsfmFinForm& f, int64_t n, hipStream_t s);
psfm_status psfm_place_sort(psfm_ctx* c, unsigned* k_half0, int* v_half0, const unsigned* k_half1, const int* v_half1, int64_t n, hipStream_t s);

// ---- solver (psfm_solver.hip: launch chain, resident solve, host driver; fused / frame / device-paced forms: psfm_solver_fused.hip) ----
// In-place solve on the trajectory log for frame index f (positions at f-1, f, f+1): enqueue `unroll`
// iterations without host synchronisation / resume a solve that raised the stall flag.
psfm_status psfm_solve_frame_enqueue(psfm_ctx* c, const PsfmTrackDims& d, const float* flow01, const float* flow12,
                                     const float* flow02, const uint8_t* occ02, int frame, int unroll, hipStream_t s);
psfm_status psfm_solve_frame_resume(psfm_ctx* c, const PsfmTrackDims& d, const float* flow01, const float* flow12,
                                    const float* flow02, const uint8_t* occ02, int frame, psfm_solve_stats* st,
                                    int try_fused_k, bool chain_stalled, hipStream_t s);
psfm_status psfm_solve_frame_fused(psfm_ctx* c, const PsfmTrackDims& d, const float* flow01, const float* flow12,
                                   const float* flow02, const uint8_t* occ02, int frame, int K, hipStream_t s);
psfm_status psfm_launch_frame(psfm_ctx* c, const PsfmTrackDims& d, const float* flow01, const float* flow12, const float* flow02,
                              const uint8_t* occ, const uint8_t* occ02, int frame, int K, hipStream_t s, double* export_sums = nullptr);
psfm_status psfm_launch_seq(psfm_ctx* c, const PsfmTrackDims& d, const float* flows, const uint8_t* occ, int64_t occ_pitch,
                            const float* flows_f2, const uint8_t* occ_s2, int n_launches, int launch_id0, hipStream_t s);
psfm_status psfm_solve_flush(psfm_ctx* c, const PsfmTrackDims& d, int frame, hipStream_t s);
psfm_status psfm_solve_prepare(psfm_ctx* c, const PsfmTrackDims& d, hipStream_t s);   // every solver buffer of a sequence, up front
int psfm_solve_kmax(void);
int psfm_resident_blocks(psfm_ctx* c);     // co-resident blocks of the resident solve on the context's device
// track-sharded runs (psfm_shard.hip)
void psfm_shard_abandon(psfm_ctx* c);   // a run that was begun and never finished (context teardown)
psfm_status psfm_solve_export(psfm_ctx* c, const PsfmTrackDims& d, const float* flow01, const float* flow12, const float* flow02,
                              const uint8_t* occ02, int frame, int kind, int K, double* sums_out, hipStream_t s);
psfm_status psfm_solve_control(psfm_ctx* c, const PsfmTrackDims& d, int frame, int kind, int K, const double* totals, hipStream_t s,
                               int* stall_host = nullptr);
psfm_status psfm_solve_state(psfm_ctx* c, int* done, int* stall, psfm_solve_stats* st, hipStream_t s);
psfm_status psfm_solve_restore(psfm_ctx* c, const PsfmTrackDims& d, int frame, hipStream_t s);
psfm_status psfm_solve_writeback(psfm_ctx* c, const PsfmTrackDims& d, int frame, hipStream_t s);
// Batch API form (psfm_optimize_location).
size_t psfm_peer_area_bytes(void);
size_t psfm_peer_lead_offset(void);
int psfm_peer_leaders(int n_blocks);
int psfm_solve_blocks(psfm_ctx* c, const PsfmTrackDims& d);
psfm_status psfm_solve_frame_enqueue_peer(psfm_ctx* c, const PsfmTrackDims& d, const float* flow01, const float* flow12,
                                          const float* flow02, const uint8_t* occ02, int frame, unsigned epoch, hipStream_t s);
psfm_status psfm_launch_pc_eval(const double* uv12, const double* ref1, const double* ref2, const double* scale, const float* flow12,
                                int64_t n, int w, int h, double* res, double* jac, hipStream_t s);
psfm_status psfm_solve_batch(psfm_ctx* c, const double* uv12, const double* ref1, const double* ref2,
                             const double* scale, const float* flow12, int64_t n, int w, int h, double* out,
                             psfm_solve_stats* st, hipStream_t s);
