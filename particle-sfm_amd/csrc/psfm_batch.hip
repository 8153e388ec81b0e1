// psfm_batch.hip -- psfm_connect_batch: B sequences (of one frame size, or each of its own) through ONE set of launches.
//
// The reference's driver walks a directory of sequences (run_particlesfm.py:168-176: connect_point_trajectory per sequence), and the
// sequences real data has are small: DAVIS 480x854 at sample_ratio 4 is 25 k grid points, Sintel 436x1024 at 2 is 112 k, ScanNet
// 640x480 dense 307 k (BASELINE configs[0] / [2] / [4]).  A frame of such a sequence is ONE dependent chain of memory round trips
// that occupies 100-1200 of the device's >= 2048 block slots for 8-45 us whatever its size: one sequence at a
// time leaves 75-97 % of the machine idle, and host threads + streams (point_trajectory.batch) buy back at most 2x
// (profiles/r05/r05_a_concurrent_small.txt) because every sequence still pays its own launches, checkpoints and finalize.
// Here blockIdx.y of every frame launch is the sequence:
//   * every sequence keeps its OWN context -- lane tables, log, counters, shard tables, solver buffers, result -- so a block only
//     needs its sequence's row of a small table in device memory (chain-step arguments of frame 1 + strides: the device-side
//     rebase of the device-paced sequence, psfm_chain_args_rebase / pc_params_rebase, turns them into any frame's);
//   * track mode: one psfm_chain_step_batch_kernel launch per frame index; track_optimize: psfm_seq_batch_kernel launches, every
//     sequence with its own device-side program counter and K -- sequences advance independently (one may continue a solve while
//     its neighbours take their next frame; a finished or stalled one turns its blocks into no-ops);
//   * ONE checkpoint (one packed copy, one synchronisation) per window of frames for all sequences, and ONE segmented finalize
//     (psfm_finalize_batch: one sort over the records of all sequences);
//   * a sequence whose solves reject steps (what the launch chain / the resident solve are for) is redone at the checkpoint like in
//     psfm_track; when a whole window of it is like that it leaves the batch and runs alone through psfm_connect afterwards
//     (redo_alone) -- or, with psfm_ctx_set_batch_redo(ctxs[0], 1), together with the others that left: one batched chain step per
//     frame and the frame's solves as the frame-mode multi-problem launch chain (redo_together, psfm_solver_multi.hip).
//   * psfm_ctx_set_motion_boundary on EVERY context of the batch: the frame launches are the MB forms of the two kernels
//     (psfm_motion_boundary.hip, psfm_solver_batch_mb.hip) and sample every sequence's kill maps (c->kill), built by ONE launch per
//     flow_check chunk for all sequences (psfm_kill_map_batch_kernel); contexts that disagree are refused.
//   * h = w = 0: every context carries its sequence's frame size (psfm_ctx_set_frame_size).  All equal: the run with that size.  Else
//     every sequence has its own dimensions wherever the run sizes, fills or launches per sequence (the rows already hold them);
//     flow_check and the kill maps run over a grid flattened over the sequences (psfm_batch_shapes.h); the records of all sequences
//     get the index bits of the widest grid, so that the one finalize sorts one key format (tests/test_gpu_batch_shapes.py).
// Results are those of psfm_connect, sequence by sequence (tests/test_gpu_batch.py: bit-identical to the oracle's).
#include <string.h>
#include <stdlib.h>
#include <algorithm>
#include <string>
#include <thread>
#include <vector>

#include "psfm_internal.h"
#include "psfm_chain_step.h"
#include "psfm_solve_policy.h"
#include "psfm_batch_chain.h"
#include "psfm_batch_shapes.h"

static_assert(PSFM_BS_MAX == PSFM_BATCH_MAX, "one bound for every batch entry point");

namespace {
struct SeqState {
    int f = 0;                   // first frame whose launch has not completed
    int first_unchecked = 1;     // first solve whose statistics have not been folded in
    bool resync = false;         // the device-side program counter must be set before the next window
    bool dropped = false;        // runs alone through psfm_connect behind the batch
    int k_dev = 3;               // solve_K as the device has it
    int64_t total_iters = 0;
    std::vector<psfm_solve_stats> hstats;
};
}  // namespace

static psfm_status batch_host_staging2(psfm_ctx* own, size_t need)
{
    if (own->host_batch2_bytes >= need) return PSFM_OK;
    if (own->host_batch2) (void)hipHostFree(own->host_batch2);
    own->host_batch2 = nullptr; own->host_batch2_bytes = 0;
    PSFM_HIP(hipHostMalloc(&own->host_batch2, need + 1024, hipHostMallocDefault));
    own->host_batch2_bytes = need + 1024;
    return PSFM_OK;
}

static psfm_status batch_host_staging(psfm_ctx* own, size_t need)
{
    if (own->host_batch_bytes >= need) return PSFM_OK;
    if (own->host_batch) (void)hipHostFree(own->host_batch);
    own->host_batch = nullptr; own->host_batch_bytes = 0;
    PSFM_HIP(hipHostMalloc(&own->host_batch, need + 4096, hipHostMallocDefault));
    own->host_batch_bytes = need + 4096;
    return PSFM_OK;
}

static psfm_status batch_run(psfm_ctx* const* ctxs, int n_seq, const float* const* flows_f, const float* const* flows_b,
                             const float* const* flows_f2, const float* const* flows_b2, const int* n_flows, int h, int w,
                             const int* hs, const int* ws, float thres, int ratio, psfm_track_info* infos, void* stream, bool trim,
                             bool* grid_too_small);

extern "C" psfm_status psfm_connect_batch(psfm_ctx* const* ctxs, int n_seq, const float* const* flows_f, const float* const* flows_b,
                                          const float* const* flows_f2, const float* const* flows_b2, const int* n_flows, int h, int w,
                                          float thres, int ratio, psfm_track_info* infos, void* stream)
{
    const bool per_ctx = h == 0 && w == 0;      // every context carries its sequence's frame size (psfm_ctx_set_frame_size)
    if (!ctxs || n_seq < 1 || n_seq > PSFM_BATCH_MAX || !flows_f || !flows_b || !n_flows || (!per_ctx && !psfm_frame_ok(h, w)) || ratio < 1 || ratio > 64 ||
        ((flows_f2 == nullptr) != (flows_b2 == nullptr))) {
        psfm_set_error("psfm_connect_batch: bad argument (n_seq=%d of at most %d, h=%d w=%d sample_ratio=%d)", n_seq, PSFM_BATCH_MAX, h, w, ratio);
        return PSFM_ERR_ARG;
    }
    const bool optimize = flows_f2 != nullptr;
    for (int i = 0; i < n_seq; ++i) if (ctxs[i]) ctxs[i]->res_gen++;
    for (int i = 0; i < n_seq; ++i) {
        if (!ctxs[i] || ctxs[i]->device != ctxs[0]->device) { psfm_set_error("psfm_connect_batch: context %d is NULL or on another device", i); return PSFM_ERR_ARG; }
        if (ctxs[i]->mb_enable != ctxs[0]->mb_enable) {      // (one kernel form per launch: all sequences with the second verdict, or none)
            psfm_set_error("psfm_connect_batch: context %d has psfm_ctx_set_motion_boundary %s and context 0 has it %s; a batch takes the option "
                           "on every context or on none (each with its own threshold)", i, ctxs[i]->mb_enable ? "on" : "off",
                           ctxs[0]->mb_enable ? "on" : "off");
            return PSFM_ERR_ARG;
        }
        for (int j = 0; j < i; ++j) if (ctxs[j] == ctxs[i]) { psfm_set_error("psfm_connect_batch: context %d given twice (one per sequence)", i); return PSFM_ERR_ARG; }
        if (n_flows[i] < 1 || !flows_f[i] || !flows_b[i] || (optimize && n_flows[i] > 1 && (!flows_f2[i] || !flows_b2[i]))) {
            psfm_set_error("psfm_connect_batch: bad sequence %d (n_flows=%d)", i, n_flows[i]);
            return PSFM_ERR_ARG;
        }
    }
    // h = w = 0: the frame sizes are the contexts'.  All equal: the call with that size; else hs / ws go with the run, and what is
    // remembered per shape below is remembered for the largest frame of the batch.
    int hsv[PSFM_BATCH_MAX], wsv[PSFM_BATCH_MAX];
    const int* hs = nullptr;
    const int* ws = nullptr;
    if (per_ctx) {
        bool same = true;
        for (int i = 0; i < n_seq; ++i) {
            if (!psfm_frame_ok(ctxs[i]->batch_h, ctxs[i]->batch_w)) {
                psfm_set_error("psfm_connect_batch: h = w = 0 and context %d has no frame size (psfm_ctx_set_frame_size)", i);
                return PSFM_ERR_ARG;
            }
            hsv[i] = ctxs[i]->batch_h; wsv[i] = ctxs[i]->batch_w;
            same = same && hsv[i] == hsv[0] && wsv[i] == wsv[0];
            if (i == 0 || (int64_t)hsv[i] * wsv[i] > (int64_t)h * w) { h = hsv[i]; w = wsv[i]; }
        }
        if (!same) { hs = hsv; ws = wsv; }
    }
    // The frame launches cover the lanes a sequence can be expected to use (its grid + 1/8), not its whole lane table (2 x the grid by
    // default): a block beyond the lanes in use leaves at once, but it still has to be dispatched -- half of the blocks of every launch
    // (PSFM_BATCH_GRID_TRIM=0: the whole table).  A launch that finds more lanes in use than it covers says so (overflow bit 16) and the
    // batch is run again with launches that cover the tables.
    static const bool trim_env = !(getenv("PSFM_BATCH_GRID_TRIM") && atoi(getenv("PSFM_BATCH_GRID_TRIM")) == 0);
    bool too_small = false;
    psfm_ctx* own0 = ctxs[0];
    const int64_t shape_key = ((int64_t)h << 40) ^ ((int64_t)w << 16) ^ (int64_t)ratio ^ (flows_f2 ? (1ll << 62) : 0);
    const bool trim = trim_env && own0->batch_notrim_shape != shape_key;      // (a shape whose sequences outgrew the trimmed launches once: not again)
    // (the counters a failed finalize reads the "grid too small" bit from are the ones THIS call refreshes: none left over from an earlier one)
    for (int i = 0; i < n_seq; ++i) if (ctxs[i]->host_pinned) ((PsfmCounters*)ctxs[i]->host_pinned)->overflow = 0;
    // A failed run leaves nothing in flight that still reads the caller's flow stacks or writes the maps: the side stream's flow_check
    // launches (and, with the motion-boundary option, the kill-map launches behind them) are drained before the error goes back (the
    // caller may free or reuse the tensors), and before the untrimmed rerun.
    auto quiesce = [&]() {
        if (hipSetDevice(own0->device) != hipSuccess) return;
        if (own0->side_stream) (void)hipStreamSynchronize(own0->side_stream);
        (void)hipStreamSynchronize((hipStream_t)stream);
    };
    psfm_status rc = PSFM_ERR_HIP;
    try {
        rc = batch_run(ctxs, n_seq, flows_f, flows_b, flows_f2, flows_b2, n_flows, h, w, hs, ws, thres, ratio, infos, stream, trim, &too_small);
        if (rc != PSFM_OK) quiesce();
        if (rc == PSFM_ERR_CAPACITY && too_small) {
            own0->batch_notrim_shape = shape_key;
            rc = batch_run(ctxs, n_seq, flows_f, flows_b, flows_f2, flows_b2, n_flows, h, w, hs, ws, thres, ratio, infos, stream, false, &too_small);
            if (rc != PSFM_OK) quiesce();
        }
    } catch (const std::exception& e) {      // (std::thread / std::vector: nothing may unwind through the extern "C" boundary)
        quiesce();
        psfm_set_error("psfm_connect_batch: %s", e.what());
        rc = PSFM_ERR_HIP;
    }
    return rc;
}

namespace {
// One run of the batch (batch_run): the call's arguments and what its steps share.
struct BatchRun {
    psfm_ctx* const* ctxs; int B;
    const float* const* flows_f; const float* const* flows_b; const float* const* flows_f2; const float* const* flows_b2;
    const int* n_flows;
    int h, w;                    // the frame size of all sequences; hs != NULL: of the largest one
    const int* hs; const int* ws;      // NULL, or the frame size of every sequence (a batch of several sizes)
    float thres; int ratio;
    hipStream_t s;
    bool trim; bool* grid_too_small;
    psfm_ctx* own;               // the batch's owner: shared workspaces, side stream, profiler
    bool optimize, mb;           // mb: psfm_ctx_set_motion_boundary, on in every context of the batch: the frame launches sample kill maps
    PsfmOccPipeline fc;          // the flow_check pipeline of all sequences, on the owner's side stream
    bool shapes() const { return hs != nullptr; }
    int fh(int i) const { return hs ? hs[i] : h; }
    int fw(int i) const { return ws ? ws[i] : w; }
    int64_t fP(int i) const { return (int64_t)fh(i) * fw(i); }      // pixels of a map of sequence i: the pitch of its map buffers
    std::vector<SeqState> S;
    std::vector<PsfmTrackDims> D;
    int n_max = 0;
    int64_t cap_max = 0, grid_lanes = 0;      // grid_lanes: lanes the frame launches cover (<= cap_max)
    static constexpr int CHECK = 16, win_max = CHECK + 2;      // frames between two checkpoints; launches of a window at the most
    size_t pack_row = 0, pack_bytes = 0;
    char* hpack = nullptr;       // the packed checkpoint of all sequences on the host
    PsfmBatchSeq* dtab = nullptr; char* dtabo = nullptr;      // the tables of sequences on the device: chain-step rows, track_optimize rows
    bool together = false;       // psfm_ctx_set_batch_redo(own, 1): sequences that leave the fused batch are redone by redo_together

    // (a sequence sent out before the first window has no maps of its own yet: redo_alone's psfm_connect makes them, redo_together
    // reads the batch's)
    bool no_maps(int i) const { return S[i].dropped && !together; }
    psfm_status prepare();
    psfm_status flow_check();
    psfm_status tables();
    psfm_status track_loop();
    psfm_status optimize_loop();
    psfm_status finalize(psfm_track_info* infos, std::vector<int>& redo);
    psfm_status redo_alone(const std::vector<int>& redo, psfm_track_info* infos, void* stream);
    psfm_status redo_together(const std::vector<int>& redo, psfm_track_info* infos);
};

// ---- dimensions (one key format for the whole batch: the time bits of its longest sequence, the index bits of its widest grid --
// psfm_bs_common_key -- written into every sequence's dimensions before anything is sized or filled from them), workspaces ----
psfm_status BatchRun::prepare()
{
    psfm_status st;
    S.resize((size_t)B); D.resize((size_t)B);
    for (int i = 0; i < B; ++i) n_max = n_flows[i] > n_max ? n_flows[i] : n_max;
    int sb[PSFM_BATCH_MAX];
    for (int i = 0; i < B; ++i) {
        psfm_shard_abandon(ctxs[i]);
        if ((st = psfm_track_dims(ctxs[i], n_flows[i], fh(i), fw(i), ratio, -1, D[i])) != PSFM_OK) return st;
        sb[i] = D[i].shift_b;
    }
    // (sequences of one frame size have one grid: their index bits are the common ones already)
    const PsfmBsKeyFmt key = psfm_bs_common_key(sb, n_flows, B);
    const int tbits = key.tbits;
    for (int i = 0; i < B; ++i) {
        psfm_ctx* c = ctxs[i];
        const size_t P = (size_t)fP(i);
        D[i].shift_b = key.shift_b;
        D[i].shift_d = key.shift_d;
        if (D[i].shift_d + tbits > 63) { psfm_set_error("psfm_connect_batch: key does not fit 64 bits"); return PSFM_ERR_ARG; }
        if ((st = psfm_track_alloc(c, D[i])) != PSFM_OK) return st;
        if ((st = c->occ_own.ensure(P * (size_t)n_flows[i])) != PSFM_OK) return st;
        if (mb && (st = c->kill.ensure(P * (size_t)n_flows[i])) != PSFM_OK) return st;
        if (optimize) {
            if ((st = c->occ2_own.ensure(P * (size_t)(n_flows[i] > 1 ? n_flows[i] - 1 : 1))) != PSFM_OK) return st;
            if ((st = psfm_solve_prepare(c, D[i], s)) != PSFM_OK) return st;
        }
        psfm_call_begin(c, n_flows[i], false);
        if (D[i].cap > cap_max) cap_max = D[i].cap;
        if (D[i].G + D[i].G / 8 + 2048 > grid_lanes) grid_lanes = D[i].G + D[i].G / 8 + 2048;
        S[i].hstats.assign((size_t)n_flows[i] + 1, psfm_solve_stats());
        // a context told to use the launch chain for every solve has nothing to gain from the fused batch: it runs alone -- or, with
        // psfm_ctx_set_batch_redo(own, 1), straight through redo_together, on the maps this run's flow_check makes for it
        if (optimize && c->solver_mode == 1 && (n_flows[i] >= 2 || together)) S[i].dropped = true;
    }
    if (trim && getenv("PSFM_BATCH_GRID_LANES")) grid_lanes = atoll(getenv("PSFM_BATCH_GRID_LANES"));      // (tests: launches that cover too little)
    if (!trim || grid_lanes > cap_max || grid_lanes < 256) grid_lanes = cap_max;
    return PSFM_OK;
}

// ---- flow_check of every stack (utils.py:94-105) ----
// Bandwidth-bound work beside a latency-bound frame loop: the maps are produced on the owner's side stream in chunks of
// frame pairs -- ONE launch per chunk for all sequences (psfm_flow_check_x2v_batch_kernel) -- and the frame loop only waits
// for the chunk it is about to read (what psfm_connect does for one sequence).  PSFM_BATCH_FC_CHUNK=0, or stacks the
// 16-byte-load kernel cannot take: every stack up front on the launch stream.
// Option on: every stride-1 chunk is followed, on the side stream, by the kill-map launch of the same frames of all sequences
// (psfm_kill_map_batch_kernel reads the occlusion bytes of those frames only) and the chunk's event is recorded behind it, so
// that waiting for a chunk is waiting for its kill maps; up front, the kill maps follow their stack's flow_check.
// Several frame sizes: the same pipeline with the two launches over a grid flattened over the sequences
// (psfm_flow_check_x2v_shapes_kernel, psfm_kill_map_shapes_kernel; psfm_batch_shapes.h); the rule for the up-front path is taken
// per batch -- ONE stack that fails the test for its own frame size sends all of them there (the per-stack launches take any size).
psfm_status BatchRun::flow_check()
{
    psfm_status st;
    const int fc_env = getenv("PSFM_BATCH_FC_CHUNK") ? atoi(getenv("PSFM_BATCH_FC_CHUNK")) : -1;
    int fc_chunk = fc_env >= 0 ? fc_env : (optimize ? 6 : 8);
    for (int i = 0; i < B && fc_chunk > 0; ++i) {
        if (no_maps(i)) continue;
        if (!psfm_flow_check_batch_ok(fh(i), fw(i), flows_f[i], flows_b[i], ctxs[i]->occ_own.p)) fc_chunk = 0;
        if (optimize && n_flows[i] > 1 && !psfm_flow_check_batch_ok(fh(i), fw(i), flows_f2[i], flows_b2[i], ctxs[i]->occ2_own.p)) fc_chunk = 0;
    }
    fc.chunk = fc_chunk;      // chunk c of the stride-1 / stride-2 maps: pairs [c * fc_chunk, (c + 1) * fc_chunk)
    own->prof.begin(PSFM_PROF_FLOW_CHECK, s);
    if (fc_chunk <= 0) {
        for (int i = 0; i < B; ++i) {
            if (no_maps(i)) continue;
            psfm_ctx* c = ctxs[i];
            const int hi = fh(i), wi = fw(i);
            if ((st = psfm_launch_flow_check(flows_f[i], flows_b[i], n_flows[i], hi, wi, thres, c->occ_own.as<uint8_t>(), nullptr, s)) != PSFM_OK) return st;
            if (optimize && n_flows[i] > 1 &&
                (st = psfm_launch_flow_check(flows_f2[i], flows_b2[i], n_flows[i] - 1, hi, wi, thres, c->occ2_own.as<uint8_t>(), nullptr, s)) != PSFM_OK) return st;
            if (mb && (st = psfm_launch_motion_boundary(flows_f[i], c->occ_own.as<uint8_t>(), n_flows[i], hi, wi, c->mb_thres, c->kill.as<uint8_t>(), s)) != PSFM_OK)
                return st;
        }
        own->prof.end(s);
        return PSFM_OK;
    }
    // (several frame sizes: the stacks are described here and their rows -- frame, chunks, place in the flattened grid,
    // psfm_batch_shapes.h -- are what is uploaded; rows of 80 bytes)
    const size_t fc_row = shapes() ? sizeof(PsfmFcShapeRow) : sizeof(PsfmFcSeq), km_row = shapes() ? sizeof(PsfmKmShapeRow) : sizeof(PsfmKmSeq);
    const size_t fc_bytes = fc_row * (size_t)B * 2;
    const size_t row_bytes = fc_bytes + (mb ? km_row * (size_t)B : 0);    // (rows of 32 bytes, both)
    // (... and behind the rows the three inclusive block prefixes, 64 entries each: stride-1 / stride-2 flow_check, kill maps)
    const size_t fbytes = row_bytes + (shapes() ? 3 * PSFM_BS_MAX * sizeof(int) : 0);
    if ((st = batch_host_staging2(own, fbytes)) != PSFM_OK) return st;
    if ((st = own->batch_fc.ensure(fbytes)) != PSFM_OK) return st;
    PsfmFcSeq fc_seq[2 * PSFM_BATCH_MAX];
    PsfmKmSeq km_seq[PSFM_BATCH_MAX];
    PsfmFcSeq* hfc = shapes() ? fc_seq : (PsfmFcSeq*)own->host_batch2;
    PsfmKmSeq* hkm = shapes() ? km_seq : (PsfmKmSeq*)((char*)own->host_batch2 + fc_bytes);
    for (int i = 0; i < B; ++i) {
        psfm_ctx* c = ctxs[i];
        hfc[i].ff = flows_f[i]; hfc[i].fb = flows_b[i]; hfc[i].occ = c->occ_own.as<uint8_t>(); hfc[i].n_pairs = no_maps(i) ? 0 : n_flows[i]; hfc[i].pad = 0;
        hfc[B + i].ff = optimize ? flows_f2[i] : nullptr; hfc[B + i].fb = optimize ? flows_b2[i] : nullptr;
        hfc[B + i].occ = optimize ? c->occ2_own.as<uint8_t>() : nullptr;
        hfc[B + i].n_pairs = (optimize && !no_maps(i) && n_flows[i] > 1) ? n_flows[i] - 1 : 0; hfc[B + i].pad = 0;
        if (mb) {
            hkm[i].flows = flows_f[i]; hkm[i].occ = c->occ_own.as<uint8_t>(); hkm[i].out = c->kill.as<uint8_t>();
            hkm[i].n = hfc[i].n_pairs; hkm[i].thres = c->mb_thres;
        }
    }
    int blocks_fc[2] = {0, 0}, blocks_km = 0;      // several frame sizes: gridDim.x of the stride-1 / stride-2 flow_check, of the kill maps
    if (shapes()) {
        PsfmFcShapeRow* rfc = (PsfmFcShapeRow*)own->host_batch2;
        PsfmKmShapeRow* rkm = (PsfmKmShapeRow*)((char*)own->host_batch2 + fc_bytes);
        for (int i = 0; i < B; ++i) {
            psfm_fc_shape_row(hfc[i], fh(i), fw(i), &rfc[i]);
            psfm_fc_shape_row(hfc[B + i], fh(i), fw(i), &rfc[B + i]);
            if (mb) psfm_km_shape_row(hkm[i], fh(i), fw(i), &rkm[i]);
        }
        int* ends = (int*)((char*)own->host_batch2 + row_bytes);
        PsfmKmShapeRow none[1];
        blocks_fc[0] = psfm_bs_fc_prefix(rfc, B, ends);
        blocks_fc[1] = psfm_bs_fc_prefix(rfc + B, B, ends + PSFM_BS_MAX);
        blocks_km = psfm_bs_km_prefix(mb ? rkm : none, mb ? B : 0, ends + 2 * PSFM_BS_MAX);
    }
    PSFM_HIP(hipMemcpyAsync(own->batch_fc.p, own->host_batch2, fbytes, hipMemcpyHostToDevice, s));
    if (!own->side_stream) PSFM_HIP(hipStreamCreateWithFlags(&own->side_stream, hipStreamNonBlocking));
    hipStream_t side = own->side_stream;
    fc.start = own->prof.get();      // the side stream starts behind whatever the caller enqueued on `stream` (the inputs, the table)
    PSFM_HIP(hipEventRecord(fc.start, s));
    PSFM_HIP(hipStreamWaitEvent(side, fc.start, 0));
    const PsfmFcSeq* dfc = own->batch_fc.as<PsfmFcSeq>();
    const PsfmKmSeq* dkm = (const PsfmKmSeq*)((const char*)own->batch_fc.p + fc_bytes);
    const PsfmFcShapeRow* dfs = own->batch_fc.as<PsfmFcShapeRow>();
    const PsfmKmShapeRow* dks = (const PsfmKmShapeRow*)((const char*)own->batch_fc.p + fc_bytes);
    const int* dends = (const int*)((const char*)own->batch_fc.p + row_bytes);
    // one launch for pairs [p0, p0 + np) of the stride-1 (s2 = 0) / stride-2 stacks of all sequences
    auto launch_fc = [&](int s2, int p0, int np) {
        if (shapes()) return psfm_launch_flow_check_shapes(dfs + s2 * B, dends + s2 * PSFM_BS_MAX, blocks_fc[s2], p0, np, thres, side);
        return psfm_launch_flow_check_batch(dfc + s2 * B, B, p0, np, h, w, thres, side);
    };
    for (int p0 = 0; p0 < n_max; p0 += fc_chunk) {
        const int np = n_max - p0 < fc_chunk ? n_max - p0 : fc_chunk;
        if ((st = launch_fc(0, p0, np)) != PSFM_OK) return st;
        // (the stacks passed psfm_flow_check_batch_ok: P even, flows 16-byte aligned -- the four-pixels-per-lane form)
        if (mb && (st = shapes() ? psfm_launch_kill_map_shapes(dks, dends + 2 * PSFM_BS_MAX, blocks_km, p0, np, side)
                                 : psfm_launch_kill_map_batch(dkm, B, p0, np, h, w, true, side)) != PSFM_OK) return st;
        hipEvent_t e = own->prof.get();
        fc.ready.push_back(e);
        PSFM_HIP(hipEventRecord(e, side));
        if (optimize && p0 < n_max - 1) {     // the stride-2 maps of the same time range follow their stride-1 chunk
            const int np2 = n_max - 1 - p0 < fc_chunk ? n_max - 1 - p0 : fc_chunk;
            if ((st = launch_fc(1, p0, np2)) != PSFM_OK) return st;
            hipEvent_t e2 = own->prof.get();
            fc.ready_s2.push_back(e2);
            PSFM_HIP(hipEventRecord(e2, side));
        }
    }
    own->prof.end(s);
    return PSFM_OK;
}

// ---- the table of sequences ----
psfm_status BatchRun::tables()
{
    psfm_status st;
    const size_t row_opt = psfm_batch_seq_opt_bytes();
    const size_t tab_bytes = sizeof(PsfmBatchSeq) * (size_t)B, tabo_bytes = optimize ? row_opt * (size_t)B : 0;
    pack_row = psfm_batch_pack_row_bytes(win_max);
    pack_bytes = pack_row * (size_t)B;
    if ((st = batch_host_staging(own, tab_bytes + tabo_bytes + pack_bytes)) != PSFM_OK) return st;
    if ((st = own->batch_tab.ensure(tab_bytes + tabo_bytes)) != PSFM_OK) return st;
    if ((st = own->batch_ws.ensure(pack_bytes)) != PSFM_OK) return st;
    PsfmBatchSeq* htab = (PsfmBatchSeq*)own->host_batch;
    char* htabo = (char*)own->host_batch + tab_bytes;
    hpack = htabo + tabo_bytes;
    dtab = own->batch_tab.as<PsfmBatchSeq>();
    dtabo = (char*)own->batch_tab.p + tab_bytes;
    for (int i = 0; i < B; ++i) {
        psfm_ctx* c = ctxs[i];
        // (a sequence that has left the batch keeps a row -- blockIdx.y indexes the table -- with no frames to run)
        // (option on: the chain step's mask bytes are the sequence's kill maps; the caller's / the solve's occlusion maps stay 0/1)
        const uint8_t* masks = mb ? c->kill.as<uint8_t>() : c->occ_own.as<uint8_t>();
        psfm_batch_fill_seq(c, D[i], flows_f[i], masks, fP(i), &htab[i]);
        if (S[i].dropped) htab[i].n_flows = 0;
        if (optimize) {
            const float* f2 = n_flows[i] > 1 ? flows_f2[i] : flows_f[i];      // (a one-pair sequence has no stride-2 stack: never read)
            if ((st = psfm_batch_fill_seq_opt(c, D[i], flows_f[i], masks, fP(i), f2, c->occ2_own.as<uint8_t>(),
                                              htabo + row_opt * (size_t)i, s)) != PSFM_OK) return st;
            // a run whose launches covered too few lanes has left the fused solve's tickets mid-count (blocks they were waiting
            // for never existed): the run that repeats it starts them from zero
            if (!trim && c->sol_fused.p) PSFM_HIP(hipMemsetAsync(c->sol_fused.p, 0, 4096 * sizeof(unsigned), s));
        }
    }
    PSFM_HIP(hipMemcpyAsync(dtab, htab, tab_bytes + tabo_bytes, hipMemcpyHostToDevice, s));
    // (dropped sequences: n_flows = 0 in the chain table keeps the init kernel's survivor loop short; their lane tables are
    // re-initialised by the psfm_connect that redoes them)
    return psfm_launch_track_init_batch(dtab, B, cap_max, s);
}

// ---- track.py:31-47: one launch per frame index for the whole batch ----
psfm_status BatchRun::track_loop()
{
    psfm_status st;
    for (int f = 0; f < n_max; ++f) {
        if ((st = fc.need(f, false, s)) != PSFM_OK) return st;
        if ((st = psfm_launch_chain_step_batch(own, dtab, B, ratio, grid_lanes, f, false, mb, s)) != PSFM_OK) return st;
    }
    return PSFM_OK;
}

// One sequence's part of a checkpoint: its packed row (counters, then the window's statistics from solve first_unchecked on) folded
// into its result and into the adaptation of mode / K (psfm_solve_policy.h), its stalled solve (if any) redone -- or the sequence
// sent out of the batch.  *progressed: the sequence completed a frame, or left.
psfm_status batch_checkpoint_seq(psfm_ctx* c, SeqState& S, const PsfmTrackDims& d, const char* row, const float* flows, const float* flows_f2,
                                 int i, int win_max, int64_t grid_lanes, bool* grid_too_small, bool* progressed, hipStream_t s)
{
    const PsfmCounters hc = *(const PsfmCounters*)row;
    const psfm_solve_stats* hw = (const psfm_solve_stats*)(row + sizeof(PsfmCounters));
    const int n_i = d.n_flows, lo = S.first_unchecked, kmax = psfm_solve_kmax();
    *progressed = false;
    if ((hc.overflow & 7) != 0 || hc.n_lanes > d.cap) {      // (as psfm_track_impl's checkpoint: a full table ends the run here)
        psfm_set_error("capacity exceeded (sequence %d of the batch): lanes used %d of %lld, overflow bits %d; raise psfm_ctx_set_capacity",
                       i, hc.n_lanes, (long long)d.cap, hc.overflow);
        return PSFM_ERR_CAPACITY;
    }
    if (hc.overflow & 16) {      // a launch covered fewer lanes than the sequence had in use: once more, with launches that cover the tables
        *grid_too_small = true;
        psfm_set_error("psfm_connect_batch: sequence %d uses more lanes (%d) than the trimmed launches cover (%lld)", i, hc.n_lanes, (long long)grid_lanes);
        return PSFM_ERR_CAPACITY;
    }
    for (int k = 0; k < win_max && lo + k <= n_i; ++k) S.hstats[(size_t)(lo + k)] = hw[k];
    const int stalled = hc.stall ? hc.stall - 1 : -1;
    int last_ok = (hc.pc_frame < n_i ? hc.pc_frame : n_i) - 1;     // frames below the device's program counter are complete
    if (psfm_batch_leaves_on_stall(c->solver_mode, stalled, S.first_unchecked)) {
        S.dropped = true; S.resync = true;
        c->solve_mode = 1;        // (what psfm_connect starts its first window with: the launch chain / the resident solve)
        *progressed = true;
        return PSFM_OK;
    }
    if (stalled >= 0) {
        // a solve that did not go as speculated (a rejected step, a dogleg interpolation, more iterations than the
        // continuation launches cover): redone by the launch chain from the values it started with, as in psfm_track
        const int fs = stalled;
        psfm_solve_stats ss;
        memset(&ss, 0, sizeof(ss));
        const PsfmSolveMaps m = psfm_solve_maps(flows, flows_f2, c->occ2_own.as<uint8_t>(), (int64_t)d.H * d.W, fs);
        psfm_status st2 = psfm_solve_frame_resume(c, d, m.flow01, m.flow12, m.flow02, m.occ02, fs, &ss, 0, false, s);
        if (st2 != PSFM_OK) return st2;
        S.hstats[(size_t)fs] = ss;
        last_ok = fs;
        S.resync = true;
    }
    PsfmWindowTally tally;
    for (int k = S.first_unchecked; k <= last_ok; ++k) {
        const psfm_solve_stats& q = S.hstats[(size_t)k];
        if (q.termination < 0) continue;      // -1: no track had a full buffer, nothing was solved
        tally.add(q, kmax);
        c->solve_stats.push_back(q);
        S.total_iters += q.iterations;
        if (k == stalled) ++c->n_fused_redone; else ++c->n_fused_ok;
    }
    if (tally.n_solved > 0) {
        c->solve_mode = tally.mode_next();
        c->solve_K = tally.k_device_paced(kmax);       // the most common need of the window (an iteration more costs one more launch)
    }
    if (last_ok + 1 > S.f) *progressed = true;
    S.first_unchecked = last_ok + 1;
    S.f = last_ok + 1;
    // a window of solves that reject steps: this sequence belongs to the launch chain / the resident solve -- it leaves the
    // batch and runs alone behind it (psfm_ctx_set_solver(ctx, 2, k) keeps it in)
    if (c->solve_mode == 1 && c->solver_mode != 2 && S.f < n_i) { S.dropped = true; S.resync = true; }
    return PSFM_OK;
}

// ---- track_optimize.py:31-50: frame 0 is a plain chain step; from frame 1 on device-paced launches ----
psfm_status BatchRun::optimize_loop()
{
    psfm_status st;
    if ((st = fc.need(0, false, s)) != PSFM_OK) return st;
    if ((st = psfm_launch_chain_step_batch(own, dtab, B, ratio, grid_lanes, 0, true, mb, s)) != PSFM_OK) return st;
    int launch_id = 0, idle_windows = 0;
    int v[PSFM_BATCH_MAX][4];
    for (int i = 0; i < B; ++i) {
        S[i].f = 1;
        S[i].resync = true;       // (track_init left pc = {frame 1, phase 0, launch 0, K 3}: set this context's K)
    }
    for (;;) {
        int left_max = 0, f_top = 0;
        bool any_set = false;
        for (int i = 0; i < B; ++i) {
            psfm_ctx* c = ctxs[i];
            v[i][0] = -1; v[i][1] = 0; v[i][2] = launch_id; v[i][3] = 0;
            const int n_i = S[i].dropped ? 0 : n_flows[i];
            const int k_now = psfm_k_now(c->solver_K, c->solve_K);
            if (S[i].f < n_i) {
                if (n_i - S[i].f > left_max) left_max = n_i - S[i].f;
                if (S[i].f > f_top) f_top = S[i].f;
                if (S[i].resync) { v[i][0] = S[i].f; v[i][3] = k_now; any_set = true; }
                else if (k_now != S[i].k_dev) { v[i][0] = -2; v[i][3] = k_now; any_set = true; }      // (K only: the device may be inside a solve)
                S[i].k_dev = k_now;
            } else if (S[i].resync) {   // finished or left the batch behind a redone solve: park its program counter at the end
                v[i][0] = n_flows[i]; v[i][3] = k_now; any_set = true;
            }
            S[i].resync = false;
        }
        if (left_max == 0) break;
        if (any_set && (st = psfm_launch_batch_set_pc(dtabo, v, B, s)) != PSFM_OK) return st;
        const int n_launch = psfm_window_launches(left_max, CHECK);
        const int f_hi = psfm_window_reach(f_top, n_launch, n_max - 1);      // the furthest frame a launch of this window can reach: the maps it reads
        if ((st = fc.need(f_hi, false, s)) != PSFM_OK) return st;
        if ((st = fc.need(f_hi - 1, true, s)) != PSFM_OK) return st;
        if ((st = psfm_launch_seq_batch(own, dtabo, B, ratio, grid_lanes, n_launch, launch_id, mb, s)) != PSFM_OK) return st;
        launch_id += n_launch;
        // ---- ONE checkpoint for all sequences ----
        int lo[PSFM_BATCH_MAX];
        for (int i = 0; i < B; ++i) lo[i] = S[i].first_unchecked;
        if ((st = psfm_launch_batch_pack(dtabo, lo, B, win_max, own->batch_ws.as<char>(), s)) != PSFM_OK) return st;
        PSFM_HIP(hipMemcpyAsync(hpack, own->batch_ws.p, pack_bytes, hipMemcpyDeviceToHost, s));
        PSFM_HIP(hipStreamSynchronize(s));
        bool progress = false;
        for (int i = 0; i < B; ++i) {
            if (S[i].dropped || S[i].f >= n_flows[i]) continue;
            bool progressed = false;
            if ((st = batch_checkpoint_seq(ctxs[i], S[i], D[i], hpack + pack_row * (size_t)i, flows_f[i], flows_f2[i], i, win_max, grid_lanes,
                                           grid_too_small, &progressed, s)) != PSFM_OK) return st;
            progress = progress || progressed;
        }
        // (no frame completed anywhere and nothing stalled: every sequence still running is inside one long solve -- all iterations
        // accepted, none terminating -- which the next window's launches continue; psfm_track_impl has the same case)
        idle_windows = progress ? 0 : idle_windows + 1;
        if (idle_windows > 8) { psfm_set_error("psfm_connect_batch: no sequence advanced in 8 windows of launches"); return PSFM_ERR_SOLVER; }
        if (trim) {
            // the next window's launches cover the lanes the sequences have in use NOW plus head-room for 18 frames of growth
            // (on a dense grid the high-water mark creeps up all through a long sequence: a death is a birth one frame later,
            // and not always on a lane of the same block)
            int64_t in_use = 0;
            for (int i = 0; i < B; ++i) {
                const PsfmCounters* hc = (const PsfmCounters*)(hpack + pack_row * (size_t)i);
                if (!S[i].dropped && hc->n_lanes > in_use) in_use = hc->n_lanes;
            }
            const int64_t want = in_use + in_use / 16 + 2048;
            if (want > grid_lanes) grid_lanes = want < cap_max ? want : cap_max;
        }
    }
    return psfm_launch_flush_batch(dtabo, B, cap_max, s);
}

// ---- ONE segmented finalize for the sequences that stayed; `redo`: the ones that left ----
psfm_status BatchRun::finalize(psfm_track_info* infos, std::vector<int>& redo)
{
    psfm_status st;
    // (every chunk of the side stream has been waited for by now unless all sequences left the batch early: the redo
    // writes the same maps)
    if ((st = fc.need(n_max - 1, false, s)) != PSFM_OK) return st;
    if (optimize && n_max >= 2 && (st = fc.need(n_max - 2, true, s)) != PSFM_OK) return st;
    std::vector<psfm_ctx*> kc;
    std::vector<PsfmTrackDims> kd;
    std::vector<int> ki;
    for (int i = 0; i < B; ++i) {
        if (S[i].dropped) redo.push_back(i);
        else { kc.push_back(ctxs[i]); kd.push_back(D[i]); ki.push_back(i); }
    }
    if (!kc.empty()) {
        own->prof.begin(PSFM_PROF_FINALIZE, s);
        st = psfm_finalize_batch(own, kc.data(), kd.data(), (int)kc.size(), s);
        own->prof.end(s);
        if (st == PSFM_ERR_CAPACITY)
            for (psfm_ctx* c : kc) if (((PsfmCounters*)c->host_pinned)->overflow & 16) *grid_too_small = true;
        if (st != PSFM_OK) return st;
    }
    PSFM_HIP(hipStreamSynchronize(s));
    own->prof.collect();
    if (infos)
        for (int i : ki) psfm_fill_track_info(&infos[i], ctxs[i], D[i].cap, S[i].total_iters, 3);
    return PSFM_OK;
}

// ---- sequences that left the batch (their solves reject steps): through psfm_connect, with everything it has for them -- the
// resident solve above all.  One sequence: the call as it is (it may take the device to itself).  Several: a few of them at a
// time on host threads of this call, every one with an equal share of the device's co-resident block slots for its resident
// solves (psfm_ctx_set_resident_budget: 1.6-1.8x one after the other on Sintel / DAVIS-sized realistic flows,
// profiles/r05/r05_f_resident_budget.txt); as many at a time as have room on chip for their tracks.  (The gate is released.) ----
psfm_status BatchRun::redo_alone(const std::vector<int>& redo, psfm_track_info* infos, void* stream)
{
    psfm_status st;
    if (redo.empty()) return PSFM_OK;
    int n_thr = 1;
    // what the redo threads may share: the CALLER's budget when it set one (psfm.h: the budgets of all contexts in flight on the device
    // add up to at most the capacity -- connect_sequences gives every worker capacity / n_threads, and two workers' batches may redo at
    // the same time), else the device's co-resident block slots
    const int room = own->resident_budget > 0 ? std::min(own->resident_budget, psfm_resident_blocks(own)) : psfm_resident_blocks(own);
    if (redo.size() >= 2 && optimize) {
        const int capacity = room;
        int64_t G = 0;                                            // (the largest grid among them)
        for (int i : redo) G = std::max(G, D[i].G);
        const int64_t need = (G * 6 / 10 + 767) / 768;            // blocks that hold ~60 % of the grid's tracks at three per thread
        int fit = need > 0 ? (int)(capacity / need) : 4;
        if (const char* e = getenv("PSFM_BATCH_REDO_THREADS")) fit = atoi(e);
        n_thr = fit < 1 ? 1 : (fit > 4 ? 4 : fit);
        if (n_thr > (int)redo.size()) n_thr = (int)redo.size();
        if (capacity <= 0) n_thr = 1;
    }
    if (n_thr == 1) {
        for (int i : redo) {
            st = psfm_connect(ctxs[i], flows_f[i], flows_b[i], optimize ? flows_f2[i] : nullptr, optimize ? flows_b2[i] : nullptr, n_flows[i], fh(i), fw(i), thres,
                              ratio, nullptr, nullptr, infos ? &infos[i] : nullptr, stream);
            if (st != PSFM_OK) return st;
        }
        return PSFM_OK;
    }
    const int share = std::max(room / n_thr, 1);
    std::vector<psfm_status> rc((size_t)n_thr, PSFM_OK);
    std::vector<std::string> msg((size_t)n_thr);
    std::vector<std::thread> workers;
    auto body = [&](int t) {
            for (size_t q = (size_t)t; q < redo.size(); q += (size_t)n_thr) {
                const int i = redo[q];
                psfm_ctx* c = ctxs[i];
                if (hipSetDevice(c->device) != hipSuccess) { rc[(size_t)t] = PSFM_ERR_HIP; msg[(size_t)t] = "hipSetDevice failed"; return; }
                if (!c->redo_stream && hipStreamCreateWithFlags(&c->redo_stream, hipStreamNonBlocking) != hipSuccess) {
                    rc[(size_t)t] = PSFM_ERR_HIP; msg[(size_t)t] = "hipStreamCreateWithFlags failed"; return;
                }
                const int budget0 = c->resident_budget;
                c->resident_budget = share;
                const psfm_status r = psfm_connect(c, flows_f[i], flows_b[i], flows_f2[i], flows_b2[i], n_flows[i], fh(i), fw(i), thres, ratio, nullptr, nullptr,
                                                   infos ? &infos[i] : nullptr, (void*)c->redo_stream);
                c->resident_budget = budget0;
                if (r != PSFM_OK) { rc[(size_t)t] = r; msg[(size_t)t] = psfm_last_error(); return; }      // (the error text is thread local)
            }
        };
    std::vector<int> inline_shares;      // shares whose thread could not be created (std::system_error): run here, behind the others
    for (int t = 0; t < n_thr; ++t) {
        try { workers.emplace_back(body, t); } catch (const std::exception&) { inline_shares.push_back(t); }
    }
    for (int t : inline_shares) body(t);
    for (auto& th : workers) th.join();
    for (int t = 0; t < n_thr; ++t)
        if (rc[(size_t)t] != PSFM_OK) { psfm_set_error("psfm_connect_batch: a sequence that left the batch failed: %s", msg[(size_t)t].c_str()); return rc[(size_t)t]; }
    return PSFM_OK;
}

// ---- sequences that left the batch, TOGETHER (psfm_ctx_set_batch_redo(own, 1)): from frame 0 again, as redo_alone does, but through
// one set of launches -- the batched chain step of every frame, and behind it the frame's solves of ALL these sequences as the
// frame-mode multi-problem launch chain (psfm_solver_multi.hip: one init launch, iteration launches paced by ONE poll and ONE
// synchronisation for the whole table, one write-back launch), then one segmented finalize.  Every sequence's launches are block
// for block those psfm_connect makes for it alone on a context pinned to the launch chain: the same bytes.  The sequences' maps
// (occlusion, stride-2 occlusion, kill maps) are the ones this run's flow_check made; launches only, the gate stays shared. ----
psfm_status BatchRun::redo_together(const std::vector<int>& redo, psfm_track_info* infos)
{
    psfm_status st;
    const int n = (int)redo.size();
    if (n == 0) return PSFM_OK;
    PsfmGate gate(own->device, 0);
    const size_t row_opt = psfm_batch_seq_opt_bytes(), row_fr = psfm_frame_row_bytes();
    const size_t tab_bytes = sizeof(PsfmBatchSeq) * (size_t)n, fr_bytes = row_fr * (size_t)n, opt_bytes = row_opt * (size_t)n;
    const size_t poll_bytes = psfm_frame_poll_bytes() * (size_t)n;
    // (nothing of the fused run is in flight: finalize synchronised the stream -- its tables and staging are free to be replaced)
    if ((st = batch_host_staging(own, tab_bytes + fr_bytes + opt_bytes + poll_bytes)) != PSFM_OK) return st;
    if ((st = own->batch_tab.ensure(tab_bytes + fr_bytes)) != PSFM_OK) return st;
    PsfmBatchSeq* htab = (PsfmBatchSeq*)own->host_batch;
    char* hfr = (char*)own->host_batch + tab_bytes;
    char* hopt = hfr + fr_bytes;                 // (the track_optimize rows the frame rows are cut from: never uploaded)
    char* hpoll = hopt + opt_bytes;
    const PsfmBatchSeq* dt = own->batch_tab.as<PsfmBatchSeq>();
    const char* dfr = (const char*)own->batch_tab.p + tab_bytes;
    int nb[PSFM_BATCH_MAX], n_top = 0;
    int64_t cap_top = 0;
    for (int q = 0; q < n; ++q) {
        const int i = redo[q];
        psfm_ctx* c = ctxs[i];
        psfm_call_begin(c, n_flows[i], false);       // (a sequence that left at a checkpoint has solves on file: from the top)
        S[i].total_iters = 0;
        const uint8_t* masks = mb ? c->kill.as<uint8_t>() : c->occ_own.as<uint8_t>();
        psfm_batch_fill_seq(c, D[i], flows_f[i], masks, fP(i), &htab[q]);      // (owner_clear: the stamp-wrap clear of the blocked map, on the device)
        const float* f2 = n_flows[i] > 1 ? flows_f2[i] : flows_f[i];
        if ((st = psfm_batch_fill_seq_opt(c, D[i], flows_f[i], masks, fP(i), f2, c->occ2_own.as<uint8_t>(), hopt + row_opt * (size_t)q, s)) != PSFM_OK) return st;
        if ((st = psfm_frame_row_fill(c, D[i], hopt + row_opt * (size_t)q, hfr + row_fr * (size_t)q, &nb[q])) != PSFM_OK) return st;
        if (n_flows[i] > n_top) n_top = n_flows[i];
        if (D[i].cap > cap_top) cap_top = D[i].cap;
    }
    const int grid_x = pc_frame_grid_x(nb, n), kmax = psfm_solve_kmax();
    std::vector<PsfmWindowTally> tally((size_t)n);
    PSFM_HIP(hipMemcpyAsync(own->batch_tab.p, htab, tab_bytes + fr_bytes, hipMemcpyHostToDevice, s));
    if ((st = psfm_launch_track_init_batch(dt, n, cap_top, s)) != PSFM_OK) return st;
    own->bt_fixed += 2;
    for (int f = 0; f < n_top; ++f) {
        if ((st = psfm_launch_chain_step_batch(own, dt, n, ratio, cap_top, f, true, mb, s)) != PSFM_OK) return st;
        own->bt_fixed += 1;
        if (f < 1) continue;
        if ((st = psfm_frame_solve_batch(dfr, grid_x, n, f, hpoll, &own->bt_fixed, &own->bt_iter, &own->bt_syncs, s)) != PSFM_OK) return st;
        for (int q = 0; q < n; ++q) {
            const int i = redo[q];
            psfm_ctx* c = ctxs[i];
            int active = 0, lanes = 0, overflow = 0, stall = 0;
            psfm_solve_stats ss;
            psfm_frame_poll_read(hpoll, q, &active, &ss, &lanes, &overflow, &stall);
            if ((overflow & 7) != 0 || lanes > D[i].cap) {      // (as the checkpoint of the fused batch: a full table ends the run here)
                psfm_set_error("capacity exceeded (sequence %d of the batch): lanes used %d of %lld, overflow bits %d; raise psfm_ctx_set_capacity",
                               i, lanes, (long long)D[i].cap, overflow);
                return PSFM_ERR_CAPACITY;
            }
            // (nothing on this path raises the stall flag -- track_init clears it, only fused and enqueued resident solves set it; a
            // raised flag means the frame's launches skipped the sequence and the polled control block is an earlier frame's)
            if (stall) { psfm_set_error("psfm_connect_batch: sequence %d has its stall flag raised (frame %d) inside the joint redo", i, stall - 1); return PSFM_ERR_SOLVER; }
            if (!active || ss.termination < 0) continue;      // -1: no track had a full buffer, nothing was solved
            c->solve_stats.push_back(ss);
            S[i].total_iters += ss.iterations;
            ++c->n_chain;
            tally[(size_t)q].add(ss, kmax);
        }
    }
    // what the context's adaptive policy takes into its next call (psfm_solve_policy.h), as the checkpoints of psfm_connect leave it:
    // a sequence that left because of a stale K, not because its solves reject steps, starts the next batch with the K it needs
    for (int q = 0; q < n; ++q) {
        if (tally[(size_t)q].n_solved == 0) continue;
        ctxs[redo[q]]->solve_mode = tally[(size_t)q].mode_next();
        ctxs[redo[q]]->solve_K = tally[(size_t)q].k_device_paced(kmax);
    }
    std::vector<psfm_ctx*> kc;
    std::vector<PsfmTrackDims> kd;
    for (int i : redo) { kc.push_back(ctxs[i]); kd.push_back(D[i]); }
    own->prof.begin(PSFM_PROF_FINALIZE, s);
    st = psfm_finalize_batch(own, kc.data(), kd.data(), n, s);
    own->prof.end(s);
    if (st != PSFM_OK) return st;
    PSFM_HIP(hipStreamSynchronize(s));
    own->bt_syncs += 1;
    own->prof.collect();
    own->bt_together = n;
    if (infos)
        for (int i : redo) psfm_fill_track_info(&infos[i], ctxs[i], D[i].cap, S[i].total_iters, 8);
    return PSFM_OK;
}
}  // namespace

static psfm_status batch_run(psfm_ctx* const* ctxs, int n_seq, const float* const* flows_f, const float* const* flows_b,
                             const float* const* flows_f2, const float* const* flows_b2, const int* n_flows, int h, int w,
                             const int* hs, const int* ws, float thres, int ratio, psfm_track_info* infos, void* stream, bool trim,
                             bool* grid_too_small)
{
    *grid_too_small = false;
    // (the flow_check pipeline's events go back into the owner's pool when the call ends, however it ends)
    BatchRun R{ctxs, n_seq, flows_f, flows_b, flows_f2, flows_b2, n_flows, h, w, hs, ws, thres, ratio, (hipStream_t)stream, trim, grid_too_small,
               ctxs[0], flows_f2 != nullptr, ctxs[0]->mb_enable, PsfmOccPipeline(ctxs[0])};
    PSFM_HIP(hipSetDevice(R.own->device));
    // how the sequences that leave the fused batch are redone: the owner's psfm_ctx_set_batch_redo; PSFM_BATCH_REDO=together|alone
    // overrides it (measurements; read per call)
    R.together = R.own->batch_redo == 1;
    if (const char* e = getenv("PSFM_BATCH_REDO")) {
        if (!strcmp(e, "together")) R.together = true;
        else if (!strcmp(e, "alone")) R.together = false;
    }
    R.together = R.together && R.optimize;
    R.own->bt_left = R.own->bt_together = R.own->bt_fixed = R.own->bt_iter = R.own->bt_syncs = 0;
    std::vector<int> redo;
    psfm_status st;
    {
        PsfmGate gate(R.own->device, 0);        // launches only: nothing here needs the device to itself
        if ((st = R.prepare()) != PSFM_OK) return st;
        if ((st = R.flow_check()) != PSFM_OK) return st;
        if ((st = R.tables()) != PSFM_OK) return st;
        if ((st = R.optimize ? R.optimize_loop() : R.track_loop()) != PSFM_OK) return st;
        if ((st = R.finalize(infos, redo)) != PSFM_OK) return st;
    }
    R.own->bt_left = (int32_t)redo.size();
    if (R.together) return R.redo_together(redo, infos);
    return R.redo_alone(redo, infos, stream);
}

extern "C" psfm_status psfm_connect_batch_census(psfm_ctx* ctx0, int32_t* n_left, int32_t* n_together, int32_t* launches_fixed,
                                                 int32_t* launches_iter, int32_t* host_syncs)
{
    if (!ctx0) { psfm_set_error("ctx is NULL"); return PSFM_ERR_ARG; }
    if (n_left) *n_left = ctx0->bt_left;
    if (n_together) *n_together = ctx0->bt_together;
    if (launches_fixed) *launches_fixed = ctx0->bt_fixed;
    if (launches_iter) *launches_iter = ctx0->bt_iter;
    if (host_syncs) *host_syncs = ctx0->bt_syncs;
    return PSFM_OK;
}

