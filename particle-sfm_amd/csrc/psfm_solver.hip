// psfm_solver.hip -- K5/K6: the path-consistency solve (trajectory.py:161-194 +
// optimize/src/trajectory_optimize.cpp:30-96) as a device-resident Ceres-compatible trust-region loop.
//
// Objective per track (path_consistency_cost.h:42-59), x = (x1,y1,x2,y2):
//     r = [ p1 - ref1 ; s (p2 - ref2) ; (p2 - p1) - F12(p1) ],   cost = 1/2 sum r^2
// F12 is the f64 clamp-to-edge bilinear interpolator of linear_interpolation.h:97-123 (NOT the fp32
// zero-padded sampler).  The Hessian is block diagonal (one 4x4 block per track), but Ceres' trust-region
// loop is global: ONE cost, ONE radius, ONE accept/reject and ONE termination test over all tracks
// (SURVEY.md Appendix B).  To land on the same iterate the whole control flow of Ceres 2.0.0
// (TrustRegionMinimizer + DoglegStrategy/TRADITIONAL_DOGLEG + Jacobi scaling + SPARSE_NORMAL_CHOLESKY,
// max 200 iterations) is reproduced with its scalars reduced over all tracks:
//
//   fused     (track_optimize's default) ONE launch per solve -- per FRAME together with the chain step (psfm_frame_kernel):
//             thread = track runs K trust-region iterations in registers, speculating what Ceres does on every solve that
//             converges without a rejection (Gauss-Newton step inside the trust region, mu = min_mu, step accepted); the K
//             x 13 sums are reduced wave -> block -> group -> grid and the last block REPLAYS the control flow below over
//             them.  The first decision that is not "Gauss-Newton step accepted" ends the belief: termination = done, anything
//             else = the solve is redone by the launch chain from the values it started with.
//   pc_init   (launch chain) per track: refs/scale (fp32 sampler, trajectory.py:173-183), Jacobi scaling, cost and the
//             Gauss-Newton system at the start values; its control step runs Ceres' iteration 0 and fixes the first step
//   pc_iter   ONE launch per trust-region iteration, one pass per track: the candidate x + a u + b d of the dogleg step the
//             control step chose, its cost, and -- evaluated AHEAD, as if the step were accepted -- the Gauss-Newton system
//             and its sums at the candidate.  The sums at an iterate (|ghat|^2, |gn|^2, ghat.gn, |J u|^2, (J u).(J d),
//             |J d|^2) price EVERY dogleg step of that iterate -- norm and model decrease -- in the control step, so a
//             rejection (radius halves, same system, new coefficients) and an acceptance (the system at the new iterate is
//             already reduced) both go on with the next launch: launches = iterations, no re-issued launches.  (Round 2
//             speculated the Gauss-Newton step per launch and re-issued the launch whenever the reduced norms prescribed
//             another dogleg case: iterations + non-Gauss-Newton steps launches.)  An invalid step (model decrease <= 0)
//             raises mu, which changes the system at the same x: one "refresh" launch.  x ping-pongs between iterate
//             buffers 1 and 2; buffer 0 (the caller's values / the log slabs) is only written by the write-back.
//   control   pc_chain_control (launch chain) / pc_control_step (replay of a fused launch): Ceres' scalar logic for one
//             iteration from the global sums -- accept / reject / radius / mu / the three tolerances.  Consecutive rejections
//             whose shrunken radius still contains the Gauss-Newton step reproduce the same candidate, so they are replayed
//             without relaunching (bit-identical to Ceres, which recomputes the same step each time).  Run by the last block
//             of each launch (ticket after write-through partials), or -- track-sharded runs -- by psfm_pc_control_kernel on
//             the totals over all ranks.  Nothing returns to the host inside the loop.
//
// All arithmetic f64 (psfm_pc_core.h: explicit fma); reductions have a fixed order (bitwise reproducible for a given
// lane assignment).
//
// This unit: the launch chain's kernels, the resident solve (the chain's loop as ONE launch, PcPeers: it stays beside the chain's
// kernels -- profiles/EXPERIMENTS.md 19), the control kernel of track-sharded runs and the host driver of a solve.  The fused / frame /
// device-paced kernels are psfm_solver_fused.hip, their batched forms psfm_solver_batch.hip; the device code the units share is in
// psfm_pc_params.h, psfm_pc_tracks.h and psfm_pc_fused.h.
#include <string.h>
#include <stdlib.h>
#include <stdio.h>

#include "psfm_pc_tracks.h"
#include "psfm_pc_fused.h"        // (pc_fused_replay: psfm_pc_control_kernel)
#include "psfm_solver_internal.h"

__global__ __launch_bounds__(PC_BLOCK) void psfm_pc_init_kernel(PcParams P)
{
    if (*P.stall) return;
    double acc[PC_NSUM];
    pc_init_tracks(P, acc);
    pc_block_reduce(acc, P.partials);
    if (pc_is_last_block(P.ticket)) pc_reduce_and_control(P.ctrl, P.partials, (int)gridDim.x, 1, P.export_sums);
}

// ------------------------------------------------------------------------------------------------
// pc_iter: one trust-region iteration at the current iterate.
// ------------------------------------------------------------------------------------------------
#ifdef PSFM_TIMELINE
// debug builds only: phase timestamps of the pc_iter launches (first 64 real launches), per block
__device__ unsigned long long g_pc_tl[64 * 1024 * 4];
__device__ int g_pc_tl_n = 0;
extern "C" int psfm_debug_solver_timeline(unsigned long long* out_host, int* n_host)
{
    if (hipMemcpyFromSymbol(n_host, HIP_SYMBOL(g_pc_tl_n), sizeof(int)) != hipSuccess) return 1;
    return hipMemcpyFromSymbol(out_host, HIP_SYMBOL(g_pc_tl), sizeof(unsigned long long) * 64 * 1024 * 4) != hipSuccess;
}
#define PC_TL(k) do { if (tl_slot >= 0 && threadIdx.x == 0) g_pc_tl[((size_t)tl_slot * 1024 + blockIdx.x) * 4 + (k)] = __builtin_amdgcn_s_memrealtime(); } while (0)
// resident solve: rounds PC_RTL_R0 .. + 7 of the launch with epoch PC_RTL_EPOCH, 16 stamps per block and round: [8][512][16]
#define PC_RTL_EPOCH 12u
#define PC_RTL_R0 8u
#define PC_RTL(k) do { if (rtl >= 0 && threadIdx.x == 0) g_pc_tl[((size_t)rtl * 512 + blockIdx.x) * 16 + (k)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define PC_TL(k) do {} while (0)
#define PC_RTL(k) do {} while (0)
#endif

__global__ __launch_bounds__(PC_BLOCK) void psfm_pc_iter_kernel(PcParams P)
{
    if (*P.stall) return;
    const PsfmSolveCtrl C = *P.ctrl;
    if (C.done) return;
#ifdef PSFM_TIMELINE
    const int tl_slot = C.iteration == 1 && g_pc_tl_n < 64 ? g_pc_tl_n : -1;   // the first pc_iter launch of a solve
    PC_TL(0);
#endif
    double acc[PC_NSUM];
#pragma unroll
    for (int k = 0; k < PC_NSUM; ++k) acc[k] = 0.0;
    pc_iter_tracks(P, (int)threadIdx.x, C.cur, C.mu, C.dl_a, C.dl_b, C.kind_next != 0, acc);
    PC_TL(1);
    pc_block_reduce(acc, P.partials);
    const bool last_block = pc_is_last_block(P.ticket);
    PC_TL(2);
    if (last_block) {
        pc_reduce_and_control(P.ctrl, P.partials, (int)gridDim.x, 0, P.export_sums);
        PC_TL(3);
#ifdef PSFM_TIMELINE
        if (threadIdx.x == 0 && tl_slot >= 0) { g_pc_tl[((size_t)tl_slot * 1024 + 1023) * 4 + 0] = blockIdx.x; g_pc_tl_n = tl_slot + 1; }
#endif
    }
}

// ------------------------------------------------------------------------------------------------
// pc_resident: the launch chain's loop inside ONE launch, with the tracks' solver state ON CHIP.  Solves that reject steps take
// 20-40 trust-region iterations.  As launches each of them is a launch gap, a tail behind the last block and a control block
// round trip; round 3's persistent form removed those but still STREAMED the tracks through every round (88 B of state in,
// 32 B of candidate out, per track and round: 46 MB at 1080p), walked a thread's 3-4 tracks one behind the other -- four
// dependent round trips each -- and re-derived the system at x that the round before had already solved (16.5 us per round, the
// SIMDs issuing VALU a quarter of the time).  Here:
//   * a thread HOLDS its tracks: slot k of thread t is entry k * PC_BLOCK + t of the block's list (pc_build_list).  Per slot in
//     registers: refs, weight, Jacobi scaling, the iterate x and its steepest-descent / Gauss-Newton directions (u, d); in LDS:
//     (u', d') at the candidate.  A round is  x' = x + a u + b d  ->  ONE gather (the taps at x', every slot's in flight
//     together)  ->  residuals, cost, the system at x' (evaluate-ahead: its sums and (u', d'))  ->  the sums.  Accepted: x <- x'
//     (recomputed, same bits), (u, d) <- (u', d'); rejected: same x, same (u, d), new (a, b).  Nothing is loaded but taps,
//     nothing stored.  Entries beyond NS slots per thread (grids larger than the register files) are streamed as the launch
//     chain does it (pc_iter_tracks), behind the slots in the same order of summation.
//   * the hand-off is an ALL-REDUCE of tagged granules, two hops: every block publishes its PC_RES_SUMS sums as 8-byte granules
//     {tag : 32 | half of a double : 32} (valid by themselves: nothing orders the stores, the poll IS the read -- form R2 of
//     MI355X_MICROARCH.md); the PC_LEADERS leaders add up their members' (pc_reduce_totals' first level) and publish theirs;
//     EVERY block adds up the leaders' (the upper levels) and runs the control step itself on its own copy of the control block --
//     same numbers, same function, same decisions everywhere; no reducer, no packet, no counter, no store acknowledgement.
//     tag = {launch epoch : 20 | round : 12}: a granule left by an earlier launch never matches.
// Same per-track functions, same order of summation, same control step as the launches: bit-identical iterates
// (tests/test_gpu_solver.py::test_launch_chain_as_one_persistent_launch_is_the_same_solve).  A block whose poll exceeds the spin
// limit (the grid was not co-resident after all) poisons its granules -- leaders pass the poison on -- and every block leaves
// without having written anything: the control block still says "not done", the write-back kernel behind raises the stall
// flag and the host redoes the solve with launches.
// ------------------------------------------------------------------------------------------------
#define PC_RES_SUMS 11          // SUM_MCC .. SUM_FAIL: what a round reduces (SUM_CNT / SUM_COST0 belong to pc_init)
#define PC_RES_ROW 32           // granules per row (256 B): 2 per sum
#define PC_RES_NS_MAX 3         // slots per thread: 3 x 27 doubles of state + the arithmetic's working set is what 256 registers
                                // and half a CU's LDS hold
#define PC_RES_BLOCKS 512       // two blocks per CU
static_assert(PC_RES_BLOCKS / PC_LEADERS / 4 <= 4, "a leader lane keeps its 4 members' granules in flight");
static_assert(sizeof(PsfmSolveCtrl) % 8 == 0, "the control block is copied as 8-byte words");
#define PC_CTRL_WORDS ((int)(sizeof(PsfmSolveCtrl) / 8))

struct PcRound { int done, cur, kind, accepted, giveup; double mu, a, b; };   // what a round of the loop needs from the control block

// ONE solve over several GPUs / processes (track-sharded runs, psfm_shard.hip): every rank runs this launch on ITS tracks and the
// second hop of the all-reduce crosses the ranks -- a leader publishes its sums into EVERY rank's leader area (its own included)
// through peer-mapped pointers (hipIpcOpenMemHandle / P2P over xGMI; plain pointers between host threads of one process), and
// every block adds up the leader rows of all ranks from its OWN rank's area, rank by rank in rank order:
//     total = (...((T_0 + T_1) + T_2) ...) + T_{world-1},   T_r = rank r's total as pc_tree_totals forms it
// -- the same numbers in the same order on every rank, hence the same control decisions everywhere, with no host and no collective
// library in the loop.  Leader area of a rank: [set 0, 1][source rank][PC_LEADERS][PC_RES_ROW] granules.  world == 1 is the
// one-GPU launch bit for bit (the template parameter only removes the loop).
struct PcPeers {
    int world, rank;
    int L[PSFM_MAX_PEERS];                       // leaders of every rank's launch: min(PC_LEADERS, its blocks)
    unsigned long long* lead[PSFM_MAX_PEERS];    // rank r's leader area as THIS process addresses it
};
__device__ __forceinline__ unsigned long long* pc_peer_rows(unsigned long long* area, int world, unsigned set, int src_rank)
{
    return area + ((size_t)(set * (unsigned)world + (unsigned)src_rank) * PC_LEADERS) * PC_RES_ROW;
}

__device__ __forceinline__ unsigned long long pc_gran_load(const unsigned long long* p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ void pc_gran_store(unsigned long long* p, unsigned tag, unsigned half)
{
    __hip_atomic_store(p, ((unsigned long long)tag << 32) | (unsigned long long)half, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ unsigned pc_half(double v, int lo)
{
    const unsigned long long bits = (unsigned long long)__double_as_longlong(v);
    return lo ? (unsigned)bits : (unsigned)(bits >> 32);
}
__device__ __forceinline__ double pc_unhalf(unsigned long long hi, unsigned long long lo)
{
    return __longlong_as_double((long long)((hi << 32) | (lo & 0xffffffffull)));
}

// The all-reduce of one round, run by WAVE 0 of every block (the other waves wait at the caller's barrier): blk[] = this
// block's sums (LDS), gran = [n_blocks rows of members][PC_LEADERS rows of leaders].  Returns 0 with the totals in tot[], 1
// when the round is given up (this block timed out, or saw the poison of one that did).  Lane (k, j) = 4 k + j works on sum k.
// ACROSS solves the two sets are safe only under a condition the CALLER keeps (PEERS): iteration 0 of the next solve is tagged into set
// 0, so a rank that ran ahead into it could overwrite, in another rank's area, leader rows whose slow blocks still poll an even last
// round of the solve before.  Every rank therefore needs a cross-rank collective (or another point all ranks reach only behind their
// launch of the solve before) between two psfm_shard_solve_peer calls -- psfm_dist.py has the all-reduce of the step marks there;
// see include/psfm.h.  (One rank: the launches of a stream follow each other.)
template <int NSUMS, bool PEERS = false>
__device__ __forceinline__ int pc_res_allreduce(const double* blk, unsigned long long* gran, int n_blocks, unsigned tag, unsigned poison,
                                                int spin_limit, bool quit, double tot[PC_NSUM], int rtl, const PcPeers* peers = nullptr)
{
    static_assert(4 * NSUMS <= PSFM_WAVE && 2 * NSUMS <= PC_RES_ROW, "one lane per (sum, quarter), two granules per sum");
    const int lane = threadIdx.x;            // (wave 0: lane == thread)
    const int b = (int)blockIdx.x;
    const int L = n_blocks < PC_LEADERS ? n_blocks : PC_LEADERS;
    unsigned long long* mine = gran + (size_t)b * PC_RES_ROW;
    // leader rows: TWO sets, used by alternate rounds (consecutive tags differ in bit 0).  A leader may publish its round r + 1 sums as
    // soon as its own members are through round r -- with one set, a block under another leader that has not yet seen every leader's
    // round-r granules would find tag r + 1 there, never match, and poison the solve at its spin limit (a spurious give-up under
    // preemption).  Round r + 2 cannot be published before every block has read round r: it needs every leader's r + 1 row, which
    // needs every member's r + 1 granule, which a member only writes behind its round-r totals.
    unsigned long long* lead = PEERS ? pc_peer_rows(peers->lead[peers->rank], peers->world, tag & 1u, peers->rank)
                                     : gran + ((size_t)n_blocks + (size_t)(tag & 1u) * PC_LEADERS) * PC_RES_ROW;
    const int k = lane >> 2, j = lane & 3;
    const bool work = lane < 4 * NSUMS;
    int bad = quit ? 1 : 0;
    if (!bad && lane < 2 * NSUMS) pc_gran_store(mine + lane, tag, pc_half(blk[lane >> 1], lane & 1));
    PC_RTL(4);
    if (!bad && b < L) {
        // ---- leader: lane (k, j) adds the sums of its Q members in member order, then the four j's in order ----
        const int Q = pc_tree_q(n_blocks);      // (<= 4: PC_RES_BLOCKS / PC_LEADERS / 4)
        const int cnt = (n_blocks - b + PC_LEADERS - 1) / PC_LEADERS;
        double v = 0.0;
        for (int spins = 0;; ++spins) {
            unsigned long long wh[4], wl[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int m = j * Q + u;
                const bool use = work && u < Q && m < cnt;
                const unsigned long long* src = gran + (size_t)(b + PC_LEADERS * (use ? m : 0)) * PC_RES_ROW + 2 * (work ? k : 0);
                wh[u] = pc_gran_load(src); wl[u] = pc_gran_load(src + 1);
            }
            bool ok = true, psn = false;
            v = 0.0;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int m = j * Q + u;
                const bool use = work && u < Q && m < cnt;
                if (!use) continue;
                const unsigned th = (unsigned)(wh[u] >> 32), tl = (unsigned)(wl[u] >> 32);
                if (th != tag || tl != tag) { ok = false; psn = psn || th == poison || tl == poison; }
                const double val = pc_unhalf(wh[u], wl[u]);
                v = (k == SUM_GMAX) ? fmax(v, val) : v + val;
            }
            if (__ballot(psn) != 0ull) { bad = 1; break; }
            if (__ballot(!ok) == 0ull) break;
            if (spins >= spin_limit) { bad = 1; break; }
            __builtin_amdgcn_s_sleep(1);
        }
        if (!bad) {
            const double s1 = __shfl(v, (lane & ~3) + 1), s2 = __shfl(v, (lane & ~3) + 2), s3 = __shfl(v, (lane & ~3) + 3);
            const double S = (k == SUM_GMAX) ? fmax(fmax(fmax(v, s1), s2), s3) : ((v + s1) + s2) + s3;   // (valid in lanes 4k)
            const double Sg = __shfl(S, 4 * (lane >> 1));        // granule lane g publishes sum g >> 1
            if (lane < 2 * NSUMS) {
                if (PEERS) {
                    for (int r = 0; r < peers->world; ++r)     // into every rank's area (this rank's slot there)
                        pc_gran_store(pc_peer_rows(peers->lead[r], peers->world, tag & 1u, peers->rank) + (size_t)b * PC_RES_ROW + lane, tag,
                                      pc_half(Sg, lane & 1));
                } else {
                    pc_gran_store(lead + (size_t)b * PC_RES_ROW + lane, tag, pc_half(Sg, lane & 1));
                }
            }
        }
        PC_RTL(5);
    }
    double total = 0.0;
    // ---- every block: lane (k, j) adds the leaders 8 j .. 8 j + 7 in order, then the four j's in order (PEERS: of every rank, rank
    //      by rank, from this rank's own area -- a rank that is late keeps everybody in its poll, bounded by the spin limit) ----
    const int n_src = PEERS ? peers->world : 1;
    for (int r = 0; r < n_src && !bad; ++r) {
        const unsigned long long* rows = PEERS ? pc_peer_rows(peers->lead[peers->rank], peers->world, tag & 1u, r) : lead;
        const int Lr = PEERS ? peers->L[r] : L;
        double t = 0.0;
        for (int spins = 0;; ++spins) {
            unsigned long long wh[8], wl[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int x = 8 * j + u;
                const unsigned long long* src = rows + (size_t)(work && x < Lr ? x : 0) * PC_RES_ROW + 2 * (work ? k : 0);
                wh[u] = pc_gran_load(src); wl[u] = pc_gran_load(src + 1);
            }
            bool ok = true, psn = false;
            t = 0.0;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int x = 8 * j + u;
                if (!work || x >= Lr) continue;
                const unsigned th = (unsigned)(wh[u] >> 32), tl = (unsigned)(wl[u] >> 32);
                if (th != tag || tl != tag) { ok = false; psn = psn || th == poison || tl == poison; }
                const double S = pc_unhalf(wh[u], wl[u]);
                t = (k == SUM_GMAX) ? fmax(t, S) : t + S;
            }
            if (__ballot(psn) != 0ull) { bad = 1; break; }
            if (__ballot(!ok) == 0ull) break;
            if (spins >= spin_limit) { bad = 1; break; }
            __builtin_amdgcn_s_sleep(1);
        }
        if (bad) break;
        const double t1 = __shfl(t, (lane & ~3) + 1), t2 = __shfl(t, (lane & ~3) + 2), t3 = __shfl(t, (lane & ~3) + 3);
        const double Tr = (k == SUM_GMAX) ? fmax(fmax(fmax(t, t1), t2), t3) : ((t + t1) + t2) + t3;       // (valid in lanes 4k)
        total = r == 0 ? Tr : ((k == SUM_GMAX) ? fmax(total, Tr) : total + Tr);
    }
    if (bad) {
        // poison: whoever waits for this block (its leader; everybody -- on every rank -- if it is a leader) leaves at its next poll
        if (lane < 2 * NSUMS) {
            pc_gran_store(mine + lane, poison, 0u);
            if (b < L) {
                if (PEERS) {
                    for (int r = 0; r < peers->world; ++r)
                        pc_gran_store(pc_peer_rows(peers->lead[r], peers->world, tag & 1u, peers->rank) + (size_t)b * PC_RES_ROW + lane, poison, 0u);
                } else {
                    pc_gran_store(lead + (size_t)b * PC_RES_ROW + lane, poison, 0u);
                }
            }
        }
        return 1;
    }
    PC_RTL(6);
#pragma unroll
    for (int q = 0; q < PC_NSUM; ++q) tot[q] = q < NSUMS ? __shfl(total, 4 * q) : 0.0;
    return 0;
}

// A resident solve that ends without a result (its hand-off timed out: the grid was not co-resident; or it ran out of rounds) has
// written nothing.  ENQUEUED inside a sequence (raise_stall) it raises the device-side stall flag itself -- everything enqueued
// behind turns into no-ops and the host redoes the solve with launches at its checkpoint.  A launch the host POLLS behind --
// a batch solve, the redo of a stalled solve (psfm_solve_frame_resume) -- must not: it just leaves its control block "not done"
// and pc_finish_sync goes on with one launch per iteration (which return at once behind a raised flag).
__device__ __forceinline__ void pc_res_stall(const PcParams& P, int raise_stall)
{
    if (raise_stall && P.birth_frame && threadIdx.x == 0) *P.stall = P.frame + 1;
}

// (PcSlot and what happens to a slot -- pc_slot_fill / _start / _round / _refresh / _accept / _candidate: psfm_pc_resident.h, host-compilable)

template <int NS, bool PEERS = false>
__global__ __launch_bounds__(PC_BLOCK) __attribute__((amdgpu_waves_per_eu(2, 2)))
void psfm_pc_resident_kernel(PcParams P, unsigned long long* gran, unsigned epoch, int spin_limit, int max_rounds, int quit_code,
                             int init_inside, int raise_stall, double* out_rows, PcPeers peers)
{
    // init_inside: iteration 0 (what psfm_pc_init_kernel does) is this launch's first round; else it runs behind that kernel.
    // When the loop ends with the solve done, every block writes its tracks back (what psfm_pc_writeback_kernel does) and the
    // control block says so.
    if (*P.stall) return;
    __shared__ PsfmSolveCtrl s_C;        // this block's copy of the control block (every block runs the same control step)
    __shared__ PcRound s_R;
    __shared__ double s_next[NS][8][PC_BLOCK];     // (u', d') at the candidate of the round
    __shared__ double s_ref[NS][4][PC_BLOCK];      // refs (r1, r2) of the slots
    __shared__ double s_blk[PC_NSUM];
    const int tid = threadIdx.x;
    const int nblk = (int)gridDim.x;
    const PcF2* F12 = (const PcF2*)P.flow12;
    const unsigned poison = (epoch << 12) | 0xfffu;
    const int* lst = P.list + (int64_t)blockIdx.x * P.list_pitch;
    PcSlot T[NS];
    int cnt;
    if (init_inside) {
        // ---- iteration 0: the block's list, the slots' tracks from their three buffered positions, the sums, Ceres' IterationZero ----
        if (blockIdx.x == 0 && tid == 0) {
            // (whatever gives up below must not leave an earlier solve's outcome to be read as this one's)
            P.ctrl->done = 0; P.ctrl->written = 0;
            if (P.sel) *P.sel = 0;      // (as pc_init_tracks)
        }
        const int n = P.n_lanes_ptr ? min(*P.n_lanes_ptr, P.n_rows) : P.n_rows;
        cnt = pc_build_list(P, n);
        double acc[PC_NSUM];
#pragma unroll
        for (int q = 0; q < PC_NSUM; ++q) acc[q] = 0.0;
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            if (pc_slot_entry(k, tid) < cnt) {
                PcInit o;
                pc_init_entry(P, lst[pc_slot_entry(k, tid)], false, acc, o);
                pc_slot_fill(T[k], o.s, o.c, o.x, o.y);
                s_ref[k][0][tid] = o.r1.x; s_ref[k][1][tid] = o.r1.y; s_ref[k][2][tid] = o.r2.x; s_ref[k][3][tid] = o.r2.y;
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        for (int p = pc_stream_first(NS, tid); p < cnt; p += PC_BLOCK) {     // (streamed entries: their constants go to memory)
            PcInit o;
            pc_init_entry(P, lst[p], true, acc, o);
        }
        pc_block_sums<PC_NSUM>(acc, s_blk);
        if (tid < PSFM_WAVE) {
            double tot[PC_NSUM];
            const int bad = pc_res_allreduce<PC_NSUM, PEERS>(s_blk, gran, nblk, (epoch << 12) | 0xffeu, poison, spin_limit, false, tot, -1, &peers);
            if (tid == 0) {
                s_R.giveup = bad; s_R.accepted = 0;
                if (!bad) {
                    PsfmSolveCtrl& C = s_C;          // (in place, in LDS: a private copy would not stay in registers behind the memset)
                    pc_chain_control(C, tot, 0);
                    C.launches = 1;
                    s_R.done = C.done; s_R.cur = C.cur; s_R.kind = C.kind_next; s_R.mu = C.mu; s_R.a = C.dl_a; s_R.b = C.dl_b;
                }
            }
        }
        __syncthreads();
        if (s_R.giveup) { pc_res_stall(P, raise_stall); return; }
    } else {
        if (tid < PC_CTRL_WORDS) ((unsigned long long*)&s_C)[tid] = ((const unsigned long long*)P.ctrl)[tid];    // (written by the launch in front)
        __syncthreads();
        if (tid == 0) {
            s_R.done = s_C.done; s_R.cur = s_C.cur; s_R.kind = s_C.kind_next; s_R.mu = s_C.mu; s_R.a = s_C.dl_a; s_R.b = s_C.dl_b;
            s_R.accepted = 0; s_R.giveup = 0;
        }
        __syncthreads();
        cnt = P.list_n[blockIdx.x];
        if (!s_R.done) {
            // ---- the slots: constants and the start values from memory (once), the system at x0 for the mu in force ----
            // (an empty slot loads lane 0's state and computes on it; nothing of it is ever added or stored)
            PcTaps tp[NS];
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                const int i = pc_slot_entry(k, tid) < cnt ? lst[pc_slot_entry(k, tid)] : 0;
                const double2 r1 = P.ref1[i], r2 = P.ref2[i], js = P.jscale[i], p1 = P.x1a[i], p2 = P.x2a[i];
                T[k].s = P.scale[i];
                T[k].S0q = js.x; T[k].S1q = js.y;
                s_ref[k][0][tid] = r1.x; s_ref[k][1][tid] = r1.y; s_ref[k][2][tid] = r2.x; s_ref[k][3][tid] = r2.y;
                T[k].x[0] = p1.x; T[k].x[1] = p1.y; T[k].x[2] = p2.x; T[k].x[3] = p2.y;
            }
#pragma unroll
            for (int k = 0; k < NS; ++k) tp[k] = pc_core_taps<PC_ITER_PAIR>(F12, P.H, P.W, T[k].x);
#pragma unroll
            for (int k = 0; k < NS; ++k)
                pc_slot_start(T[k], tp[k], s_ref[k][0][tid], s_ref[k][1][tid], s_ref[k][2][tid], s_ref[k][3][tid], s_R.mu);
        }
    }
    for (unsigned it = 0; it < (unsigned)max_rounds; ++it) {
        if (s_R.done) break;
        const double mu = s_R.mu, a = s_R.a, b = s_R.b;
        const int cur = s_R.cur;
        const bool refresh = s_R.kind != 0;
#ifdef PSFM_TIMELINE
        const int rtl = (epoch == PC_RTL_EPOCH && it >= PC_RTL_R0 && it < PC_RTL_R0 + 8u) ? (int)(it - PC_RTL_R0) : -1;
        if (rtl >= 0 && tid == 0 && blockIdx.x == 0) g_pc_tl_n = rtl + 1;
#else
        const int rtl = -1;
#endif
        PC_RTL(0);
        double acc[PC_NSUM];
#pragma unroll
        for (int q = 0; q < PC_NSUM; ++q) acc[q] = 0.0;
        if (!refresh) {
            // the candidate of (a, b), its cost and -- ahead of the decision -- the system there
            const double mu_next = pc_mu_next(mu);
            PcTaps tp[NS];
#pragma unroll
            for (int k = 0; k < NS; ++k) {     // every slot's taps in flight together
                double xe[4];
                (void)pc_slot_candidate(T[k], a, b, xe);
                tp[k] = pc_core_taps<PC_ITER_PAIR>(F12, P.H, P.W, xe);
            }
            PC_RTL(1);
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                // (a lane without a track in this slot skips it; the sums receive ONE term per track, in list order, like the launches')
                if (pc_slot_entry(k, tid) < cnt) {
                    // (pc_slot_round recomputes the candidate: the same bits, 8 registers fewer across the gather)
                    double nx[8];
                    pc_slot_round(T[k], tp[k], s_ref[k][0][tid], s_ref[k][1][tid], s_ref[k][2][tid], s_ref[k][3][tid], a, b, mu_next, acc, nx);
#pragma unroll
                    for (int q = 0; q < 8; ++q) s_next[k][q][tid] = nx[q];
                }
                __builtin_amdgcn_sched_barrier(0);      // (one slot at a time: interleaving them costs more registers than it hides)
            }
        } else {
            // the system at x for the mu an invalid step has raised: (u, d) of the slots are replaced (rare)
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                if (pc_slot_entry(k, tid) < cnt)
                    pc_slot_refresh<PC_ITER_PAIR>(T[k], F12, P.H, P.W, s_ref[k][0][tid], s_ref[k][1][tid], s_ref[k][2][tid], s_ref[k][3][tid], mu, acc);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        // entries beyond the slots: streamed, as the launches do it
        if (cnt > NS * PC_BLOCK) pc_iter_tracks(P, pc_stream_first(NS, tid), cur, mu, a, b, refresh, acc);
        PC_RTL(2);
        pc_block_sums<PC_RES_SUMS>(acc, s_blk);
        PC_RTL(3);
        if (tid < PSFM_WAVE) {
            double tot[PC_NSUM];
            const bool quit = quit_code != 0 && (quit_code >> 16) == (int)blockIdx.x + 1 && (quit_code & 0xffff) == (int)it;
            const int bad = pc_res_allreduce<PC_RES_SUMS, PEERS>(s_blk, gran, nblk, (epoch << 12) | (it + 1u), poison, spin_limit, quit, tot, rtl, &peers);
            PC_RTL(9);
            // what the control step may need from the totals (pc_derive), one quantity per lane instead of one behind the other
            PcDerived D;
            {
                const int lane = tid;
                const double rad = lane == 0 ? tot[SUM_STEP2] : (lane == 1 ? tot[SUM_XN2] : (lane == 2 ? tot[SUM_G2] : tot[SUM_GN2]));
                const double num = lane == 4 ? tot[SUM_G2] : s_C.x_cost - tot[SUM_COST];
                const double den = lane == 4 ? tot[SUM_JG2] : s_C.mcc;
                const double res = lane < 4 ? sqrt(rad) : num / den;
                D.step_norm = __shfl(res, 0); D.x_norm = __shfl(res, 1); D.gnorm = __shfl(res, 2); D.gnn = __shfl(res, 3);
                D.alpha = __shfl(res, 4); D.rho = __shfl(res, 5);
            }
            PC_RTL(10);
            if (tid == 0) {
                if (bad) s_R.giveup = 1;
                else {
                    // (in place, in LDS; run by every lane of the wave on private copies instead -- uniform branches, no one-lane exec
                    // mask -- it takes the same 1.3 us: a dependent chain of ~150 f64 operations, a few of them square roots / quotients)
                    PsfmSolveCtrl& C = s_C;
                    const int cur0 = C.cur;
                    pc_chain_control_d(C, tot, D, 1);
                    C.launches += 1;
                    s_R.accepted = C.cur != cur0;
                    s_R.done = C.done; s_R.cur = C.cur; s_R.kind = C.kind_next; s_R.mu = C.mu; s_R.a = C.dl_a; s_R.b = C.dl_b;
                }
            }
            PC_RTL(7);
        }
        __syncthreads();
        PC_RTL(8);
        if (s_R.giveup) { pc_res_stall(P, raise_stall); return; }
        if (s_R.accepted) {
            // x <- the candidate (the same operations: the same bits), (u, d) <- what was solved there
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                double nx[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) nx[q] = s_next[k][q][tid];
                pc_slot_accept(T[k], a, b, nx);
            }
        }
    }
    if (!s_R.done) { pc_res_stall(P, raise_stall); return; }            // (ran out of rounds)
    // ---- write-back (block 0 also: statistics, the control block) ----
    const PsfmSolveCtrl C = s_C;
    const bool moved = pc_res_moved(C);                  // (a failed solve hands the parameters back as they came in)
    if (moved || out_rows) {
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            if (pc_slot_entry(k, tid) >= cnt) continue;
            const int i = lst[pc_slot_entry(k, tid)];
            double2 p1 = make_double2(T[k].x[0], T[k].x[1]), p2 = make_double2(T[k].x[2], T[k].x[3]);
            if (!moved) { p1 = P.x1a[i]; p2 = P.x2a[i]; }
            if (out_rows) {
                out_rows[4 * (int64_t)i + 0] = p1.x; out_rows[4 * (int64_t)i + 1] = p1.y;
                out_rows[4 * (int64_t)i + 2] = p2.x; out_rows[4 * (int64_t)i + 3] = p2.y;
            } else {
                P.x1a[i] = p1; P.x2a[i] = p2;
            }
        }
        const int src = pc_res_stream_source(C);
        const double2* xc1 = pc_buf1(P, src);
        const double2* xc2 = pc_buf2(P, src);
        for (int p = pc_stream_first(NS, tid); p < cnt; p += PC_BLOCK) {
            const int i = lst[p];
            const double2 p1 = xc1[i], p2 = xc2[i];
            if (out_rows) {
                out_rows[4 * (int64_t)i + 0] = p1.x; out_rows[4 * (int64_t)i + 1] = p1.y;
                out_rows[4 * (int64_t)i + 2] = p2.x; out_rows[4 * (int64_t)i + 3] = p2.y;
            } else if (src != 0) {
                P.x1a[i] = p1; P.x2a[i] = p2;
            }
        }
    }
    if (blockIdx.x == 0 && tid == 0) {
        pc_writeback_scalars(P, C);
        PsfmSolveCtrl Cw = C;
        Cw.written = 1;
        *P.ctrl = Cw;
    }
}

// Track-sharded runs: the control step on the totals over all ranks (every rank runs it on the same numbers).
// mode 0: replay over the K iterations of a fused launch; 1 / 2: one step behind pc_init / pc_iter.
// stall_host (mode 0, may be NULL): the stall flag as this control step leaves it, written straight into pinned host memory, where
// psfm_shard_peek_stall reads it without a synchronisation (round 3 sent a 4-byte copy behind every control launch: one more
// command on the stream per frame)
__global__ __launch_bounds__(128) void psfm_pc_control_kernel(PcParams P, const double* totals, int K, int mode, int* stall_host)
{
    if (blockIdx.x != 0) return;
    if (mode == 0) {
        // one round trip for everything the replay reads -- the stall flag, the control block, the K x 13 totals -- instead of three
        // dependent ones by a single lane (7.7 us per frame of a sharded sequence went into this launch)
        __shared__ double s_tot[PC_KMAX * PC_NSUM];
        __shared__ PsfmSolveCtrl s_ctrl;
        __shared__ int s_stall;
        const int tid = threadIdx.x;
        const int kk = K < 1 ? 1 : (K > PC_KMAX ? PC_KMAX : K);
        if (tid < kk * PC_NSUM) s_tot[tid] = totals[tid];
        static_assert(sizeof(PsfmSolveCtrl) % 4 == 0 && PC_KMAX * PC_NSUM <= 128, "control kernel: one load per thread");
        for (int q = tid; q < (int)(sizeof(PsfmSolveCtrl) / 4); q += 128) ((unsigned*)&s_ctrl)[q] = ((const unsigned*)P.ctrl)[q];
        if (tid == 0) s_stall = *P.stall;
        __syncthreads();
        if (tid != 0) return;
        if (!s_stall) pc_fused_replay(P, s_tot, kk, true, nullptr, 0, &s_ctrl);
        if (stall_host) __hip_atomic_store(stall_host, *P.stall, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }
    if (threadIdx.x != 0) return;
    PsfmSolveCtrl C = *P.ctrl;
    if (mode == 2 && C.done) return;
    pc_chain_control(C, totals, mode == 1 ? 0 : 1);
    C.launches += 1;
    *P.ctrl = C;
}

// Copy the accepted iterate of the last fused solve from buffer *sel into the log (what the next chain step does on
// its way; needed behind the LAST solve of a sequence, whose positions no chain step picks up).
__global__ __launch_bounds__(PC_BLOCK) void psfm_pc_flush_kernel(PcParams P)
{
    if (*P.stall) return;
    const int m = *P.sel;
    if (m == 0) return;
    const int n = P.n_lanes_ptr ? min(*P.n_lanes_ptr, P.n_rows) : P.n_rows;
    const int i = blockIdx.x * PC_BLOCK + threadIdx.x;
    if (pc_participates(P, i, n)) {
        P.x1a[i] = pc_buf1(P, m)[i];
        P.x2a[i] = pc_buf2(P, m)[i];
    }
}
__global__ void psfm_pc_clear_sel_kernel(int* sel, const int* stall) { if (!*stall) *sel = 0; }
__global__ void psfm_pc_raise_stall_kernel(int* stall, int frame) { if (!*stall) *stall = frame + 1; }

__global__ __launch_bounds__(PC_BLOCK) void psfm_pc_writeback_kernel(PcParams P, double* out_rows)
{
    if (*P.stall) return;
    const PsfmSolveCtrl C = *P.ctrl;
    if (!C.done) {
        // the unrolled iterations did not suffice: poison everything that was enqueued behind this solve; the
        // host resumes it (psfm_track polls `stall` at its checkpoints) and re-enqueues the later frames
        if (blockIdx.x == 0 && threadIdx.x == 0) *P.stall = P.frame + 1;
        return;
    }
    if (C.written) return;       // (the persistent solve has written back itself)
    pc_writeback_tracks(P, C, out_rows);
}

// batch mode: split (n,4) rows into the (x1, x2) pair and (n,2) refs into double2 arrays
__global__ __launch_bounds__(PC_BLOCK) void psfm_pc_load_rows_kernel(const double* __restrict__ uv12, int64_t n,
                                                                     double2* __restrict__ x1, double2* __restrict__ x2)
{
    const int64_t i = (int64_t)blockIdx.x * PC_BLOCK + threadIdx.x;
    if (i >= n) return;
    x1[i] = make_double2(uv12[4 * i], uv12[4 * i + 1]);
    x2[i] = make_double2(uv12[4 * i + 2], uv12[4 * i + 3]);
}

// ------------------------------------------------------------------------------------------------
// host driver
// ------------------------------------------------------------------------------------------------
static int pc_blocks(const psfm_ctx* c, int n_rows_upper)
{
    // grid of the launch chain's grid-stride kernels; PSFM_PC_BLOCKS (<= PC_MAX_BLOCKS) overrides for measurements.  A context with a
    // resident budget (psfm_ctx_set_resident_budget: its resident solves share the device with other contexts') stays inside it
    static const int limit_env = getenv("PSFM_PC_BLOCKS") ? atoi(getenv("PSFM_PC_BLOCKS")) : 0;
    int limit = limit_env >= 1 && limit_env <= PC_MAX_BLOCKS ? limit_env : PC_CHAIN_BLOCKS;
    if (c->resident_budget > 0 && c->resident_budget < limit) limit = c->resident_budget;
    return pc_frame_blocks(n_rows_upper, limit);      // (clamp(ceil(rows / PC_BLOCK), 1, limit): psfm_batch_chain.h, run by the CPU suite)
}

// sol_ctrl layout: [PsfmSolveCtrl][ticket u32][zero word used as the `stall` flag of batch solves]
static psfm_status pc_setup(psfm_ctx* c, PcParams& P, hipStream_t s)
{
    psfm_status rc;
    if ((rc = c->sol_partials.ensure(sizeof(double) * PC_MAX_BLOCKS * PC_NSUM)) != PSFM_OK) return rc;
    const bool fresh = c->sol_ctrl.p == nullptr;
    if ((rc = c->sol_ctrl.ensure(sizeof(PsfmSolveCtrl) + 64)) != PSFM_OK) return rc;
    if (fresh) PSFM_HIP(hipMemsetAsync(c->sol_ctrl.p, 0, sizeof(PsfmSolveCtrl) + 64, s));
    P.partials = c->sol_partials.as<double>();
    P.ctrl = c->sol_ctrl.as<PsfmSolveCtrl>();
    P.ticket = (unsigned*)((char*)c->sol_ctrl.p + sizeof(PsfmSolveCtrl));
    if (!P.stall) P.stall = (int*)((char*)c->sol_ctrl.p + sizeof(PsfmSolveCtrl) + 16);
    // the blocks' lists (pc_build_list): block b of the chain's grid sees the lane chunks b, b + n_blocks, ...
    const int n_blocks = pc_blocks(c, P.n_rows);
    const int chunks = (P.n_rows + PC_BLOCK - 1) / PC_BLOCK;
    // (a banded block takes every (n_blocks / 8)-th chunk of a band of ceil(chunks / 8): at most one chunk more than in block order)
    P.list_pitch = ((chunks + n_blocks - 1) / n_blocks + 1) * PC_BLOCK;
    {
        static const int band = getenv("PSFM_PC_BAND") ? atoi(getenv("PSFM_PC_BAND")) : 1;      // (0: chunks in block order; measurements)
        P.list_banded = band;
    }
    if ((rc = c->sol_list.ensure(sizeof(int) * ((size_t)n_blocks * P.list_pitch + PC_MAX_BLOCKS))) != PSFM_OK) return rc;
    P.list_n = c->sol_list.as<int>();
    P.list = P.list_n + PC_MAX_BLOCKS;
    return PSFM_OK;
}

static void pc_fill_stats(const PsfmSolveCtrl* h, psfm_solve_stats* st)
{
    st->iterations = h->iteration;
    st->successful_steps = h->successful;
    st->termination = h->n_tracks == 0 ? -1 : h->termination;   // -1: nothing to solve (the reference would raise here)
    st->dogleg_nonGN = h->nonGN;
    st->initial_cost = h->initial_cost;
    st->final_cost = h->x_cost;
}

// Keep launching iterations, polling `done` between chunks, until the solve terminates; then write back.
// resident: a resident launch is what has been enqueued -- not done behind it means its hand-off gave up (it has written nothing: the
// control block is as iteration 0 left it, the launches below take the solve from there); a call that sees that twice stops trying
static psfm_status pc_finish_sync(psfm_ctx* c, PcParams& P, int n_blocks, double* out_rows, psfm_solve_stats* st, hipStream_t s,
                                  bool resident = false)
{
    PsfmSolveCtrl* hctrl = psfm_host_solve_ctrl(c);
    int launched = 0, chunk = 6;
    for (;;) {
        PSFM_HIP(hipMemcpyAsync(hctrl, P.ctrl, sizeof(PsfmSolveCtrl), hipMemcpyDeviceToHost, s));
        PSFM_HIP(hipStreamSynchronize(s));
        if (hctrl->done) break;
        if (resident && launched == 0) c->pc_giveups += 1;
        if (launched > 2 * 200 + 64) { psfm_set_error("path-consistency solver did not terminate"); return PSFM_ERR_SOLVER; }
        for (int k = 0; k < chunk; ++k) hipLaunchKernelGGL(psfm_pc_iter_kernel, dim3(n_blocks), dim3(PC_BLOCK), 0, s, P);
        c->n_iter_launches += chunk;
        PSFM_HIP(hipGetLastError());
        launched += chunk;
        chunk = chunk < 32 ? chunk * 2 : 32;
    }
    hipLaunchKernelGGL(psfm_pc_writeback_kernel, dim3(n_blocks), dim3(PC_BLOCK), 0, s, P, out_rows);
    PSFM_HIP(hipGetLastError());
    if (st) pc_fill_stats(hctrl, st);
    // (a failed solve -- invalid steps / a system that is not positive definite / non-finite residuals -- is not an error: like the reference,
    // which ignores Ceres' FAILURE at trajectory_optimize.cpp:81-82, the parameters stay as they came in; stats say 5)
    return PSFM_OK;
}

psfm_status pc_workspace(psfm_ctx* c, int64_t rows, int n_buf)
{
    psfm_status rc;
    // iterate buffers 1..n_buf (two double2 arrays each); ref1, ref2, jscale (double2 each) + scale (double)
    if ((rc = c->sol_x.ensure(sizeof(double2) * rows * 2 * n_buf)) != PSFM_OK) return rc;
    if ((rc = c->sol_state.ensure(sizeof(double2) * rows * 3 + sizeof(double) * rows)) != PSFM_OK) return rc;
    return PSFM_OK;
}

psfm_status pc_frame_params(psfm_ctx* c, const PsfmTrackDims& d, const float* flow01, const float* flow12,
                            const float* flow02, const uint8_t* occ02, int frame, PcParams& P, hipStream_t s)
{
    psfm_status rc;
    if ((rc = pc_workspace(c, d.cap, PC_KMAX)) != PSFM_OK) return rc;
    if ((rc = c->sol_stats.ensure(sizeof(psfm_solve_stats) * (size_t)(d.n_flows + 1))) != PSFM_OK) return rc;
    memset(&P, 0, sizeof(P));
    P.H = d.H; P.W = d.W; P.cw = d.cw; P.ch = d.ch;
    P.birth_frame = c->birth_frame.as<int>();
    P.max_birth = frame - 1;    // three buffered positions: times frame-1, frame, frame+1
    PsfmCounters* ctr = c->counters.as<PsfmCounters>();
    P.n_lanes_ptr = &ctr->n_lanes;
    P.stall = &ctr->stall;
    P.n_rows = (int)d.cap;
    double2* lg = c->log.as<double2>();
    P.p0 = lg + (int64_t)(frame - 1) * d.cap;
    P.x1a = lg + (int64_t)frame * d.cap;
    P.x2a = lg + (int64_t)(frame + 1) * d.cap;
    P.xs = c->sol_x.as<double2>(); P.xs_stride = d.cap;
    P.sel = &ctr->sel;
    P.n_lanes_snap = ctr->n_lanes_snap;
    P.ref1 = c->sol_state.as<double2>();
    P.ref2 = P.ref1 + d.cap;
    P.jscale = P.ref2 + d.cap;
    P.scale = (double*)(P.jscale + d.cap);
    P.flow12 = (const float2*)flow12; P.flow01 = (const float2*)flow01; P.flow02 = (const float2*)flow02;
    P.occ02 = occ02;
    P.frame = frame;
    P.stats_dev = c->sol_stats.as<psfm_solve_stats>();
    return pc_setup(c, P, s);
}

// The trust-region loop of the launch chain as ONE persistent launch behind pc_init (psfm_pc_resident_kernel), when this call
// has the device to itself and the grid is co-resident; returns false when it is not used (the caller launches iterations).
// PSFM_PC_PERSIST=0 keeps one launch per iteration (measurements, tests).
template <int NS>
static int pc_resident_capacity(psfm_ctx* c)
{
    if (c->pc_persist_blocks[NS] < 0) {
        c->pc_persist_blocks[NS] = 0;
        int per_cu = 0;
        hipDeviceProp_t prop;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, psfm_pc_resident_kernel<NS, false>, PC_BLOCK, 0) == hipSuccess &&
            hipGetDeviceProperties(&prop, c->device) == hipSuccess)
            c->pc_persist_blocks[NS] = per_cu * prop.multiProcessorCount;
    }
    return c->pc_persist_blocks[NS];
}

// the launch of psfm_pc_resident_kernel<ns, PEERS> (a...: the kernel's arguments)
template <bool PEERS, class... A>
static void pc_launch_resident(int ns, int n_blocks, hipStream_t s, A... a)
{
    const dim3 grid((unsigned)n_blocks), block(PC_BLOCK);
    if (ns == 1) hipLaunchKernelGGL((psfm_pc_resident_kernel<1, PEERS>), grid, block, 0, s, a...);
    else if (ns == 2) hipLaunchKernelGGL((psfm_pc_resident_kernel<2, PEERS>), grid, block, 0, s, a...);
    else hipLaunchKernelGGL((psfm_pc_resident_kernel<3, PEERS>), grid, block, 0, s, a...);
}

// peers != nullptr: the launch of ONE rank of a solve that spans several (PcPeers); `peer_epoch` is the epoch all ranks tag this
// solve's granules with, the member rows live in front of the leader area of the context's peer buffer (never in sol_bar, whose
// granules carry the context's own launch counter)
static bool pc_persist_enqueue(psfm_ctx* c, const PcParams& P, int n_blocks, double* out_rows, bool init_inside, bool raise_stall, hipStream_t s,
                               const PcPeers* peers = nullptr, unsigned peer_epoch = 0)
{
    const char* env = getenv("PSFM_PC_PERSIST");          // (read per call: the tests switch it inside one process)
    if ((env && atoi(env) == 0) || !c->pc_persist_ok || c->pc_giveups >= 2 || P.export_sums) return false;
    if (n_blocks > PC_RES_BLOCKS) return false;
    // slots per thread: what the longest possible list needs, at most PC_RES_NS_MAX (longer lists are streamed behind the slots)
    int ns = P.list_pitch / PC_BLOCK - 1;           // (the pitch has one chunk of head-room, see pc_setup)
    if (getenv("PSFM_PC_SLOTS")) ns = atoi(getenv("PSFM_PC_SLOTS"));      // (measurements, tests: fewer slots = a streamed tail)
    ns = ns < 1 ? 1 : (ns > PC_RES_NS_MAX ? PC_RES_NS_MAX : ns);
    const int capacity = ns == 1 ? pc_resident_capacity<1>(c) : (ns == 2 ? pc_resident_capacity<2>(c) : pc_resident_capacity<3>(c));
    if (n_blocks > capacity) return false;                 // (every block must be resident at once)
    // granules: one row per block + one per leader; zeroed once -- tags carry the launch epoch, so what an earlier launch left
    // never matches (the 20-bit epoch wraps after a million solves: cleared again then)
    const size_t gbytes = sizeof(unsigned long long) * PC_RES_ROW * (PC_RES_BLOCKS + 2 * PC_LEADERS);      // (two sets of leader rows)
    const bool fresh = c->sol_bar.bytes < gbytes;
    if (c->sol_bar.ensure(gbytes) != PSFM_OK) return false;
    c->pc_epoch += 1;
    if (fresh || c->pc_epoch >= (1u << 20)) {
        if (hipMemsetAsync(c->sol_bar.p, 0, gbytes, s) != hipSuccess) return false;
        c->pc_epoch = 1;
    }
    // polls of (s_sleep 1 + a batch of uncached loads, ~1.5 us): ~10 ms
    const int spin_limit = getenv("PSFM_PC_SPIN") ? atoi(getenv("PSFM_PC_SPIN")) : 8000;      // (read per call: a test forces the give-up with 0)
    // tests: "block,round" makes that block give up in that round (what a grid that is not co-resident looks like to the others)
    int quit_code = 0;
    if (const char* q = getenv("PSFM_PC_QUIT")) {
        int qb = 0, qr = 0;
        if (sscanf(q, "%d,%d", &qb, &qr) == 2 && qb >= 0 && qr >= 0) quit_code = ((qb + 1) << 16) | (qr & 0xffff);
    }
    unsigned long long* gran = c->sol_bar.as<unsigned long long>();
    const int max_rounds = 2 * 200 + 64;
    PcPeers pp;
    memset(&pp, 0, sizeof(pp));
    // (the write-back is in the launch too)
    if (peers) {
        pp = *peers;
        // ranks start this launch up to a host-side scheduling delay apart: the polls wait longer before they give a solve up (~100 ms)
        const int spin_peer = getenv("PSFM_PC_SPIN") ? spin_limit : 80000;
        unsigned long long* members = c->peer_area.as<unsigned long long>();      // [PC_RES_BLOCKS rows], in front of the leader area
        const unsigned ep = peer_epoch & 0xfffffu;
        pc_launch_resident<true>(ns, n_blocks, s, P, members, ep, spin_peer, max_rounds, quit_code, init_inside ? 1 : 0, raise_stall ? 1 : 0, out_rows, pp);
    }
    else pc_launch_resident<false>(ns, n_blocks, s, P, gran, c->pc_epoch, spin_limit, max_rounds, quit_code, init_inside ? 1 : 0, raise_stall ? 1 : 0, out_rows, pp);
    c->n_resident += 1;
    return true;
}

// ---- ONE solve over several ranks (psfm_shard.hip) ----
size_t psfm_peer_area_bytes(void) { return sizeof(unsigned long long) * PC_RES_ROW * ((size_t)PC_RES_BLOCKS + 2 * PSFM_MAX_PEERS * PC_LEADERS); }
size_t psfm_peer_lead_offset(void) { return sizeof(unsigned long long) * PC_RES_ROW * (size_t)PC_RES_BLOCKS; }
int psfm_peer_leaders(int n_blocks) { return n_blocks < PC_LEADERS ? n_blocks : PC_LEADERS; }
int psfm_solve_blocks(psfm_ctx* c, const PsfmTrackDims& d) { return pc_blocks(c, (int)d.cap); }

// This rank's launch of the solve of `frame` over all ranks of c->peers: iteration 0, the trust-region loop with the cross-rank
// all-reduce, the write-back -- enqueued, nothing read back.  There is no launch-chain form of it (launches cannot add sums across
// ranks): a launch that cannot be made, or that gives up, leaves the stall flag raised, every rank's polls run into this rank's
// poison (or their limit), and the caller redoes the solve in the exchange form at its checkpoint.
psfm_status psfm_solve_frame_enqueue_peer(psfm_ctx* c, const PsfmTrackDims& d, const float* flow01, const float* flow12,
                                          const float* flow02, const uint8_t* occ02, int frame, unsigned epoch, hipStream_t s)
{
    PcParams P;
    psfm_status rc = pc_frame_params(c, d, flow01, flow12, flow02, occ02, frame, P, s);
    if (rc != PSFM_OK) return rc;
    const int n_blocks = pc_blocks(c, (int)d.cap);
    PcPeers pp;
    memset(&pp, 0, sizeof(pp));
    pp.world = c->peer_world; pp.rank = c->peer_rank;
    for (int r = 0; r < c->peer_world; ++r) { pp.L[r] = c->peer_L[r]; pp.lead[r] = (unsigned long long*)c->peer_lead[r]; }
    if (pp.L[pp.rank] != psfm_peer_leaders(n_blocks)) {
        psfm_set_error("psfm_shard_solve_peer: this rank's launch has %d blocks, the ranks were told %d leaders", n_blocks, pp.L[pp.rank]);
        return PSFM_ERR_ARG;
    }
    const bool saved_ok = c->pc_persist_ok;
    const int saved_giveups = c->pc_giveups;
    c->pc_persist_ok = true; c->pc_giveups = 0;          // (the caller decided for all ranks at once: psfm_shard_peer_connect)
    const bool ok = pc_persist_enqueue(c, P, n_blocks, nullptr, true, true, s, &pp, epoch);
    c->pc_persist_ok = saved_ok; c->pc_giveups = saved_giveups;
    if (!ok) {
        // (the other ranks must not wait for sums that will never come: raise the flag, they give up at their spin limit)
        hipLaunchKernelGGL(psfm_pc_raise_stall_kernel, dim3(1), dim3(1), 0, s, P.stall, frame);
    }
    PSFM_HIP(hipGetLastError());
    return PSFM_OK;
}

// Enqueue one frame's solve with NO host synchronisation: the resident solve (iteration 0, the trust-region loop and the
// write-back in ONE launch) when the call has the device to itself, else pc_init + `unroll` launches of one iteration each; a
// solve that is not done behind them -- the loop gave up on its hand-off, the launches did not suffice -- has its write-back
// kernel raise the device-side stall flag, which turns everything enqueued behind it into no-ops; the host redoes it at its
// checkpoint.
psfm_status psfm_solve_frame_enqueue(psfm_ctx* c, const PsfmTrackDims& d, const float* flow01, const float* flow12,
                                     const float* flow02, const uint8_t* occ02, int frame, int unroll, hipStream_t s)
{
    PcParams P;
    psfm_status rc = pc_frame_params(c, d, flow01, flow12, flow02, occ02, frame, P, s);
    if (rc != PSFM_OK) return rc;
    const int n_blocks = pc_blocks(c, (int)d.cap);
    // iteration 0, then the loop and the write-back in one launch when possible (a loop that gave up on its barrier leaves the
    // control block "not done": the write-back kernel behind it then raises the stall flag and the host redoes the solve at its
    // checkpoint), else `unroll` launches of one iteration each + write-back
    // (PSFM_PC_INIT_INSIDE=0: iteration 0 as its own launch in front of the resident solve -- measurements, tests)
    const bool inside = !(getenv("PSFM_PC_INIT_INSIDE") && atoi(getenv("PSFM_PC_INIT_INSIDE")) == 0);
    if (!inside || !pc_persist_enqueue(c, P, n_blocks, nullptr, true, true, s)) {
        hipLaunchKernelGGL(psfm_pc_init_kernel, dim3(n_blocks), dim3(PC_BLOCK), 0, s, P);
        if (!pc_persist_enqueue(c, P, n_blocks, nullptr, false, true, s)) {
            for (int k = 0; k < unroll; ++k) hipLaunchKernelGGL(psfm_pc_iter_kernel, dim3(n_blocks), dim3(PC_BLOCK), 0, s, P);
            c->n_iter_launches += unroll;
            // (the resident solve writes back, or raises the stall flag, itself)
            hipLaunchKernelGGL(psfm_pc_writeback_kernel, dim3(n_blocks), dim3(PC_BLOCK), 0, s, P, (double*)nullptr);
        }
    }
    PSFM_HIP(hipGetLastError());
    return PSFM_OK;
}

// The stalled solve of `frame`: clear the flag, iterate to termination with host polling, write back.
psfm_status psfm_solve_frame_resume(psfm_ctx* c, const PsfmTrackDims& d, const float* flow01, const float* flow12,
                                    const float* flow02, const uint8_t* occ02, int frame, psfm_solve_stats* st,
                                    int try_fused_k, bool chain_stalled, hipStream_t s)
{
    // chain_stalled: the solve that raised the flag was a launch-chain solve already -- it ran out of unrolled launches or its
    // resident launch gave up (the grid was not co-resident: another process on the device); this redo uses launches, and a
    // call that sees it happen twice stops trying the resident form
    if (chain_stalled && c->pc_persist_ok) c->pc_giveups += 1;
    PcParams P;
    psfm_status rc = pc_frame_params(c, d, flow01, flow12, flow02, occ02, frame, P, s);
    if (rc != PSFM_OK) return rc;
    PSFM_HIP(hipMemsetAsync(P.stall, 0, sizeof(int), s));
    // from the top: the launch chain never writes buffer 0 (the log slabs) before its write-back; a fused solve that gave
    // up left the values it started from in the iterate buffer PsfmCounters::sel names -- back into the log first
    const int nb_all = (int)((d.cap + PC_BLOCK - 1) / PC_BLOCK);
    hipLaunchKernelGGL(psfm_pc_flush_kernel, dim3(nb_all), dim3(PC_BLOCK), 0, s, P);
    hipLaunchKernelGGL(psfm_pc_clear_sel_kernel, dim3(1), dim3(1), 0, s, P.sel, (const int*)P.stall);
    if (try_fused_k > 0) {
        // most redos are solves that needed one or two iterations more than the sequence's usual: the fused solve with
        // try_fused_k iterations settles those in one launch; anything else falls through to the chain
        psfm_status rc2 = psfm_solve_frame_fused(c, d, flow01, flow12, flow02, occ02, frame, try_fused_k, s);
        if (rc2 != PSFM_OK) return rc2;
        PsfmCounters* hc = (PsfmCounters*)c->host_pinned;
        psfm_solve_stats* hs = (psfm_solve_stats*)((char*)c->host_pinned + 288);
        PSFM_HIP(hipMemcpyAsync(hc, c->counters.p, sizeof(PsfmCounters), hipMemcpyDeviceToHost, s));
        PSFM_HIP(hipMemcpyAsync(hs, c->sol_stats.as<psfm_solve_stats>() + frame, sizeof(psfm_solve_stats), hipMemcpyDeviceToHost, s));
        PSFM_HIP(hipStreamSynchronize(s));
        if (!hc->stall) { if (st) *st = *hs; return PSFM_OK; }
        PSFM_HIP(hipMemsetAsync(P.stall, 0, sizeof(int), s));
        hipLaunchKernelGGL(psfm_pc_flush_kernel, dim3(nb_all), dim3(PC_BLOCK), 0, s, P);
        hipLaunchKernelGGL(psfm_pc_clear_sel_kernel, dim3(1), dim3(1), 0, s, P.sel, (const int*)P.stall);
    }
    const int n_blocks = pc_blocks(c, (int)d.cap);
    hipLaunchKernelGGL(psfm_pc_init_kernel, dim3(n_blocks), dim3(PC_BLOCK), 0, s, P);
    // (the host polls behind this launch: a resident solve that gives up must leave the stall flag alone -- see pc_res_stall)
    bool resident = false;
    if (chain_stalled || !(resident = pc_persist_enqueue(c, P, n_blocks, nullptr, false, false, s))) {
        for (int k = 0; k < 4; ++k) hipLaunchKernelGGL(psfm_pc_iter_kernel, dim3(n_blocks), dim3(PC_BLOCK), 0, s, P);
        c->n_iter_launches += 4;
    }
    PSFM_HIP(hipGetLastError());
    return pc_finish_sync(c, P, n_blocks, nullptr, st, s, resident);
}

int psfm_solve_kmax(void) { return PC_KMAX; }
int psfm_resident_blocks(psfm_ctx* c) { return pc_resident_capacity<PC_RES_NS_MAX>(c); }

// ---- track-sharded runs (psfm_shard.hip): one launch of the solve of `frame` that only exports its sums
//      (kind 0 fused with K iterations, 1 pc_init, 2 pc_iter), the control step on the combined totals, the write-back ----
psfm_status psfm_solve_export(psfm_ctx* c, const PsfmTrackDims& d, const float* flow01, const float* flow12, const float* flow02,
                              const uint8_t* occ02, int frame, int kind, int K, double* sums_out, hipStream_t s)
{
    PcParams P;
    psfm_status rc = pc_frame_params(c, d, flow01, flow12, flow02, occ02, frame, P, s);
    if (rc != PSFM_OK) return rc;
    P.export_sums = sums_out;
    if (kind == 0) return pc_launch_fused_export(c, d, P, K, s);
    const int n_blocks = pc_blocks(c, (int)d.cap);
    if (kind == 1) hipLaunchKernelGGL(psfm_pc_init_kernel, dim3(n_blocks), dim3(PC_BLOCK), 0, s, P);
    else hipLaunchKernelGGL(psfm_pc_iter_kernel, dim3(n_blocks), dim3(PC_BLOCK), 0, s, P);
    PSFM_HIP(hipGetLastError());
    return PSFM_OK;
}

psfm_status psfm_solve_control(psfm_ctx* c, const PsfmTrackDims& d, int frame, int kind, int K, const double* totals, hipStream_t s,
                               int* stall_host)
{
    PcParams P;
    psfm_status rc = pc_frame_params(c, d, nullptr, nullptr, nullptr, nullptr, frame, P, s);
    if (rc != PSFM_OK) return rc;
    hipLaunchKernelGGL(psfm_pc_control_kernel, dim3(1), dim3(128), 0, s, P, totals, K, kind, kind == 0 ? stall_host : nullptr);
    PSFM_HIP(hipGetLastError());
    return PSFM_OK;
}

// solver state after a control step: done flag, stall flag, statistics (synchronises)
psfm_status psfm_solve_state(psfm_ctx* c, int* done, int* stall, psfm_solve_stats* st, hipStream_t s)
{
    PsfmSolveCtrl* hctrl = psfm_host_solve_ctrl(c);
    PsfmCounters* hc = (PsfmCounters*)c->host_pinned;
    PSFM_HIP(hipMemcpyAsync(hctrl, c->sol_ctrl.p, sizeof(PsfmSolveCtrl), hipMemcpyDeviceToHost, s));
    PSFM_HIP(hipMemcpyAsync(hc, c->counters.p, sizeof(PsfmCounters), hipMemcpyDeviceToHost, s));
    PSFM_HIP(hipStreamSynchronize(s));
    if (done) *done = hctrl->done;
    if (stall) *stall = hc->stall;
    if (st) pc_fill_stats(hctrl, st);
    if (st && hctrl->failed) st->termination = PSFM_TERM_FAILURE;
    return PSFM_OK;
}

// redo of a fused solve that gave up: the values it started from back into the log, stall flag cleared
psfm_status psfm_solve_restore(psfm_ctx* c, const PsfmTrackDims& d, int frame, hipStream_t s)
{
    PcParams P;
    psfm_status rc = pc_frame_params(c, d, nullptr, nullptr, nullptr, nullptr, frame, P, s);
    if (rc != PSFM_OK) return rc;
    PSFM_HIP(hipMemsetAsync(P.stall, 0, sizeof(int), s));
    const int nb = (int)((d.cap + PC_BLOCK - 1) / PC_BLOCK);
    hipLaunchKernelGGL(psfm_pc_flush_kernel, dim3(nb), dim3(PC_BLOCK), 0, s, P);
    hipLaunchKernelGGL(psfm_pc_clear_sel_kernel, dim3(1), dim3(1), 0, s, P.sel, (const int*)P.stall);
    PSFM_HIP(hipGetLastError());
    return PSFM_OK;
}

psfm_status psfm_solve_writeback(psfm_ctx* c, const PsfmTrackDims& d, int frame, hipStream_t s)
{
    PcParams P;
    psfm_status rc = pc_frame_params(c, d, nullptr, nullptr, nullptr, nullptr, frame, P, s);
    if (rc != PSFM_OK) return rc;
    hipLaunchKernelGGL(psfm_pc_writeback_kernel, dim3(pc_blocks(c, (int)d.cap)), dim3(PC_BLOCK), 0, s, P, (double*)nullptr);
    PSFM_HIP(hipGetLastError());
    return PSFM_OK;
}

// Behind the last solve of a sequence: the accepted iterate into the log (no chain step follows to do it).
psfm_status psfm_solve_flush(psfm_ctx* c, const PsfmTrackDims& d, int frame, hipStream_t s)
{
    PcParams P;
    psfm_status rc = pc_frame_params(c, d, nullptr, nullptr, nullptr, nullptr, frame, P, s);
    if (rc != PSFM_OK) return rc;
    const int n_blocks = (int)((d.cap + PC_BLOCK - 1) / PC_BLOCK);
    hipLaunchKernelGGL(psfm_pc_flush_kernel, dim3(n_blocks), dim3(PC_BLOCK), 0, s, P);
    hipLaunchKernelGGL(psfm_pc_clear_sel_kernel, dim3(1), dim3(1), 0, s, P.sel, (const int*)P.stall);
    PSFM_HIP(hipGetLastError());
    return PSFM_OK;
}

// path_consistency_cost.h:42-59 as ceres::AutoDiffCostFunction<PathConsistencyError, 6, 4>::Evaluate sees it, one residual block per
// thread: the six residuals and the 6 x 4 Jacobian (row-major, like Ceres' jacobians[0]) at uv12 -- through the SAME pc_core_eval the
// solver kernels call, written out in full so that a test can hold it against the functor differentiated by an independent mechanism
// (tests/test_pc_eval_autograd.py: f64 torch.autograd of the reference's formulas as written).
__global__ void __launch_bounds__(PC_BLOCK) psfm_pc_eval_kernel(const double* __restrict__ uv12, const double* __restrict__ ref1,
                                                                const double* __restrict__ ref2, const double* __restrict__ scale,
                                                                const float2* __restrict__ flow12, long long n, int W, int H,
                                                                double* __restrict__ res, double* __restrict__ jac)
{
    const long long i = (long long)blockIdx.x * PC_BLOCK + threadIdx.x;
    if (i >= n) return;
    const double x[4] = {uv12[4 * i], uv12[4 * i + 1], uv12[4 * i + 2], uv12[4 * i + 3]};
    const double s = scale[i];
    double r[6], j[4];
    pc_core_eval<true>((const PcF2*)flow12, H, W, x, ref1[2 * i], ref1[2 * i + 1], ref2[2 * i], ref2[2 * i + 1], s, r, j);
    if (res) for (int k = 0; k < 6; ++k) res[6 * i + k] = r[k];
    if (jac) {
        double* J = jac + 24 * i;
        for (int k = 0; k < 24; ++k) J[k] = 0.0;
        J[0] = 1.0; J[5] = 1.0; J[10] = s; J[15] = s;              // d r0 / d x0, d r1 / d x1, d r2 / d x2, d r3 / d x3
        J[16] = j[0]; J[17] = j[1]; J[18] = 1.0;                   // r4 = (x2 - x0) - F12.x(row = x1, col = x0)
        J[20] = j[2]; J[21] = j[3]; J[23] = 1.0;                   // r5 = (x3 - x1) - F12.y
    }
}

psfm_status psfm_launch_pc_eval(const double* uv12, const double* ref1, const double* ref2, const double* scale, const float* flow12,
                                int64_t n, int w, int h, double* res, double* jac, hipStream_t s)
{
    if (n == 0) return PSFM_OK;
    const unsigned nb = (unsigned)((n + PC_BLOCK - 1) / PC_BLOCK);
    hipLaunchKernelGGL(psfm_pc_eval_kernel, dim3(nb), dim3(PC_BLOCK), 0, s, uv12, ref1, ref2, scale, (const float2*)flow12,
                       (long long)n, w, h, res, jac);
    PSFM_HIP(hipGetLastError());
    return PSFM_OK;
}

psfm_status psfm_solve_batch(psfm_ctx* c, const double* uv12, const double* ref1, const double* ref2,
                             const double* scale, const float* flow12, int64_t n, int w, int h, double* out,
                             psfm_solve_stats* st, hipStream_t s)
{
    if (n == 0) return PSFM_OK;
    if (n > 0x3fffffff) { psfm_set_error("psfm_optimize_location: n too large"); return PSFM_ERR_ARG; }
    psfm_status rc;
    if ((rc = pc_workspace(c, n, 2)) != PSFM_OK) return rc;
    if ((rc = c->sol_misc.ensure(sizeof(double2) * n * 2)) != PSFM_OK) return rc;
    PcParams P;
    memset(&P, 0, sizeof(P));
    P.H = h; P.W = w;
    P.cw = (float)((double)(w - 1) / 2.0); P.ch = (float)((double)(h - 1) / 2.0);
    P.n_rows = (int)n;
    P.x1a = c->sol_misc.as<double2>();
    P.x2a = P.x1a + n;
    P.xs = c->sol_x.as<double2>(); P.xs_stride = n;
    P.ref1 = c->sol_state.as<double2>();
    P.ref2 = P.ref1 + n;
    P.jscale = P.ref2 + n;
    P.scale = (double*)(P.jscale + n);
    P.flow12 = (const float2*)flow12;
    if ((rc = pc_setup(c, P, s)) != PSFM_OK) return rc;
    const int n_blocks = pc_blocks(c, (int)n);
    const unsigned nb = (unsigned)((n + PC_BLOCK - 1) / PC_BLOCK);
    hipLaunchKernelGGL(psfm_pc_load_rows_kernel, dim3(nb), dim3(PC_BLOCK), 0, s, uv12, n, P.x1a, P.x2a);
    PSFM_HIP(hipMemcpyAsync(P.ref1, ref1, sizeof(double2) * n, hipMemcpyDeviceToDevice, s));
    PSFM_HIP(hipMemcpyAsync(P.ref2, ref2, sizeof(double2) * n, hipMemcpyDeviceToDevice, s));
    PSFM_HIP(hipMemcpyAsync(P.scale, scale, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(psfm_pc_init_kernel, dim3(n_blocks), dim3(PC_BLOCK), 0, s, P);
    bool resident = false;
    if (!(resident = pc_persist_enqueue(c, P, n_blocks, out, false, false, s))) {
        for (int k = 0; k < 4; ++k) hipLaunchKernelGGL(psfm_pc_iter_kernel, dim3(n_blocks), dim3(PC_BLOCK), 0, s, P);
        c->n_iter_launches += 4;
    }
    PSFM_HIP(hipGetLastError());
    rc = pc_finish_sync(c, P, n_blocks, out, st, s, resident);
    if (rc != PSFM_OK) return rc;
    PSFM_HIP(hipStreamSynchronize(s));
    return PSFM_OK;
}

// ---- the multi-problem launch chain (psfm_solver_multi.hip): one problem's buffers in its own context, as psfm_solve_batch sets them up ----
psfm_status pc_multi_problem(psfm_ctx* c, int64_t cap, int h, int w, PcParams& P, int* limit, hipStream_t s)
{
    if (cap < 1 || cap > 0x3fffffff) { psfm_set_error("path-consistency solver: %lld rows", (long long)cap); return PSFM_ERR_ARG; }
    psfm_status rc;
    if ((rc = pc_workspace(c, cap, 2)) != PSFM_OK) return rc;
    if ((rc = c->sol_misc.ensure(sizeof(double2) * cap * 2)) != PSFM_OK) return rc;
    memset(&P, 0, sizeof(P));
    P.H = h; P.W = w;
    P.cw = (float)((double)(w - 1) / 2.0); P.ch = (float)((double)(h - 1) / 2.0);
    P.n_rows = (int)cap;
    P.x1a = c->sol_misc.as<double2>();
    P.x2a = P.x1a + cap;
    P.xs = c->sol_x.as<double2>(); P.xs_stride = cap;
    P.ref1 = c->sol_state.as<double2>();
    P.ref2 = P.ref1 + cap;
    P.jscale = P.ref2 + cap;
    P.scale = (double*)(P.jscale + cap);
    if ((rc = pc_setup(c, P, s)) != PSFM_OK) return rc;       // (lists sized for cap rows: the most entries per block of any row count)
    *limit = pc_blocks(c, 0x3fffffff);
    return PSFM_OK;
}

void pc_multi_stats(const PsfmSolveCtrl* C, psfm_solve_stats* st) { pc_fill_stats(C, st); }
