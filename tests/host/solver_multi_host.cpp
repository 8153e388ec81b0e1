// Host build of the MULTI-PROBLEM launch chain's index rules (particle-sfm_amd/csrc/psfm_solver_multi.h) for
// tests/test_solver_multi_host.py, beside the single chain's: psfm_pc_resident.h (the list plan, the tree of the block sums) and
// psfm_pc_core.h / psfm_pc_control.h (per-track arithmetic, the control step) -- the device's own code, as tests/host/pc_chain_host.cpp
// compiles it.
//
// One "launch" is a loop over the blocks of a grid; what a block does -- compact its chunks into its list, add its entries' terms in
// list order into its row of the partial sums, and, after the launch, the tree over the rows and the control step -- is written ONCE
// (block_init / block_iter / finish_launch) and called two ways:
//   single   the problem alone, the way psfm_pc_init_kernel / psfm_pc_iter_kernel see it: gridDim.x = pc_blocks' count, computed on the
//            host (single_blocks below restates pc_blocks of psfm_solver.hip), every block of the grid works
//   multi    a table of problems under one grid (grid_x, problems), the way psfm_pc_multi_*_kernel see it: per block the rules of
//            psfm_solver_multi.h decide whether it works and with which block count; launches go on until no problem is left undone,
//            so a problem that is done sees further launches
// and everything the two leave -- the lists, every launch's rows of block sums, every control block, the final iterates -- is
// compared byte for byte.  (A block's own sum is formed in list order here; on the device it is the DPP / LDS tree of
// psfm_pc_reduce.h, the same function in both forms.)  Test infrastructure (g++ -O2 -mfma -ffp-contract=off).
#include <string.h>
#include <vector>

#include "psfm_pc_resident.h"
#include "psfm_solver_multi.h"

namespace {
struct Problem {
    long n;                    // rows the step's scan counted
    const double *x0, *ref1, *ref2, *scale;
    const float* flow;
    int H, W, limit, banded;
    int n_flows;               // steps of the sequence (the problem takes part in steps 1 .. n_flows - 1)
};

// what a run leaves: compared between the two forms
struct Trace {
    std::vector<int> lists;            // per block: count, then entries
    std::vector<double> rows;          // per launch that worked: n_blocks x PC_NSUM
    std::vector<PsfmSolveCtrl> ctrl;   // the control block behind every launch that worked
    std::vector<double> x;             // final iterate (4 n)
    int launches_seen = 0;             // launches the problem was offered (multi: including those behind its end)
};

struct State {
    const Problem* p;
    int n_blocks = 0;
    std::vector<std::vector<int>> list;
    std::vector<double> b1, b2, js, part;
    PsfmSolveCtrl C;
    bool started = false;
    const double* buf(int m) const { return m == 0 ? p->x0 : (m == 1 ? b1.data() : b2.data()); }
    double* wbuf(int m) { return m == 1 ? b1.data() : b2.data(); }
};

void eval(const Problem& p, const double* x, long i, double* r, double* j)
{
    pc_core_eval<true>((const PcF2*)p.flow, p.H, p.W, x, p.ref1[2 * i], p.ref1[2 * i + 1], p.ref2[2 * i], p.ref2[2 * i + 1], p.scale[i], r, j);
}

// pc_build_list + pc_init_tracks of block `blk` among n_blocks
void block_init(State& S, int blk, int n_blocks, int n)
{
    const Problem& p = *S.p;
    std::vector<int>& lst = S.list[blk];
    lst.clear();
    const PcListPlan plan = pc_list_plan(blk, n_blocks, n, p.banded);
    for (int q = plan.first; pc_list_chunk_ok(plan, q); q += plan.step)
        for (int t = 0; t < PC_BLOCK; ++t) {
            const int i = (plan.band0 + q) * PC_BLOCK + t;
            if (i < n) lst.push_back(i);
        }
    double* acc = S.part.data() + (size_t)blk * PC_NSUM;
    for (int k = 0; k < PC_NSUM; ++k) acc[k] = 0.0;
    const double mu = 1e-8;
    for (int i : lst) {
        double r0[6], j0[4];
        eval(p, p.x0 + 4 * (long)i, i, r0, j0);
        const PcConst c = pc_core_const(p.scale[i], j0);
        S.js[2 * (long)i] = c.S0q; S.js[2 * (long)i + 1] = c.S1q;
        acc[SUM_CNT] += 1.0;
        acc[SUM_COST0] += pc_core_cost(r0);
        PcSys y;
        pc_core_system<true>(p.x0 + 4 * (long)i, r0, j0, c, mu, pc_core_iA22(c, mu), acc, y, CH_QUD, CH_QDD);
    }
}

// pc_iter_tracks of block `blk`
void block_iter(State& S, int blk)
{
    const Problem& p = *S.p;
    const PsfmSolveCtrl& C = S.C;
    const double* xc = S.buf(C.cur);
    double* xn = S.wbuf(pc_other(C.cur));
    const double mu = C.mu, a = C.dl_a, b = C.dl_b, mu_next = fmax(1e-8, 2.0 * mu / 10.0);
    const bool refresh = C.kind_next != 0;
    double* acc = S.part.data() + (size_t)blk * PC_NSUM;
    for (int k = 0; k < PC_NSUM; ++k) acc[k] = 0.0;
    for (int i : S.list[blk]) {
        const double s = p.scale[i];
        PcConst c;
        c.s = s; c.S0q = S.js[2 * (long)i]; c.S1q = S.js[2 * (long)i + 1]; c.H22 = fma(s, s, 1.0);
        const double* x = xc + 4 * (long)i;
        double r[6], jac[4];
        PcSys y;
        eval(p, x, i, r, jac);
        if (refresh) { pc_core_system<true>(x, r, jac, c, mu, pc_core_iA22(c, mu), acc, y, CH_QUD, CH_QDD); continue; }
        double unused[PC_NSUM], xp[4];
        for (int k = 0; k < PC_NSUM; ++k) unused[k] = 0.0;
        pc_core_system<false>(x, r, jac, c, mu, pc_core_iA22(c, mu), unused, y, 0, 0);
        pc_core_step<false, false>(x, r, jac, c, y, a, b, acc, xp);
        for (int k = 0; k < 4; ++k) xn[4 * (long)i + k] = xp[k];
        eval(p, xp, i, r, jac);
        acc[SUM_COST] += pc_core_cost(r);
        pc_core_system<true>(xp, r, jac, c, mu_next, pc_core_iA22(c, mu_next), acc, y, CH_QUD, CH_QDD);
    }
}

// the last block of a launch: pc_reduce_totals over n_blocks rows + pc_chain_control
void finish_launch(State& S, int n_blocks, int is_init, Trace& T)
{
    double tot[PC_NSUM];
    pc_tree_totals(S.part.data(), PC_NSUM, n_blocks, PC_NSUM, tot);
    pc_chain_control(S.C, tot, is_init ? 0 : 1);
    S.C.launches += 1;
    T.rows.insert(T.rows.end(), S.part.begin(), S.part.begin() + (size_t)n_blocks * PC_NSUM);
    T.ctrl.push_back(S.C);
}

void prepare(State& S, const Problem& p, int max_blocks)
{
    S.p = &p;
    S.list.assign(max_blocks, {});
    S.b1.assign(4 * (size_t)(p.n > 0 ? p.n : 1), 0.0); S.b2 = S.b1;
    S.js.assign(2 * (size_t)(p.n > 0 ? p.n : 1), 0.0);
    S.part.assign((size_t)max_blocks * PC_NSUM, -7.0);       // (stale rows of an earlier launch: must never be read)
    memset(&S.C, 0xab, sizeof(S.C));                        // (a stale control block: iteration 0 must replace all of it)
}

void conclude(State& S, Trace& T)
{
    const Problem& p = *S.p;
    T.x.assign(p.x0, p.x0 + 4 * p.n);
    if (S.started) {
        const double* xf = S.buf(S.C.failed ? 0 : S.C.cur);        // pc_writeback_tracks
        T.x.assign(xf, xf + 4 * p.n);
    }
    for (size_t b = 0; b < S.list.size(); ++b) {
        T.lists.push_back((int)S.list[b].size());
        T.lists.insert(T.lists.end(), S.list[b].begin(), S.list[b].end());
    }
}

// pc_blocks of psfm_solver.hip, restated
int single_blocks(long n, int limit)
{
    int nb = (int)((n + PC_BLOCK - 1) / PC_BLOCK);
    if (nb > limit) nb = limit;
    return nb < 1 ? 1 : nb;
}

// the problem alone: psfm_solve_batch's chain (a solve without rows is not run at all)
void run_single(const Problem& p, int max_blocks, int max_launches, Trace& T)
{
    State S;
    prepare(S, p, max_blocks);
    if (p.n > 0) {
        const int nb = single_blocks(p.n, p.limit);
        S.started = true;
        for (int blk = 0; blk < nb; ++blk) block_init(S, blk, nb, (int)p.n);
        finish_launch(S, nb, 1, T);
        for (int l = 0; l < max_launches && !S.C.done; ++l) {
            for (int blk = 0; blk < nb; ++blk) block_iter(S, blk);
            finish_launch(S, nb, 0, T);
        }
    }
    conclude(S, T);
}
}  // namespace

// Runs the table both ways and compares.  Returns 0 when everything is byte-equal, else 1000 * (problem + 1) + what differed
// (1 lists, 2 block sums, 3 control blocks, 4 iterates), or -1 when a solve did not end within max_launches.
// k: the step; counted[b]: what the scan left for problem b (bounded by cap[b] through pc_multi_rows).
// x_out: the multi form's final iterates, problems one behind the other (4 * rows each); stats: 4 ints per problem (iterations,
// termination, launches that worked, launches offered).
extern "C" int pc_host_multi_compare(int n_problems, const long* counted, const int* cap, const int* limit, const int* n_flows, int banded,
                                     int k, const double* const* x0, const double* const* ref1, const double* const* ref2,
                                     const double* const* scale, const float* const* flow, const int* H, const int* W, int max_launches,
                                     double* x_out, int* stats)
{
    const int grid_x = pc_multi_grid_x(cap, limit, n_problems);
    std::vector<Problem> P(n_problems);
    std::vector<State> S(n_problems);
    std::vector<Trace> multi(n_problems), single(n_problems);
    for (int b = 0; b < n_problems; ++b) {
        const int n = pc_multi_active(k, n_flows[b]) ? pc_multi_rows(k, n_flows[b], (int)counted[b], cap[b]) : 0;
        P[b] = Problem{n, x0[b], ref1[b], ref2[b], scale[b], flow[b], H[b], W[b], limit[b], banded, n_flows[b]};
    }
    for (int b = 0; b < n_problems; ++b) prepare(S[b], P[b], grid_x);
    // ---- multi: launches over the grid (x, y); the rules of psfm_solver_multi.h per block ----
    int extra = 0;
    for (int launch = 0; launch <= max_launches; ++launch) {
        bool undone = false;
        for (int y = 0; y < n_problems; ++y) {
            State& s = S[y];
            const int n = (int)P[y].n;
            multi[y].launches_seen += 1;
            int worked = 0, nb = 0;
            for (int x = 0; x < grid_x; ++x) {
                if (!pc_multi_block_works(x, n, P[y].limit)) continue;
                nb = pc_multi_blocks(n, P[y].limit);
                if (launch == 0) { s.started = true; block_init(s, x, nb, n); }
                else {
                    if (s.C.done) continue;                          // (psfm_pc_multi_iter_kernel: a done problem costs a few loads)
                    block_iter(s, x);
                }
                ++worked;
            }
            if (worked) {
                if (worked != nb) return -2;                         // every block of the effective count works, no other
                finish_launch(s, nb, launch == 0, multi[y]);
            }
            if (s.started && !s.C.done) undone = true;
        }
        if (!undone && ++extra > 3) break;                           // (three launches behind everybody's end: they change nothing)
        if (launch == max_launches && undone) return -1;
    }
    long off = 0;
    for (int b = 0; b < n_problems; ++b) {
        conclude(S[b], multi[b]);
        run_single(P[b], grid_x, max_launches, single[b]);
        const Trace &m = multi[b], &s = single[b];
        if (m.lists != s.lists) return 1000 * (b + 1) + 1;
        if (m.rows.size() != s.rows.size() || (m.rows.size() && memcmp(m.rows.data(), s.rows.data(), m.rows.size() * sizeof(double)))) return 1000 * (b + 1) + 2;
        if (m.ctrl.size() != s.ctrl.size() || (m.ctrl.size() && memcmp(m.ctrl.data(), s.ctrl.data(), m.ctrl.size() * sizeof(PsfmSolveCtrl)))) return 1000 * (b + 1) + 3;
        if (m.x.size() != s.x.size() || (m.x.size() && memcmp(m.x.data(), s.x.data(), m.x.size() * sizeof(double)))) return 1000 * (b + 1) + 4;
        for (size_t q = 0; q < m.x.size(); ++q) x_out[off + q] = m.x[q];
        off += (long)m.x.size();
        stats[4 * b + 0] = m.ctrl.empty() ? 0 : m.ctrl.back().iteration;
        stats[4 * b + 1] = m.ctrl.empty() ? -1 : m.ctrl.back().termination;
        stats[4 * b + 2] = (int)m.ctrl.size();
        stats[4 * b + 3] = m.launches_seen;
    }
    return 0;
}

// the index rules by themselves, for the table of the test
extern "C" int pc_host_multi_blocks(int n_rows, int limit) { return pc_multi_blocks(n_rows, limit); }
extern "C" int pc_host_multi_works(int blk, int n_rows, int limit) { return pc_multi_block_works(blk, n_rows, limit) ? 1 : 0; }
extern "C" int pc_host_multi_pitch(int cap, int limit) { return pc_multi_list_pitch(cap, limit); }
extern "C" int pc_host_multi_map(int k, int n_flows, int back) { return pc_multi_map(k, n_flows, back); }
extern "C" int pc_host_multi_active(int k, int n_flows) { return pc_multi_active(k, n_flows) ? 1 : 0; }
// the first chunk of block b's list
extern "C" int pc_host_first_chunk(int b, int n_blocks, int n, int banded)
{
    const PcListPlan plan = pc_list_plan(b, n_blocks, n, banded);
    return plan.band0 + plan.first;
}
// the longest list any block of the plan gets for n rows under `limit` (what the pitch must hold)
extern "C" int pc_host_longest_list(int n, int limit, int banded)
{
    const int nb = pc_multi_blocks(n, limit);
    int longest = 0;
    for (int b = 0; b < nb; ++b) {
        const PcListPlan plan = pc_list_plan(b, nb, n, banded);
        int cnt = 0;
        for (int q = plan.first; pc_list_chunk_ok(plan, q); q += plan.step)
            for (int t = 0; t < PC_BLOCK; ++t) cnt += (plan.band0 + q) * PC_BLOCK + t < n ? 1 : 0;
        if (cnt > longest) longest = cnt;
    }
    return longest;
}
