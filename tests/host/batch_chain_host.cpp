// Host build of the FRAME-MODE multi-problem launch chain's index rules (particle-sfm_amd/csrc/psfm_batch_chain.h) for
// tests/test_batch_chain_host.py, beside the single chain's list plan (psfm_pc_resident.h).
//
// One "launch" is a loop over the blocks of a grid (grid_x, sequences); what a block does that the rules decide -- does it work at
// all, with which block count, on which lanes, which chunks go into its list and which lanes of them take part -- is written once
// (block_list) and called two ways: `single`, the sequence alone with gridDim.x = pc_blocks of its context (restated below, resident
// budget applied), and `multi`, the table under one grid with the rules of psfm_batch_chain.h.  Lists, the set of blocks that worked
// and the count the last-block ticket waits for are compared.  The per-track arithmetic, the tree of the block sums and the control
// step are the single chain's functions on both sides and are held byte for byte by tests/host/solver_multi_host.cpp.
//
// With -DBATCH_CHAIN_MAIN this file is a stand-alone program (its own main) that runs a table through every rule: what the suite
// builds with -fsanitize=address,undefined and runs on the CPU.  Test infrastructure (g++ -O2).
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>

#include "psfm_pc_resident.h"
#include "psfm_batch_chain.h"

namespace {
// What the single chain's grid must be for a lane table of `cap` lanes, the context's resident budget applied, written out
// independently: pc_blocks of psfm_solver.hip picks the limit (PC_CHAIN_BLOCKS or the smaller budget) and calls pc_frame_blocks,
// the rule under test, for the clamp
int single_blocks(long long cap, int chain_blocks, int budget)
{
    int limit = chain_blocks;
    if (budget > 0 && budget < limit) limit = budget;
    long long nb = (cap + PC_BLOCK - 1) / PC_BLOCK;
    if (nb > limit) nb = limit;
    return nb < 1 ? 1 : (int)nb;
}
int effective_limit(int chain_blocks, int budget) { return (budget > 0 && budget < chain_blocks) ? budget : chain_blocks; }

// the members of PcParams that move with the frame, with the element types of the device's (double2 / float2 / u8): what
// pc_frame_rebase -- the function pc_params_rebase (psfm_pc_params.h) applies to PcParams -- is run over here
struct D2 { double x, y; };
struct F2 { float x, y; };
struct MockParams { const D2* p0; D2* x1a; D2* x2a; const F2 *flow12, *flow01, *flow02; const uint8_t* occ02; int frame, max_birth; int other; };

// pc_build_list of block `blk` among n_blocks over n lanes: the chunks of the plan, the lanes of them that take part
// (pc_participates: 0 <= birth frame <= max_birth)
void block_list(int blk, int n_blocks, int n, int banded, const int* birth, int max_birth, std::vector<int>& lst)
{
    lst.clear();
    const PcListPlan plan = pc_list_plan(blk, n_blocks, n, banded);
    for (int q = plan.first; pc_list_chunk_ok(plan, q); q += plan.step)
        for (int t = 0; t < PC_BLOCK; ++t) {
            const int i = (plan.band0 + q) * PC_BLOCK + t;
            if (i < n && birth[i] >= 0 && birth[i] <= max_birth) lst.push_back(i);
        }
}
}  // namespace

extern "C" int bc_blocks(long long cap, int limit) { return pc_frame_blocks(cap, limit); }
extern "C" int bc_single_blocks(long long cap, int chain_blocks, int budget) { return single_blocks(cap, chain_blocks, budget); }
extern "C" int bc_active(int f, int n_flows) { return pc_frame_active(f, n_flows) ? 1 : 0; }
extern "C" int bc_works(int blk, int n_blocks) { return pc_frame_block_works(blk, n_blocks) ? 1 : 0; }
extern "C" int bc_grid_x(const int* n_blocks, int n) { return pc_frame_grid_x(n_blocks, n); }
extern "C" int bc_rows(int lanes, int cap) { return pc_frame_rows(lanes, cap); }
extern "C" int bc_pitch(long long cap, int n_blocks) { return pc_frame_list_pitch(cap, n_blocks); }

// the longest list any block of a chain of n_blocks gets for n lanes that all take part (what the pitch must hold)
extern "C" int bc_longest_list(int n, int n_blocks, int banded)
{
    std::vector<int> birth((size_t)(n > 0 ? n : 1), 0), lst;
    int longest = 0;
    for (int b = 0; b < n_blocks; ++b) {
        block_list(b, n_blocks, n, banded, birth.data(), 0, lst);
        if ((int)lst.size() > longest) longest = (int)lst.size();
    }
    return longest;
}

// the rebase of a row that holds the arguments of frame 1 to frame f (pc_frame_rebase, the rule behind pc_params_rebase) on a
// sequence of n_flows flows, `cap` lanes and `pix` pixels per map, against what the frame's solve must read, worked out here from
// the frame alone; rebasing twice (1 -> g -> f) must land where 1 -> f lands.  0: all as expected; else what differed.
extern "C" int bc_rebase_check(int n_flows, long long cap, long long pix, int f)
{
    std::vector<D2> log((size_t)(n_flows + 1) * (size_t)cap);
    std::vector<F2> flows((size_t)n_flows * (size_t)pix), flows2((size_t)(n_flows > 1 ? n_flows - 1 : 1) * (size_t)pix);
    std::vector<uint8_t> occ2((size_t)(n_flows > 1 ? n_flows - 1 : 1) * (size_t)pix);
    MockParams row;
    memset(&row, 0, sizeof(row));
    // pc_frame_params at frame 1 (pc_seq_args): slabs 0, 1, 2; flow01 = map 0, flow12 = map 1, flow02 / occ02 = stride-2 map 0
    row.p0 = log.data(); row.x1a = log.data() + cap; row.x2a = log.data() + 2 * cap;
    row.flow01 = flows.data(); row.flow12 = flows.data() + pix; row.flow02 = flows2.data(); row.occ02 = occ2.data();
    row.frame = 1; row.max_birth = 0; row.other = 77;
    MockParams a = row, b = row;
    pc_frame_rebase(a, cap, pix, pix, f > 1 ? f - 1 : 1);
    pc_frame_rebase(a, cap, pix, pix, f);
    pc_frame_rebase(b, cap, pix, pix, f);
    if (memcmp(&a, &b, sizeof(a)) != 0) return 1;
    if (b.other != 77) return 2;
    if (!pc_frame_active(f, n_flows)) return 0;
    // what the frame's solve reads lies inside the sequence's own stacks: slabs f - 1, f, f + 1; maps f - 1, f; stride-2 map f - 1
    if (b.p0 != log.data() + (int64_t)(f - 1) * cap || b.x2a != log.data() + (int64_t)(f + 1) * cap || b.x1a != log.data() + (int64_t)f * cap) return 3;
    if (b.flow01 != flows.data() + (int64_t)(f - 1) * pix || b.flow12 != flows.data() + (int64_t)f * pix) return 4;
    if (b.flow02 != flows2.data() + (int64_t)(f - 1) * pix || b.occ02 != occ2.data() + (int64_t)(f - 1) * pix) return 5;
    if (b.frame != f || b.max_birth != f - 1) return 6;
    return 0;
}

// A table of sequences in frame f, both ways.  lanes[b]: lanes in use; cap[b]: lanes the tables hold; chain_blocks / budget[b]: what
// pc_blocks reads; birth[b]: birth frame per lane (-1 free).  worked[b]: blocks that worked in the multi form.  Returns 0 when the
// two forms agree on everything, else 1000 * (b + 1) + what differed (1 a sequence took part that must not / did not that must,
// 2 the block set, 3 a list, 4 a list longer than the pitch, 5 the ticket count).
extern "C" int bc_table_compare(int n_problems, const int* lanes, const int* cap, int chain_blocks, const int* budget, const int* n_flows,
                                const int* const* birth, int f, int banded, int* worked)
{
    std::vector<int> nb((size_t)n_problems);
    for (int b = 0; b < n_problems; ++b) nb[(size_t)b] = pc_frame_blocks(cap[b], effective_limit(chain_blocks, budget[b]));
    const int grid_x = pc_frame_grid_x(nb.data(), n_problems);
    std::vector<int> lm, ls;
    for (int y = 0; y < n_problems; ++y) {
        const bool solve_alone = f >= 1 && f < n_flows[y];       // track_optimize.py:49-50 on this sequence alone
        const int nb_single = single_blocks(cap[y], chain_blocks, budget[y]);
        const int n_single = lanes[y] < cap[y] ? lanes[y] : cap[y];
        const int pitch = pc_frame_list_pitch(cap[y], nb[(size_t)y]);
        worked[y] = 0;
        for (int x = 0; x < grid_x; ++x) {
            const bool works = pc_frame_active(f, n_flows[y]) && pc_frame_block_works(x, nb[(size_t)y]);
            if (works != (solve_alone && x < nb_single)) return 1000 * (y + 1) + (pc_frame_active(f, n_flows[y]) != solve_alone ? 1 : 2);
            if (!works) continue;
            ++worked[y];
            const int n = pc_frame_rows(lanes[y], cap[y]);
            block_list(x, nb[(size_t)y], n, banded, birth[y], f - 1, lm);
            block_list(x, nb_single, n_single, banded, birth[y], f - 1, ls);
            if (lm != ls) return 1000 * (y + 1) + 3;
            if ((int)lm.size() > pitch) return 1000 * (y + 1) + 4;
        }
        // the last-block ticket of the sequence waits for nb arrivals: every block of the single grid, no other
        if (worked[y] != (solve_alone ? nb_single : 0)) return 1000 * (y + 1) + 5;
    }
    return 0;
}

#ifdef BATCH_CHAIN_MAIN
// stand-alone: a table of sequences of different lane counts, capacities, budgets and lengths through every rule, frame by frame
int main()
{
    const int B = 7;
    const int cap[B] = {1, 255, 257, 700, 2049, 16400, 40000};
    const int lanes[B] = {1, 200, 300, 700, 2100, 9000, 40000};       // (2100 > 2049: more lanes than the tables hold)
    const int budget[B] = {0, 0, 1, 2, 8, 0, 16};
    const int n_flows[B] = {1, 2, 3, 5, 9, 4, 2};
    std::vector<std::vector<int>> birth((size_t)B);
    const int* bp[B];
    unsigned s = 12345u;
    for (int b = 0; b < B; ++b) {
        birth[(size_t)b].resize((size_t)cap[b]);
        for (int i = 0; i < cap[b]; ++i) { s = s * 1664525u + 1013904223u; birth[(size_t)b][(size_t)i] = (int)((s >> 16) % 11u) - 2; }      // -2 .. 8
        bp[b] = birth[(size_t)b].data();
    }
    int worked[B];
    for (int banded = 0; banded < 2; ++banded)
        for (int f = -1; f <= 10; ++f) {
            const int rc = bc_table_compare(B, lanes, cap, 512, budget, n_flows, bp, f, banded, worked);
            if (rc) { fprintf(stderr, "table: frame %d banded %d -> %d\n", f, banded, rc); return 1; }
            for (int b = 0; b < B; ++b)
                if ((worked[b] > 0) != (f >= 1 && f < n_flows[b])) { fprintf(stderr, "participation: frame %d sequence %d\n", f, b); return 1; }
        }
    for (int b = 0; b < B; ++b) {
        const int fs[3] = {1, 2, n_flows[b] - 1};
        for (int f : fs)
            if (f >= 1 && f < n_flows[b] && bc_rebase_check(n_flows[b], cap[b], 35, f)) { fprintf(stderr, "rebase: sequence %d frame %d\n", b, f); return 1; }
        const int nb = bc_blocks(cap[b], effective_limit(512, budget[b]));
        if (nb != bc_single_blocks(cap[b], 512, budget[b])) { fprintf(stderr, "blocks: sequence %d\n", b); return 1; }
        for (int n = 1; n <= cap[b]; n += (cap[b] > 3000 ? 257 : 1))
            if (bc_longest_list(n, nb, 1) > bc_pitch(cap[b], nb) || bc_longest_list(n, nb, 0) > bc_pitch(cap[b], nb)) {
                fprintf(stderr, "pitch: sequence %d at %d lanes\n", b, n);
                return 1;
            }
    }
    printf("batch_chain_host: ok\n");
    return 0;
}
#endif
