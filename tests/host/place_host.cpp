// Host build of the placed finalize's decision and index arithmetic (particle-sfm_amd/csrc/psfm_place.h through tests/host/shim) for
// tests/test_place_host.py: the decision as one integer, and a run of scan + placement + one stable pass over records the test hands
// in, with every index formed by the header's functions -- the ones psfm_place.hip's kernels call.  Test infrastructure.
#include <algorithm>
#include <vector>

#include "psfm_chain.h"
#include "psfm_place.h"

extern "C" int psfm_host_place_form(int persist_ran, int shift_b, int shift_d, int n_flows, long long n, long long cap, int sort_switch,
                                    int place_switch)
{
    const PsfmFinForm f = psfm_fin_form(shift_b, shift_d, n_flows, 1, (int64_t)n, sort_switch, 1, 1);
    return psfm_place_form(persist_ran, f, n_flows, (int64_t)n, (int64_t)cap, place_switch);
}
extern "C" int psfm_host_place_blocks(long long G) { return psfm_place_blocks((int64_t)G); }
extern "C" long long psfm_host_place_table_words(int n_flows, long long G) { return (long long)psfm_place_table_words(n_flows, (int64_t)G); }
extern "C" int psfm_host_place_count(const unsigned long long* bmask, long long G, int n_flows, int b, int vb)
{
    return psfm_place_count(bmask, (int64_t)G, n_flows, b, vb);
}

// n records (last, birth, idx) on log columns lane[i]; bmask: the birth masks as the loop leaves them ((n_flows + 1) rows of
// psfm_place_words(G) words, rows 0 and n_flows never looked at: the caller poisons them).  Packs the 64-bit records, runs scan ->
// placement -> a stable sort on the pass's digit, and returns the sorted 32-bit keys' fields and the lanes the pass leaves.
// Returns 0, or a negative code when a record is not in the masks, a position falls outside [0, n) or is taken twice (the placement is
// no permutation).
extern "C" int psfm_host_place_run(const int* last, const int* birth, const int* idx, const int* lane, long long n,
                                   const unsigned long long* bmask, long long G, int n_flows, int shift_b, int shift_d, int* out_last,
                                   int* out_birth, int* out_idx, int* out_lane)
{
    const int gb = psfm_place_blocks((int64_t)G), gw = psfm_place_words((int64_t)G);
    PsfmKeyFmt fmt;
    fmt.shift_b = shift_b; fmt.shift_d = shift_d; fmt.use32 = 1;
    std::vector<int> start((size_t)(n_flows + 1) * gb, -(1 << 30)), total((size_t)n_flows, 0);
    psfm_place_scan_rows(bmask, (int64_t)G, n_flows, start.data(), total.data());
    std::vector<long long> base((size_t)n_flows, 0);
    for (int b = 1; b < n_flows; ++b) base[b] = base[b - 1] + total[b - 1];
    std::vector<unsigned> keys((size_t)n, 0u);
    std::vector<int> vals((size_t)n, -1);
    std::vector<char> taken((size_t)n, 0);
    for (long long i = 0; i < n; ++i) {
        const unsigned long long k = psfm_key(last[i], birth[i], idx[i], shift_b, shift_d);
        int l, b, gi;
        psfm_key64_fields(k, shift_b, shift_d, &l, &b, &gi);
        if (b >= n_flows || gi >= G || l >= PSFM_PLACE_MAX_TIMES) return -3;
        int64_t pos = gi;
        if (b > 0) {
            const unsigned long long* w = bmask + (int64_t)b * gw + (int64_t)PSFM_PLACE_VB_WORDS * (gi / PSFM_PLACE_VB);
            if (!psfm_place_born(w, gi)) return -4;
            pos = psfm_place_pos(base[b], start[(size_t)b * gb + gi / PSFM_PLACE_VB], psfm_place_ordinal(w, gi));
        }
        if (pos < 0 || pos >= n) return -1;
        if (taken[pos]) return -2;
        taken[pos] = 1;
        keys[pos] = psfm_key32(k, fmt);
        vals[pos] = psfm_place_pack(lane[i], l);
    }
    std::vector<long long> order((size_t)n);
    for (long long i = 0; i < n; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](long long a, long long b) { return psfm_place_digit(vals[a]) < psfm_place_digit(vals[b]); });
    for (long long i = 0; i < n; ++i) {
        psfm_key32_fields(keys[order[i]], shift_b, &out_last[i], &out_birth[i], &out_idx[i]);
        out_lane[i] = psfm_place_lane(vals[order[i]]);
    }
    return 0;
}
