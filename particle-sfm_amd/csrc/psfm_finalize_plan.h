// psfm_finalize_plan.h -- what the finalize (psfm_finalize.hip) DECIDES, and the one place that knows the layout of its sort keys:
// the key codec, the form plan psfm_fin_form() -- one pure function of integers that each entry point computes once -- and the shard
// accounting of the per-frame path.  No HIP runtime calls, no psfm_ctx: the CPU suite compiles this header with g++ through
// tests/host/shim (tests/host/finalize_plan_host.cpp) and pins every decision at its switching points.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#define PSFM_NSHARD 64                  // (as psfm_internal.h, which a host build cannot include: a different value there does not compile clean)
#define PSFM_PLAN_MAX_GROUPS 16384      // groups the one-block plan kernel holds in LDS
#define PSFM_SORT64_MAX_N 5000000ll     // 64-bit keys: this library's sort up to here, rocPRIM's above (profiles/EXPERIMENTS.md 20)

#define PSFM_HD __host__ __device__ __forceinline__

// ---- key codec --------------------------------------------------------------------------------------------------------------
// The frame loop writes 64-bit records  last << shift_d | birth << shift_b | idx  (psfm_key, psfm_chain.h).  birth <= last: the
// pair (last, birth) is re-coded as the triangular index  tri = last (last + 1) / 2 + birth,  which orders like the pair and needs
// ~1 bit less.  When  tri << shift_b | idx  fits 32 bits (100 frames at 1080p / r = 2: 13 + 19) the sort runs on 4-byte keys in 4
// passes instead of 8-byte keys in 5.  tri is also the number of the key's GROUP (same last and birth, hence same length).
// A batch sorts (sequence << seq_shift | key) with either key format.
struct PsfmKeyFmt { int shift_b, shift_d; int use32; };

PSFM_HD unsigned psfm_key32(unsigned long long k, const PsfmKeyFmt& f)
{
    const unsigned last = (unsigned)(k >> f.shift_d);
    const unsigned birth = (unsigned)((k >> f.shift_b) & ((1ull << (f.shift_d - f.shift_b)) - 1ull));
    const unsigned idx = (unsigned)(k & ((1ull << f.shift_b) - 1ull));
    return ((last * (last + 1u) / 2u + birth) << f.shift_b) | idx;
}
// record k of sequence `seq` -> keys[pos] in format f (entries of 4 or 8 bytes).  seq_shift == 32 beside a 32-bit key: a batch of one
// sequence whose key fills the word -- no sequence bits to write.
PSFM_HD void psfm_put_key(unsigned long long* keys, int64_t pos, unsigned long long k, const PsfmKeyFmt& f, int seq = 0, int seq_shift = 0)
{
    if (f.use32) ((unsigned*)keys)[pos] = psfm_key32(k, f) | (seq_shift < 32 ? (unsigned)seq << seq_shift : 0u);
    else keys[pos] = k | ((unsigned long long)seq << seq_shift);
}
PSFM_HD unsigned long long psfm_key_at(const void* keys, int64_t id, int use32)
{
    return use32 ? (unsigned long long)((const unsigned*)keys)[id] : ((const unsigned long long*)keys)[id];
}
// combined key of a batch -> the sequence's own key; *seq = the sequence.  (Key words narrower than seq_shift hold no sequence.)
PSFM_HD unsigned long long psfm_batch_split(unsigned long long kk, int use32, int seq_shift, int* seq)
{
    if (seq_shift >= (use32 ? 32 : 64)) { *seq = 0; return kk; }
    *seq = (int)(kk >> seq_shift);
    return kk & ((1ull << seq_shift) - 1ull);
}
// tri -> (last, birth): last = the largest l with l (l + 1) / 2 <= tri.
// Exact for every tri a 32-bit key can carry, i.e. tri <= L (L + 1) / 2 + L with L = 65534: psfm_track_dims gives shift_b >= 1 and the
// format is chosen only when tri_bits + shift_b <= 32, so tri < 2^31, L (L + 3) < 2^32, L <= 65534.  There the float estimate is off by
// less than 0.02 (two roundings of 2^-24 under a root of at most 131071), so it starts at last + 1 at the most, and the largest product
// the loops form is (last + 1) (last + 2) <= 65535 * 65536 < 2^32: none wraps.  (One step further, last = 65535, the second loop's does.)
PSFM_HD void psfm_tri_invert(unsigned tri, int* last, int* birth)
{
    int l = (int)((sqrtf(8.0f * (float)tri + 1.0f) - 1.0f) * 0.5f);
    while (l > 0 && (unsigned)l * (unsigned)(l + 1) / 2u > tri) --l;
    while ((unsigned)(l + 1) * (unsigned)(l + 2) / 2u <= tri) ++l;
    *last = l;
    *birth = (int)(tri - (unsigned)l * (unsigned)(l + 1) / 2u);
}
PSFM_HD int psfm_key_idx(unsigned long long k, int shift_b) { return (int)(k & ((1ull << shift_b) - 1ull)); }
// the fields of one key by format; of keys[id] in either format; its group
PSFM_HD void psfm_key32_fields(unsigned k, int shift_b, int* last, int* birth, int* idx)
{
    psfm_tri_invert(k >> shift_b, last, birth);
    *idx = (int)(k & ((1u << shift_b) - 1u));
}
PSFM_HD void psfm_key64_fields(unsigned long long k, int shift_b, int shift_d, int* last, int* birth, int* idx)
{
    *last = (int)(k >> shift_d);
    *birth = (int)((k >> shift_b) & ((1ull << (shift_d - shift_b)) - 1ull));
    *idx = psfm_key_idx(k, shift_b);
}
PSFM_HD void psfm_key_fields(const void* keys, int64_t id, int use32, int shift_b, int shift_d, int* last, int* birth, int* idx)
{
    if (use32) psfm_key32_fields(((const unsigned*)keys)[id], shift_b, last, birth, idx);
    else psfm_key64_fields(((const unsigned long long*)keys)[id], shift_b, shift_d, last, birth, idx);
}
PSFM_HD int psfm_key_group(const void* keys, int64_t id, int use32, int shift_b, int shift_d)
{
    if (use32) return (int)(((const unsigned*)keys)[id] >> shift_b);      // the 32-bit key carries the group number itself
    int last, birth, idx;
    psfm_key64_fields(((const unsigned long long*)keys)[id], shift_b, shift_d, &last, &birth, &idx);
    return (int)((unsigned)last * ((unsigned)last + 1u) / 2u + (unsigned)birth);
}

// ---- form plan --------------------------------------------------------------------------------------------------------------
// Which half of sort_keys / sort_lanes the compaction fills: the second (rocPRIM sorts second half -> first half), unless this
// library's own sort (psfm_sort.hip / psfm_sort64.hip) runs an even number of passes -- it ping-pongs between the halves and has to
// END in the first.  64-bit keys: the own sort up to PSFM_SORT64_MAX_N records, rocPRIM's above -- inside the finalize the own sort
// wins where the sort is bound by its launches and loses where it is bound by bandwidth (its scatter kernel holds two blocks per
// CU: 53 KB of LDS each).  Offsets: the one-block group plan while its groups fit LDS, else decode + scan over the trajectories.
struct PsfmFinForm {
    PsfmKeyFmt fmt;
    int ok;                 // 0: the batch's key does not fit 64 bits (nothing else is valid then)
    int seq_bits;           // bits of the sequence number in front of the key (0 outside a batch)
    int seq_shift;          // bits of one sequence's key = where the sequence number starts
    unsigned end_bit;       // the sort's key bits: seq_shift + seq_bits
    int sort_form;          // 1 own sort on 32-bit keys, 2 own sort on 64-bit keys, 3 rocPRIM   (psfm_ctx_get_finalize_forms)
    int passes;             // 8-bit digits in end_bit (psfm_sort_pairs32_passes / psfm_sort_pairs64_passes)
    int first_half;         // the compaction writes the first halves of sort_keys / sort_lanes
    long long ng;           // group numbers last (last + 1) / 2 + birth, birth <= last <= n_flows + 1
    int offsets_form;       // 1 group plan, 3 decode + scan
};
static inline int psfm_bits_for(long long count) { int b = 1; while ((1ll << b) < count) ++b; return b; }      // 2^b >= count, b >= 1

// shift_b, shift_d, n_flows: of the sequence (psfm_track_dims; a batch: common shifts, its longest sequence).  n_seq sequences, n records
// in all.  sort_switch: PSFM_FIN_SORT (1; 0: rocPRIM's sort always; 2: the own sort at any size).  plan_switch: PSFM_FIN_PLAN (1; 0: decode
// + scan always).  plan_allowed: 0 for the batch, whose offsets come from one scan over all sequences.
static inline PsfmFinForm psfm_fin_form(int shift_b, int shift_d, int n_flows, int n_seq, int64_t n, int sort_switch, int plan_switch,
                                        int plan_allowed)
{
    PsfmFinForm f;
    f.fmt.shift_b = shift_b; f.fmt.shift_d = shift_d;
    const long long lmax = (long long)n_flows + 1;            // last valid time <= n_flows
    f.ng = lmax * (lmax + 1) / 2 + lmax + 1;
    const int tri_bits = psfm_bits_for(f.ng);
    const int bits64 = shift_d + psfm_bits_for((long long)n_flows + 2);
    f.seq_bits = 0;
    while ((1 << f.seq_bits) < n_seq) ++f.seq_bits;
    // 32-bit triangular keys when they fit, with the sequence number beside them
    f.fmt.use32 = (tri_bits + shift_b + f.seq_bits <= 32) ? 1 : 0;
    f.seq_shift = f.fmt.use32 ? tri_bits + shift_b : bits64;
    f.end_bit = (unsigned)(f.seq_shift + f.seq_bits);
    f.ok = f.end_bit <= 64u;
    const bool own = sort_switch && n < (1ll << 31) && (f.fmt.use32 || sort_switch == 2 || n <= PSFM_SORT64_MAX_N);
    f.sort_form = own ? (f.fmt.use32 ? 1 : 2) : 3;
    f.passes = (int)((f.end_bit + 7u) / 8u);
    f.first_half = own && f.passes % 2 == 0;
    f.offsets_form = (plan_allowed && plan_switch && f.ng <= PSFM_PLAN_MAX_GROUPS && n < (1ll << 31)) ? 1 : 3;
    return f;
}

// ---- shard accounting -------------------------------------------------------------------------------------------------------
// The per-frame path leaves its records in PSFM_NSHARD slices of shard_cap entries; fin_cnt[k] counts what shard k was ASKED to hold.
struct PsfmShardOffsets { int count[PSFM_NSHARD]; int64_t start[PSFM_NSHARD]; };
// -> records kept per shard and where they start in the sort's input; *n = their sum; returns true when a shard overflowed
static inline bool psfm_shard_offsets(const int* fin_cnt, int shard_cap, PsfmShardOffsets* so, int64_t* n)
{
    bool over = false;
    *n = 0;
    for (int k = 0; k < PSFM_NSHARD; ++k) {
        if (fin_cnt[k] > shard_cap) over = true;
        so->count[k] = fin_cnt[k] > shard_cap ? shard_cap : fin_cnt[k];
        so->start[k] = *n;
        *n += so->count[k];
    }
    return over;
}
