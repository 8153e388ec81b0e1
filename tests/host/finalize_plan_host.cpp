// Host build of the finalize's decisions and key codec (particle-sfm_amd/csrc/psfm_finalize_plan.h through tests/host/shim) for
// tests/test_finalize_plan_host.py: the form plan as a row of integers, the shard accounting, and sweeps over (last, birth, idx) that
// run every key through the codec the kernels use -- pack (psfm_key, psfm_chain.h) -> psfm_put_key -> psfm_key_fields /
// psfm_key_group -- and report the first input that does not come back.  Test infrastructure.
#include "psfm_chain.h"
#include "psfm_finalize_plan.h"

// out: use32, ok, seq_bits, seq_shift, end_bit, sort_form, passes, first_half, ng, offsets_form
extern "C" void psfm_host_fin_form(int shift_b, int shift_d, int n_flows, int n_seq, long long n, int sort_switch, int plan_switch,
                                   int plan_allowed, long long* out)
{
    const PsfmFinForm f = psfm_fin_form(shift_b, shift_d, n_flows, n_seq, (int64_t)n, sort_switch, plan_switch, plan_allowed);
    const long long v[10] = {f.fmt.use32, f.ok, f.seq_bits, f.seq_shift, (long long)f.end_bit, f.sort_form, f.passes, f.first_half, f.ng,
                             f.offsets_form};
    for (int i = 0; i < 10; ++i) out[i] = v[i];
}

extern "C" int psfm_host_shard_offsets(const int* fin_cnt, int shard_cap, int* count, long long* start, long long* n)
{
    PsfmShardOffsets so;
    int64_t total = 0;
    const bool over = psfm_shard_offsets(fin_cnt, shard_cap, &so, &total);
    for (int k = 0; k < PSFM_NSHARD; ++k) { count[k] = so.count[k]; start[k] = (long long)so.start[k]; }
    *n = (long long)total;
    return over ? 1 : 0;
}
extern "C" int psfm_host_nshard() { return PSFM_NSHARD; }

// one key through the codec in both formats; the expected 32-bit key is formed here in 64-bit arithmetic
static bool codec_ok(int last, int birth, int idx, const PsfmKeyFmt& f32)
{
    PsfmKeyFmt f64 = f32;
    f64.use32 = 0;
    const unsigned long long k = psfm_key(last, birth, idx, f32.shift_b, f32.shift_d);
    const unsigned long long tri = (unsigned long long)last * (unsigned long long)(last + 1) / 2ull + (unsigned long long)birth;
    const unsigned long long want32 = (tri << f32.shift_b) | (unsigned long long)idx;
    if (want32 >> 32) return false;                       // (the caller asked for a key the 32-bit format cannot carry)
    unsigned long long slot[2] = {~0ull, ~0ull};          // entry 1 of 4-byte and of 8-byte entries
    unsigned long long slot64[2] = {~0ull, ~0ull};
    psfm_put_key(slot, 1, k, f32);
    psfm_put_key(slot64, 1, k, f64);
    if (psfm_key32(k, f32) != (unsigned)want32 || psfm_key_at(slot, 1, 1) != want32 || psfm_key_at(slot64, 1, 0) != k) return false;
    int l = -1, b = -1, i = -1;
    psfm_key_fields(slot, 1, 1, f32.shift_b, f32.shift_d, &l, &b, &i);
    if (l != last || b != birth || i != idx) return false;
    l = b = i = -1;
    psfm_key_fields(slot64, 1, 0, f32.shift_b, f32.shift_d, &l, &b, &i);
    if (l != last || b != birth || i != idx) return false;
    if (psfm_key_idx(psfm_key_at(slot, 1, 1), f32.shift_b) != idx || psfm_key_idx(psfm_key_at(slot64, 1, 0), f32.shift_b) != idx) return false;
    const int g32 = psfm_key_group(slot, 1, 1, f32.shift_b, f32.shift_d), g64 = psfm_key_group(slot64, 1, 0, f32.shift_b, f32.shift_d);
    return g32 == g64 && (unsigned long long)g32 == tri;
}

// every last <= lmax with every birth <= last (edges_only: birth in {0, 1, last - 1, last}) and idx in {0, 1, all ones, 0101..}.
// Returns the number of keys that did not come back; bad[0..2] = the first of them.  *n_keys = keys tried.
extern "C" long long psfm_host_codec_sweep(int lmax, int shift_b, int shift_d, int edges_only, int* bad, long long* n_keys)
{
    PsfmKeyFmt f;
    f.shift_b = shift_b; f.shift_d = shift_d; f.use32 = 1;
    const int ones = (int)((1u << shift_b) - 1u);
    const int idxs[4] = {0, 1 & ones, ones, 0x55555555 & ones};
    long long fails = 0, tried = 0;
    for (int last = 0; last <= lmax; ++last) {
        const int edge[4] = {0, last < 1 ? last : 1, last > 0 ? last - 1 : 0, last};
        const int nb = edges_only ? 4 : last + 1;
        for (int q = 0; q < nb; ++q) {
            const int birth = edges_only ? edge[q] : q;
            for (int u = 0; u < 4; ++u) {
                ++tried;
                if (!codec_ok(last, birth, idxs[u], f) && fails++ == 0) { bad[0] = last; bad[1] = birth; bad[2] = idxs[u]; }
            }
        }
    }
    *n_keys = tried;
    return fails;
}

extern "C" void psfm_host_tri_invert(unsigned tri, int* last, int* birth) { psfm_tri_invert(tri, last, birth); }

// record k of sequence seq -> a combined batch key (psfm_put_key) -> read back (psfm_key_at) and split: *seq_out, returns the key
extern "C" unsigned long long psfm_host_batch_roundtrip(unsigned long long k, int shift_b, int shift_d, int use32, int seq, int seq_shift,
                                                        unsigned long long* stored, int* seq_out)
{
    PsfmKeyFmt f;
    f.shift_b = shift_b; f.shift_d = shift_d; f.use32 = use32;
    unsigned long long slot[2] = {0ull, 0ull};
    psfm_put_key(slot, 1, k, f, seq, seq_shift);
    *stored = psfm_key_at(slot, 1, use32);
    return psfm_batch_split(*stored, use32, seq_shift, seq_out);
}
extern "C" unsigned psfm_host_key32(unsigned long long k, int shift_b, int shift_d)
{
    PsfmKeyFmt f;
    f.shift_b = shift_b; f.shift_d = shift_d; f.use32 = 1;
    return psfm_key32(k, f);
}
