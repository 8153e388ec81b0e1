// HOST driver of particle-sfm_amd/csrc/psfm_window_batch.h for tests/test_window_batch_host.py: the per-element rules of
// psfm_window_sample_batch (eligibility, the splitmix64 key, the cap rule, the normalisation), the lookup a block of the flattened
// grids performs and the offsets of a plan, compiled through tests/host/shim.  Test infrastructure.
#include "psfm_window_batch.h"

extern "C" int psfm_host_winb_max(void) { return PSFM_WINB_MAX; }
extern "C" int psfm_host_winb_block(void) { return PSFM_WINB_BLOCK; }

extern "C" void psfm_host_winb_eligible(long n, const int* birth, const int* len, const int* f0, const int* L, const int* traj_min_len,
                                        const int* min_length, int* overlap, unsigned char* flag)
{
    for (long i = 0; i < n; i++) {
        overlap[i] = psfm_winb_overlap(birth[i], len[i], f0[i], L[i]);
        flag[i] = psfm_winb_eligible(birth[i], len[i], f0[i], L[i], traj_min_len[i], min_length[i]) ? 1 : 0;
    }
}

extern "C" void psfm_host_winb_hash(long n, const unsigned long long* seed, const int* id, unsigned long long* key)
{
    for (long i = 0; i < n; i++) key[i] = psfm_winb_hash(seed[i], id[i]);
}

extern "C" long psfm_host_winb_rows(long count, long max_num) { return (long)psfm_winb_rows(count, max_num); }

extern "C" double psfm_host_winb_normalise(double v, double ratio, double target) { return psfm_winb_normalise(v, ratio, target); }

// k[0 .. n_win) -> row0[65], blk0[64]; returns the blocks of all windows
extern "C" long psfm_host_winb_offsets(const long* k, int n_win, long units_per_row, long per_block, long* row0, long* blk0)
{
    static PsfmWinbOffsets O;
    int64_t kk[PSFM_WINB_MAX] = {0};
    for (int b = 0; b < n_win && b < PSFM_WINB_MAX; b++) kk[b] = k[b];
    psfm_winb_offsets(O, kk, n_win, units_per_row, per_block);
    for (int b = 0; b <= PSFM_WINB_MAX; b++) row0[b] = (long)O.row0[b];
    for (int b = 0; b < PSFM_WINB_MAX; b++) blk0[b] = O.blk0[b];
    return (long)O.blocks;
}

// the lookup of a block: first[64] as the offsets wrote it
extern "C" int psfm_host_winb_find(const long* first, int blk)
{
    int f[PSFM_WINB_MAX];
    for (int i = 0; i < PSFM_WINB_MAX; i++) f[i] = (int)first[i];
    return psfm_winb_find(f, blk);
}
