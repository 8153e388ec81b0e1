// HOST driver of particle-sfm_amd/csrc/psfm_database.h for tests/test_database_host.py: the per-element rules of the kernels of
// psfm_database.hip (import_feature_matches.py:76-104, colmap_utils/database.py:181-225) compiled through tests/host/shim, with plain
// loops where the kernels have threads.  Built with -ffp-contract=off.  Test infrastructure.
#include "psfm_database.h"

extern "C" void psfm_host_db_keypoints(const double* v, long n, float* out)
{
    for (long i = 0; i < n; i++) out[i] = psfm_db_keypoint(v[i]);
}

// keep[p] for every directed pair of the ascending pair_key
extern "C" void psfm_host_db_keep(const int64_t* pair_key, long n_pairs, long n_img, const int32_t* pos, uint8_t* keep)
{
    for (long p = 0; p < n_pairs; p++) keep[p] = psfm_db_keep(pair_key, n_pairs, n_img, pos, pair_key[p]) ? 1 : 0;
}

// row i = [rows_in[2i], rows_in[2i+1]] of a pair between images with ids (id_s[i], id_t[i])
extern "C" void psfm_host_db_rows(const int32_t* id_s, const int32_t* id_t, const int32_t* rows_in, long n, int64_t* pair_id, uint32_t* rows_out)
{
    for (long i = 0; i < n; i++) {
        pair_id[i] = psfm_db_pair_id(id_s[i], id_t[i]);
        const PsfmDbRow r = psfm_db_row(rows_in[2 * i], rows_in[2 * i + 1], psfm_db_swap(id_s[i], id_t[i]));
        rows_out[2 * i] = r.a;
        rows_out[2 * i + 1] = r.b;
    }
}
