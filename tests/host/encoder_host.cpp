// HOST driver of particle-sfm_amd/csrc/psfm_encoder.h for tests/test_encoder_host.py: the arithmetic of psfm_traj_encode_kernel
// (the classifier's trajectory transformer, traj_oa_depth.py:25-60) compiled through tests/host/shim, with plain loops over
// trajectories, phases and tokens where the kernel has waves, barriers and lanes, and two row buffers where the kernel has LDS.
// Built with -ffp-contract=off: fmaf is the correctly rounded fused operation.  Test infrastructure.
#include "psfm_encoder.h"

extern "C" int psfm_host_encoder_weight_count(void) { return PSFM_ENC_WEIGHTS; }

extern "C" void psfm_host_traj_encode(const float* features, const double* mask_absent, const float* weights, long k, int n_frames, float* out)
{
    const int L = n_frames;
    static PsfmEncTok tok[PSFM_ENC_MAX_L];
    static float rows[PSFM_ENC_MAX_L * PSFM_ENC_ROW];
    for (long t = 0; t < k; t++) {
        uint64_t pad = 0;
        for (int l = 0; l < L; l++) pad |= (uint64_t)psfm_enc_padded(mask_absent, (int)(t * L + l)) << l;
        for (int p = 0; p < PSFM_ENC_PHASES; p++) {
            for (int l = 0; l < L; l++) {
                float f[PSFM_ENC_IN];
                for (int c = 0; c < PSFM_ENC_IN; c++) f[c] = features[(int64_t)c * k * L + t * L + l];
                psfm_enc_phase(p, tok[l], weights, f, rows, L, pad);
            }
            for (int l = 0; l < L; l++)
                for (int i = 0; i < 2 * PSFM_ENC_D; i++) rows[l * PSFM_ENC_ROW + i] = tok[l].pub[i];
        }
        for (int c = 0; c < PSFM_ENC_D; c++) out[(int64_t)c * k + t] = psfm_enc_max(rows, L, c);
    }
}

// The same through the kernel's own lane mapping (psfm_enc_lane, psfm_enc_pad_bits): blocks of `waves` waves emulated thread by
// thread, a loop over the threads where the kernel has a barrier, the ballot formed per wave.  Every row index is checked against the
// wave's 64 rows of the slab.  Returns the number of violations (0).
extern "C" long psfm_host_traj_encode_blocks(const float* features, const double* mask_absent, const float* weights, long k, int n_frames,
                                             int waves, float* out)
{
    const int L = n_frames, per_wave = 64 / L, threads = 64 * waves;
    const long per_block = (long)waves * per_wave, blocks = (k + per_block - 1) / per_block;
    PsfmEncTok* tok = new PsfmEncTok[threads]();
    PsfmEncLane* lane = new PsfmEncLane[threads];
    uint64_t* pad = new uint64_t[threads];
    float* slab = new float[(size_t)threads * PSFM_ENC_ROW];
    long bad = 0;
    for (long b = 0; b < blocks; b++) {
        for (int i = 0; i < threads * PSFM_ENC_ROW; i++) slab[i] = NAN;              // (LDS starts out undefined)
        for (int t = 0; t < threads; t++) {
            lane[t] = psfm_enc_lane(t, b, waves, L, per_wave, k);
            const int w0 = (t >> 6) * 64;
            bad += lane[t].my_row < w0 || lane[t].my_row >= w0 + 64 || lane[t].row0 < w0 || lane[t].row0 + L > w0 + 64;
            bad += lane[t].traj < 0 || lane[t].traj >= k || lane[t].tok < 0 || lane[t].tok >= L;
            if (lane[t].active) bad += lane[t].my_row != lane[t].row0 + lane[t].tok;
        }
        for (int w = 0; w < waves; w++) {
            uint64_t ballot = 0;
            for (int l = 0; l < 64; l++) {
                const PsfmEncLane& m = lane[w * 64 + l];
                ballot |= (uint64_t)(m.active && psfm_enc_padded(mask_absent, m.traj * L + m.tok)) << l;
            }
            for (int l = 0; l < 64; l++) pad[w * 64 + l] = psfm_enc_pad_bits(ballot, lane[w * 64 + l], L);
        }
        for (int p = 0; p < PSFM_ENC_PHASES; p++) {
            for (int t = 0; t < threads; t++) {
                const PsfmEncLane& m = lane[t];
                float f[PSFM_ENC_IN];
                for (int c = 0; c < PSFM_ENC_IN; c++) f[c] = features[(int64_t)c * k * L + m.traj * L + m.tok];
                psfm_enc_phase(p, tok[t], weights, f, slab + m.row0 * PSFM_ENC_ROW, L, pad[t]);
            }
            for (int t = 0; t < threads; t++)
                if (lane[t].active)
                    for (int i = 0; i < 2 * PSFM_ENC_D; i++) slab[lane[t].my_row * PSFM_ENC_ROW + i] = tok[t].pub[i];
        }
        for (int t = 0; t < threads; t++)
            if (lane[t].active)
                for (int c = lane[t].tok; c < PSFM_ENC_D; c += L)
                    out[(int64_t)c * k + lane[t].traj] = psfm_enc_max(slab + lane[t].row0 * PSFM_ENC_ROW, L, c);
    }
    delete[] tok; delete[] lane; delete[] pad; delete[] slab;
    return bad;
}

