// HOST driver of particle-sfm_amd/csrc/psfm_batch_shapes.h for tests/test_batch_shapes_host.py: the tables of the two flattened
// launches of psfm_connect_batch over sequences of different frame sizes, every block of their grids walked as the kernels walk them
// (psfm_flow_check_x2v_shapes_kernel + psfm_flow_check_x2v_body_at of psfm_track.hip, psfm_kill_map_shapes_kernel of
// psfm_motion_boundary.hip), and the batch's common key format against a sequence's own (psfm_finalize_plan.h), compiled through
// tests/host/shim.  Test infrastructure.
#include "psfm_batch_shapes.h"
#include "psfm_finalize_plan.h"

#include <vector>

extern "C" int psfm_host_bs_row_bytes(int km) { return km ? (int)sizeof(PsfmKmShapeRow) : (int)sizeof(PsfmFcShapeRow); }

// what a walk over a grid found.  out[0] blocks (gridDim.x); [1] items of the sequences' domains that are not owned exactly once;
// [2] items owned outside a sequence's domain (or by a block that found no sequence); [3] blocks of banded sequences that do not sit on
// the XCD of their band; [4] sequence starts that are no multiple of 8; [5] dispatched blocks (x, y) that return at once; [6] all
// dispatched blocks
enum { BS_BLOCKS, BS_NOT_ONCE, BS_OUTSIDE, BS_OFF_BAND, BS_UNALIGNED, BS_IDLE, BS_DISPATCHED, BS_N };

// flow_check: sequence i has frames of H[i] x W[i] and n_pairs[i] pairs; the launch covers pairs [0, n_y).  An item is a pixel PAIR.
extern "C" void psfm_host_bs_fc_walk(int n_seq, const int* H, const int* W, const int* n_pairs, int n_y, int* blk0, int* blk_end, int* chunks,
                                     int* xcd_per, long* out)
{
    std::vector<PsfmFcShapeRow> T((size_t)n_seq);
    for (int i = 0; i < n_seq; i++) {
        memset(&T[i], 0, sizeof(T[i]));
        T[i].H = H[i]; T[i].W = W[i]; T[i].n_pairs = n_pairs[i];
        T[i].chunks = psfm_bs_fc_chunks((int64_t)H[i] * W[i]);
        T[i].xcd_per = psfm_bs_xcd_per(T[i].chunks);
    }
    int ends[PSFM_BS_MAX];
    const int blocks = psfm_bs_fc_prefix(T.data(), n_seq, ends);
    for (int k = 0; k < BS_N; k++) out[k] = 0;
    out[BS_BLOCKS] = blocks;
    std::vector<std::vector<unsigned char>> own((size_t)n_seq);
    for (int i = 0; i < n_seq; i++) {
        blk0[i] = T[i].blk0; blk_end[i] = T[i].blk_end; chunks[i] = T[i].chunks; xcd_per[i] = T[i].xcd_per;
        if (T[i].blk0 % 8) out[BS_UNALIGNED]++;
        own[i].assign((size_t)(n_pairs[i] > 0 ? n_pairs[i] : 0) * (size_t)((int64_t)H[i] * W[i] / 2), 0);
    }
    for (int y = 0; y < n_y; y++)
        for (int blk = 0; blk < blocks; blk++) {
            out[BS_DISPATCHED]++;
            const int b = psfm_bs_find(ends, blk);
            if (b >= n_seq) { out[BS_OUTSIDE]++; continue; }
            const PsfmFcShapeRow& t = T[b];
            if (blk < t.blk0 || blk >= t.blk_end) { out[BS_OUTSIDE]++; continue; }
            if (y >= t.n_pairs) { out[BS_IDLE]++; continue; }
            const int local = blk - t.blk0;
            const int c = psfm_bs_chunk(local, t.chunks, t.xcd_per);
            if (c < 0) { out[BS_IDLE]++; continue; }
            if (t.xcd_per > 0 && (blk % 8 != local % 8 || c / t.xcd_per != blk % 8)) out[BS_OFF_BAND]++;
            // the body: thread tid takes the pixel pairs at p = (c * 512 + tid) * 2 + k * 512 of the frame pair, k = 0, 1
            const int64_t P = (int64_t)t.H * t.W;
            for (int tid = 0; tid < 256; tid++)
                for (int k = 0; k < 2; k++) {
                    const int64_t p = ((int64_t)c * 512 + tid) * 2 + (int64_t)k * 512;
                    if (p >= P) continue;
                    unsigned char& o = own[b][(size_t)y * (size_t)(P / 2) + (size_t)(p / 2)];
                    if (o < 255) o++;
                }
        }
    for (int i = 0; i < n_seq; i++)
        for (unsigned char o : own[i]) if (o != 1) out[BS_NOT_ONCE]++;
}

// kill maps: sequence i has n[i] frames of H[i] x W[i] in form form[i]; the launch covers frames [0, n_y).  An item is a four-pixel
// lane (form 2: a pixel).
extern "C" void psfm_host_bs_km_walk(int n_seq, const int* H, const int* W, const int* n, const int* form, int n_y, int* blk0, int* blk_end,
                                     int* chunks, int* xcd_per, long* out)
{
    std::vector<PsfmKmShapeRow> T((size_t)n_seq);
    for (int i = 0; i < n_seq; i++) {
        memset(&T[i], 0, sizeof(T[i]));
        T[i].H = H[i]; T[i].W = W[i]; T[i].P = H[i] * W[i]; T[i].n = n[i]; T[i].form = form[i];
        T[i].chunks = psfm_bs_km_chunks(T[i].P, form[i]);
        T[i].xcd_per = form[i] == PSFM_BS_KM_PX ? 0 : psfm_bs_xcd_per(T[i].chunks);
    }
    int ends[PSFM_BS_MAX];
    const int blocks = psfm_bs_km_prefix(T.data(), n_seq, ends);
    for (int k = 0; k < BS_N; k++) out[k] = 0;
    out[BS_BLOCKS] = blocks;
    std::vector<std::vector<unsigned char>> own((size_t)n_seq);
    std::vector<int64_t> items((size_t)n_seq);
    for (int i = 0; i < n_seq; i++) {
        blk0[i] = T[i].blk0; blk_end[i] = T[i].blk_end; chunks[i] = T[i].chunks; xcd_per[i] = T[i].xcd_per;
        if (T[i].blk0 % 8) out[BS_UNALIGNED]++;
        items[i] = form[i] == PSFM_BS_KM_PX ? T[i].P : (T[i].P + PSFM_BS_KM_PPL - 1) / PSFM_BS_KM_PPL;
        own[i].assign((size_t)(n[i] > 0 ? n[i] : 0) * (size_t)items[i], 0);
    }
    for (int y = 0; y < n_y; y++)
        for (int blk = 0; blk < blocks; blk++) {
            out[BS_DISPATCHED]++;
            const int b = psfm_bs_find(ends, blk);
            if (b >= n_seq) { out[BS_OUTSIDE]++; continue; }
            const PsfmKmShapeRow& t = T[b];
            if (blk < t.blk0 || blk >= t.blk_end) { out[BS_OUTSIDE]++; continue; }
            if (y >= t.n) { out[BS_IDLE]++; continue; }
            const int local = blk - t.blk0;
            const int c = psfm_bs_chunk(local, t.chunks, t.xcd_per);
            if (c < 0) { out[BS_IDLE]++; continue; }
            if (t.xcd_per > 0 && (blk % 8 != local % 8 || c / t.xcd_per != blk % 8)) out[BS_OFF_BAND]++;
            for (int tid = 0; tid < PSFM_BS_KM_LANES; tid++) {
                const int64_t item = (int64_t)c * PSFM_BS_KM_LANES + tid;      // lane r0 / 4 of the frame, or pixel p
                const int64_t first = t.form == PSFM_BS_KM_PX ? item : item * PSFM_BS_KM_PPL;
                if (first >= t.P) continue;
                unsigned char& o = own[b][(size_t)y * (size_t)items[b] + (size_t)item];
                if (o < 255) o++;
            }
        }
    for (int i = 0; i < n_seq; i++)
        for (unsigned char o : own[i]) if (o != 1) out[BS_NOT_ONCE]++;
}

extern "C" int psfm_host_bs_km_form(long P, int W, int al16) { return psfm_bs_km_form(P, W, al16 != 0); }

// the index bits psfm_track_dims gives a grid of G points
static int own_shift_b(long G) { int s = 1; while ((1ll << s) < G) ++s; return s; }

// -> out[0] shift_b, [1] time bits, [2] shift_d of the batch; [3] the finalize takes 32-bit keys for it (n_seq sequences, n records)
extern "C" void psfm_host_bs_common_key(int n_seq, const long* G, const int* n_flows, long n, int* out)
{
    int sb[PSFM_BS_MAX], n_max = 0;
    for (int i = 0; i < n_seq; i++) { sb[i] = own_shift_b(G[i]); if (n_flows[i] > n_max) n_max = n_flows[i]; }
    const PsfmBsKeyFmt k = psfm_bs_common_key(sb, n_flows, n_seq);
    out[0] = k.shift_b; out[1] = k.tbits; out[2] = k.shift_d;
    out[3] = psfm_fin_form(k.shift_b, k.shift_d, n_max, n_seq, n, 1, 1, 0).fmt.use32;
}

// Every record a sequence of G grid points and n_flows flows can write -- (last, birth, index), birth <= last <= n_flows, in
// lexicographic order -- as a key with the sequence's own shifts and with the batch's (shift_b, shift_d; use32: re-coded as the
// finalize's 32-bit key).  Returns the number of neighbours that either format does not order strictly ascending, or whose fields the
// batch's format does not give back; -1 if a 32-bit key of the batch's format does not fit 32 bits.
extern "C" long psfm_host_bs_key_order(long G, int n_flows, int shift_b, int shift_d, int use32)
{
    const int sb = own_shift_b(G);
    int tbits = 1;
    while ((1ll << tbits) < (long long)n_flows + 2) ++tbits;
    const int sd = sb + tbits;
    PsfmKeyFmt own_f, bat_f;
    own_f.shift_b = sb; own_f.shift_d = sd; own_f.use32 = use32;
    bat_f.shift_b = shift_b; bat_f.shift_d = shift_d; bat_f.use32 = use32;
    long bad = 0;
    bool have = false;
    unsigned long long prev_own = 0, prev_bat = 0;
    for (int last = 0; last <= n_flows; last++)
        for (int birth = 0; birth <= last; birth++)
            for (long idx = 0; idx < G; idx++) {
                unsigned long long ko = ((unsigned long long)last << sd) | ((unsigned long long)birth << sb) | (unsigned long long)idx;
                unsigned long long kb = ((unsigned long long)last << shift_d) | ((unsigned long long)birth << shift_b) | (unsigned long long)idx;
                int l2, b2, i2;
                if (use32) {
                    const unsigned long long tri = (unsigned long long)last * (last + 1) / 2 + birth;
                    if (((tri << shift_b) | (unsigned long long)idx) >> 32) return -1;
                    ko = psfm_key32(ko, own_f); kb = psfm_key32(kb, bat_f);
                    psfm_key32_fields((unsigned)kb, shift_b, &l2, &b2, &i2);
                } else {
                    psfm_key64_fields(kb, shift_b, shift_d, &l2, &b2, &i2);
                }
                if (l2 != last || b2 != birth || i2 != (int)idx) bad++;
                if (have && !(ko > prev_own && kb > prev_bat)) bad++;
                prev_own = ko; prev_bat = kb; have = true;
            }
    return bad;
}
