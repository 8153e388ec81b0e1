// HOST driver of particle-sfm_amd/csrc/psfm_result_set.h for tests/test_result_set_host.py: the per-entry rules of psfm_result_set
// (validation verdict, expansion), the footer check and the record decode of psfm_load_track_npy -- the decode block by block as
// the kernel stages it: aligned 16-byte vectors into a block-sized buffer, then one lane per record -- compiled through
// tests/host/shim.  Test infrastructure.
#include "psfm_result_set.h"

extern "C" int psfm_host_rs_block(void) { return PSFM_RS_BLOCK; }
extern "C" int psfm_host_rs_rec_max(void) { return PSFM_RS_REC_MAX; }
extern "C" int psfm_host_rs_lds_vecs(void) { return PSFM_RS_LDS_VECS; }
extern "C" long psfm_host_rs_id_end(void) { return PSFM_RS_ID_END; }
extern "C" long psfm_host_rs_frame_end(void) { return PSFM_RS_FRAME_END; }

static unsigned long long vmin(unsigned long long a, unsigned long long b) { return a < b ? a : b; }

// the verdict of the validation launch: lanes in any order, one minimum
extern "C" unsigned long long psfm_host_rs_validate(long n, const int* ids, const int* birth, const int* len, int reverse)
{
    unsigned long long v = PSFM_RS_NONE;
    for (long k = 0; k < n; k++) {
        const long i = reverse ? n - 1 - k : k;
        const int why = psfm_rs_entry(ids, birth, len, i);
        if (why != PSFM_RS_OK) v = vmin(v, psfm_rs_verdict(i, why));
    }
    return v;
}
extern "C" long psfm_host_rs_verdict_index(unsigned long long v) { return (long)psfm_rs_verdict_index(v); }
extern "C" int psfm_host_rs_verdict_reason(unsigned long long v) { return psfm_rs_verdict_reason(v); }

// the expansion: zero fill, scatter, exclusive scan; dense arrays of n_result entries, off of n_result + 1
extern "C" void psfm_host_rs_expand(long n, const int* ids, const int* birth, const int* len, long n_result, int* dense_birth, int* dense_len,
                                    long* off)
{
    int64_t* len64 = new int64_t[n_result + 1];
    for (long r = 0; r < n_result; r++) dense_birth[r] = dense_len[r] = 0;
    for (long r = 0; r <= n_result; r++) len64[r] = 0;
    for (long i = n - 1; i >= 0; i--) psfm_rs_scatter(ids, birth, len, i, dense_birth, dense_len, len64);
    int64_t sum = 0;
    for (long r = 0; r <= n_result; r++) { off[r] = (long)sum; sum += len64[r]; }
    delete[] len64;
}

extern "C" unsigned long long psfm_host_rs_spans(long n, const int* ids, const int* s, const int* e, const long* off)
{
    unsigned long long v = PSFM_RS_NONE;
    for (long i = 0; i < n; i++)
        if (!psfm_rs_span_ok(s[i], e[i], (const int64_t*)off, ids[i])) v = vmin(v, psfm_rs_verdict(i, PSFM_RS_BAD_SPAN));
    return v;
}

extern "C" int psfm_host_rs_footer(const unsigned char* f, long file_size, long rec_size, long* out /*[6]*/)
{
    PsfmRsFooter F;
    const int code = psfm_rs_footer_parse(f, file_size, rec_size, &F);
    if (code == PSFM_RS_FOOT_OK) {
        out[0] = (long)F.xy_data; out[1] = (long)F.n_points; out[2] = (long)F.rec_start; out[3] = (long)F.n; out[4] = (long)F.rec_size;
        out[5] = (long)F.end;
    }
    return code;
}

extern "C" int psfm_host_rs_template_ok(const unsigned char* rec, int rec_size, const int* field_at)
{
    PsfmRsTemplate T;
    return psfm_rs_template_make(rec, rec_size, field_at, &T) ? 1 : 0;
}

// The decode launch over a workspace of ws_bytes bytes whose record 0 sits at byte rec0.  Returns the verdict; *fault is set when a
// block would read a vector outside the workspace or more vectors than its LDS holds (what must never happen).
extern "C" unsigned long long psfm_host_rs_decode(const unsigned char* ws, long ws_bytes, long rec0, long n, const unsigned char* rec,
                                                  int rec_size, const int* field_at, int* ids, int* birth, int* len, int* s, int* e, int* fault)
{
    PsfmRsTemplate T;
    *fault = 0;
    if (!psfm_rs_template_make(rec, rec_size, field_at, &T)) { *fault = 3; return PSFM_RS_NONE; }
    unsigned long long v = PSFM_RS_NONE;
    static unsigned char lds[16 * PSFM_RS_LDS_VECS];
    const long blocks = (n + PSFM_RS_BLOCK - 1) / PSFM_RS_BLOCK;
    for (long b = 0; b < blocks; b++) {
        const PsfmRsSpan S = psfm_rs_span(rec0, n, b, rec_size);
        const long nv = (long)(S.v1 - S.v0);
        if (nv > PSFM_RS_LDS_VECS) { *fault = 1; return v; }
        if (S.v0 < 0 || 16 * S.v1 > ws_bytes) { *fault = 2; return v; }
        memset(lds, 0xA5, sizeof(lds));
        for (long q = 0; q < nv; q++) memcpy(lds + 16 * q, ws + 16 * (S.v0 + q), 16);
        for (int r = 0; r < S.count; r++) {
            int f[6];
            const int why = psfm_rs_decode(lds + S.shift + r * rec_size, T, f);
            const long i = b * PSFM_RS_BLOCK + r;
            ids[i] = f[0]; birth[i] = f[1]; len[i] = f[5]; s[i] = f[3]; e[i] = f[4];
            if (why != PSFM_RS_OK) v = vmin(v, psfm_rs_verdict(i, why));
        }
    }
    return v;
}
