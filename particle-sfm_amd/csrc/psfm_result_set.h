// psfm_result_set.h -- a trajectory set from elsewhere as the context's result (psfm_result_set) and this package's own track.npy
// files straight into HBM (psfm_load_track_npy): the per-element rules the kernels of psfm_result_set.hip apply, the footer check
// and the record decode.  Also compiled for the host by the CPU suite (tests/host/result_set_host.cpp through tests/host/shim).
//
// The given set is what psfm_result_filtered_copy returns without `off`: ids strictly ascending, trajectory i on frames
// birth[i] .. birth[i] + len[i] - 1.  The context's result is a CSR in which index == id, so the set is expanded to
// ids[n - 1] + 1 entries; an id the set does not hold becomes an entry with len = 0, birth = 0 and no points.
//
// The file: save_track_npy(layout="reference") leaves a 64-byte footer behind the pickle (point_trajectory/reference_pickle.py,
// _FOOTER): magic, offset of the raw f64 point bytes, n_points, offset of the records, n, record size, file size in front of the
// footer, magic -- all little-endian i64.  A record is a fixed number of bytes of pickle opcodes (63 as the writer stands, at most
// PSFM_RS_REC_MAX here) with six i32 fields (id, b, b + n, s, e, n) at offsets the caller passes along with the zero-field template
// and its size; nothing here knows the opcodes or the size.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#define PSFM_RS_BLOCK 256                   // lanes per block = records per block of the decode
#define PSFM_RS_REC_MAX 68                  // bytes of one record at most (the caller's template says how many)
#define PSFM_RS_REC_WORDS 17                // ... in dwords
#define PSFM_RS_ID_END (1 << 28)            // ids lie in [0, 2^28): the dense arrays stay below 2^31 bytes of i32
#define PSFM_RS_FRAME_END (1 << 30)         // birth + len <= 2^30: frame arithmetic stays in i32 everywhere behind
#define PSFM_RS_FOOTER 64
#define PSFM_RS_NONE 0xffffffffffffffffull  // the verdict word when no lane objected

// why an entry is refused; the verdict is (index << 8 | reason), so the minimum names the lowest bad index and its first reason
enum { PSFM_RS_OK = 0, PSFM_RS_BAD_ID = 1, PSFM_RS_BAD_ORDER = 2, PSFM_RS_BAD_LEN = 3, PSFM_RS_BAD_BIRTH = 4, PSFM_RS_BAD_END = 5,
       PSFM_RS_BAD_TEMPLATE = 8, PSFM_RS_BAD_BN = 9, PSFM_RS_BAD_SPAN = 10 };

__host__ __device__ __forceinline__ unsigned long long psfm_rs_verdict(int64_t i, int reason)
{
    return ((unsigned long long)i << 8) | (unsigned long long)reason;
}
__host__ __device__ __forceinline__ int64_t psfm_rs_verdict_index(unsigned long long v) { return (int64_t)(v >> 8); }
__host__ __device__ __forceinline__ int psfm_rs_verdict_reason(unsigned long long v) { return (int)(v & 0xffull); }

// entry i of the given set (the ascending test reads ids[i - 1])
__host__ __device__ __forceinline__ int psfm_rs_entry(const int* ids, const int* birth, const int* len, int64_t i)
{
    const int id = ids[i], b = birth[i], n = len[i];
    if (id < 0 || id >= PSFM_RS_ID_END) return PSFM_RS_BAD_ID;
    if (i > 0 && ids[i - 1] >= id) return PSFM_RS_BAD_ORDER;
    if (n < 1) return PSFM_RS_BAD_LEN;
    if (b < 0) return PSFM_RS_BAD_BIRTH;
    if ((int64_t)b + (int64_t)n > (int64_t)PSFM_RS_FRAME_END) return PSFM_RS_BAD_END;
    return PSFM_RS_OK;
}

// entry i into the zero-filled dense arrays: index == id
__host__ __device__ __forceinline__ void psfm_rs_scatter(const int* ids, const int* birth, const int* len, int64_t i, int* dense_birth,
                                                         int* dense_len, int64_t* dense_len64)
{
    const int id = ids[i];
    dense_birth[id] = birth[i];
    dense_len[id] = len[i];
    dense_len64[id] = (int64_t)len[i];
}

// a record's (s, e) against the scanned offsets: its points are [off[id], off[id + 1])
__host__ __device__ __forceinline__ bool psfm_rs_span_ok(int s, int e, const int64_t* off, int id)
{
    return (int64_t)s == off[id] && (int64_t)e == off[id + 1];
}

// ---- the record: template, fields ---------------------------------------------------------------------------------------------

// The template as the kernel takes it BY VALUE (kernel arguments are read through scalar loads): the record's bytes with zeroed
// fields, one bit per byte that is NOT a field byte, the fields' offsets, the record's size.
struct PsfmRsTemplate {
    uint32_t w[PSFM_RS_REC_WORDS];
    uint32_t keep[3];
    int at[6];              // id, b, b + n, s, e, n
    int rec_size;
};

// false: a field outside the record or two fields that overlap
inline bool psfm_rs_template_make(const uint8_t* rec, int rec_size, const int* field_at, PsfmRsTemplate* T)
{
    if (rec_size < 24 || rec_size > PSFM_RS_REC_MAX || !rec || !field_at) return false;
    uint8_t b[4 * PSFM_RS_REC_WORDS];
    memset(b, 0, sizeof(b));
    memcpy(b, rec, (size_t)rec_size);
    T->rec_size = rec_size;
    for (int q = 0; q < 3; q++) {
        const int bits = rec_size - 32 * q;
        T->keep[q] = bits >= 32 ? 0xffffffffu : (bits <= 0 ? 0u : (1u << bits) - 1u);
    }
    for (int k = 0; k < 6; k++) {
        const int a = field_at[k];
        if (a < 0 || a + 4 > rec_size) return false;
        T->at[k] = a;
        for (int j = a; j < a + 4; j++) {
            if (!((T->keep[j >> 5] >> (j & 31)) & 1u)) return false;
            T->keep[j >> 5] &= ~(1u << (j & 31));
            b[j] = 0;
        }
    }
    memcpy(T->w, b, sizeof(b));
    return true;
}

__host__ __device__ __forceinline__ int psfm_rs_field(const uint8_t* rec, int at)
{
    return (int)((unsigned)rec[at] | ((unsigned)rec[at + 1] << 8) | ((unsigned)rec[at + 2] << 16) | ((unsigned)rec[at + 3] << 24));
}

// one record: its six fields; PSFM_RS_OK, or what is wrong with it (a byte outside the fields differs from the template; bn != b + n)
__host__ __device__ __forceinline__ int psfm_rs_decode(const uint8_t* rec, const PsfmRsTemplate& T, int* f /*[6]*/)
{
    unsigned diff = 0;
    for (int j = 0; j < T.rec_size; j++) {              // (j, want and keep are uniform: scalar work beside one byte load per lane)
        const unsigned want = (T.w[j >> 2] >> (8 * (j & 3))) & 0xffu;
        const unsigned keep = (T.keep[j >> 5] >> (j & 31)) & 1u;
        diff |= keep ? ((unsigned)rec[j] ^ want) : 0u;
    }
#pragma unroll
    for (int k = 0; k < 6; k++) f[k] = psfm_rs_field(rec, T.at[k]);
    if (diff != 0) return PSFM_RS_BAD_TEMPLATE;
    if ((int64_t)f[2] != (int64_t)f[1] + (int64_t)f[5]) return PSFM_RS_BAD_BN;
    return PSFM_RS_OK;
}

// What block `blk` of the decode stages: the records [256 blk, 256 blk + count) lie at bytes [lo, hi) of the workspace (record 0 at
// byte rec0, R bytes per record); the block loads the 16-byte vectors [v0, v1) -- the first aligned down inside the workspace, the
// last the one that holds byte hi - 1 -- and record r of the block starts at byte `shift` + R r of what it loaded.
struct PsfmRsSpan { int64_t v0, v1; int shift, count; };
__host__ __device__ __forceinline__ PsfmRsSpan psfm_rs_span(int64_t rec0, int64_t n, int64_t blk, int R)
{
    PsfmRsSpan S;
    const int64_t r0 = blk * PSFM_RS_BLOCK;
    const int64_t left = n - r0;
    S.count = left <= 0 ? 0 : (left < PSFM_RS_BLOCK ? (int)left : PSFM_RS_BLOCK);
    const int64_t lo = rec0 + r0 * R, hi = lo + (int64_t)S.count * R;
    S.v0 = lo >> 4;
    S.v1 = S.count > 0 ? ((hi + 15) >> 4) : S.v0;
    S.shift = (int)(lo & 15);
    return S;
}
// 16-byte vectors of LDS a block needs at most: 256 records, a shift of up to 15 bytes, rounded up
#define PSFM_RS_LDS_VECS ((PSFM_RS_BLOCK * PSFM_RS_REC_MAX + 15 + 15) / 16)

// ---- the footer -----------------------------------------------------------------------------------------------------------------

struct PsfmRsFooter { int64_t xy_data, n_points, rec_start, n, rec_size, end; };

enum { PSFM_RS_FOOT_OK = 0, PSFM_RS_FOOT_SHORT = 1, PSFM_RS_FOOT_MAGIC = 2, PSFM_RS_FOOT_END = 3, PSFM_RS_FOOT_REC_SIZE = 4,
       PSFM_RS_FOOT_RECORDS = 5, PSFM_RS_FOOT_POINTS = 6 };

inline const char* psfm_rs_footer_what(int code)
{
    switch (code) {
    case PSFM_RS_FOOT_SHORT: return "the file is too short to hold a footer";
    case PSFM_RS_FOOT_MAGIC: return "no footer behind the pickle (another writer's file, or a truncated one)";
    case PSFM_RS_FOOT_END: return "the footer's file size differs from the file's";
    case PSFM_RS_FOOT_REC_SIZE: return "the footer's record size differs from the template's";
    case PSFM_RS_FOOT_RECORDS: return "the footer's records do not lie inside the file";
    case PSFM_RS_FOOT_POINTS: return "the footer's point bytes do not lie in front of the records";
    default: return "ok";
    }
}

// the last 64 bytes of a file of `file_size` bytes; every product is checked before it is formed
inline int psfm_rs_footer_parse(const uint8_t* f, int64_t file_size, int64_t rec_size, PsfmRsFooter* out)
{
    if (file_size <= PSFM_RS_FOOTER) return PSFM_RS_FOOT_SHORT;
    static const char magic[9] = "PSFMTRK1";
    if (memcmp(f, magic, 8) != 0 || memcmp(f + 56, magic, 8) != 0) return PSFM_RS_FOOT_MAGIC;
    int64_t v[6];
    memcpy(v, f + 8, 48);            // (little-endian i64, as every host this builds for)
    PsfmRsFooter o;
    o.xy_data = v[0]; o.n_points = v[1]; o.rec_start = v[2]; o.n = v[3]; o.rec_size = v[4]; o.end = v[5];
    if (o.end != file_size - PSFM_RS_FOOTER) return PSFM_RS_FOOT_END;
    if (rec_size < 1 || o.rec_size != rec_size) return PSFM_RS_FOOT_REC_SIZE;
    if (o.n < 0 || o.rec_start < 0 || o.rec_start >= o.end) return PSFM_RS_FOOT_RECORDS;
    if (o.n > (o.end - o.rec_start) / rec_size || o.n * rec_size >= o.end - o.rec_start) return PSFM_RS_FOOT_RECORDS;   // rec_start + n R < end
    if (o.n_points < 0) return PSFM_RS_FOOT_POINTS;
    if (o.n_points > 0) {
        if (o.xy_data <= 0 || o.xy_data >= o.rec_start) return PSFM_RS_FOOT_POINTS;
        if (o.n_points > (o.rec_start - o.xy_data) / 16) return PSFM_RS_FOOT_POINTS;      // xy_data + 16 n_points <= rec_start
    }
    *out = o;
    return PSFM_RS_FOOT_OK;
}
