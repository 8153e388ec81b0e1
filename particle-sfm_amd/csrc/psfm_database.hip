// psfm_database.hip -- sfm/import_feature_matches.py:76-104 (import_keypoints_matches) on the device: the match tables that the last
// psfm_traj_to_matches / psfm_labels_to_matches left in the context become the blobs of the COLMAP database's keypoints / matches /
// two_view_geometries rows.  The per-element rules (keypoint conversion, which directed pair is written, pair_id, column swap) are
// psfm_database.h; this file is the data movement around them:
//   select    one lane per directed pair: keep predicate (one binary search in pair_key) -> the pair's kept row count
//   scan      exclusive scan of (kept flag, kept rows) over the pairs: per-block totals, one block scans those, every block scans
//             its own 256 pairs again on top of its base.  Integers in a fixed order: two calls give identical bytes.
//   scatter   kept pair g: pair_id, pair_key, out_off[g], source offset + swap flag
//   compact   the kept pairs' rows -> ONE contiguous (n_rows_kept, 2) u32 table in ascending pair_key order of the kept pairs,
//             columns swapped where id_s > id_t.  Pair sizes differ by orders of magnitude (neighbouring frames hold most rows), so
//             the work is dealt by OUTPUT rows: block b owns rows [b * PD_CHUNK, (b + 1) * PD_CHUNK).  It finds the pairs that overlap
//             its chunk with two searches in out_off (the same for every lane: scalar loads), puts their descriptors in LDS, and every
//             lane then moves two output rows -- one 16-byte store, always aligned because the chunk and the lane's offset are even --
//             per step; which pair a row belongs to is a search over the few LDS descriptors, never over global memory.  A pair's
//             source offset is an arbitrary row index (8-byte aligned): the two rows come as one 16-byte load when they lie in one
//             pair at an even source row, as two 8-byte loads otherwise (odd source row, or the pair ends between them).  An odd
//             last row of the table is moved by one thread behind the loop, so that the loop body ends in exactly one store.  Rows
//             of dropped pairs are never read.  Bytes: 8 read + 8 written per kept row.
//   keypoints elementwise f64 (x, y) -> f32 (x + 0.5, y + 0.5): 16 bytes read, 8 written per keypoint
// The database tables are buffers of their own: they stay valid when the match tables are rebuilt.
#include <algorithm>
#include <vector>

#include "psfm_database.h"
#include "psfm_internal.h"

#define PD_BLOCK 256
#define PD_CHUNK 2048                      // output rows per block of the compaction (even; 16 KB read + 16 KB written)
#define PD_SWAP_BIT (1ll << 62)            // in a pair's source offset: swap the columns

static unsigned pd_grid(int64_t n) { return (unsigned)((n + PD_BLOCK - 1) / PD_BLOCK); }

// block-wide exclusive scan of two i64 per thread (Hillis-Steele in LDS: fixed order); returns the block totals
__device__ __forceinline__ void pd_block_scan(int64_t& k, int64_t& c, int64_t* s_k, int64_t* s_c, int64_t& tot_k, int64_t& tot_c)
{
    const int tid = threadIdx.x;
    s_k[tid] = k; s_c[tid] = c;
    __syncthreads();
    for (int d = 1; d < PD_BLOCK; d <<= 1) {
        const int64_t ak = tid >= d ? s_k[tid - d] : 0, ac = tid >= d ? s_c[tid - d] : 0;
        __syncthreads();
        s_k[tid] += ak; s_c[tid] += ac;
        __syncthreads();
    }
    tot_k = s_k[PD_BLOCK - 1]; tot_c = s_c[PD_BLOCK - 1];
    k = s_k[tid] - k; c = s_c[tid] - c;
    __syncthreads();
}

// cnt[p] = rows of pair p when it is written, 0 when it is dropped (a pair of the table has at least one row: kept <=> cnt > 0);
// bsum[2b], bsum[2b+1] = kept pairs, kept rows of block b
__global__ __launch_bounds__(PD_BLOCK) void pd_select_kernel(const int64_t* __restrict__ pair_key, const int64_t* __restrict__ pair_off,
                                                            int64_t n_pairs, int64_t n_img, const int32_t* __restrict__ pos,
                                                            int64_t* __restrict__ cnt, int64_t* __restrict__ bsum)
{
    __shared__ int64_t s_k[PD_BLOCK], s_c[PD_BLOCK];
    const int64_t p = (int64_t)blockIdx.x * PD_BLOCK + threadIdx.x;
    int64_t c = 0;
    if (p < n_pairs) {
        if (psfm_db_keep(pair_key, n_pairs, n_img, pos, pair_key[p])) c = pair_off[p + 1] - pair_off[p];
        cnt[p] = c;
    }
    int64_t k = c > 0 ? 1 : 0, tk, tc;
    pd_block_scan(k, c, s_k, s_c, tk, tc);
    if (threadIdx.x == 0) { bsum[2 * (int64_t)blockIdx.x] = tk; bsum[2 * (int64_t)blockIdx.x + 1] = tc; }
}

// ONE block: bsum -> its exclusive scan in place, tile after tile with a carry; totals[0] = kept pairs, totals[1] = kept rows
__global__ __launch_bounds__(PD_BLOCK) void pd_scan_blocks_kernel(int64_t* __restrict__ bsum, int64_t n_blocks, int64_t* __restrict__ totals)
{
    __shared__ int64_t s_k[PD_BLOCK], s_c[PD_BLOCK];
    int64_t carry_k = 0, carry_c = 0;
    for (int64_t base = 0; base < n_blocks; base += PD_BLOCK) {
        const int64_t i = base + threadIdx.x;
        int64_t k = i < n_blocks ? bsum[2 * i] : 0, c = i < n_blocks ? bsum[2 * i + 1] : 0, tk, tc;
        pd_block_scan(k, c, s_k, s_c, tk, tc);
        if (i < n_blocks) { bsum[2 * i] = carry_k + k; bsum[2 * i + 1] = carry_c + c; }
        carry_k += tk; carry_c += tc;
    }
    if (threadIdx.x == 0) { totals[0] = carry_k; totals[1] = carry_c; }
}

__global__ __launch_bounds__(PD_BLOCK) void pd_scatter_kernel(const int64_t* __restrict__ pair_key, const int64_t* __restrict__ pair_off,
                                                             const int64_t* __restrict__ cnt, int64_t n_pairs, int64_t n_img,
                                                             const int32_t* __restrict__ ids, const int64_t* __restrict__ bsum,
                                                             const int64_t* __restrict__ totals, int64_t* __restrict__ out_id,
                                                             int64_t* __restrict__ out_key, int64_t* __restrict__ out_off,
                                                             int64_t* __restrict__ out_src)
{
    __shared__ int64_t s_k[PD_BLOCK], s_c[PD_BLOCK];
    const int64_t p = (int64_t)blockIdx.x * PD_BLOCK + threadIdx.x;
    int64_t c = p < n_pairs ? cnt[p] : 0, tk, tc;
    const bool kept = c > 0;
    int64_t k = kept ? 1 : 0;
    pd_block_scan(k, c, s_k, s_c, tk, tc);
    if (kept) {
        const int64_t g = bsum[2 * (int64_t)blockIdx.x] + k;        // g < kept pairs <= n_pairs
        const int64_t key = pair_key[p], s = key / n_img, t = key - s * n_img;
        const int32_t id_s = ids[s], id_t = ids[t];
        out_id[g] = psfm_db_pair_id(id_s, id_t);
        out_key[g] = key;
        out_off[g] = bsum[2 * (int64_t)blockIdx.x + 1] + c;
        out_src[g] = pair_off[p] | (psfm_db_swap(id_s, id_t) ? PD_SWAP_BIT : 0);
    }
    if (p == 0) out_off[totals[0]] = totals[1];
}

__device__ __forceinline__ uint2 pd_row(int2 r, bool swap)
{
    const PsfmDbRow o = psfm_db_row(r.x, r.y, swap);
    return make_uint2(o.a, o.b);
}

// out_off (n_kept + 1) strictly ascending from 0 to n_rows; out_src (n_kept): first source row | swap bit.  Grid: ceil(n_rows / PD_CHUNK).
__global__ __launch_bounds__(PD_BLOCK) void pd_compact_kernel(const int2* __restrict__ rows_in, const int64_t* __restrict__ out_off,
                                                             const int64_t* __restrict__ out_src, int64_t n_kept, int64_t n_rows,
                                                             uint2* __restrict__ rows_out)
{
    __shared__ int s_out[PD_CHUNK + 1];     // first row of local pair j inside the chunk; [n_loc] = rows of the chunk
    __shared__ int64_t s_src[PD_CHUNK];     // the source row of that row | swap bit
    const int64_t r0 = (int64_t)blockIdx.x * PD_CHUNK;
    if (r0 >= n_rows) return;
    const int n_out = (int)((n_rows - r0 < PD_CHUNK) ? n_rows - r0 : PD_CHUNK);
    const int64_t r1 = r0 + n_out;
    // the block's pairs [g0, g1): g0 = the last pair that starts at or before r0, g1 = the first that starts at or behind r1.  The
    // pairs behind g0 start at distinct rows inside (r0, r1): at most PD_CHUNK of them together with g0.
    int64_t lo = 0, hi = n_kept;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (out_off[mid] <= r0) lo = mid; else hi = mid;
    }
    const int64_t g0 = lo;
    lo = g0 + 1; hi = n_kept;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (out_off[mid] < r1) lo = mid + 1; else hi = mid;
    }
    const int n_loc = (int)((lo - g0 < PD_CHUNK) ? lo - g0 : PD_CHUNK);
    for (int j = threadIdx.x; j < n_loc; j += PD_BLOCK) {
        const int64_t e = out_src[g0 + j];
        int64_t src = e & ~PD_SWAP_BIT, rel = out_off[g0 + j] - r0;
        if (rel < 0) { src -= rel; rel = 0; }                       // (pair g0 began in an earlier chunk)
        s_out[j] = (int)rel;
        s_src[j] = src | (e & PD_SWAP_BIT);
    }
    if (threadIdx.x == 0) s_out[n_loc] = n_out;
    __syncthreads();
    for (int i = 2 * threadIdx.x; i + 1 < n_out; i += 2 * PD_BLOCK) {
        int a = 0, b = n_loc;                                        // the last local pair that starts at or before row i
        while (b - a > 1) {
            const int mid = (a + b) >> 1;
            if (s_out[mid] <= i) a = mid; else b = mid;
        }
        const int64_t e = s_src[a];
        const bool swap = (e & PD_SWAP_BIT) != 0;
        const int64_t src = (e & ~PD_SWAP_BIT) + (i - s_out[a]);
        uint2 x, y;
        if (i + 1 < s_out[a + 1]) {                                  // both rows in this pair
            int2 u, v;
            if ((src & 1) == 0) {
                const int4 w = *(const int4*)(rows_in + src);
                u = make_int2(w.x, w.y); v = make_int2(w.z, w.w);
            } else {
                u = rows_in[src]; v = rows_in[src + 1];
            }
            x = pd_row(u, swap); y = pd_row(v, swap);
        } else {                                                     // the next pair starts at row i + 1
            const int64_t e2 = s_src[a + 1];
            x = pd_row(rows_in[src], swap); y = pd_row(rows_in[e2 & ~PD_SWAP_BIT], (e2 & PD_SWAP_BIT) != 0);
        }
        *(uint4*)(rows_out + r0 + i) = make_uint4(x.x, x.y, y.x, y.y);
    }
    if ((n_out & 1) && threadIdx.x == 0) {                           // the table's last row (n_rows odd): it ends the last pair
        const int64_t e = s_src[n_loc - 1];
        rows_out[r1 - 1] = pd_row(rows_in[(e & ~PD_SWAP_BIT) + (n_out - 1 - s_out[n_loc - 1])], (e & PD_SWAP_BIT) != 0);
    }
}

__global__ __launch_bounds__(PD_BLOCK) void pd_keypoint_kernel(const double2* __restrict__ xy, int64_t n, float2* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * PD_BLOCK + threadIdx.x;
    if (i >= n) return;
    const double2 v = xy[i];
    out[i] = make_float2(psfm_db_keypoint(v.x), psfm_db_keypoint(v.y));
}

extern "C" int psfm_database_chunk_rows(void) { return PD_CHUNK; }

extern "C" psfm_status psfm_matches_to_database(psfm_ctx* c, int n_img, const int32_t* db_id_host, const int32_t* db_pos_host,
                                                int64_t* n_pairs_kept_host, int64_t* n_rows_kept_host, void* stream)
{
    if (!c || !db_id_host || !db_pos_host || !n_pairs_kept_host || !n_rows_kept_host || n_img < 1) {
        psfm_set_error("psfm_matches_to_database: bad argument (n_img=%d)", n_img);
        return PSFM_ERR_ARG;
    }
    *n_pairs_kept_host = *n_rows_kept_host = 0;
    if (!c->mt_kp_off.p || c->mt_n_img < 1) {
        psfm_set_error("psfm_matches_to_database: no match tables in the context (psfm_traj_to_matches / psfm_labels_to_matches)");
        return PSFM_ERR_ARG;
    }
    if (n_img != c->mt_n_img) {
        psfm_set_error("psfm_matches_to_database: n_img=%d, the match tables were built with %d images", n_img, c->mt_n_img);
        return PSFM_ERR_ARG;
    }
    {
        std::vector<int32_t> sorted(db_id_host, db_id_host + n_img);
        std::vector<char> seen((size_t)n_img, 0);
        for (int i = 0; i < n_img; ++i) {
            if (sorted[i] < 1 || (int64_t)sorted[i] > PSFM_DB_MAX_IMAGE_ID - 1) {
                psfm_set_error("psfm_matches_to_database: image %d has id %d, outside [1, 2^31 - 2]", i, sorted[i]);
                return PSFM_ERR_ARG;
            }
            const int32_t q = db_pos_host[i];
            if (q < 0 || q >= n_img || seen[q]) {
                psfm_set_error("psfm_matches_to_database: db_pos is not a permutation of 0..%d (image %d: %d)", n_img - 1, i, q);
                return PSFM_ERR_ARG;
            }
            seen[q] = 1;
        }
        std::sort(sorted.begin(), sorted.end());
        for (int i = 1; i < n_img; ++i)
            if (sorted[i] == sorted[i - 1]) { psfm_set_error("psfm_matches_to_database: id %d is given to two images", sorted[i]); return PSFM_ERR_ARG; }
    }
    PSFM_HIP(hipSetDevice(c->device));
    PsfmGate gate(c->device, 0);
    hipStream_t s = (hipStream_t)stream;
    psfm_status st;
    c->db_valid = c->db_src_live = false;
    const int64_t n_kp = c->mt_n_kp, n_m = c->mt_n_m, n_p = n_m > 0 ? c->mt_n_pairs : 0;
    // ---- keypoints ----
    if ((st = c->db_kp.ensure(8 * (size_t)(n_kp > 0 ? n_kp : 1))) != PSFM_OK) return st;
    if (n_kp > 0)
        hipLaunchKernelGGL(pd_keypoint_kernel, dim3(pd_grid(n_kp)), dim3(PD_BLOCK), 0, s, (const double2*)c->mt_kp_xy.as<double2>(), n_kp,
                           c->db_kp.as<float2>());
    c->db_n_kp = n_kp; c->db_n_img = n_img; c->db_n_pairs = c->db_n_rows = 0; c->db_cap = n_p;
    if ((st = c->db_pairs.ensure(8 * (size_t)(3 * n_p + 1))) != PSFM_OK) return st;
    if (n_p == 0) {                                                  // no pair: pair_off = [0]
        PSFM_HIP(hipMemsetAsync(c->db_pairs.p, 0, 8, s));
        PSFM_HIP(hipGetLastError());
        PSFM_HIP(hipStreamSynchronize(s));
        c->db_valid = true;
        return PSFM_OK;
    }
    // ---- select, scan, scatter ----
    const int64_t nb = pd_grid(n_p);
    const size_t a_img = ((size_t)n_img * 4 + 255) / 256 * 256, a_p = ((size_t)n_p * 8 + 255) / 256 * 256;
    const size_t a_b = ((size_t)nb * 16 + 255) / 256 * 256;
    if ((st = c->db_ws.ensure(2 * a_img + 2 * a_p + a_b + 256)) != PSFM_OK) return st;
    char* w = (char*)c->db_ws.p;
    int32_t* ids = (int32_t*)w; int32_t* pos = (int32_t*)(w + a_img);
    int64_t* cnt = (int64_t*)(w + 2 * a_img); int64_t* src = (int64_t*)(w + 2 * a_img + a_p);
    int64_t* bsum = (int64_t*)(w + 2 * a_img + 2 * a_p); int64_t* totals = (int64_t*)(w + 2 * a_img + 2 * a_p + a_b);
    const int64_t* pk = c->mt_pairs.as<int64_t>();
    const int64_t* poff = pk + c->mt_n_pairs;
    int64_t* out_id = c->db_pairs.as<int64_t>(); int64_t* out_key = out_id + n_p; int64_t* out_off = out_id + 2 * n_p;
    PSFM_HIP(hipMemcpyAsync(ids, db_id_host, 4 * (size_t)n_img, hipMemcpyHostToDevice, s));
    PSFM_HIP(hipMemcpyAsync(pos, db_pos_host, 4 * (size_t)n_img, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(pd_select_kernel, dim3((unsigned)nb), dim3(PD_BLOCK), 0, s, pk, poff, n_p, (int64_t)n_img, (const int32_t*)pos, cnt, bsum);
    hipLaunchKernelGGL(pd_scan_blocks_kernel, dim3(1), dim3(PD_BLOCK), 0, s, bsum, nb, totals);
    hipLaunchKernelGGL(pd_scatter_kernel, dim3((unsigned)nb), dim3(PD_BLOCK), 0, s, pk, poff, (const int64_t*)cnt, n_p, (int64_t)n_img,
                       (const int32_t*)ids, (const int64_t*)bsum, (const int64_t*)totals, out_id, out_key, out_off, src);
    int64_t* h = (int64_t*)((char*)c->host_pinned + 384);           // [0] kept pairs, [1] kept rows
    PSFM_HIP(hipMemcpyAsync(h, totals, 16, hipMemcpyDeviceToHost, s));
    PSFM_HIP(hipStreamSynchronize(s));
    const int64_t n_kept = h[0], n_rows = h[1];
    if (n_kept < 0 || n_kept > n_p || n_rows < n_kept || n_rows > n_m) {
        psfm_set_error("psfm_matches_to_database: inconsistent totals (%lld pairs, %lld rows)", (long long)n_kept, (long long)n_rows);
        return PSFM_ERR_HIP;
    }
    // ---- rows ----
    if ((st = c->db_rows.ensure(8 * (size_t)(n_rows > 0 ? n_rows : 1))) != PSFM_OK) return st;
    if (n_rows > 0)
        hipLaunchKernelGGL(pd_compact_kernel, dim3((unsigned)((n_rows + PD_CHUNK - 1) / PD_CHUNK)), dim3(PD_BLOCK), 0, s,
                           (const int2*)c->mt_rows.as<int2>(), (const int64_t*)out_off, (const int64_t*)src, n_kept, n_rows,
                           c->db_rows.as<uint2>());
    PSFM_HIP(hipGetLastError());
    PSFM_HIP(hipStreamSynchronize(s));
    c->db_n_pairs = n_kept; c->db_n_rows = n_rows;
    *n_pairs_kept_host = n_kept; *n_rows_kept_host = n_rows;
    c->db_valid = true;
    c->db_src_live = true;
    return PSFM_OK;
}

// the compaction launch of the last psfm_matches_to_database once more (for measurement: same input, same output bytes)
extern "C" psfm_status psfm_database_compact_again(psfm_ctx* c, void* stream)
{
    if (!c) { psfm_set_error("ctx is NULL"); return PSFM_ERR_ARG; }
    if (!c->db_valid || !c->db_src_live) {
        psfm_set_error("psfm_database_compact_again: the match tables changed since psfm_matches_to_database (or it never ran)");
        return PSFM_ERR_ARG;
    }
    PSFM_HIP(hipSetDevice(c->device));
    PsfmGate gate(c->device, 0);
    const int64_t n_p = c->db_cap, n_kept = c->db_n_pairs, n_rows = c->db_n_rows;
    if (n_rows == 0) return PSFM_OK;
    const size_t a_img = ((size_t)c->db_n_img * 4 + 255) / 256 * 256, a_p = ((size_t)n_p * 8 + 255) / 256 * 256;
    const int64_t* src = (const int64_t*)((char*)c->db_ws.p + 2 * a_img + a_p);
    hipLaunchKernelGGL(pd_compact_kernel, dim3((unsigned)((n_rows + PD_CHUNK - 1) / PD_CHUNK)), dim3(PD_BLOCK), 0, (hipStream_t)stream,
                       (const int2*)c->mt_rows.as<int2>(), c->db_pairs.as<int64_t>() + 2 * n_p, src, n_kept, n_rows, c->db_rows.as<uint2>());
    PSFM_HIP(hipGetLastError());
    return PSFM_OK;
}

// hipMemcpyDefault: the destinations may be host buffers or device buffers
extern "C" psfm_status psfm_database_copy(psfm_ctx* c, float* kp_f32, int64_t* pair_id, int64_t* pair_key, int64_t* pair_off, uint32_t* rows,
                                          void* stream)
{
    if (!c) { psfm_set_error("ctx is NULL"); return PSFM_ERR_ARG; }
    if (!c->db_valid) { psfm_set_error("psfm_database_copy: no database tables in the context (psfm_matches_to_database)"); return PSFM_ERR_ARG; }
    PSFM_HIP(hipSetDevice(c->device));
    PsfmGate gate(c->device, 0);
    hipStream_t s = (hipStream_t)stream;
    const int64_t n_kp = c->db_n_kp, n_p = c->db_n_pairs, n_r = c->db_n_rows, cap = c->db_cap;
    const int64_t* base = c->db_pairs.as<int64_t>();
    if (kp_f32 && n_kp > 0) PSFM_HIP(hipMemcpyAsync(kp_f32, c->db_kp.p, 8 * (size_t)n_kp, hipMemcpyDefault, s));
    if (pair_id && n_p > 0) PSFM_HIP(hipMemcpyAsync(pair_id, base, 8 * (size_t)n_p, hipMemcpyDefault, s));
    if (pair_key && n_p > 0) PSFM_HIP(hipMemcpyAsync(pair_key, base + cap, 8 * (size_t)n_p, hipMemcpyDefault, s));
    if (pair_off) PSFM_HIP(hipMemcpyAsync(pair_off, base + 2 * cap, 8 * (size_t)(n_p + 1), hipMemcpyDefault, s));
    if (rows && n_r > 0) PSFM_HIP(hipMemcpyAsync(rows, c->db_rows.p, 8 * (size_t)n_r, hipMemcpyDefault, s));
    PSFM_HIP(hipStreamSynchronize(s));
    return PSFM_OK;
}
