// psfm_result_set.hip -- a trajectory set from elsewhere becomes the context's result (psfm_result_set), and this package's own
// track.npy files go straight into HBM (psfm_load_track_npy).  The reference connects its stages through files
// (trajectories/track.npy -> trajectories_labeled/track.npy -> database.db); with these two calls a stage that starts from a file
// runs the same device kernels as one that follows psfm_connect in the same process.  Rules: psfm_result_set.h.
//
// Both calls stage the metadata in a workspace of their own, validate it there (one lane per given trajectory, the lowest bad
// index through one integer atomicMin), expand it behind a clean verdict (scatter into zero-filled dense arrays, one exclusive
// scan) and only then exchange the workspace with the result: a refused call leaves the previous result as it was.
#include <errno.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include <string>
#include <utility>

#include <rocprim/device/device_scan.hpp>

#include "psfm_device.h"
#include "psfm_internal.h"
#include "psfm_result_set.h"

// verdict block in device memory: [0] first pass, [1] second pass (0xff-filled = PSFM_RS_NONE), [2] max(birth + len) | last id << 32
#define RS_VERDICT_BYTES 256

static unsigned rs_grid(int64_t n) { return (unsigned)((n + PSFM_RS_BLOCK - 1) / PSFM_RS_BLOCK); }

__global__ __launch_bounds__(PSFM_RS_BLOCK) void psfm_rs_validate_kernel(const int* __restrict__ ids, const int* __restrict__ birth,
                                                                        const int* __restrict__ len, int64_t n,
                                                                        unsigned long long* __restrict__ verdict)
{
    const int64_t i = (int64_t)blockIdx.x * PSFM_RS_BLOCK + threadIdx.x;
    int end = 0;
    if (i < n) {
        const int why = psfm_rs_entry(ids, birth, len, i);
        if (why != PSFM_RS_OK) atomicMin(verdict, psfm_rs_verdict(i, why));
        else end = birth[i] + len[i];
        if (i == n - 1) ((unsigned*)(verdict + 2))[1] = (unsigned)ids[i];
    }
#pragma unroll
    for (int d = PSFM_WAVE / 2; d > 0; d >>= 1) { const int o = __shfl_xor(end, d, PSFM_WAVE); end = o > end ? o : end; }
    if ((threadIdx.x & (PSFM_WAVE - 1)) == 0 && end > 0) atomicMax((unsigned*)(verdict + 2), (unsigned)end);
}

__global__ __launch_bounds__(PSFM_RS_BLOCK) void psfm_rs_scatter_kernel(const int* __restrict__ ids, const int* __restrict__ birth,
                                                                       const int* __restrict__ len, int64_t n, int* __restrict__ dense_birth,
                                                                       int* __restrict__ dense_len, int64_t* __restrict__ dense_len64)
{
    const int64_t i = (int64_t)blockIdx.x * PSFM_RS_BLOCK + threadIdx.x;
    if (i < n) psfm_rs_scatter(ids, birth, len, i, dense_birth, dense_len, dense_len64);
}

// One lane per record, 256 records per block: the block's bytes go into LDS as aligned 16-byte vectors, then every lane compares
// its record with the template (kernel arguments: scalar loads) and assembles its fields from bytes.
__global__ __launch_bounds__(PSFM_RS_BLOCK) void psfm_rs_decode_kernel(const uint4* __restrict__ ws, int64_t rec0, int64_t n, PsfmRsTemplate T,
                                                                      int* __restrict__ ids, int* __restrict__ birth, int* __restrict__ len,
                                                                      int* __restrict__ s_out, int* __restrict__ e_out,
                                                                      unsigned long long* __restrict__ verdict)
{
    __shared__ uint4 lds[PSFM_RS_LDS_VECS];
    const PsfmRsSpan S = psfm_rs_span(rec0, n, (int64_t)blockIdx.x, T.rec_size);
    const int nv = (int)(S.v1 - S.v0);                    // <= PSFM_RS_LDS_VECS
    for (int v = threadIdx.x; v < nv; v += PSFM_RS_BLOCK) lds[v] = ws[S.v0 + v];
    __syncthreads();
    const int r = threadIdx.x;
    if (r >= S.count) return;
    const uint8_t* rec = (const uint8_t*)lds + S.shift + r * T.rec_size;
    int f[6];
    const int why = psfm_rs_decode(rec, T, f);
    const int64_t i = (int64_t)blockIdx.x * PSFM_RS_BLOCK + r;
    ids[i] = f[0]; birth[i] = f[1]; len[i] = f[5]; s_out[i] = f[3]; e_out[i] = f[4];
    if (why != PSFM_RS_OK) atomicMin(verdict, psfm_rs_verdict(i, why));
}

// behind the scan: a record's (s, e) must be its points' place in the point array
__global__ __launch_bounds__(PSFM_RS_BLOCK) void psfm_rs_span_kernel(const int* __restrict__ ids, const int* __restrict__ s_in,
                                                                    const int* __restrict__ e_in, int64_t n, const int64_t* __restrict__ off,
                                                                    unsigned long long* __restrict__ verdict)
{
    const int64_t i = (int64_t)blockIdx.x * PSFM_RS_BLOCK + threadIdx.x;
    if (i >= n) return;
    if (!psfm_rs_span_ok(s_in[i], e_in[i], off, ids[i])) atomicMin(verdict + 1, psfm_rs_verdict(i, PSFM_RS_BAD_SPAN));
}

static const char* rs_reason(int why)
{
    switch (why) {
    case PSFM_RS_BAD_ID: return "its id lies outside [0, 2^28)";
    case PSFM_RS_BAD_ORDER: return "its id is not above its predecessor's (ids must ascend strictly)";
    case PSFM_RS_BAD_LEN: return "its len is below 1";
    case PSFM_RS_BAD_BIRTH: return "its birth is negative";
    case PSFM_RS_BAD_END: return "its birth + len exceeds 2^30";
    case PSFM_RS_BAD_TEMPLATE: return "its record differs from the template outside the six fields";
    case PSFM_RS_BAD_BN: return "its record's b + n field is not birth + len";
    case PSFM_RS_BAD_SPAN: return "its record's slice is not its place in the point array";
    default: return "refused";
    }
}

// the staged arrays of one call inside c->rs_ws: the verdict block, then five i32 arrays of n entries, 256 bytes apart at least
struct RsStage {
    unsigned long long* verdict;
    int *ids, *birth, *len, *s, *e;
};
static psfm_status rs_stage(psfm_ctx* c, int64_t n, RsStage& g)
{
    const size_t a4 = ((size_t)(n > 0 ? n : 1) * 4 + 255) / 256 * 256;
    psfm_status st;
    if ((st = c->rs_ws.ensure(RS_VERDICT_BYTES + 5 * a4)) != PSFM_OK) return st;
    char* w = (char*)c->rs_ws.p;
    g.verdict = (unsigned long long*)w;
    g.ids = (int*)(w + RS_VERDICT_BYTES); g.birth = (int*)(w + RS_VERDICT_BYTES + a4); g.len = (int*)(w + RS_VERDICT_BYTES + 2 * a4);
    g.s = (int*)(w + RS_VERDICT_BYTES + 3 * a4); g.e = (int*)(w + RS_VERDICT_BYTES + 4 * a4);
    return PSFM_OK;
}
static psfm_status rs_verdict_reset(const RsStage& g, hipStream_t s)
{
    PSFM_HIP(hipMemsetAsync(g.verdict, 0xff, 16, s));
    PSFM_HIP(hipMemsetAsync(g.verdict + 2, 0, 8, s));
    return PSFM_OK;
}

// the context holds the (empty or new) set result from here on
static void rs_commit(psfm_ctx* c, int64_t n_result, int64_t n_points, int n_flows)
{
    c->solve_stats.clear();
    c->res_n_traj = n_result; c->res_n_points = n_points; c->res_n_flows = n_flows;
    c->res_is_query = false;
    c->res_is_set = true;
    c->res_gen++;            // (a live label merge and a sampler plan are void)
}

// The staged set (g.ids / birth / len filled, the verdict block reset and possibly holding the decode's objections; with_spans: g.s /
// g.e too) -> validated, expanded, exchanged with the result.  xy: the points, HOST or DEVICE, copied in front of the second
// synchronisation; NULL: the caller fills res_xy behind this call (the result then reports its points only once they are there).
// Two host synchronisations: the verdict, the point total.
static psfm_status rs_core(psfm_ctx* c, const char* who, const RsStage& g, int64_t n, int64_t n_points, bool with_spans, const double* xy,
                           int64_t* n_result_host, hipStream_t s)
{
    psfm_status st;
    hipLaunchKernelGGL(psfm_rs_validate_kernel, dim3(rs_grid(n)), dim3(PSFM_RS_BLOCK), 0, s, (const int*)g.ids, (const int*)g.birth,
                       (const int*)g.len, n, g.verdict);
    PSFM_HIP(hipGetLastError());
    unsigned long long* h = (unsigned long long*)((char*)c->host_pinned + 472);     // [0] verdict, [1] second verdict, [2] end | last id; [3] total
    PSFM_HIP(hipMemcpyAsync(h, g.verdict, 24, hipMemcpyDeviceToHost, s));
    PSFM_HIP(hipStreamSynchronize(s));
    if (h[0] != PSFM_RS_NONE) {
        psfm_set_error("%s: trajectory %lld is refused: %s (the context is untouched)", who, (long long)psfm_rs_verdict_index(h[0]),
                       rs_reason(psfm_rs_verdict_reason(h[0])));
        return PSFM_ERR_ARG;
    }
    const int64_t n_result = (int64_t)(h[2] >> 32) + 1;
    const int n_flows = (int)(h[2] & 0xffffffffull) - 1;
    if ((st = c->rs_birth.ensure(4 * (size_t)n_result)) != PSFM_OK) return st;
    if ((st = c->rs_len.ensure(4 * (size_t)n_result)) != PSFM_OK) return st;
    if ((st = c->rs_off.ensure(8 * (size_t)(n_result + 1))) != PSFM_OK) return st;
    if ((st = c->scan_tmp.ensure(8 * (size_t)(n_result + 1))) != PSFM_OK) return st;
    if (xy && (st = c->rs_xy.ensure(16 * (size_t)(n_points > 0 ? n_points : 1))) != PSFM_OK) return st;
    PSFM_HIP(hipMemsetAsync(c->rs_birth.p, 0, 4 * (size_t)n_result, s));
    PSFM_HIP(hipMemsetAsync(c->rs_len.p, 0, 4 * (size_t)n_result, s));
    PSFM_HIP(hipMemsetAsync(c->scan_tmp.p, 0, 8 * (size_t)(n_result + 1), s));
    hipLaunchKernelGGL(psfm_rs_scatter_kernel, dim3(rs_grid(n)), dim3(PSFM_RS_BLOCK), 0, s, (const int*)g.ids, (const int*)g.birth,
                       (const int*)g.len, n, c->rs_birth.as<int>(), c->rs_len.as<int>(), c->scan_tmp.as<int64_t>());
    PSFM_HIP(hipGetLastError());
    {
        size_t bytes = 0;
        PSFM_HIP(rocprim::exclusive_scan(nullptr, bytes, (int64_t*)nullptr, (int64_t*)nullptr, (int64_t)0, (size_t)(n_result + 1),
                                         rocprim::plus<int64_t>(), s));
        if ((st = c->sort_tmp.ensure(bytes)) != PSFM_OK) return st;
        PSFM_HIP(rocprim::exclusive_scan(c->sort_tmp.p, bytes, c->scan_tmp.as<int64_t>(), c->rs_off.as<int64_t>(), (int64_t)0,
                                         (size_t)(n_result + 1), rocprim::plus<int64_t>(), s));
    }
    if (with_spans) {
        hipLaunchKernelGGL(psfm_rs_span_kernel, dim3(rs_grid(n)), dim3(PSFM_RS_BLOCK), 0, s, (const int*)g.ids, (const int*)g.s, (const int*)g.e,
                           n, (const int64_t*)c->rs_off.as<int64_t>(), g.verdict);
        PSFM_HIP(hipGetLastError());
    }
    PSFM_HIP(hipMemcpyAsync(h + 1, g.verdict + 1, 8, hipMemcpyDeviceToHost, s));
    PSFM_HIP(hipMemcpyAsync(h + 3, c->rs_off.as<int64_t>() + n_result, 8, hipMemcpyDeviceToHost, s));
    if (xy && n_points > 0) PSFM_HIP(hipMemcpyAsync(c->rs_xy.p, xy, 16 * (size_t)n_points, hipMemcpyDefault, s));
    PSFM_HIP(hipStreamSynchronize(s));
    if (h[1] != PSFM_RS_NONE) {
        psfm_set_error("%s: trajectory %lld is refused: %s (the context is untouched)", who, (long long)psfm_rs_verdict_index(h[1]),
                       rs_reason(psfm_rs_verdict_reason(h[1])));
        return PSFM_ERR_ARG;
    }
    if ((int64_t)h[3] != n_points) {
        psfm_set_error("%s: the lengths add up to %lld points, n_points is %lld (the context is untouched)", who, (long long)h[3],
                       (long long)n_points);
        return PSFM_ERR_ARG;
    }
    std::swap(c->res_birth, c->rs_birth);
    std::swap(c->res_len, c->rs_len);
    std::swap(c->res_off, c->rs_off);
    if (xy) std::swap(c->res_xy, c->rs_xy);
    rs_commit(c, n_result, xy ? n_points : 0, n_flows);
    *n_result_host = n_result;
    return PSFM_OK;
}

extern "C" psfm_status psfm_result_set(psfm_ctx* c, int64_t n_traj, int64_t n_points, const int32_t* ids, const int32_t* birth,
                                       const int32_t* len, const double* xy, int64_t* n_result_host, void* stream)
{
    const char* who = "psfm_result_set";
    if (!c) { psfm_set_error("ctx is NULL"); return PSFM_ERR_ARG; }
    if (!n_result_host) { psfm_set_error("%s: n_result_host is NULL", who); return PSFM_ERR_ARG; }
    if (n_traj < 0 || n_points < 0) {
        psfm_set_error("%s: negative size (n_traj=%lld n_points=%lld)", who, (long long)n_traj, (long long)n_points);
        return PSFM_ERR_ARG;
    }
    if ((n_traj > 0 && (!ids || !birth || !len)) || (n_points > 0 && !xy)) { psfm_set_error("%s: a NULL array that is not empty", who); return PSFM_ERR_ARG; }
    if (n_traj > (int64_t)PSFM_RS_ID_END) {
        psfm_set_error("%s: trajectory %lld is refused: %s", who, (long long)PSFM_RS_ID_END, rs_reason(PSFM_RS_BAD_ID));   // (ids ascend strictly)
        return PSFM_ERR_ARG;
    }
    if (n_traj == 0 && n_points != 0) { psfm_set_error("%s: the lengths add up to 0 points, n_points is %lld", who, (long long)n_points); return PSFM_ERR_ARG; }
    PSFM_HIP(hipSetDevice(c->device));
    PsfmGate gate(c->device, 0);
    hipStream_t s = (hipStream_t)stream;
    if (n_traj == 0) {
        PSFM_HIP(hipStreamSynchronize(s));
        rs_commit(c, 0, 0, 0);
        *n_result_host = 0;
        return PSFM_OK;
    }
    psfm_status st;
    RsStage g;
    if ((st = rs_stage(c, n_traj, g)) != PSFM_OK) return st;
    if ((st = rs_verdict_reset(g, s)) != PSFM_OK) return st;
    PSFM_HIP(hipMemcpyAsync(g.ids, ids, 4 * (size_t)n_traj, hipMemcpyDefault, s));
    PSFM_HIP(hipMemcpyAsync(g.birth, birth, 4 * (size_t)n_traj, hipMemcpyDefault, s));
    PSFM_HIP(hipMemcpyAsync(g.len, len, 4 * (size_t)n_traj, hipMemcpyDefault, s));
    return rs_core(c, who, g, n_traj, n_points, false, xy ? xy : (const double*)c->rs_ws.p /* (n_points == 0: nothing is read) */, n_result_host, s);
}

// ---- the file -----------------------------------------------------------------------------------------------------------------

namespace {
struct RsFd {
    int fd = -1;
    ~RsFd() { if (fd >= 0) close(fd); }
};
}  // namespace

extern "C" psfm_status psfm_load_track_npy(psfm_ctx* c, const char* path, const uint8_t* rec_template, int rec_size, const int32_t* field_at,
                                           int n_threads, int64_t* n_traj_host, int64_t* n_points_host, int64_t* n_result_host, void* stream)
{
    const char* who = "psfm_load_track_npy";
    if (!c) { psfm_set_error("ctx is NULL"); return PSFM_ERR_ARG; }
    if (!path || !rec_template || !field_at || !n_traj_host || !n_points_host || !n_result_host) { psfm_set_error("%s: NULL argument", who); return PSFM_ERR_ARG; }
    PsfmRsTemplate T;
    if (!psfm_rs_template_make(rec_template, rec_size, field_at, &T)) {
        psfm_set_error("%s: the record template must have 24 .. %d bytes and six 4-byte fields inside it that do not overlap (rec_size=%d)",
                       who, PSFM_RS_REC_MAX, rec_size);
        return PSFM_ERR_ARG;
    }
    RsFd f;
    f.fd = open(path, O_RDONLY);
    if (f.fd < 0) { psfm_set_error("%s: %s: %s", who, path, strerror(errno)); return PSFM_ERR_ARG; }
    struct stat sb;
    if (fstat(f.fd, &sb) != 0 || !S_ISREG(sb.st_mode)) { psfm_set_error("%s: %s is not a regular file", who, path); return PSFM_ERR_ARG; }
    const int64_t size = (int64_t)sb.st_size;
    uint8_t foot[PSFM_RS_FOOTER];
    PsfmRsFooter F;
    int code = PSFM_RS_FOOT_SHORT;
    if (size > PSFM_RS_FOOTER) {
        size_t have = 0;
        while (have < sizeof(foot)) {
            const ssize_t got = pread(f.fd, foot + have, sizeof(foot) - have, (off_t)(size - PSFM_RS_FOOTER + (int64_t)have));
            if (got < 0 && errno == EINTR) continue;
            if (got <= 0) break;
            have += (size_t)got;
        }
        if (have != sizeof(foot)) { psfm_set_error("%s: %s: cannot read the footer", who, path); return PSFM_ERR_ARG; }
        code = psfm_rs_footer_parse(foot, size, rec_size, &F);
    }
    if (code != PSFM_RS_FOOT_OK) { psfm_set_error("%s: %s: %s (the context is untouched)", who, path, psfm_rs_footer_what(code)); return PSFM_ERR_ARG; }
    if (F.n > (int64_t)PSFM_RS_ID_END) { psfm_set_error("%s: %s: more than 2^28 trajectories", who, path); return PSFM_ERR_ARG; }
    if (F.n == 0 && F.n_points != 0) { psfm_set_error("%s: %s: points without trajectories", who, path); return PSFM_ERR_ARG; }
    PSFM_HIP(hipSetDevice(c->device));
    PsfmGate gate(c->device, 0);
    hipStream_t s = (hipStream_t)stream;
    *n_traj_host = *n_points_host = *n_result_host = 0;
    if (F.n == 0) {
        PSFM_HIP(hipStreamSynchronize(s));
        rs_commit(c, 0, 0, 0);
        return PSFM_OK;
    }
    psfm_status st;
    std::string err;
    RsStage g;
    if ((st = rs_stage(c, F.n, g)) != PSFM_OK) return st;
    const size_t rec_bytes = (size_t)F.n * (size_t)rec_size;
    if ((st = c->rs_rec.ensure(rec_bytes + 64)) != PSFM_OK) return st;      // (the last vector of the last block ends inside)
    if ((st = psfm_ring_stream_file(c, who, f.fd, F.rec_start, rec_bytes, (char*)c->rs_rec.p, n_threads, s, err)) != PSFM_OK) {
        if (!err.empty()) psfm_set_error("%s: %s: the records: %s (the context is untouched)", who, path, err.c_str());
        return st;
    }
    if ((st = rs_verdict_reset(g, s)) != PSFM_OK) return st;
    hipLaunchKernelGGL(psfm_rs_decode_kernel, dim3(rs_grid(F.n)), dim3(PSFM_RS_BLOCK), 0, s, (const uint4*)c->rs_rec.p, (int64_t)0, F.n, T, g.ids,
                       g.birth, g.len, g.s, g.e, g.verdict);
    PSFM_HIP(hipGetLastError());
    int64_t n_result = 0;
    if ((st = rs_core(c, who, g, F.n, F.n_points, true, nullptr, &n_result, s)) != PSFM_OK) return st;
    // the metadata is in place; the points go straight into res_xy
    if ((st = c->res_xy.ensure(16 * (size_t)(F.n_points > 0 ? F.n_points : 1))) != PSFM_OK) { rs_commit(c, 0, 0, 0); return st; }
    if ((st = psfm_ring_stream_file(c, who, f.fd, F.xy_data, 16 * (size_t)F.n_points, (char*)c->res_xy.p, n_threads, s, err)) != PSFM_OK) {
        rs_commit(c, 0, 0, 0);
        if (!err.empty()) psfm_set_error("%s: %s: the points: %s; the previous result is gone and the context holds an EMPTY result", who, path, err.c_str());
        return st;
    }
    PSFM_HIP(hipStreamSynchronize(s));
    c->res_n_points = F.n_points;
    *n_traj_host = F.n; *n_points_host = F.n_points; *n_result_host = n_result;
    return PSFM_OK;
}
