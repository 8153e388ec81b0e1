// psfm_ingest.hip -- point_trajectory/utils.py:26-56 (load_flows / read_flo) for a whole stack, straight into HBM.
//
// A .flo file (Middlebury): 12-byte header {f32 magic 202021.25, i32 width, i32 height} + h * w interleaved (u, v) f32 pairs -- the
// layout the kernels read.  The Python mirror's ingest (reader threads -> pinned staging -> async H2D) moves a 1080p stack at 30-40 GB/s
// but pays ~100 us of interpreter work per FILE, which is what a stack of small frames is made of: 2 x 49 files of 3.3 MB (a DAVIS-sized
// sequence) took 15-18 ms = 18-21 GB/s, two thirds of that sequence's whole disk-to-disk time (profiles/r05/r05_k_e2e_small.txt).  Here the
// same pipeline without the interpreter: `n_threads` reader threads take files in order, read() each into its slot of a ring of pinned
// buffers owned by the context (a slot is reused once the copy that last read it has completed), and enqueue the H2D copy on the
// context's copy stream themselves; the caller's stream waits for the last copy.
#include <errno.h>
#include <fcntl.h>
#include <string.h>
#include <unistd.h>
#include <atomic>
#include <functional>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "psfm_internal.h"

namespace {
struct FloHeader { float magic; int32_t w, h; };
static_assert(sizeof(FloHeader) == 12, ".flo header");
}  // namespace

// The pipeline itself, for any list of items that fit a slot: `n_threads` reader threads take items in order, fill(i, slot, &bytes, err)
// reads item i into its slot of the ring of pinned buffers owned by the context (a slot is reused once the copy that last read it has
// completed) and the thread enqueues the copy of `bytes` bytes to dst(i) on one of the context's copy streams itself.  Returns when
// the last copy has completed; `s` only orders the copies behind what the caller enqueued.  A fill that returns false ends the call
// with PSFM_ERR_ARG and its message in `err` (the caller words the error); the caller holds the device gate.
psfm_status psfm_ring_stream(psfm_ctx* c, const char* who, int64_t n, size_t bytes, int n_threads, hipStream_t s,
                             const std::function<bool(int64_t, char*, size_t*, std::string&)>& fill,
                             const std::function<char*(int64_t)>& dst, std::string& err)
{
    err.clear();
    if (n <= 0) return PSFM_OK;
    if (n_threads < 1) n_threads = 1;
    if (n_threads > 32) n_threads = 32;
    if ((int64_t)n_threads > n) n_threads = (int)n;
    // ---- the ring of pinned staging buffers (grow-only, owned by the context) ----
    int n_slots = 2 * n_threads;
    while (n_slots > 2 && (size_t)n_slots * bytes > ((size_t)1 << 30)) --n_slots;       // (at most 1 GiB of pinned memory)
    if ((int64_t)n_slots > n) n_slots = (int)n;
    if (c->ingest_slot_bytes < bytes || (int)c->ingest_slots.size() < n_slots) {
        for (void* p : c->ingest_slots) (void)hipHostFree(p);
        c->ingest_slots.clear();
        c->ingest_slot_bytes = 0;
        for (int k = 0; k < n_slots; ++k) {
            void* p = nullptr;
            if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) { psfm_set_error("%s: hipHostMalloc(%zu) failed", who, bytes); return PSFM_ERR_HIP; }
            c->ingest_slots.push_back(p);
        }
        c->ingest_slot_bytes = bytes;
    }
    n_slots = (int)c->ingest_slots.size() < n_slots ? (int)c->ingest_slots.size() : n_slots;
    if (!c->copy_stream) PSFM_HIP(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    while ((int)c->ingest_events.size() < n_slots) {
        hipEvent_t e;
        PSFM_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        c->ingest_events.push_back(e);
    }
    // two copy streams, the slots alternating between them: the runtime gives streams their own SDMA engine, and one engine moves
    // ~35 GB/s of a PCIe Gen5 x16 link's ~55 (PSFM_FLO_COPY_STREAMS=1: one stream, as in round 5)
    static const int n_copy_env = getenv("PSFM_FLO_COPY_STREAMS") ? atoi(getenv("PSFM_FLO_COPY_STREAMS")) : 2;
    const bool two = n_copy_env >= 2;
    if (two && !c->copy_stream2) PSFM_HIP(hipStreamCreateWithFlags(&c->copy_stream2, hipStreamNonBlocking));
    hipStream_t cs = c->copy_stream;
    hipStream_t cs2 = two ? c->copy_stream2 : c->copy_stream;
    {   // the copies start behind whatever the caller has enqueued on `stream` (e.g. the allocation of dst on that stream)
        hipEvent_t e = c->prof.get();
        PSFM_HIP(hipEventRecord(e, s));
        PSFM_HIP(hipStreamWaitEvent(cs, e, 0));
        if (two) PSFM_HIP(hipStreamWaitEvent(cs2, e, 0));
        c->prof.pool.push_back(e);
    }
    // ---- the readers ----
    std::atomic<int64_t> next(0);
    std::atomic<bool> failed(false);
    std::mutex mu;
    std::condition_variable cv;
    std::vector<int64_t> enqueued((size_t)n_slots, -1);  // last item whose copy out of slot k has been enqueued (-1: the slot is fresh)
    bool hip_failed = false;
    const int device = c->device;
    auto fail = [&](const std::string& m, bool hip) {
        std::lock_guard<std::mutex> lk(mu);
        if (!failed.exchange(true)) { err = m; hip_failed = hip; }
        cv.notify_all();
    };
    auto worker = [&]() {
        if (hipSetDevice(device) != hipSuccess) { fail("hipSetDevice failed", true); return; }
        for (;;) {
            const int64_t i = next.fetch_add(1);
            if (i >= n || failed.load()) return;
            const int k = (int)(i % n_slots);
            if (i >= n_slots) {      // the slot's previous tenant: its copy must have been enqueued, then completed
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return enqueued[(size_t)k] == i - n_slots || failed.load(); });
                if (failed.load()) return;
                lk.unlock();
                if (hipEventSynchronize(c->ingest_events[(size_t)k]) != hipSuccess) { fail("hipEventSynchronize failed", true); return; }
            }
            char* slot = (char*)c->ingest_slots[(size_t)k];
            size_t have = 0;
            std::string why;
            if (!fill(i, slot, &have, why) || have > bytes) { fail(why.empty() ? "an item does not fit its slot" : why, false); return; }
            {   // copies are enqueued in any order (each waits only for its own slot); the event tells when the slot is free again
                std::lock_guard<std::mutex> lk(mu);
                hipStream_t q = (k & 1) ? cs2 : cs;
                if (hipMemcpyAsync(dst(i), slot, have, hipMemcpyHostToDevice, q) != hipSuccess ||
                    hipEventRecord(c->ingest_events[(size_t)k], q) != hipSuccess) {
                    if (!failed.exchange(true)) { err = "hipMemcpyAsync / hipEventRecord failed"; hip_failed = true; }
                    cv.notify_all();
                    return;
                }
                enqueued[(size_t)k] = i;
            }
            cv.notify_all();
        }
    };
    std::vector<std::thread> ths;
    // (a thread that cannot be created -- std::system_error -- must not unwind through the extern "C" entry point with joinable threads
    // behind it: the workers pull items from one queue, so the ones that did start, or this thread, read everything)
    for (int t = 0; t < n_threads; ++t) {
        try { ths.emplace_back(worker); } catch (const std::exception&) { break; }
    }
    if (ths.empty()) worker();
    for (auto& t : ths) t.join();
    // the staging buffers belong to the context: nothing may still read them when the call returns; `stream` continues behind the copies
    hipError_t e1 = hipStreamSynchronize(cs);
    if (two) { const hipError_t e2 = hipStreamSynchronize(cs2); if (e1 == hipSuccess) e1 = e2; }
    if (failed.load()) {
        if (hip_failed) { psfm_set_error("%s: %s", who, err.c_str()); return PSFM_ERR_HIP; }
        return PSFM_ERR_ARG;
    }
    PSFM_HIP(e1);
    return PSFM_OK;
}

// `nbytes` of an open file from `file_off` on into dst_dev, in chunks of 8 MiB through psfm_ring_stream (psfm_load_track_npy)
psfm_status psfm_ring_stream_file(psfm_ctx* c, const char* who, int fd, int64_t file_off, size_t nbytes, char* dst_dev, int n_threads,
                                  hipStream_t s, std::string& err)
{
    const size_t chunk = (size_t)8 << 20;
    const int64_t n = (int64_t)((nbytes + chunk - 1) / chunk);
    auto fill = [&](int64_t i, char* slot, size_t* have, std::string& why) {
        const size_t at = (size_t)i * chunk;
        const size_t want = nbytes - at < chunk ? nbytes - at : chunk;
        size_t got_all = 0;
        while (got_all < want) {
            const ssize_t got = pread(fd, slot + got_all, want - got_all, (off_t)(file_off + (int64_t)(at + got_all)));
            if (got < 0 && errno == EINTR) continue;
            if (got < 0) { why = std::string("read error: ") + strerror(errno); return false; }
            if (got == 0) break;
            got_all += (size_t)got;
        }
        if (got_all != want) { why = "the file ends inside the data (" + std::to_string(at + got_all) + " of " + std::to_string(nbytes) + " bytes)"; return false; }
        *have = want;
        return true;
    };
    return psfm_ring_stream(c, who, n, chunk, n_threads, s, fill, [&](int64_t i) { return dst_dev + (size_t)i * chunk; }, err);
}

extern "C" psfm_status psfm_load_flo_stack(psfm_ctx* c, const char* const* paths, int n, int h, int w, float* dst_dev, int n_threads, void* stream)
{
    if (!c || n < 0 || h < 1 || w < 1 || (n > 0 && (!paths || !dst_dev))) { psfm_set_error("psfm_load_flo_stack: bad argument (n=%d h=%d w=%d)", n, h, w); return PSFM_ERR_ARG; }
    if (n == 0) return PSFM_OK;
    PSFM_HIP(hipSetDevice(c->device));
    PsfmGate gate(c->device, 0);
    const size_t bytes = (size_t)h * w * 2 * sizeof(float);
    auto fill = [&](int64_t i, char* slot, size_t* have_out, std::string& why) {
        const char* path = paths[i];
        const int fd = open(path, O_RDONLY);
        if (fd < 0) { why = std::string(path) + ": " + strerror(errno); return false; }
        FloHeader hd;
        ssize_t got = read(fd, &hd, sizeof(hd));
        if (got != (ssize_t)sizeof(hd) || hd.magic != 202021.25f) { close(fd); why = std::string(path) + " does not start with the .flo magic number 202021.25"; return false; }
        if (hd.w != w || hd.h != h) {
            close(fd);
            why = std::string(path) + ": frame size " + std::to_string(hd.w) + " x " + std::to_string(hd.h) + " differs from the stack's " + std::to_string(w) + " x " + std::to_string(h);
            return false;
        }
        size_t have = 0;
        while (have < bytes) {
            got = read(fd, slot + have, bytes - have);
            if (got < 0 && errno == EINTR) continue;
            if (got <= 0) break;
            have += (size_t)got;
        }
        close(fd);
        if (have != bytes) { why = std::string(path) + ": truncated (" + std::to_string(have) + " of " + std::to_string(bytes) + " data bytes)"; return false; }
        *have_out = bytes;
        return true;
    };
    std::string err;
    const psfm_status st = psfm_ring_stream(c, "psfm_load_flo_stack", n, bytes, n_threads, (hipStream_t)stream, fill,
                                            [&](int64_t i) { return (char*)dst_dev + (size_t)i * bytes; }, err);
    if (st == PSFM_ERR_ARG) psfm_set_error("psfm_load_flo_stack: %s", err.c_str());
    return st;
}
