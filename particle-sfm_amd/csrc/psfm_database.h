// psfm_database.h -- the per-element rules that turn the match tables (psfm_matches.hip) into the rows of the COLMAP database, shared
// by the kernels (psfm_database.hip) and the host build of the CPU suite (tests/host/database_host.cpp through tests/host/shim).
// Reference: sfm/import_feature_matches.py:76-104 (import_keypoints_matches) writing through sfm/colmap_utils/database.py:181-225.
//
// KEYPOINT rule (:82-84, database.py:185).  The blob of an image is float32(xy + 0.5): the add in f64, then ONE round-to-nearest-even
// to f32 -- not an f32 add of the rounded coordinate.
//
// KEEP rule (:88-99).  The reference walks the images in the iteration order of its `image_ids` mapping, inside an image the pairs in
// dict order, and skips a pair whose unordered id pair was written before.  The reverse of (s, t) belongs to image t, so whether it
// was written before depends only on the order of the two images: directed pair (s, t) is dropped exactly when the reverse pair
// (t, s) exists in the table and pos[t] < pos[s], pos = position in that iteration order.  One binary search for t * n_img + s in the
// ascending pair_key.  A self pair (s == t) is its own reverse and pos[s] < pos[s] is false: kept.  With more than sample_k kept
// points in a trajectory the two directions hold different matches, so the reference loses data here; this reproduces it.
//
// ROW rule (database.py:113-116, :196-207).  pair_id = min(id_s, id_t) * (2^31 - 1) + max(id_s, id_t) in 64 bits; the rows are u32 and
// their two columns are swapped when id_s > id_t -- by COLMAP id, not by position or frame.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define PSFM_DB_MAX_IMAGE_ID 2147483647ll      // database.py:41; valid ids here: [1, 2^31 - 2]

struct PsfmDbRow { uint32_t a, b; };           // one match row as the blob holds it

__device__ __forceinline__ float psfm_db_keypoint(double v) { return (float)(v + 0.5); }

// is `key` in the ascending pair_key[0, n_pairs)?
__device__ __forceinline__ bool psfm_db_has_pair(const int64_t* __restrict__ pair_key, int64_t n_pairs, int64_t key)
{
    int64_t lo = 0, hi = n_pairs;      // first g with pair_key[g] >= key
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (pair_key[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo < n_pairs && pair_key[lo] == key;
}

// directed pair key = s * n_img + t (an entry of pair_key): is it written?  pos (n_img): position of an image in the iteration order
__device__ __forceinline__ bool psfm_db_keep(const int64_t* __restrict__ pair_key, int64_t n_pairs, int64_t n_img,
                                             const int32_t* __restrict__ pos, int64_t key)
{
    const int64_t s = key / n_img, t = key - s * n_img;
    if (!(pos[t] < pos[s])) return true;                    // (the common half, and every self pair: no search)
    return !psfm_db_has_pair(pair_key, n_pairs, t * n_img + s);
}

__device__ __forceinline__ bool psfm_db_swap(int32_t id_s, int32_t id_t) { return id_s > id_t; }

__device__ __forceinline__ int64_t psfm_db_pair_id(int32_t id_s, int32_t id_t)
{
    const int64_t lo = id_s < id_t ? id_s : id_t, hi = id_s < id_t ? id_t : id_s;
    return lo * PSFM_DB_MAX_IMAGE_ID + hi;
}

// the row [own keypoint index, other keypoint index] of the match table as the blob holds it
__device__ __forceinline__ PsfmDbRow psfm_db_row(int32_t own, int32_t other, bool swap)
{
    PsfmDbRow r;
    r.a = (uint32_t)(swap ? other : own);
    r.b = (uint32_t)(swap ? own : other);
    return r;
}
