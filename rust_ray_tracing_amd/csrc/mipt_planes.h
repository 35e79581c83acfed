// mipt_planes.h -- what the image-space entries of include/mipt.h (denoise, variance filter, upsampling, temporal accumulation, sample
// map) share and that needs no device: the description of an entry's planes and the argument checks over it.  An entry file keeps its
// plane table, its own option checks and its launch; the order in which it calls the checks below is the order in which a caller sees
// them fire (tests/test_plane_entry_messages.py).  Host C++ only and no HIP type: tests/cpp/plane_checks.cpp builds it for the CPU.
// What needs HIP -- the device-entry checks and the staging of the host entries -- is at the end of mipt_host_util.h.
#pragma once
#include "mipt_internal.h"
#include "tile_shape.h"                                      // tiles_across, tiles_down: the kernels' tiles over a frame

#include <cmath>
#include <cstdint>
#include <cstring>

namespace mipt {

// n_views * width * height for the entries that take planes of n_views frames; 0 = an invalid size: a zero, or not below
// MIPT_BATCH_MAX_PIXELS
inline uint64_t batch_pixels(uint32_t width, uint32_t height, uint32_t n_views) {
    if (width == 0 || height == 0 || n_views == 0) return 0;
    const uint64_t wh = (uint64_t)width * height;                            // < 2^64
    if (wh >= MIPT_BATCH_MAX_PIXELS || wh * n_views >= MIPT_BATCH_MAX_PIXELS) return 0;
    return wh * n_views;
}

// do the byte ranges [a, a + a_bytes) and [b, b + b_bytes) share a byte.  The ends are formed in uintptr_t and wrap: a range that
// reaches past the top of the address space overlaps nothing above its start (no allocation is such a range).
inline bool ranges_overlap(const void *a, uint64_t a_bytes, const void *b, uint64_t b_bytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

// 1 / sigma^2 in f32 as include/mipt.h forms it; false unless sigma and the result are finite and greater than 0
inline bool inverse_square(float sigma, float *k) {
    if (!std::isfinite(sigma) || !(sigma > 0.0f)) return false;
    *k = 1.0f / (sigma * sigma);
    return std::isfinite(*k) && *k > 0.0f;
}

// One plane of an entry's buffers struct.  pixel_bytes: its size per pixel of the full frame (planes_bind sizes it; an entry sizes
// what is otherwise -- a low-resolution plane, a history -- itself).  over: for an output, the input plane it may be given as
// (out == hdr: the one alias allowed, and the host entry then writes the result over its copy of that input), else -1.
enum PlaneUse : uint8_t { kPlaneIn, kPlaneOut };
struct Plane { const char *name; uint32_t pixel_bytes; uint32_t align; bool required; PlaneUse use; int over; };

constexpr int kMaxPlanes = 12;
struct PlaneSet {
    const Plane *plane;                                          // the entry's table, in the order of its buffers struct
    int n;
    const void *ptr[kMaxPlanes];
    uint64_t bytes[kMaxPlanes];
};

// `set` over the first n pointers of a buffers struct (every Mipt*Buffers is its plane pointers, then `reserved`); no size yet
inline void planes_bind(PlaneSet &set, const Plane *table, int n, const void *buffers_struct) {
    set.plane = table; set.n = n;
    memcpy(set.ptr, buffers_struct, (size_t)n * sizeof(void *));
}
inline void planes_size(PlaneSet &set, uint64_t n_pix) {
    for (int i = 0; i < set.n; i++) set.bytes[i] = n_pix * set.plane[i].pixel_bytes;
}

// ---- the checks, each MIPT_OK or MIPT_ERR_INVALID_ARG with "<who>: ..." as mipt_last_error() ----
inline int not_null(const char *who, const void *p, const char *name) {
    return p ? MIPT_OK : fail(MIPT_ERR_INVALID_ARG, "%s: null %s", who, name);
}
inline int planes_required(const char *who, const PlaneSet &set) {
    for (int i = 0; i < set.n; i++)
        if (set.plane[i].required && !set.ptr[i]) return fail(MIPT_ERR_INVALID_ARG, "%s: null %s", who, set.plane[i].name);
    return MIPT_OK;
}
inline int frame_nonzero(const char *who, uint32_t width, uint32_t height, uint32_t n_views) {
    if (width == 0 || height == 0) return fail(MIPT_ERR_INVALID_ARG, "%s: width and height must be greater than 0", who);
    if (n_views == 0) return fail(MIPT_ERR_INVALID_ARG, "%s: n_views == 0", who);
    return MIPT_OK;
}
inline int frame_pixels(const char *who, uint32_t width, uint32_t height, uint32_t n_views, uint64_t *n_pix) {
    if ((*n_pix = batch_pixels(width, height, n_views)) == 0)
        return fail(MIPT_ERR_INVALID_ARG, "%s: %u views of %ux%u: n_views*width*height must stay below 2^32", who, n_views, width, height);
    return MIPT_OK;
}
inline int flags_zero(const char *who, uint32_t flags) {
    return flags ? fail(MIPT_ERR_INVALID_ARG, "%s: flags 0x%x: must be 0", who, flags) : MIPT_OK;
}
// the reserved words of the options, then the reserved pointers of the buffers
template <size_t NO, size_t NB>
int reserved_zero(const char *who, const uint32_t (&opt_reserved)[NO], void *const (&buf_reserved)[NB]) {
    for (uint32_t r : opt_reserved)
        if (r) return fail(MIPT_ERR_INVALID_ARG, "%s: reserved option fields must be 0", who);
    for (const void *r : buf_reserved)
        if (r) return fail(MIPT_ERR_INVALID_ARG, "%s: reserved buffer pointers must be NULL", who);
    return MIPT_OK;
}
// no two given planes share a byte, but for an output that is exactly the input it may go over
inline int planes_disjoint(const char *who, const PlaneSet &set) {
    const Plane *alias = nullptr;
    for (int i = 0; i < set.n; i++)
        if (set.plane[i].over >= 0) alias = &set.plane[i];
    for (int i = 0; i < set.n; i++)
        for (int j = i + 1; j < set.n; j++) {
            if (!set.ptr[i] || !set.ptr[j] || (set.plane[j].over == i && set.ptr[i] == set.ptr[j])) continue;
            if (!ranges_overlap(set.ptr[i], set.bytes[i], set.ptr[j], set.bytes[j])) continue;
            if (!alias) return fail(MIPT_ERR_INVALID_ARG, "%s: %s overlaps %s", who, set.plane[j].name, set.plane[i].name);
            return fail(MIPT_ERR_INVALID_ARG, "%s: %s overlaps %s (only %s == %s is allowed)", who, set.plane[j].name, set.plane[i].name, alias->name,
                        set.plane[alias->over].name);
        }
    return MIPT_OK;
}
// plane i sits where its table says it must (a device entry's check: kernels load whole words, the histories whole float4s)
inline int plane_aligned(const char *who, const PlaneSet &set, int i) {
    if ((uintptr_t)set.ptr[i] & (set.plane[i].align - 1u))
        return fail(MIPT_ERR_INVALID_ARG, "%s: %s must be %u-byte aligned", who, set.plane[i].name, set.plane[i].align);
    return MIPT_OK;
}

} // namespace mipt
