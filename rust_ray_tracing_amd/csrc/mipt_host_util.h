// mipt_host_util.h -- the host plumbing every translation unit of libmipt.so shares and that needs HIP types: the HIP-call macro,
// the owners of device memory, pinned memory, streams and events, the scope guards and the grow-on-demand device buffer.  Internal;
// mipt_scene.h includes it.  What needs no HIP type -- mipt::fail, the MIPT_NO_THROW fence, mipt::Owned -- is in mipt_internal.h,
// which the CPU builds of tests/cpp/ include.
#pragma once
#include "mipt_internal.h"

#include <hip/hip_runtime.h>

#include <cstring>
#include <thread>

// A HIP call, or `return MIPT_ERR_HIP` with "<the call> failed: <HIP's text>" as mipt_last_error().  MIPT_HIP_OR first runs
// `cleanup`, an expression such as drain(m), for what is not a matter of ownership (mipt_multi.cpp: the other devices' streams).
// A file may set its own "%s ... %s" text before including this header.
#ifndef MIPT_HIP_FAIL_FMT
#define MIPT_HIP_FAIL_FMT "%s failed: %s"
#endif
#define MIPT_HIP(expr)                                                                                                  \
    do {                                                                                                               \
        hipError_t e__ = (expr);                                                                                       \
        if (e__ != hipSuccess) return mipt::fail(MIPT_ERR_HIP, MIPT_HIP_FAIL_FMT, #expr, hipGetErrorString(e__));      \
    } while (0)
#define MIPT_HIP_OR(cleanup, expr)                                                                                      \
    do {                                                                                                               \
        hipError_t e__ = (expr);                                                                                       \
        if (e__ != hipSuccess) { cleanup; return mipt::fail(MIPT_ERR_HIP, MIPT_HIP_FAIL_FMT, #expr, hipGetErrorString(e__)); } \
    } while (0)

namespace mipt {

// ---- owners: what a function holds for the length of a call, released on every way out (a return, a failed MIPT_HIP, an exception
// on its way to the C-ABI fence).  Release runs in reverse order of declaration: a function declares its events first, then its
// buffers, then its streams, and last a SyncOnExit where work may still be queued when it leaves, which therefore runs first. ----
template <class T> struct DevPtr : Owned<T *, hipFree> {         // alloc: `count` elements of device memory (current device)
    hipError_t alloc(size_t count) { return hipMalloc((void **)this->put(), count * sizeof(T)); }
};
template <class T> struct PinnedPtr : Owned<T *, hipHostFree> {
    hipError_t alloc(size_t count) { return hipHostMalloc((void **)this->put(), count * sizeof(T), hipHostMallocDefault); }
};
using Stream = Owned<hipStream_t, hipStreamDestroy>;
using Event = Owned<hipEvent_t, hipEventDestroy>;

// Waits, when the scope ends, for the work the scope queued: for one stream -- after hipSetDevice(set_device) if that is given -- or,
// made with kWholeDevice, for the whole current device.  dismiss(): the function has synchronised itself and succeeded.
class SyncOnExit {
  public:
    enum WholeDevice { kWholeDevice };
    explicit SyncOnExit(hipStream_t stream, int set_device = -1) : stream_(stream), device_(set_device) {}
    explicit SyncOnExit(WholeDevice) : whole_(true) {}
    SyncOnExit(const SyncOnExit &) = delete;
    ~SyncOnExit() {
        if (!armed_) return;
        if (device_ >= 0) (void)hipSetDevice(device_);
        (void)(whole_ ? hipDeviceSynchronize() : hipStreamSynchronize(stream_));
    }
    void dismiss() { armed_ = false; }
  private:
    hipStream_t stream_ = nullptr; int device_ = -1; bool whole_ = false, armed_ = true;
};

// a helper thread that is joined on every way out of the scope (a joinable std::thread's destructor calls std::terminate)
struct JoinOnExit { std::thread t; ~JoinOnExit() { if (t.joinable()) t.join(); } };

// *p holds at least want_bytes of device memory (current device) afterwards; a buffer that is too small is freed and replaced, its
// contents are not kept.  *have is its size in bytes.
inline int grow_device_buffer(void **p, size_t *have, size_t want_bytes) {
    if (*have >= want_bytes && *p) return MIPT_OK;
    if (*p) { (void)hipFree(*p); *p = nullptr; *have = 0; }
    MIPT_HIP(hipMalloc(p, want_bytes));
    *have = want_bytes;
    return MIPT_OK;
}

// n_views * width * height for the entries that take planes of n_views frames (denoise, temporal); 0 = an invalid size: a zero, or
// not below MIPT_BATCH_MAX_PIXELS
inline uint64_t batch_pixels(uint32_t width, uint32_t height, uint32_t n_views) {
    if (width == 0 || height == 0 || n_views == 0) return 0;
    const uint64_t wh = (uint64_t)width * height;                            // < 2^64
    if (wh >= MIPT_BATCH_MAX_PIXELS || wh * n_views >= MIPT_BATCH_MAX_PIXELS) return 0;
    return wh * n_views;
}

// do the byte ranges [a, a + a_bytes) and [b, b + b_bytes) share a byte
inline bool ranges_overlap(const void *a, uint64_t a_bytes, const void *b, uint64_t b_bytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

// MIPT_OK if `p` is device memory of HIP device `device`, else MIPT_ERR_INVALID_ARG with "<who>: <name> is not device memory of
// <whose> <device>".  device < 0: of any device.  *found (may be NULL) receives the device `p` lives on.
inline int device_buffer_check(const char *who, const void *p, int device, const char *name, const char *whose = "the scene's device",
                               int *found = nullptr) {
    hipPointerAttribute_t a;
    memset(&a, 0, sizeof a);
    const hipError_t e = hipPointerGetAttributes(&a, p);
    if (e != hipSuccess) (void)hipGetLastError();         // an unregistered host pointer is reported as an error: clear it
    if (e != hipSuccess || a.type != hipMemoryTypeDevice || (device >= 0 && a.device != device)) {
        if (device < 0) return fail(MIPT_ERR_INVALID_ARG, "%s: %s is not device memory", who, name);
        return fail(MIPT_ERR_INVALID_ARG, "%s: %s is not device memory of %s %d", who, name, whose, device);
    }
    if (found) *found = a.device;
    return MIPT_OK;
}

} // namespace mipt
