// mipt_host_util.h -- the host plumbing every translation unit of libmipt.so shares and that needs HIP types: the HIP-call macro,
// the owners of device memory, pinned memory, streams and events, the scope guards, the grow-on-demand device buffer and, at the
// end, the device half of an image-space entry: its device-entry checks and the staging of its host entry.  Internal; mipt_scene.h
// includes it.  What needs no HIP type -- mipt::fail, the MIPT_NO_THROW fence, mipt::Owned and mipt::Grown in mipt_internal.h, the
// plane description and its checks in mipt_planes.h, the option checks of the ray entries in mipt_rays.h -- is what the CPU builds of
// tests/cpp/ include.
#pragma once
#include "mipt_planes.h"                                         // and with it mipt_internal.h
#include "mipt_rays.h"

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

// ---- what lives as long as a scene or a multi-GPU handle: a device buffer that grows on demand.  grow(): at least want_bytes of
// device memory (current device) afterwards; a buffer that is too small is freed and replaced, its contents are not kept.  bytes()
// is its size.  Freed with its holder. ----
inline hipError_t device_alloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
template <class T> struct DevBuf : Grown<T, device_alloc, hipFree> {
    int grow(size_t want_bytes) {
        const hipError_t e = Grown<T, device_alloc, hipFree>::grow(want_bytes);
        if (e != hipSuccess) return fail(MIPT_ERR_HIP, MIPT_HIP_FAIL_FMT, "hipMalloc(p, want_bytes)", hipGetErrorString(e));
        return MIPT_OK;
    }
};

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

// ---- the device half of an image-space entry (mipt_planes.h has the plane description and what needs no device) ----
// The workspace a device entry is handed.  `need` bytes of it are used; sizer: the entry's *_workspace_bytes function, which the
// caller is told of when `bytes` is less (null: the entry is not given a size).
struct Workspace { const void *p; uint64_t bytes, need; const char *sizer; };

// What a device entry checks after mipt_planes.h's: the workspace (if the entry takes one) is there, large enough and 16-byte
// aligned, every plane is aligned and apart from it, and all of it is memory of one device -- the first plane's, which becomes the
// current device.
inline int device_entry_check(const char *who, const PlaneSet &set, const Workspace *ws) {
    if (ws) {
        if (!ws->p) return fail(MIPT_ERR_INVALID_ARG, "%s: null workspace", who);
        if (ws->sizer && ws->bytes < ws->need)
            return fail(MIPT_ERR_INVALID_ARG, "%s: workspace of %llu bytes is too small: %s() is %llu", who, (unsigned long long)ws->bytes, ws->sizer,
                        (unsigned long long)ws->need);
        if ((uintptr_t)ws->p & 15u) return fail(MIPT_ERR_INVALID_ARG, "%s: workspace must be 16-byte aligned", who);
    }
    int rc, device = -1;
    for (int i = 0; i < set.n; i++) {
        if ((rc = plane_aligned(who, set, i))) return rc;
        if (ws && set.ptr[i] && ranges_overlap(set.ptr[i], set.bytes[i], ws->p, ws->need))
            return fail(MIPT_ERR_INVALID_ARG, "%s: %s overlaps the workspace", who, set.plane[i].name);
    }
    if ((rc = device_buffer_check(who, set.ptr[0], -1, set.plane[0].name, "", &device))) return rc;
    const std::string whose = std::string(set.plane[0].name) + "'s device";
    for (int i = 1; i < set.n; i++)
        if (set.ptr[i] && (rc = device_buffer_check(who, set.ptr[i], device, set.plane[i].name, whose.c_str()))) return rc;
    if (ws && (rc = device_buffer_check(who, ws->p, device, "workspace", whose.c_str()))) return rc;
    MIPT_HIP(hipSetDevice(device));
    return MIPT_OK;
}

// the device a host entry was asked for becomes the current one
inline int select_device(const char *who, int device_id) {
    const hipError_t e = hipSetDevice(device_id);
    if (e == hipSuccess) return MIPT_OK;
    (void)hipGetLastError();                                      // or the next launch of this thread would report this ordinal's error
    return fail(MIPT_ERR_HIP, "%s: hipSetDevice(device_id = %d) failed: %s", who, device_id, hipGetErrorString(e));
}

// The planes of a host entry in memory of the current device, freed when it goes out of scope.  stage(): every given plane gets its
// bytes and the inputs are copied in; an output that may go over an input (Plane::over) gets none and is that input's copy.  ptr[] is
// then what PlaneSet::ptr is for a device entry.  fetch(), after the launches on the null stream: the outputs back to the caller's
// planes; each copy blocks until the launches are done.
struct StagedPlanes {
    DevPtr<unsigned char> mem[kMaxPlanes];
    void *ptr[kMaxPlanes] = {};

    int stage(const PlaneSet &set) {
        for (int i = 0; i < set.n; i++) {
            if (!set.ptr[i] || set.plane[i].over >= 0) continue;
            MIPT_HIP(mem[i].alloc(set.bytes[i]));
            if (set.plane[i].use == kPlaneIn) MIPT_HIP(hipMemcpy(mem[i].get(), set.ptr[i], set.bytes[i], hipMemcpyHostToDevice));
        }
        for (int i = 0; i < set.n; i++) ptr[i] = mem[set.plane[i].over >= 0 ? set.plane[i].over : i].get();
        return MIPT_OK;
    }
    int fetch(const PlaneSet &set) const {
        for (int i = 0; i < set.n; i++)
            if (set.ptr[i] && set.plane[i].use == kPlaneOut) MIPT_HIP(hipMemcpy((void *)set.ptr[i], ptr[i], set.bytes[i], hipMemcpyDeviceToHost));
        return MIPT_OK;
    }
};

} // namespace mipt
