// mipt_internal.h -- functions shared between the translation units of libmipt.so.  None of them is exported: the library is built
// with -fvisibility=hidden and only the MIPT_API declarations of include/mipt.h leave it.  (Host C++ only: no HIP types here, so the
// CPU sanitizer builds of tests/cpp/ can include it.)
// The plumbing that needs no HIP type lives here: mipt::fail (defined below), the MIPT_NO_THROW fence, mipt::Owned, the owner of
// one handle, and mipt::Grown, the owner of a block that grows on demand.  The HIP-call macros and the HIP instances of both owners
// are in mipt_host_util.h.
#pragma once
#include "../../include/mipt.h"

#include <cstdarg>
#include <cstdio>
#include <exception>
#include <new>
#include <string>
#include <utility>

void mipt_internal_set_error(const char *msg);          // sets the calling thread's mipt_last_error() text (mipt_api.cpp)

namespace mipt {

// Sets the calling thread's mipt_last_error() text (printf-style, any length) and returns `code`.  Defined here, over
// mipt_internal_set_error, and not beside the text in mipt_api.cpp: obj_loader.cpp reports through it, and the CPU sanitizer build
// of tests/cpp/sanitize_host.cpp links the loader without mipt_api.cpp, with its own mipt_internal_set_error.
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
inline int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap, ap2;
    va_start(ap, fmt);
    va_copy(ap2, ap);
    const int n = vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (n >= (int)sizeof buf) {                          // a long path or a nested message: format again into a buffer that fits
        std::string big((size_t)n + 1, '\0');
        vsnprintf(&big[0], big.size(), fmt, ap2);
        mipt_internal_set_error(big.c_str());
    } else
        mipt_internal_set_error(n < 0 ? "" : buf);
    va_end(ap2);
    return code;
}

} // namespace mipt

// No C++ exception may cross the C ABI (the caller may be Rust or C): allocation failures become status codes.  The body of an
// extern "C" entry is `MIPT_NO_THROW(impl(args))`; MIPT_NO_THROW_AS names the status code (the loaders report MIPT_ERR_IO).
#define MIPT_NO_THROW_AS(code, call)                                                                                    \
    try { return call; }                                                                                               \
    catch (const std::bad_alloc &) { return mipt::fail(code, "out of host memory"); }                                  \
    catch (const std::exception &e) { return mipt::fail(code, "internal error: %s", e.what()); }
#define MIPT_NO_THROW(call) MIPT_NO_THROW_AS(MIPT_ERR_INVALID_ARG, call)

namespace mipt {

// The one owner of a handle that `Free` releases (a device pointer and hipFree, a stream and hipStreamDestroy, ...; the HIP instances
// are in mipt_host_util.h).  Move-only (the move operations delete the copies); empty (T{}) by default and after a move.  The
// destructor releases a non-empty handle exactly once and ignores Free's status.  Locals go in reverse order of declaration.
template <class T, auto Free>
class Owned {
  public:
    Owned() = default;
    explicit Owned(T h) : h_(h) {}
    Owned(Owned &&o) noexcept : h_(o.release()) {}
    Owned &operator=(Owned &&o) noexcept { if (this != &o) reset(o.release()); return *this; }
    ~Owned() { reset(); }
    T get() const { return h_; }
    operator T() const { return h_; }                            // a kernel argument, a HIP call's stream: used like the bare handle --
                                                                 // but NEVER handed to Free (hipFree(d_x)): reset() is the early release
    template <class U> explicit operator U *() const { return (U *)h_; }   // and cast like it: (const uint32_t *)d_geom
    explicit operator bool() const { return h_ != T{}; }
    T release() { const T h = h_; h_ = T{}; return h; }          // gives the handle up; nothing is freed
    void reset(T h = T{}) { if (h_ != T{}) (void)Free(h_); h_ = h; }
    T *put() { reset(); return &h_; }                            // for the call that allocates: hipStreamCreate(s.put())
  private:
    T h_{};
};

// The one owner of a block that grows on demand and lives as long as what holds it (a scene's workspace; the HIP instance is
// mipt::DevBuf in mipt_host_util.h).  Alloc(void **, bytes) returns 0 when it has stored a block, Free releases one.  Move-only;
// empty, with bytes() 0, by default and after a move.  Used like the bare pointer, and like Owned never handed to Free.
template <class T, auto Alloc, auto Free>
class Grown {
  public:
    Grown() = default;
    Grown(Grown &&o) noexcept : p_(std::move(o.p_)), bytes_(o.bytes_) { o.bytes_ = 0; }
    Grown &operator=(Grown &&o) noexcept {
        if (this != &o) { p_ = std::move(o.p_); bytes_ = o.bytes_; o.bytes_ = 0; }
        return *this;
    }
    T *get() const { return p_.get(); }
    operator T *() const { return p_.get(); }
    explicit operator bool() const { return (bool)p_; }
    size_t bytes() const { return bytes_; }
    // At least want_bytes afterwards, or Alloc's status and an empty owner.  A block that is large enough stays, pointer and all; one
    // that is too small is freed first and replaced: its contents are not kept.
    auto grow(size_t want_bytes) -> decltype(Alloc((void **)nullptr, want_bytes)) {
        if (p_ && bytes_ >= want_bytes) return {};
        reset();
        const auto status = Alloc((void **)p_.put(), want_bytes);
        if (status == decltype(status){}) bytes_ = want_bytes; else p_.release();     // a failed Alloc owes no block
        return status;
    }
    void reset() { p_.reset(); bytes_ = 0; }
  private:
    Owned<T *, Free> p_;
    size_t bytes_ = 0;
};

// ---- device-layout orders ----
// Number of breadth-first levels at the top of the pair-record order (scene_device.hip LevelOp; 8 ... 14 measure the same, 2.005 - 2.03 G
// line fills per frame of config M; 16: 2.20, 18: 2.31, 0: 2.23).
constexpr uint32_t kPairLayoutTop = 12;
inline uint32_t pair_order_top() { return kPairLayoutTop; }
// The host restatements of both orders -- NOT in libmipt.so: tests/cpp/layout_order.cpp, linked into libmipt_diag.so only, where they
// are the reference the layout kernels are checked against.
// Order of the 64-B pair records in HBM: order_out[j] = reference pair index of record j, 0xffffffff = pad record.
int pair_order(const MiptNode *nodes, uint32_t n_nodes, uint32_t *order_out, uint32_t cap, uint32_t *n_records_out);
// Slot of every triangle's 64-B record in the intersection stream.
int tri_slots(const MiptNode *nodes, uint32_t n_nodes, uint32_t n_tris, uint32_t *slot_out, uint32_t *n_slots_out);

// ---- scene_device.hip ----
// mipt_scene_create_from_triangles without the exception fence.
int scene_create_from_triangles(const MiptSceneDesc *desc, int device_id, MiptScene **out);
// the same with the caller's node array (ALREADY validated: mipt_scene_create's host checks) instead of a build; triangles in the tree's order
int scene_create_from_nodes(const MiptSceneDesc *desc, int device_id, MiptScene **out);

// mipt_scene_create_from_triangles from triangles that are in HBM of `device_id` already (scene_mesh.hip: the expanded mesh); they stay
// the caller's.  desc supplies the materials and textures only.
int scene_create_from_resident_triangles(const MiptSceneDesc *desc, const MiptTriangle *d_tris, uint32_t n_tris, int device_id, MiptScene **out);

// ---- scene_update.hip, used by mipt_multi.cpp ----
// mipt_scene_update_triangles without the exception fence
int scene_update_host(MiptScene *s, const MiptTriangle *tris, uint32_t n_tris, uint32_t mode, MiptUpdateInfo *info);
// dst := src's geometry by device-to-device copies (mipt_multi_update_triangles: the replicas after the root changed); a failed copy
// leaves dst as it was
int replica_refresh(const MiptScene *src, MiptScene *dst);

// ---- mipt_api.cpp, used by mipt_multi.cpp ----
// One scene on device_ids[0] -- from the caller's nodes or, with from_triangles, built on that device -- and device-to-device
// replicas on the others.
int scene_create_replicas(const MiptSceneDesc *desc, const int *device_ids, int n_dev, MiptScene **outs, bool from_triangles);
// the argument checks of mipt_render_batch* that need no device: scene, cameras, n_views, the options and the batch limits (used by
// mipt_adaptive.cpp, whose entries take the same arguments under the same rules)
int check_batch_args(const MiptScene *scene, const MiptCamera *cameras, uint32_t n_views, const MiptOptions *opt, const char *who);
// mipt_render_device with `pack_single`: honour MIPT_FLAG_PACKED also at tile_world == 1.
int render_device_impl(MiptScene *scene, const MiptCamera *camera, const MiptOptions *opt, float *d_hdr_rgb, uint8_t *d_rgba8,
                       void *hip_stream, MiptStats *stats, bool pack_single);

} // namespace mipt
