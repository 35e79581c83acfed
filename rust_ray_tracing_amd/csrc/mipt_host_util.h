// mipt_host_util.h -- the host plumbing every translation unit of libmipt.so shares and that needs HIP types: the HIP-call macro
// pair, the grow-on-demand device buffer and the launch scaffold of the traversal kernels.  Internal, like mipt_scene.h.  What needs
// no HIP type -- mipt::fail, the MIPT_NO_THROW fence -- is in mipt_internal.h, which the CPU builds of tests/cpp/ include.
#pragma once
#include "mipt_internal.h"
#include "mipt_scene.h"

// A HIP call, or `return MIPT_ERR_HIP` with "<the call> failed: <HIP's text>" as mipt_last_error().  MIPT_HIP_OR first runs
// `cleanup`, an expression such as cleanup() or drain(m).  A file may set its own "%s ... %s" text before including this header.
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

// *p holds at least want_bytes of device memory (current device) afterwards; a buffer that is too small is freed and replaced, its
// contents are not kept.  *have is its size in bytes.
inline int grow_device_buffer(void **p, size_t *have, size_t want_bytes) {
    if (*have >= want_bytes && *p) return MIPT_OK;
    if (*p) { (void)hipFree(*p); *p = nullptr; *have = 0; }
    MIPT_HIP(hipMalloc(p, want_bytes));
    *have = want_bytes;
    return MIPT_OK;
}

// ---- the launch scaffold of the traversal kernels (mipt_api.cpp: the trace kernels; mipt_query.cpp: the ray queries) ----
// Renders and queries of one scene share its workspace: d_stats, the events and the spill slots of the traversal stack (d_ovf, one
// set per wave of the grid).  These two functions are the only code that sizes, grows and hands out that workspace.
//
// The grid of a launch: n_cu x blocks_per_cu blocks, at most ceil(work / kBlockThreads), at least 1; the scene's spill slots are
// grown to the grid's wave count (the current device is the scene's).
inline int traversal_grid(MiptScene *scene, int blocks_per_cu, unsigned long long work, int *grid_out) {
    long long grid = (long long)scene->n_cu * blocks_per_cu;
    const long long need_blocks = (long long)((work + kBlockThreads - 1) / kBlockThreads);
    if (grid > need_blocks) grid = need_blocks;
    if (grid < 1) grid = 1;
    const size_t waves = (size_t)grid * kWavesPerBlock;
    if (waves > scene->ovf_waves) {
        if (scene->d_ovf) { (void)hipFree(scene->d_ovf); scene->d_ovf = nullptr; scene->ovf_waves = 0; }
        MIPT_HIP(hipMalloc((void **)&scene->d_ovf, waves * (size_t)mipt::kStackOvf * 64 * sizeof(uint32_t)));
        scene->ovf_waves = waves;
    }
    *grid_out = (int)grid;
    return MIPT_OK;
}

// One timed launch on `stream`: d_stats zeroed, ev0, launch(), ev1, after_ev1(), the counters copied to `hs`, the stream
// synchronised, `ms` = ev0 ... ev1 (the kernel alone).  `launch` and `after_ev1` queue their work on `stream` and return a status.
// MIPT_ERR_STACK (hs and ms are valid, the results are written) when a traversal stack overflowed.
template <class Launch, class After>
int traversal_launch(MiptScene *scene, hipStream_t stream, Launch launch, After after_ev1, DevStats &hs, float &ms) {
    int rc;
    MIPT_HIP(hipMemsetAsync(scene->d_stats, 0, sizeof(mipt::DevStats), stream));
    MIPT_HIP(hipEventRecord(scene->ev0, stream));
    if ((rc = launch())) return rc;
    MIPT_HIP(hipEventRecord(scene->ev1, stream));
    if ((rc = after_ev1())) return rc;
    MIPT_HIP(hipMemcpyAsync(&hs, scene->d_stats, sizeof hs, hipMemcpyDeviceToHost, stream));
    MIPT_HIP(hipStreamSynchronize(stream));
    MIPT_HIP(hipEventElapsedTime(&ms, scene->ev0, scene->ev1));
    if (hs.stack_overflows)
        return fail(MIPT_ERR_STACK, "traversal stack overflowed %llu times (capacity %d; the reference panics at 32, ray.rs:85)",
                    hs.stack_overflows, kStackLds + kStackOvf);
    return MIPT_OK;
}

} // namespace mipt
