// mipt_query.cpp -- the ray-query entry points of include/mipt.h (mipt_query_closest*, mipt_query_occluded*): argument checks,
// staging for the host entries and the launch of ray_query.hip's kernel.  Host C++ only; every device operation is stream-ordered HIP.
#include "../../include/mipt.h"
#include "pt_kernel.h"
#include "mipt_scene.h"                                          // and with it mipt_host_util.h, mipt_internal.h

#include <cmath>
#include <cstring>

static_assert(sizeof(MiptRay) == 32 && sizeof(MiptHit) == 16 && sizeof(MiptQueryOptions) == 32, "ABI struct sizes (tests/test_query_abi.py)");

namespace {

using mipt::fail;

// everything that needs neither the scene's contents nor a device
int validate(const char *who, const MiptScene *scene, const void *rays, const void *out, uint64_t n_rays, const MiptQueryOptions *opt) {
    if (!scene || !rays || !out) return fail(MIPT_ERR_INVALID_ARG, "%s: null scene, rays or output", who);
    if (n_rays >= MIPT_QUERY_MAX_RAYS) return fail(MIPT_ERR_INVALID_ARG, "%s: n_rays %llu: must stay below 2^31", who, (unsigned long long)n_rays);
    if (opt) {
        if (opt->traversal > MIPT_TRAVERSAL_CULLED) return fail(MIPT_ERR_INVALID_ARG, "%s: unknown traversal %u", who, opt->traversal);
        if (opt->flags & ~(uint32_t)MIPT_FLAG_COUNT) return fail(MIPT_ERR_INVALID_ARG, "%s: flags 0x%x: only MIPT_FLAG_COUNT is accepted", who, opt->flags);
        if (!(opt->cull_margin >= 0.0f) || !std::isfinite(opt->cull_margin))
            return fail(MIPT_ERR_INVALID_ARG, "%s: cull_margin must be finite and >= 0", who);
        for (uint32_t r : opt->reserved)
            if (r) return fail(MIPT_ERR_INVALID_ARG, "%s: reserved option fields must be 0", who);
    }
    return MIPT_OK;
}

using mipt::device_buffer_check;                               // mipt_host_util.h

// the launch, with every argument already checked; d_rays / d_out in HBM of the scene's device
int query_launch(MiptScene *scene, const MiptRay *d_rays, uint64_t n_rays, const MiptQueryOptions *opt, void *d_out, bool anyhit,
                 hipStream_t stream, MiptStats *stats) {
    if (stats) memset(stats, 0, sizeof *stats);
    if (n_rays == 0) return MIPT_OK;
    const bool count = opt && (opt->flags & MIPT_FLAG_COUNT) != 0;
    const bool cull = opt && opt->traversal == MIPT_TRAVERSAL_CULLED;
    MIPT_HIP(hipSetDevice(scene->device));

    mipt::DevQuery q{};
    q.rays = reinterpret_cast<const float4 *>(d_rays);
    q.out = d_out;
    q.tri_order = scene->d_tri_order;
    q.n_rays = n_rays;
    q.cull_scale = 1.0f + (opt ? opt->cull_margin : 0.0f);
    q.stats = scene->d_stats;

    int grid = 0, rc = mipt::traversal_grid(scene, mipt::query_blocks_per_cu(count, cull, anyhit), n_rays, &grid);
    if (rc) return rc;
    q.ovf = scene->d_ovf;

    mipt::DevStats hs;
    float ms = 0.0f;
    rc = mipt::traversal_launch(
        scene, stream,
        [&]() -> int {
            MIPT_HIP(mipt::launch_ray_query(scene->dev, q, count, cull, anyhit, (int)grid, stream));
            return MIPT_OK;
        },
        []() -> int { return MIPT_OK; }, hs, ms);
    if (rc && rc != MIPT_ERR_STACK) return rc;
    if (stats) {
        stats->kernel_ms = ms;
        stats->stack_overflows = hs.stack_overflows;
        if (count) {
            stats->rays = hs.rays; stats->inner_steps = hs.inner_steps; stats->tri_tests = hs.tri_tests;
            stats->hits = hs.hits; stats->max_stack = hs.max_stack;
        }
    }
    return rc;                                                    // MIPT_OK, or MIPT_ERR_STACK with the results and the stats delivered
}

int query_device(const char *who, MiptScene *scene, const MiptRay *d_rays, uint64_t n_rays, const MiptQueryOptions *opt, void *d_out,
                 bool anyhit, void *hip_stream, MiptStats *stats) {
    int rc = validate(who, scene, d_rays, d_out, n_rays, opt);
    if (rc) return rc;
    if (((uintptr_t)d_rays & 15u) || (!anyhit && ((uintptr_t)d_out & 15u)))
        return fail(MIPT_ERR_INVALID_ARG, "%s: %s must be 16-byte aligned", who, ((uintptr_t)d_rays & 15u) ? "d_rays" : "d_hits");
    if (n_rays == 0) return query_launch(scene, nullptr, 0, opt, nullptr, anyhit, nullptr, stats);       // MIPT_OK, no device work
    if ((rc = device_buffer_check(who, d_rays, scene->device, "d_rays"))) return rc;
    if ((rc = device_buffer_check(who, d_out, scene->device, anyhit ? "d_occluded" : "d_hits"))) return rc;
    return query_launch(scene, d_rays, n_rays, opt, d_out, anyhit, (hipStream_t)hip_stream, stats);
}

int query_host(const char *who, MiptScene *scene, const MiptRay *rays, uint64_t n_rays, const MiptQueryOptions *opt, void *out, bool anyhit,
               MiptStats *stats) {
    int rc = validate(who, scene, rays, out, n_rays, opt);
    if (rc) return rc;
    if (n_rays == 0) return query_launch(scene, nullptr, 0, opt, nullptr, anyhit, nullptr, stats);
    MIPT_HIP(hipSetDevice(scene->device));
    const size_t out_bytes = (size_t)n_rays * (anyhit ? 1u : sizeof(MiptHit));
    if ((rc = mipt::grow_device_buffer(&scene->d_qrays, &scene->qrays_bytes, (size_t)n_rays * sizeof(MiptRay)))) return rc;
    if ((rc = mipt::grow_device_buffer(&scene->d_qout, &scene->qout_bytes, out_bytes < 16 ? 16 : out_bytes))) return rc;
    MIPT_HIP(hipMemcpy(scene->d_qrays, rays, (size_t)n_rays * sizeof(MiptRay), hipMemcpyHostToDevice));
    rc = query_launch(scene, (const MiptRay *)scene->d_qrays, n_rays, opt, scene->d_qout, anyhit, nullptr, stats);
    if (rc && rc != MIPT_ERR_STACK) return rc;
    MIPT_HIP(hipMemcpy(out, scene->d_qout, out_bytes, hipMemcpyDeviceToHost));
    return rc;
}

} // namespace

extern "C" {

int mipt_query_closest(MiptScene *scene, const MiptRay *rays, uint64_t n_rays, const MiptQueryOptions *opt, MiptHit *hits, MiptStats *stats) {
    MIPT_NO_THROW(query_host("mipt_query_closest", scene, rays, n_rays, opt, hits, false, stats))
}
int mipt_query_closest_device(MiptScene *scene, const MiptRay *d_rays, uint64_t n_rays, const MiptQueryOptions *opt, MiptHit *d_hits,
                              void *hip_stream, MiptStats *stats) {
    MIPT_NO_THROW(query_device("mipt_query_closest_device", scene, d_rays, n_rays, opt, d_hits, false, hip_stream, stats))
}
int mipt_query_occluded(MiptScene *scene, const MiptRay *rays, uint64_t n_rays, const MiptQueryOptions *opt, uint8_t *occluded, MiptStats *stats) {
    MIPT_NO_THROW(query_host("mipt_query_occluded", scene, rays, n_rays, opt, occluded, true, stats))
}
int mipt_query_occluded_device(MiptScene *scene, const MiptRay *d_rays, uint64_t n_rays, const MiptQueryOptions *opt, uint8_t *d_occluded,
                               void *hip_stream, MiptStats *stats) {
    MIPT_NO_THROW(query_device("mipt_query_occluded_device", scene, d_rays, n_rays, opt, d_occluded, true, hip_stream, stats))
}

} // extern "C"
