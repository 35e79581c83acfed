// mipt_query.cpp -- the ray-query entry points of include/mipt.h (mipt_query_closest*, mipt_query_occluded*): argument checks,
// staging for the host entries and the launch of ray_query.hip's kernel.  Host C++ only; every device operation is stream-ordered HIP.
#include "../../include/mipt.h"
#include "pt_kernel.h"
#include "mipt_scene.h"                                          // and with it mipt_host_util.h, mipt_internal.h

#include <cstring>

static_assert(sizeof(MiptRay) == 32 && sizeof(MiptHit) == 16 && sizeof(MiptQueryOptions) == 32, "ABI struct sizes (tests/test_query_abi.py)");

namespace {

using mipt::fail;

// everything that needs neither the scene's contents nor a device
int validate(const char *who, const MiptScene *scene, const void *rays, const void *out, uint64_t n_rays, const MiptQueryOptions *opt) {
    if (!scene || !rays || !out) return fail(MIPT_ERR_INVALID_ARG, "%s: null scene, rays or output", who);
    int rc = mipt::ray_count_check(who, "n_rays", n_rays);
    if (rc || !opt) return rc;
    return mipt::ray_options_check(who, *opt, nullptr, MIPT_FLAG_COUNT, "MIPT_FLAG_COUNT is");
}

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
    // overlapping d_rays and d_hits are not refused (a follow-up)
    const mipt::ItemBuffers b{"d_rays", d_rays, n_rays * sizeof(MiptRay), anyhit ? "d_occluded" : "d_hits", d_out, n_rays * (anyhit ? 1u : sizeof(MiptHit)),
                              anyhit ? 1u : 16u, false, false};
    return mipt::device_call(who, scene, b, n_rays == 0, stats,
                             [&] { return query_launch(scene, d_rays, n_rays, opt, d_out, anyhit, (hipStream_t)hip_stream, stats); });
}

int query_host(const char *who, MiptScene *scene, const MiptRay *rays, uint64_t n_rays, const MiptQueryOptions *opt, void *out, bool anyhit,
               MiptStats *stats) {
    int rc = validate(who, scene, rays, out, n_rays, opt);
    if (rc) return rc;
    if (n_rays == 0) return query_launch(scene, nullptr, 0, opt, nullptr, anyhit, nullptr, stats);
    return mipt::staged_call(scene, rays, (size_t)n_rays * sizeof(MiptRay), out, (size_t)n_rays * (anyhit ? 1u : sizeof(MiptHit)),
                             [&](const void *d_rays, void *d_out) { return query_launch(scene, (const MiptRay *)d_rays, n_rays, opt, d_out, anyhit, nullptr, stats); });
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
