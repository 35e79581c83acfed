// mipt_radiance.cpp -- the radiance-query entry points of include/mipt.h (mipt_query_radiance, mipt_query_radiance_device): argument
// checks, staging for the host entry and the launch of pt_kernel.hip's ray kernel -- the trace loop of the renders with the caller's
// rays as its source of work.  Host C++ only; every device operation is stream-ordered HIP.
#include "../../include/mipt.h"
#include "pt_kernel.h"
#include "mipt_scene.h"                                          // and with it mipt_host_util.h, mipt_internal.h

#include <cstring>

static_assert(sizeof(MiptRadianceOptions) == 64 && sizeof(MiptRay) == 32, "ABI struct sizes (tests/test_radiance_abi.py)");
static_assert(offsetof(MiptRay, reserved) == 28, "the seed is the last word of the ray record (pt_kernel.hip reads it as rays[2 i + 1].w)");

namespace {

using mipt::fail;

// everything that needs neither the scene's contents nor a device
int check(const char *who, const MiptScene *scene, const void *rays, uint64_t n_rays, const MiptRadianceOptions *opt, const void *radiance,
          bool device_entry) {
    if (!scene || !rays || !opt || !radiance) return fail(MIPT_ERR_INVALID_ARG, "%s: null scene, rays, options or radiance", who);
    int rc;
    if ((rc = mipt::ray_count_check(who, "n_rays", n_rays)) || (rc = mipt::ray_sampling_check(who, opt->samples, opt->max_ray_depth)) ||
        (rc = mipt::path_options_check(who, *opt)))
        return rc;
    return mipt::accum_check(who, opt->flags, device_entry ? nullptr : "mipt_query_radiance_device");
}

} // namespace

// the launch, with every argument already checked; d_rays / d_radiance in HBM of the scene's device
int mipt::radiance_launch(MiptScene *scene, const MiptRay *d_rays, uint64_t n_rays, const MiptRadianceOptions *opt, float *d_radiance,
                          hipStream_t stream, MiptStats *stats) {
    if (stats) memset(stats, 0, sizeof *stats);
    if (n_rays == 0) return MIPT_OK;
    MIPT_HIP(hipSetDevice(scene->device));

    mipt::DevParams pr{};
    pr.samples = opt->samples; pr.max_depth = opt->max_ray_depth;
    pr.sum_only = (opt->flags & MIPT_FLAG_SUM) ? 1u : 0u;
    pr.accumulate = (opt->flags & MIPT_FLAG_ACCUM) ? 1u : 0u;
    pr.total_work = n_rays;
    pr.samples_f = (float)opt->samples;                       // cpu.rs:60
    pr.cull_scale = 1.0f + opt->cull_margin;
    pr.service_num = 3; pr.service_den = 8; pr.leaf_den = 4u;   // the adaptive launch's schedule (mipt_adaptive.cpp render_launch)
    pr.hdr = d_radiance;
    pr.stats = scene->d_stats;

    const bool count = (opt->flags & MIPT_FLAG_COUNT) != 0;
    const bool cull = opt->traversal == MIPT_TRAVERSAL_CULLED;
    const int occ = mipt::trace_rays_blocks_per_cu(count, cull, (int)opt->shading);
    int bpc = occ;
    {   // few rays per lane: fewer co-resident waves, as for a batch launch
        const long long fit = (long long)(pr.total_work / (unsigned long long)(1.25 * scene->n_cu * mipt::kBlockThreads));
        const int cap = (int)(fit < 2 ? 2 : fit);
        if (cap < bpc) bpc = cap;
    }
    pr.leaf_period = (pr.total_work >= 4ull * (unsigned long long)scene->n_cu * (unsigned long long)occ * mipt::kBlockThreads) ? 4u : 1u;
    int grid = 0, rc = mipt::traversal_grid(scene, bpc, pr.total_work, &grid);
    if (rc) return rc;
    pr.ovf = scene->d_ovf;

    // no memset: every ray writes its slot
    mipt::DevStats hs;
    float ms = 0.0f;
    rc = mipt::traversal_launch(
        scene, stream,
        [&]() -> int {
            MIPT_HIP(mipt::launch_trace_rays(scene->dev, pr, reinterpret_cast<const float4 *>(d_rays), count, cull, (int)opt->shading, grid, stream));
            return MIPT_OK;
        },
        []() -> int { return MIPT_OK; }, hs, ms);
    if (rc && rc != MIPT_ERR_STACK) return rc;
    if (stats) mipt::stats_from_device(hs, ms, stats);
    return rc;                                                    // MIPT_OK, or MIPT_ERR_STACK with the results and the stats delivered
}

namespace {

using mipt::radiance_launch;

int radiance_device(MiptScene *scene, const MiptRay *d_rays, uint64_t n_rays, const MiptRadianceOptions *opt, float *d_radiance,
                    void *hip_stream, MiptStats *stats) {
    const char *who = "mipt_query_radiance_device";
    int rc = check(who, scene, d_rays, n_rays, opt, d_radiance, true);
    if (rc) return rc;
    const mipt::ItemBuffers b{"d_rays", d_rays, n_rays * sizeof(MiptRay), "d_radiance", d_radiance, n_rays * 12, 4, true, false};
    return mipt::device_call(who, scene, b, n_rays == 0, stats,
                             [&] { return radiance_launch(scene, d_rays, n_rays, opt, d_radiance, (hipStream_t)hip_stream, stats); });
}

int radiance_host(MiptScene *scene, const MiptRay *rays, uint64_t n_rays, const MiptRadianceOptions *opt, float *radiance, MiptStats *stats) {
    int rc = check("mipt_query_radiance", scene, rays, n_rays, opt, radiance, false);
    if (rc) return rc;
    if (n_rays == 0) return radiance_launch(scene, nullptr, 0, opt, nullptr, nullptr, stats);
    return mipt::staged_call(scene, rays, (size_t)n_rays * sizeof(MiptRay), radiance, (size_t)n_rays * 3 * sizeof(float),
                             [&](const void *d_rays, void *d_out) { return radiance_launch(scene, (const MiptRay *)d_rays, n_rays, opt, (float *)d_out, nullptr, stats); });
}

} // namespace

extern "C" {

int mipt_query_radiance(MiptScene *scene, const MiptRay *rays, uint64_t n_rays, const MiptRadianceOptions *opt, float *radiance, MiptStats *stats) {
    MIPT_NO_THROW(radiance_host(scene, rays, n_rays, opt, radiance, stats))
}
int mipt_query_radiance_device(MiptScene *scene, const MiptRay *d_rays, uint64_t n_rays, const MiptRadianceOptions *opt, float *d_radiance,
                               void *hip_stream, MiptStats *stats) {
    MIPT_NO_THROW(radiance_device(scene, d_rays, n_rays, opt, d_radiance, hip_stream, stats))
}

} // extern "C"
