// mipt_features.cpp -- the first-hit feature entry points of include/mipt.h (mipt_render_features, mipt_render_features_device):
// argument checks, device staging for the host entry, the camera table and the launch of first_hit.hip's kernel.  Host C++ only; every
// device operation is stream-ordered HIP.
#include "../../include/mipt.h"
#include "pt_kernel.h"
#include "mipt_scene.h"                                          // and with it mipt_host_util.h, mipt_internal.h

#include <cmath>
#include <cstring>

static_assert(sizeof(MiptFeatureBuffers) == 96, "ABI struct size (tests/test_features_model.py)");

namespace {

using mipt::fail;

constexpr int kBuffers = 8;
struct BufferField { const char *name; uint32_t words; };       // in the order of MiptFeatureBuffers; every value is 4 bytes
constexpr BufferField kFields[kBuffers] = {{"depth", 1}, {"prim", 1}, {"material", 1}, {"position", 3}, {"uv", 2}, {"normal", 3}, {"albedo", 3}, {"emission", 3}};

void unpack(const MiptFeatureBuffers *b, void *p[kBuffers]) {
    p[0] = b->depth; p[1] = b->prim; p[2] = b->material; p[3] = b->position; p[4] = b->uv; p[5] = b->normal; p[6] = b->albedo; p[7] = b->emission;
}

} // namespace

// the checks of a first-hit pass that concern neither its buffers nor a device (mipt_scene.h): mipt_render_features* and, with
// count_allowed = false, mipt_render_motion*
int mipt::first_hit_check(const char *who, const MiptScene *scene, const MiptCamera *cameras, uint32_t n_views, const MiptOptions *opt,
                          const void *buffers, bool count_allowed) {
    if (!scene || !cameras || !opt || !buffers) return fail(MIPT_ERR_INVALID_ARG, "%s: null scene, cameras, opt or buffers", who);
    if (n_views == 0) return fail(MIPT_ERR_INVALID_ARG, "%s: n_views == 0", who);
    if (opt->width == 0 || opt->height == 0) return fail(MIPT_ERR_INVALID_ARG, "%s: width and height must be greater than 0", who);
    if (opt->max_ray_depth == 0) return fail(MIPT_ERR_INVALID_ARG, "%s: max_ray_depth must be greater than 0", who);
    if (opt->samples == 0) return fail(MIPT_ERR_INVALID_ARG, "%s: samples must be greater than 0", who);
    if (opt->seed_mode > MIPT_SEED_PER_SAMPLE) return fail(MIPT_ERR_INVALID_ARG, "%s: unknown seed_mode %u", who, opt->seed_mode);
    if (opt->seed_mode == MIPT_SEED_PIXEL_STREAM && opt->samples != 1)
        return fail(MIPT_ERR_INVALID_ARG, "%s: samples %u with MIPT_SEED_PIXEL_STREAM: a pixel's second camera ray depends on how many numbers the "
                    "first sample's whole path drew, so only one sample is defined without path tracing (use MIPT_SEED_PER_SAMPLE)", who, opt->samples);
    if (opt->traversal > MIPT_TRAVERSAL_CULLED) return fail(MIPT_ERR_INVALID_ARG, "%s: unknown traversal %u", who, opt->traversal);
    if (!(opt->cull_margin >= 0.0f) || opt->cull_margin > 1.0f) return fail(MIPT_ERR_INVALID_ARG, "%s: cull_margin must be in [0, 1]", who);
    if (!count_allowed && opt->flags) return fail(MIPT_ERR_INVALID_ARG, "%s: flags 0x%x: no flag is accepted (MIPT_FLAG_COUNT included)", who, opt->flags);
    if (opt->flags & ~(uint32_t)MIPT_FLAG_COUNT) return fail(MIPT_ERR_INVALID_ARG, "%s: flags 0x%x: only MIPT_FLAG_COUNT is accepted", who, opt->flags);
    if (opt->tile_world > 1 || opt->tile_rank != 0)
        return fail(MIPT_ERR_INVALID_ARG, "%s: tile_rank %u / tile_world %u: a feature pass is not tile-sharded (tile_world 0 or 1)", who, opt->tile_rank, opt->tile_world);
    if (opt->shading != MIPT_SHADING_CPU)
        return fail(MIPT_ERR_INVALID_ARG, "%s: shading %u: only MIPT_SHADING_CPU; the first hit of the wgpu material model (normal maps, bilinear "
                    "sampler, cut-outs) is out of scope", who, opt->shading);
    for (uint32_t r : opt->reserved)
        if (r) return fail(MIPT_ERR_INVALID_ARG, "%s: reserved option fields must be 0", who);
    // seed wrap / absorbing zero seed, as mipt_render: index + 87636354 must stay below 2^31
    if ((uint64_t)opt->width * opt->height >= 2147483648ull - 87636354ull)
        return fail(MIPT_ERR_INVALID_ARG, "%s: width*height too large for the reference's 32-bit pixel seed", who);
    if ((uint64_t)n_views * opt->width * opt->height >= MIPT_BATCH_MAX_PIXELS)
        return fail(MIPT_ERR_INVALID_ARG, "%s: %u views of %ux%u: n_views*width*height must stay below 2^32", who, n_views, opt->width, opt->height);
    return MIPT_OK;
}

// what every first-hit launch needs besides its buffers (mipt_scene.h): the frame and tile constants, the grid with the scene's spill
// slots, and the camera table -- one 64-B record per view {look_at column 0, 1, 2, position}, copied on the launch stream
// (mipt_render_batch_device's).  The current device is the scene's.
int mipt::first_hit_setup(MiptScene *scene, const MiptCamera *cameras, uint32_t n_views, const MiptOptions *opt, int blocks_per_cu,
                          hipStream_t stream, DevFeatures *fp, int *grid_out) {
    mipt::DevFeatures &f = *fp;
    f.tri_order = scene->d_tri_order;
    f.width = opt->width; f.height = opt->height; f.samples = opt->samples; f.seed_mode = opt->seed_mode;
    f.sample_begin = opt->sample_begin ? opt->sample_begin : 1u;
    f.tiles_x = (opt->width + 7u) / 8u;
    f.n_tiles = f.tiles_x * ((opt->height + 7u) / 8u);
    f.tiles_recip = 0xffffffffu / f.n_tiles;
    f.view_pixels = opt->width * opt->height;
    f.total_work = (unsigned long long)f.n_tiles * 64ull * n_views;
    f.aspect = (float)opt->width / (float)opt->height;        // cpu.rs:34
    f.samples_f = (float)opt->samples;                        // cpu.rs:60
    f.cull_scale = 1.0f + opt->cull_margin;
    f.stats = scene->d_stats;

    int grid = 0, rc = mipt::traversal_grid(scene, blocks_per_cu, f.total_work, &grid);
    if (rc) return rc;
    f.ovf = scene->d_ovf;

    if ((rc = mipt::upload_camera_table(scene, cameras, n_views, stream))) return rc;
    f.cams = scene->d_cams;
    *grid_out = grid;
    return MIPT_OK;
}

namespace {

// everything that needs neither the scene's contents nor a device
int validate(const char *who, const MiptScene *scene, const MiptCamera *cameras, uint32_t n_views, const MiptOptions *opt,
             const MiptFeatureBuffers *out) {
    { const int rc = mipt::first_hit_check(who, scene, cameras, n_views, opt, out, true); if (rc) return rc; }
    for (const void *r : out->reserved)
        if (r) return fail(MIPT_ERR_INVALID_ARG, "%s: reserved buffer pointers must be NULL", who);
    void *p[kBuffers];
    unpack(out, p);
    bool any = false;
    for (void *q : p) any = any || q != nullptr;
    if (!any) return fail(MIPT_ERR_INVALID_ARG, "%s: no buffer wanted: at least one of depth, prim, material, position, uv, normal, albedo, emission must be set", who);
    return MIPT_OK;
}

using mipt::device_buffer_check;                               // mipt_host_util.h

// the launch, with every argument already checked; the wanted buffers in HBM of the scene's device
int features_launch(MiptScene *scene, const MiptCamera *cameras, uint32_t n_views, const MiptOptions *opt, const MiptFeatureBuffers *d_out,
                    hipStream_t stream, MiptStats *stats) {
    if (stats) memset(stats, 0, sizeof *stats);
    const bool count = (opt->flags & MIPT_FLAG_COUNT) != 0;
    const bool cull = opt->traversal == MIPT_TRAVERSAL_CULLED;
    MIPT_HIP(hipSetDevice(scene->device));

    mipt::DevFeatures f{};
    f.depth = d_out->depth; f.prim = d_out->prim; f.material = d_out->material; f.position = d_out->position;
    f.uv = d_out->uv; f.normal = d_out->normal; f.albedo = d_out->albedo; f.emission = d_out->emission;

    int grid = 0, rc = mipt::first_hit_setup(scene, cameras, n_views, opt, mipt::first_hit_blocks_per_cu(count, cull), stream, &f, &grid);
    if (rc) return rc;

    mipt::DevStats hs;
    float ms = 0.0f;
    rc = mipt::traversal_launch(
        scene, stream,
        [&]() -> int {
            MIPT_HIP(mipt::launch_first_hit(scene->dev, f, count, cull, grid, stream));
            return MIPT_OK;
        },
        []() -> int { return MIPT_OK; }, hs, ms);
    if (rc && rc != MIPT_ERR_STACK) return rc;
    if (stats) {
        stats->kernel_ms = ms;
        stats->stack_overflows = hs.stack_overflows;
        stats->tex_clamped = hs.tex_clamped;
        stats->pixels = hs.pixels;
        if (count) {
            stats->rays = hs.rays; stats->inner_steps = hs.inner_steps; stats->tri_tests = hs.tri_tests;
            stats->hits = hs.hits; stats->texel_fetches = hs.texel_fetches; stats->max_stack = hs.max_stack;
        }
    }
    return rc;                                                    // MIPT_OK, or MIPT_ERR_STACK with the buffers and the stats delivered
}

int features_device(MiptScene *scene, const MiptCamera *cameras, uint32_t n_views, const MiptOptions *opt, const MiptFeatureBuffers *d_out,
                    void *hip_stream, MiptStats *stats) {
    const char *who = "mipt_render_features_device";
    int rc = validate(who, scene, cameras, n_views, opt, d_out);
    if (rc) return rc;
    void *p[kBuffers];
    unpack(d_out, p);
    for (int i = 0; i < kBuffers; i++)
        if ((uintptr_t)p[i] & 3u) return fail(MIPT_ERR_INVALID_ARG, "%s: %s must be 4-byte aligned", who, kFields[i].name);
    for (int i = 0; i < kBuffers; i++)
        if (p[i] && (rc = device_buffer_check(who, p[i], scene->device, kFields[i].name))) return rc;
    return features_launch(scene, cameras, n_views, opt, d_out, (hipStream_t)hip_stream, stats);
}

int features_host(MiptScene *scene, const MiptCamera *cameras, uint32_t n_views, const MiptOptions *opt, const MiptFeatureBuffers *out,
                  MiptStats *stats) {
    int rc = validate("mipt_render_features", scene, cameras, n_views, opt, out);
    if (rc) return rc;
    MIPT_HIP(hipSetDevice(scene->device));
    const size_t n_pix = (size_t)n_views * opt->width * opt->height;
    void *h[kBuffers];
    unpack(out, h);
    mipt::DevPtr<uint32_t> dev[kBuffers];                         // one per wanted buffer, freed on every way out
    for (int i = 0; i < kBuffers; i++)
        if (h[i]) MIPT_HIP(dev[i].alloc(n_pix * kFields[i].words));
    MiptFeatureBuffers d{};
    d.depth = (float *)dev[0].get(); d.prim = dev[1].get(); d.material = dev[2].get(); d.position = (float *)dev[3].get();
    d.uv = (float *)dev[4].get(); d.normal = (float *)dev[5].get(); d.albedo = (float *)dev[6].get(); d.emission = (float *)dev[7].get();
    rc = features_launch(scene, cameras, n_views, opt, &d, nullptr, stats);
    if (rc && rc != MIPT_ERR_STACK) return rc;
    for (int i = 0; i < kBuffers; i++)
        if (h[i]) MIPT_HIP(hipMemcpy(h[i], dev[i].get(), n_pix * kFields[i].words * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return rc;
}

} // namespace

extern "C" {

int mipt_render_features(MiptScene *scene, const MiptCamera *cameras, uint32_t n_views, const MiptOptions *opt,
                         const MiptFeatureBuffers *host_out, MiptStats *stats) {
    MIPT_NO_THROW(features_host(scene, cameras, n_views, opt, host_out, stats))
}
int mipt_render_features_device(MiptScene *scene, const MiptCamera *cameras, uint32_t n_views, const MiptOptions *opt,
                                const MiptFeatureBuffers *device_out, void *hip_stream, MiptStats *stats) {
    MIPT_NO_THROW(features_device(scene, cameras, n_views, opt, device_out, hip_stream, stats))
}

} // extern "C"
