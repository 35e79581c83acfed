// mipt_adaptive.cpp -- the adaptive-sampling entry points of include/mipt.h (mipt_render_adaptive, mipt_render_adaptive_device,
// mipt_sample_map_workspace_bytes, mipt_sample_map, mipt_sample_map_device and their _fill forms): the render's argument checks, device
// staging and the launch of pt_kernel.hip's adaptive kernel; the sample map's plane table, the checks of its own options, the frame
// constants and the launches of sample_map.hip.  The checks every image-space entry makes, the device-entry checks and the host
// entry's staging are mipt_planes.h's and mipt_host_util.h's.  Host C++ only; every device operation is stream-ordered HIP.
#include "../../include/mipt.h"
#include "pt_kernel.h"
#include "mipt_scene.h"                                          // and with it mipt_host_util.h, mipt_internal.h

#include <cmath>
#include <cstring>

static_assert(sizeof(MiptSampleMapOptions) == 64 && sizeof(MiptSampleMapBuffers) == 64, "ABI struct sizes (tests/test_adaptive_abi.py)");
static_assert(sizeof(mipt::SampleMapWork) == 32, "mipt_sample_map_workspace_bytes");
static_assert(sizeof(MiptSampleMapFillOptions) == 64 && sizeof(mipt::SampleMapFillWork) == 32, "ABI struct size, mipt_sample_map_fill_workspace_bytes");

namespace {

using mipt::fail;

// ---------------------------------------------------------------------------------------------------------------------------------
// mipt_render_adaptive*
// ---------------------------------------------------------------------------------------------------------------------------------

// everything that needs no device; the buffers are only tested for null
int render_check(const char *who, const MiptScene *scene, const MiptCamera *cameras, uint32_t n_views, const MiptOptions *opt,
                 const uint32_t *counts, const uint8_t *rgba8) {
    const int rc = mipt::check_batch_args(scene, cameras, n_views, opt, who);
    if (rc) return rc;
    if (!counts) return fail(MIPT_ERR_INVALID_ARG, "%s: null counts", who);
    if (opt->flags & MIPT_FLAG_TOUCHED) return fail(MIPT_ERR_INVALID_ARG, "%s: MIPT_FLAG_TOUCHED: the line bitmap is a diagnostic of the plain launches", who);
    if ((opt->flags & MIPT_FLAG_ACCUM) && !(opt->flags & MIPT_FLAG_SUM))
        return fail(MIPT_ERR_INVALID_ARG, "MIPT_FLAG_ACCUM needs MIPT_FLAG_SUM (a running sum, divided once at the end)");
    if (rgba8 && (opt->flags & MIPT_FLAG_SUM))
        return fail(MIPT_ERR_INVALID_ARG, "RGBA8 output needs a full-frame mean buffer (not PACKED / SUM)");
    return MIPT_OK;
}

// the launch, with every argument already checked; all buffers in HBM of the scene's device
int render_launch(MiptScene *scene, const MiptCamera *cameras, uint32_t n_views, const MiptOptions *opt, const uint32_t *d_counts,
                  float *d_hdr_rgb, uint8_t *d_rgba8, hipStream_t stream, MiptStats *stats) {
    MIPT_HIP(hipSetDevice(scene->device));
    const uint64_t n_pix = (uint64_t)n_views * opt->width * opt->height;

    mipt::DevParams pr{};
    pr.width = opt->width; pr.height = opt->height; pr.samples = opt->samples; pr.max_depth = opt->max_ray_depth;
    pr.seed_mode = opt->shading == MIPT_SHADING_WGPU ? (uint32_t)MIPT_SEED_PER_SAMPLE : opt->seed_mode;   // the shader seeds per sample
    pr.sample_begin = opt->sample_begin ? opt->sample_begin : 1u;
    pr.sum_only = (opt->flags & MIPT_FLAG_SUM) ? 1u : 0u;
    pr.accumulate = (opt->flags & MIPT_FLAG_ACCUM) ? 1u : 0u;
    pr.tile_rank = 0u; pr.tile_world = 1u;
    pr.tiles_x = (opt->width + 7u) / 8u; pr.tiles_y = (opt->height + 7u) / 8u;
    pr.n_local_tiles = pr.tiles_x * pr.tiles_y;
    pr.total_work = (unsigned long long)pr.n_local_tiles * 64ull * n_views;
    pr.aspect = (float)opt->width / (float)opt->height;       // cpu.rs:34
    pr.samples_f = (float)opt->samples;                       // unused: the kernel divides by the pixel's own (float)n
    pr.cull_scale = 1.0f + opt->cull_margin;
    pr.service_num = 3; pr.service_den = 8; pr.leaf_den = 4u;   // the batch launch's schedule (mipt_api.cpp render_launch)
    pr.hdr = d_hdr_rgb;
    pr.stats = scene->d_stats;

    const bool count = (opt->flags & MIPT_FLAG_COUNT) != 0;
    const bool cull = opt->traversal == MIPT_TRAVERSAL_CULLED;
    const int occ = mipt::trace_adaptive_blocks_per_cu(count, cull, (int)opt->shading);
    int bpc = occ;
    {   // few pixels per lane: fewer co-resident waves, as for a batch launch
        const long long fit = (long long)(pr.total_work / (unsigned long long)(1.25 * scene->n_cu * mipt::kBlockThreads));
        const int cap = (int)(fit < 2 ? 2 : fit);
        if (cap < bpc) bpc = cap;
    }
    pr.leaf_period = (pr.total_work >= 4ull * (unsigned long long)scene->n_cu * (unsigned long long)occ * mipt::kBlockThreads) ? 4u : 1u;
    int grid = 0, rc = mipt::traversal_grid(scene, bpc, pr.total_work, &grid);
    if (rc) return rc;
    pr.ovf = scene->d_ovf;

    // the camera table of a batch launch: one 64-B record per view, copied on the launch stream
    if ((rc = mipt::upload_camera_table(scene, cameras, n_views, stream))) return rc;
    mipt::DevBatch bt{};
    bt.cams = scene->d_cams;
    bt.view_pixels = opt->width * opt->height;
    bt.tiles_recip = 0xffffffffu / pr.n_local_tiles;

    // a pixel without a sample is dropped at the fetch and never written: its +0 comes from here (a running sum stays as it is)
    if (!pr.accumulate) MIPT_HIP(hipMemsetAsync(d_hdr_rgb, 0, (size_t)n_pix * 3 * sizeof(float), stream));

    mipt::DevStats hs;
    float ms = 0.0f;
    rc = mipt::traversal_launch(
        scene, stream,
        [&]() -> int {
            MIPT_HIP(mipt::launch_trace_adaptive(scene->dev, pr, bt, d_counts, count, cull, (int)opt->shading, grid, stream));
            return MIPT_OK;
        },
        [&]() -> int {
            if (d_rgba8) MIPT_HIP(mipt::launch_tonemap(d_hdr_rgb, (unsigned long long)n_pix, 1.0f, d_rgba8, stream));
            return MIPT_OK;
        },
        hs, ms);
    if (rc && rc != MIPT_ERR_STACK) return rc;
    if (stats) mipt::stats_from_device(hs, ms, stats);
    return rc;                                                    // MIPT_OK, or MIPT_ERR_STACK with the frame and the stats delivered
}

int render_device(MiptScene *scene, const MiptCamera *cameras, uint32_t n_views, const MiptOptions *opt, const uint32_t *d_counts,
                  float *d_hdr_rgb, uint8_t *d_rgba8, void *hip_stream, MiptStats *stats) {
    const char *who = "mipt_render_adaptive_device";
    int rc = render_check(who, scene, cameras, n_views, opt, d_counts, d_rgba8);
    if (rc) return rc;
    if (!d_hdr_rgb) return fail(MIPT_ERR_INVALID_ARG, "%s: d_hdr_rgb == NULL", who);
    if ((uintptr_t)d_counts & 3u) return fail(MIPT_ERR_INVALID_ARG, "%s: counts must be 4-byte aligned", who);
    if ((uintptr_t)d_hdr_rgb & 3u) return fail(MIPT_ERR_INVALID_ARG, "%s: d_hdr_rgb must be 4-byte aligned", who);
    const uint64_t n_pix = (uint64_t)n_views * opt->width * opt->height;
    if (mipt::ranges_overlap(d_counts, n_pix * 4, d_hdr_rgb, n_pix * 12)) return fail(MIPT_ERR_INVALID_ARG, "%s: counts overlaps d_hdr_rgb", who);
    if (d_rgba8 && mipt::ranges_overlap(d_counts, n_pix * 4, d_rgba8, n_pix * 4)) return fail(MIPT_ERR_INVALID_ARG, "%s: counts overlaps d_rgba8", who);
    int device = -1;
    if ((rc = mipt::device_buffer_check(who, d_hdr_rgb, -1, "d_hdr_rgb", "", &device))) return rc;
    if ((rc = mipt::device_buffer_check(who, d_counts, device, "counts", "d_hdr_rgb's device"))) return rc;
    return render_launch(scene, cameras, n_views, opt, d_counts, d_hdr_rgb, d_rgba8, (hipStream_t)hip_stream, stats);
}

int render_host(MiptScene *scene, const MiptCamera *cameras, uint32_t n_views, const MiptOptions *opt, const uint32_t *counts,
                float *hdr_rgb, uint8_t *rgba8, MiptStats *stats) {
    const char *who = "mipt_render_adaptive";
    int rc = render_check(who, scene, cameras, n_views, opt, counts, rgba8);
    if (rc) return rc;
    if (opt->flags & MIPT_FLAG_ACCUM) return fail(MIPT_ERR_INVALID_ARG, "MIPT_FLAG_ACCUM needs a caller-owned device buffer: use mipt_render_adaptive_device");
    MIPT_HIP(hipSetDevice(scene->device));
    const uint64_t n_pix = (uint64_t)n_views * opt->width * opt->height;
    mipt::DevPtr<uint32_t> d_counts;                              // a local: freed on every way out
    MIPT_HIP(d_counts.alloc((size_t)n_pix));
    MIPT_HIP(hipMemcpy(d_counts.get(), counts, (size_t)n_pix * sizeof(uint32_t), hipMemcpyHostToDevice));
    if ((rc = scene->d_hdr.grow((size_t)n_pix * 3 * sizeof(float)))) return rc;
    uint8_t *d_rgba = nullptr;
    if (rgba8) {
        if ((rc = scene->d_rgba.grow((size_t)n_pix * 4))) return rc;
        d_rgba = scene->d_rgba;
    }
    rc = render_launch(scene, cameras, n_views, opt, d_counts.get(), scene->d_hdr, d_rgba, nullptr, stats);
    if (rc && rc != MIPT_ERR_STACK) return rc;
    if (hdr_rgb) MIPT_HIP(hipMemcpy(hdr_rgb, scene->d_hdr, (size_t)n_pix * 3 * sizeof(float), hipMemcpyDeviceToHost));
    if (rgba8) MIPT_HIP(hipMemcpy(rgba8, scene->d_rgba, (size_t)n_pix * 4, hipMemcpyDeviceToHost));
    return rc;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// mipt_sample_map*
// ---------------------------------------------------------------------------------------------------------------------------------

// in the order of MiptSampleMapBuffers
constexpr int kBuffers = 4;
constexpr mipt::Plane kPlanes[kBuffers] = {{"variance", 4, 4, true, mipt::kPlaneIn, -1}, {"hdr", 12, 4, false, mipt::kPlaneIn, -1},
                                           {"albedo", 12, 4, false, mipt::kPlaneIn, -1}, {"counts", 4, 4, true, mipt::kPlaneOut, -1}};
static_assert(kBuffers <= mipt::kMaxPlanes, "a PlaneSet holds the table");

// everything that needs no device: on success d holds the sizes and the frame constants T, E and the S == 0 share, set the caller's planes
int map_validate(const char *who, const MiptSampleMapOptions *opt, const MiptSampleMapBuffers *buf, mipt::DevSampleMap &d, mipt::PlaneSet &set) {
    int rc;
    if ((rc = mipt::not_null(who, opt, "opt")) || (rc = mipt::not_null(who, buf, "buffers"))) return rc;
    mipt::planes_bind(set, kPlanes, kBuffers, buf);
    if ((rc = mipt::planes_required(who, set))) return rc;
    if (buf->albedo && !buf->hdr) return fail(MIPT_ERR_INVALID_ARG, "%s: null hdr: albedo is given only with hdr", who);
    uint64_t n_pix = 0;
    if ((rc = mipt::frame_nonzero(who, opt->width, opt->height, opt->n_views)) ||
        (rc = mipt::frame_pixels(who, opt->width, opt->height, opt->n_views, &n_pix)) || (rc = mipt::flags_zero(who, opt->flags)) ||
        (rc = mipt::reserved_zero(who, opt->reserved, buf->reserved)))
        return rc;
    if (opt->max_samples < 1 || opt->max_samples > 65535) return fail(MIPT_ERR_INVALID_ARG, "%s: max_samples %u: must be 1 ... 65535", who, opt->max_samples);
    if (opt->min_samples > opt->max_samples)
        return fail(MIPT_ERR_INVALID_ARG, "%s: min_samples %u: must be at most max_samples %u", who, opt->min_samples, opt->max_samples);
    if (!std::isfinite(opt->budget) || !(opt->budget >= (float)opt->min_samples) || !(opt->budget <= (float)opt->max_samples))
        return fail(MIPT_ERR_INVALID_ARG, "%s: budget %g: must be finite and in [min_samples, max_samples] = [%u, %u]", who, (double)opt->budget,
                    opt->min_samples, opt->max_samples);
    mipt::planes_size(set, n_pix);
    if ((rc = mipt::planes_disjoint(who, set))) return rc;

    d = mipt::DevSampleMap{};
    d.n_pixels = n_pix;
    d.min_samples = opt->min_samples;
    d.span = opt->max_samples - opt->min_samples;
    // budget >= min_samples and min_samples * N < 2^48 is a binary64 number: the rounded product is not below it
    const uint64_t total = (uint64_t)std::floor((double)opt->budget * (double)n_pix);
    d.extra = total - (uint64_t)opt->min_samples * n_pix;
    const uint64_t share = d.extra / n_pix;
    d.uniform_extra = share < d.span ? (uint32_t)share : d.span;
    return MIPT_OK;
}

// the planes (the caller's, or the host entry's staged copies) and the launch: rounds == 0 = the plain map, whose workspace is one
// SampleMapWork; otherwise the fill form's `rounds` slots of the same 32 B
int map_launch(mipt::DevSampleMap &d, const void *const p[], void *workspace, uint32_t rounds, hipStream_t stream) {
    d.variance = (const float *)p[0]; d.hdr = (const float *)p[1]; d.albedo = (const float *)p[2]; d.counts = (uint32_t *)p[3];
    d.work = (mipt::SampleMapWork *)workspace;
    if (rounds) MIPT_HIP(mipt::launch_sample_map_fill(d, (mipt::SampleMapFillWork *)workspace, rounds, stream));
    else MIPT_HIP(mipt::launch_sample_map(d, stream));
    return MIPT_OK;
}
uint64_t map_workspace_bytes(uint32_t rounds) { return rounds ? sizeof(mipt::SampleMapFillWork) * rounds : sizeof(mipt::SampleMapWork); }

// what the fill entries check before the plain map's checks -- the two structs, `rounds` -- and their options as the plain map's for
// map_validate: the same fields in the same places
int fill_args(const char *who, const MiptSampleMapFillOptions *fill, const MiptSampleMapBuffers *buf, MiptSampleMapOptions &opt) {
    int rc;
    if ((rc = mipt::not_null(who, fill, "opt")) || (rc = mipt::not_null(who, buf, "buffers"))) return rc;
    if (fill->rounds < 1 || fill->rounds > mipt::kSampleMapMaxRounds)
        return fail(MIPT_ERR_INVALID_ARG, "%s: rounds %u: must be 1 ... %u", who, fill->rounds, mipt::kSampleMapMaxRounds);
    opt = MiptSampleMapOptions{};
    opt.width = fill->width; opt.height = fill->height; opt.n_views = fill->n_views; opt.flags = fill->flags;
    opt.min_samples = fill->min_samples; opt.max_samples = fill->max_samples; opt.budget = fill->budget;
    for (int i = 0; i < 8; i++) opt.reserved[i] = fill->reserved[i];
    return MIPT_OK;
}

// rounds == 0: mipt_sample_map_device; otherwise mipt_sample_map_fill_device
int map_device(const char *who, const MiptSampleMapOptions *opt, const MiptSampleMapBuffers *buf, uint32_t rounds, void *d_workspace,
               void *hip_stream) {
    mipt::DevSampleMap d;
    mipt::PlaneSet set;
    int rc = map_validate(who, opt, buf, d, set);
    if (rc) return rc;
    const mipt::Workspace ws = {d_workspace, 0, map_workspace_bytes(rounds), nullptr};
    if ((rc = mipt::device_entry_check(who, set, &ws))) return rc;
    return map_launch(d, set.ptr, d_workspace, rounds, (hipStream_t)hip_stream);
}

int map_host(const char *who, const MiptSampleMapOptions *opt, const MiptSampleMapBuffers *buf, uint32_t rounds, int device_id) {
    mipt::DevSampleMap d;
    mipt::PlaneSet set;
    int rc = map_validate(who, opt, buf, d, set);
    if (rc || (rc = mipt::select_device(who, device_id))) return rc;
    mipt::StagedPlanes staged;
    mipt::DevPtr<unsigned char> workspace;
    if ((rc = staged.stage(set))) return rc;
    MIPT_HIP(workspace.alloc(map_workspace_bytes(rounds)));
    if ((rc = map_launch(d, staged.ptr, workspace.get(), rounds, nullptr))) return rc;
    return staged.fetch(set);
}

int fill_host(const MiptSampleMapFillOptions *fill, const MiptSampleMapBuffers *buf, int device_id) {
    const char *who = "mipt_sample_map_fill";
    MiptSampleMapOptions opt;
    const int rc = fill_args(who, fill, buf, opt);
    return rc ? rc : map_host(who, &opt, buf, fill->rounds, device_id);
}

int fill_device(const MiptSampleMapFillOptions *fill, const MiptSampleMapBuffers *buf, void *d_workspace, void *hip_stream) {
    const char *who = "mipt_sample_map_fill_device";
    MiptSampleMapOptions opt;
    const int rc = fill_args(who, fill, buf, opt);
    return rc ? rc : map_device(who, &opt, buf, fill->rounds, d_workspace, hip_stream);
}

} // namespace

extern "C" {

int mipt_render_adaptive(MiptScene *scene, const MiptCamera *cameras, uint32_t n_views, const MiptOptions *opt, const uint32_t *counts,
                         float *hdr_rgb, uint8_t *rgba8, MiptStats *stats) {
    MIPT_NO_THROW(render_host(scene, cameras, n_views, opt, counts, hdr_rgb, rgba8, stats))
}
int mipt_render_adaptive_device(MiptScene *scene, const MiptCamera *cameras, uint32_t n_views, const MiptOptions *opt,
                                const uint32_t *d_counts, float *d_hdr_rgb, uint8_t *d_rgba8, void *hip_stream, MiptStats *stats) {
    MIPT_NO_THROW(render_device(scene, cameras, n_views, opt, d_counts, d_hdr_rgb, d_rgba8, hip_stream, stats))
}

uint64_t mipt_sample_map_workspace_bytes(uint32_t width, uint32_t height, uint32_t n_views) {
    return mipt::batch_pixels(width, height, n_views) ? sizeof(mipt::SampleMapWork) : 0u;
}
int mipt_sample_map(const MiptSampleMapOptions *opt, const MiptSampleMapBuffers *host, int device_id) {
    MIPT_NO_THROW(map_host("mipt_sample_map", opt, host, 0u, device_id))
}
int mipt_sample_map_device(const MiptSampleMapOptions *opt, const MiptSampleMapBuffers *device, void *d_workspace, void *hip_stream) {
    MIPT_NO_THROW(map_device("mipt_sample_map_device", opt, device, 0u, d_workspace, hip_stream))
}

uint64_t mipt_sample_map_fill_workspace_bytes(uint32_t width, uint32_t height, uint32_t n_views, uint32_t rounds) {
    if (rounds < 1 || rounds > mipt::kSampleMapMaxRounds || !mipt::batch_pixels(width, height, n_views)) return 0u;
    return sizeof(mipt::SampleMapFillWork) * rounds;
}
int mipt_sample_map_fill(const MiptSampleMapFillOptions *opt, const MiptSampleMapBuffers *host, int device_id) {
    MIPT_NO_THROW(fill_host(opt, host, device_id))
}
int mipt_sample_map_fill_device(const MiptSampleMapFillOptions *opt, const MiptSampleMapBuffers *device, void *d_workspace, void *hip_stream) {
    MIPT_NO_THROW(fill_device(opt, device, d_workspace, hip_stream))
}

} // extern "C"
