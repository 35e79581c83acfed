// mipt_adaptive.cpp -- the adaptive-sampling entry points of include/mipt.h (mipt_render_adaptive, mipt_render_adaptive_device,
// mipt_sample_map_workspace_bytes, mipt_sample_map, mipt_sample_map_device and their _fill forms): argument checks, device staging for the host entries, the
// camera table and the launches of pt_kernel.hip's adaptive kernel and of sample_map.hip.  Host C++ only; every device operation is
// stream-ordered HIP.
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
    scene->h_cams.assign((size_t)n_views * 4, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    for (uint32_t v = 0; v < n_views; v++) {
        const MiptCamera &c = cameras[v];
        for (int col = 0; col < 3; col++) scene->h_cams[(size_t)v * 4 + col] = make_float4(c.look_at[col][0], c.look_at[col][1], c.look_at[col][2], 0.0f);
        scene->h_cams[(size_t)v * 4 + 3] = make_float4(c.position.x, c.position.y, c.position.z, 0.0f);
    }
    const size_t cam_bytes = scene->h_cams.size() * sizeof(float4);
    if ((rc = mipt::grow_device_buffer((void **)&scene->d_cams, &scene->cams_bytes, cam_bytes))) return rc;
    MIPT_HIP(hipMemcpyAsync(scene->d_cams, scene->h_cams.data(), cam_bytes, hipMemcpyHostToDevice, stream));
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
    if (stats) {
        memset(stats, 0, sizeof *stats);
        stats->kernel_ms = ms;
        stats->rays = hs.rays; stats->inner_steps = hs.inner_steps; stats->tri_tests = hs.tri_tests;
        stats->hits = hs.hits; stats->texel_fetches = hs.texel_fetches; stats->stack_overflows = hs.stack_overflows;
        stats->tex_clamped = hs.tex_clamped; stats->max_stack = hs.max_stack; stats->pixels = hs.pixels;
        stats->diag[0] = hs.d_iters; stats->diag[1] = hs.d_inner_lanes; stats->diag[2] = hs.d_leaf_lanes;
        stats->diag[3] = hs.d_iters_inner; stats->diag[4] = hs.d_iters_leaf; stats->diag[5] = hs.d_services;
        stats->diag[6] = hs.d_service_lanes; stats->diag[7] = hs.d_cycles_service; stats->diag[8] = hs.d_cycles_total; stats->diag[9] = hs.d_cycles_mem; stats->diag[10] = hs.d_cycles_tail;
    }
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
    if ((rc = mipt::grow_device_buffer((void **)&scene->d_hdr, &scene->hdr_bytes, (size_t)n_pix * 3 * sizeof(float)))) return rc;
    uint8_t *d_rgba = nullptr;
    if (rgba8) {
        if ((rc = mipt::grow_device_buffer((void **)&scene->d_rgba, &scene->rgba_bytes, (size_t)n_pix * 4))) return rc;
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

constexpr int kBuffers = 4, kVariance = 0, kHdrBuf = 1, kAlbedo = 2, kCounts = 3;
struct BufferField { const char *name; uint32_t words; };           // in the order of MiptSampleMapBuffers; every value is 4 bytes
constexpr BufferField kFields[kBuffers] = {{"variance", 1}, {"hdr", 3}, {"albedo", 3}, {"counts", 1}};

void unpack(const MiptSampleMapBuffers *b, const void *p[kBuffers]) { p[0] = b->variance; p[1] = b->hdr; p[2] = b->albedo; p[3] = b->counts; }

// everything that needs no device: on success d holds the sizes and the frame constants T, E and the S == 0 share
int map_validate(const char *who, const MiptSampleMapOptions *opt, const MiptSampleMapBuffers *buf, mipt::DevSampleMap &d) {
    if (!opt) return fail(MIPT_ERR_INVALID_ARG, "%s: null opt", who);
    if (!buf) return fail(MIPT_ERR_INVALID_ARG, "%s: null buffers", who);
    if (!buf->variance) return fail(MIPT_ERR_INVALID_ARG, "%s: null variance", who);
    if (!buf->counts) return fail(MIPT_ERR_INVALID_ARG, "%s: null counts", who);
    if (buf->albedo && !buf->hdr) return fail(MIPT_ERR_INVALID_ARG, "%s: null hdr: albedo is given only with hdr", who);
    if (opt->width == 0 || opt->height == 0) return fail(MIPT_ERR_INVALID_ARG, "%s: width and height must be greater than 0", who);
    if (opt->n_views == 0) return fail(MIPT_ERR_INVALID_ARG, "%s: n_views == 0", who);
    const uint64_t n_pix = mipt::batch_pixels(opt->width, opt->height, opt->n_views);
    if (n_pix == 0)
        return fail(MIPT_ERR_INVALID_ARG, "%s: %u views of %ux%u: n_views*width*height must stay below 2^32", who, opt->n_views, opt->width, opt->height);
    if (opt->flags) return fail(MIPT_ERR_INVALID_ARG, "%s: flags 0x%x: must be 0", who, opt->flags);
    for (uint32_t r : opt->reserved)
        if (r) return fail(MIPT_ERR_INVALID_ARG, "%s: reserved option fields must be 0", who);
    for (const void *r : buf->reserved)
        if (r) return fail(MIPT_ERR_INVALID_ARG, "%s: reserved buffer pointers must be NULL", who);
    if (opt->max_samples < 1 || opt->max_samples > 65535) return fail(MIPT_ERR_INVALID_ARG, "%s: max_samples %u: must be 1 ... 65535", who, opt->max_samples);
    if (opt->min_samples > opt->max_samples)
        return fail(MIPT_ERR_INVALID_ARG, "%s: min_samples %u: must be at most max_samples %u", who, opt->min_samples, opt->max_samples);
    if (!std::isfinite(opt->budget) || !(opt->budget >= (float)opt->min_samples) || !(opt->budget <= (float)opt->max_samples))
        return fail(MIPT_ERR_INVALID_ARG, "%s: budget %g: must be finite and in [min_samples, max_samples] = [%u, %u]", who, (double)opt->budget,
                    opt->min_samples, opt->max_samples);
    const void *p[kBuffers];
    unpack(buf, p);
    for (int i = 0; i < kBuffers; i++)
        for (int j = i + 1; j < kBuffers; j++)
            if (p[i] && p[j] && mipt::ranges_overlap(p[i], n_pix * kFields[i].words * 4, p[j], n_pix * kFields[j].words * 4))
                return fail(MIPT_ERR_INVALID_ARG, "%s: %s overlaps %s", who, kFields[j].name, kFields[i].name);

    d = mipt::DevSampleMap{};
    d.variance = buf->variance; d.hdr = buf->hdr; d.albedo = buf->albedo; d.counts = buf->counts;
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

// the fill entries' options as the plain map's, for map_validate: the same fields in the same places, `rounds` checked apart
int fill_options(const char *who, const MiptSampleMapFillOptions *fill, MiptSampleMapOptions &opt) {
    if (!fill) return fail(MIPT_ERR_INVALID_ARG, "%s: null opt", who);
    opt = MiptSampleMapOptions{};
    opt.width = fill->width; opt.height = fill->height; opt.n_views = fill->n_views; opt.flags = fill->flags;
    opt.min_samples = fill->min_samples; opt.max_samples = fill->max_samples; opt.budget = fill->budget;
    for (int i = 0; i < 8; i++) opt.reserved[i] = fill->reserved[i];
    return MIPT_OK;
}
int fill_rounds(const char *who, const MiptSampleMapFillOptions *fill) {
    if (fill->rounds < 1 || fill->rounds > mipt::kSampleMapMaxRounds)
        return fail(MIPT_ERR_INVALID_ARG, "%s: rounds %u: must be 1 ... %u", who, fill->rounds, mipt::kSampleMapMaxRounds);
    return MIPT_OK;
}

// rounds == 0: mipt_sample_map_device; otherwise mipt_sample_map_fill_device
int map_device(const char *who, const MiptSampleMapOptions *opt, const MiptSampleMapBuffers *buf, uint32_t rounds, void *d_workspace,
               void *hip_stream) {
    mipt::DevSampleMap d;
    int rc = map_validate(who, opt, buf, d);
    if (rc) return rc;
    const uint64_t need = rounds ? sizeof(mipt::SampleMapFillWork) * rounds : sizeof(mipt::SampleMapWork);
    if (!d_workspace) return fail(MIPT_ERR_INVALID_ARG, "%s: null workspace", who);
    if ((uintptr_t)d_workspace & 15u) return fail(MIPT_ERR_INVALID_ARG, "%s: workspace must be 16-byte aligned", who);
    const void *p[kBuffers];
    unpack(buf, p);
    for (int i = 0; i < kBuffers; i++) {
        if ((uintptr_t)p[i] & 3u) return fail(MIPT_ERR_INVALID_ARG, "%s: %s must be 4-byte aligned", who, kFields[i].name);
        if (p[i] && mipt::ranges_overlap(p[i], d.n_pixels * kFields[i].words * 4, d_workspace, need))
            return fail(MIPT_ERR_INVALID_ARG, "%s: %s overlaps the workspace", who, kFields[i].name);
    }
    int device = -1;
    if ((rc = mipt::device_buffer_check(who, buf->variance, -1, "variance", "", &device))) return rc;
    for (int i = 1; i < kBuffers; i++)
        if (p[i] && (rc = mipt::device_buffer_check(who, p[i], device, kFields[i].name, "variance's device"))) return rc;
    if ((rc = mipt::device_buffer_check(who, d_workspace, device, "workspace", "variance's device"))) return rc;
    MIPT_HIP(hipSetDevice(device));
    if (rounds) {
        MIPT_HIP(mipt::launch_sample_map_fill(d, (mipt::SampleMapFillWork *)d_workspace, rounds, (hipStream_t)hip_stream));
        return MIPT_OK;
    }
    d.work = (mipt::SampleMapWork *)d_workspace;
    MIPT_HIP(mipt::launch_sample_map(d, (hipStream_t)hip_stream));
    return MIPT_OK;
}

int map_host(const char *who, const MiptSampleMapOptions *opt, const MiptSampleMapBuffers *buf, uint32_t rounds, int device_id) {
    mipt::DevSampleMap d;
    const int rc = map_validate(who, opt, buf, d);
    if (rc) return rc;
    const hipError_t e = hipSetDevice(device_id);
    if (e != hipSuccess) {
        (void)hipGetLastError();                                  // or the next launch of this thread would report this ordinal's error
        return fail(MIPT_ERR_HIP, "%s: hipSetDevice(device_id = %d) failed: %s", who, device_id, hipGetErrorString(e));
    }
    const void *h[kBuffers];
    unpack(buf, h);
    mipt::DevPtr<float> dev[kCounts];                             // variance, hdr, albedo
    mipt::DevPtr<uint32_t> counts;
    mipt::DevPtr<mipt::SampleMapFillWork> work;                  // one slot is also the plain map's workspace: the same 32 B
    for (int i = 0; i < kCounts; i++)
        if (h[i]) {
            MIPT_HIP(dev[i].alloc(d.n_pixels * kFields[i].words));
            MIPT_HIP(hipMemcpy(dev[i].get(), h[i], d.n_pixels * kFields[i].words * sizeof(float), hipMemcpyHostToDevice));
        }
    MIPT_HIP(counts.alloc(d.n_pixels));
    MIPT_HIP(work.alloc(rounds ? rounds : 1u));
    d.variance = dev[kVariance].get(); d.hdr = dev[kHdrBuf].get(); d.albedo = dev[kAlbedo].get();
    d.counts = counts.get(); d.work = (mipt::SampleMapWork *)work.get();
    if (rounds) MIPT_HIP(mipt::launch_sample_map_fill(d, work.get(), rounds, nullptr));
    else MIPT_HIP(mipt::launch_sample_map(d, nullptr));
    MIPT_HIP(hipMemcpy(buf->counts, counts.get(), d.n_pixels * sizeof(uint32_t), hipMemcpyDeviceToHost));   // ordered after the passes: blocks until done
    return MIPT_OK;
}

int fill_host(const MiptSampleMapFillOptions *fill, const MiptSampleMapBuffers *buf, int device_id) {
    const char *who = "mipt_sample_map_fill";
    MiptSampleMapOptions opt;
    int rc = fill_options(who, fill, opt);
    if (rc) return rc;
    if (!buf) return fail(MIPT_ERR_INVALID_ARG, "%s: null buffers", who);
    if ((rc = fill_rounds(who, fill))) return rc;
    return map_host(who, &opt, buf, fill->rounds, device_id);
}

int fill_device(const MiptSampleMapFillOptions *fill, const MiptSampleMapBuffers *buf, void *d_workspace, void *hip_stream) {
    const char *who = "mipt_sample_map_fill_device";
    MiptSampleMapOptions opt;
    int rc = fill_options(who, fill, opt);
    if (rc) return rc;
    if (!buf) return fail(MIPT_ERR_INVALID_ARG, "%s: null buffers", who);
    if ((rc = fill_rounds(who, fill))) return rc;
    return map_device(who, &opt, buf, fill->rounds, d_workspace, hip_stream);
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
