// mipt_motion.cpp -- the previous-position entry points of include/mipt.h (mipt_render_motion, mipt_render_motion_device): argument
// checks, device staging for the host entry, the choice of the source of the previous geometry and the launch of first_hit.hip's
// kernel in its MOTION form.  Host C++ only; every device operation is stream-ordered HIP.
#include "../../include/mipt.h"
#include "pt_kernel.h"
#include "mipt_scene.h"                                          // and with it mipt_host_util.h, mipt_internal.h

#include <cstring>

static_assert(sizeof(MiptMotionBuffers) == 64, "ABI struct size (tests/test_motion_model.py)");

namespace {

using mipt::fail;

// everything that needs neither the scene's contents nor a device: the feature pass's checks (MIPT_FLAG_COUNT refused), then the buffers
int validate(const char *who, const MiptScene *scene, const MiptCamera *cameras, uint32_t n_views, const MiptOptions *opt,
             const MiptMotionBuffers *b, bool device) {
    { const int rc = mipt::first_hit_check(who, scene, cameras, n_views, opt, b, false); if (rc) return rc; }
    if (b->reserved0) return fail(MIPT_ERR_INVALID_ARG, "%s: reserved0 must be 0", who);
    for (const void *r : b->reserved)
        if (r) return fail(MIPT_ERR_INVALID_ARG, "%s: reserved buffer pointers must be NULL", who);
    if (!b->prev_position) return fail(MIPT_ERR_INVALID_ARG, "%s: null prev_position", who);
    if (!b->prev_tris && b->n_prev_tris) return fail(MIPT_ERR_INVALID_ARG, "%s: n_prev_tris %u without prev_tris", who, b->n_prev_tris);
    if (device) {
        if ((uintptr_t)b->prev_position & 3u) return fail(MIPT_ERR_INVALID_ARG, "%s: prev_position must be 4-byte aligned", who);
        if ((uintptr_t)b->prev_tris & 3u) return fail(MIPT_ERR_INVALID_ARG, "%s: prev_tris must be 4-byte aligned", who);
    }
    return MIPT_OK;
}

// the source of the previous geometry against the scene: still host work only
int check_source(const char *who, const MiptScene *scene, const MiptMotionBuffers *b, mipt::MeshMotionSource *tracked) {
    if (b->prev_tris) {
        if ((size_t)b->n_prev_tris != scene->n_tris)
            return fail(MIPT_ERR_INVALID_ARG, "%s: n_prev_tris %u, the scene has %zu triangles", who, b->n_prev_tris, scene->n_tris);
    } else {
        if (!mipt::mesh_motion_source(scene, tracked))
            return fail(MIPT_ERR_INVALID_ARG, "%s: prev_tris is NULL and the scene is not a mesh that tracks motion (mipt_scene_track_motion)", who);
    }
    return MIPT_OK;
}

// the launch, with every argument already checked; prev_position and prev_tris (if any) in HBM of the scene's device
int motion_launch(MiptScene *scene, const MiptCamera *cameras, uint32_t n_views, const MiptOptions *opt, const MiptMotionBuffers *d,
                  const mipt::MeshMotionSource &tracked, hipStream_t stream, MiptStats *stats) {
    if (stats) memset(stats, 0, sizeof *stats);
    const bool cull = opt->traversal == MIPT_TRAVERSAL_CULLED;
    MIPT_HIP(hipSetDevice(scene->device));

    mipt::DevFeatures f{};
    f.prev_position = d->prev_position;
    if (d->prev_tris) {
        f.prev_tris = (const float *)d->prev_tris;
    } else {
        f.prev_rec = tracked.prev_rec; f.prev_pos = tracked.prev_pos; f.prev_idx = tracked.idx;
        f.prev_n_parts = tracked.n_parts; f.prev_n_pos = tracked.n_pos;
    }
    int grid = 0, rc = mipt::first_hit_setup(scene, cameras, n_views, opt, mipt::motion_blocks_per_cu(d->prev_tris != nullptr, cull), stream, &f, &grid);
    if (rc) return rc;
    f.samples = 1u; f.samples_f = 1.0f;                            // only the first sample is traced

    mipt::DevStats hs;
    float ms = 0.0f;
    rc = mipt::traversal_launch(
        scene, stream,
        [&]() -> int {
            MIPT_HIP(mipt::launch_motion(scene->dev, f, cull, grid, stream));
            return MIPT_OK;
        },
        []() -> int { return MIPT_OK; }, hs, ms);
    if (rc && rc != MIPT_ERR_STACK) return rc;
    if (stats) {
        stats->kernel_ms = ms;
        stats->stack_overflows = hs.stack_overflows;
        stats->tex_clamped = 0;
        stats->pixels = hs.pixels;
    }
    return rc;                                                    // MIPT_OK, or MIPT_ERR_STACK with the buffer and the stats delivered
}

int motion_device(MiptScene *scene, const MiptCamera *cameras, uint32_t n_views, const MiptOptions *opt, const MiptMotionBuffers *d,
                  void *hip_stream, MiptStats *stats) {
    const char *who = "mipt_render_motion_device";
    mipt::MeshMotionSource tracked{};
    int rc = validate(who, scene, cameras, n_views, opt, d, true);
    if (rc || (rc = check_source(who, scene, d, &tracked))) return rc;
    if ((rc = mipt::device_buffer_check(who, d->prev_position, scene->device, "prev_position"))) return rc;
    if (d->prev_tris && (rc = mipt::device_buffer_check(who, d->prev_tris, scene->device, "prev_tris"))) return rc;
    return motion_launch(scene, cameras, n_views, opt, d, tracked, (hipStream_t)hip_stream, stats);
}

int motion_host(MiptScene *scene, const MiptCamera *cameras, uint32_t n_views, const MiptOptions *opt, const MiptMotionBuffers *h,
                MiptStats *stats) {
    mipt::MeshMotionSource tracked{};
    int rc = validate("mipt_render_motion", scene, cameras, n_views, opt, h, false);
    if (rc || (rc = check_source("mipt_render_motion", scene, h, &tracked))) return rc;
    MIPT_HIP(hipSetDevice(scene->device));
    const size_t n_pix = (size_t)n_views * opt->width * opt->height;
    mipt::DevPtr<float> out;                                      // freed on every way out
    mipt::DevPtr<MiptTriangle> tris;
    MIPT_HIP(out.alloc(n_pix * 3));
    MiptMotionBuffers d{};
    d.prev_position = out.get();
    if (h->prev_tris) {
        MIPT_HIP(tris.alloc(h->n_prev_tris));
        if ((rc = mipt::upload_staged(tris.get(), h->prev_tris, (size_t)h->n_prev_tris * sizeof(MiptTriangle)))) return rc;
        d.prev_tris = tris.get(); d.n_prev_tris = h->n_prev_tris;
    }
    rc = motion_launch(scene, cameras, n_views, opt, &d, tracked, nullptr, stats);
    if (rc && rc != MIPT_ERR_STACK) return rc;
    MIPT_HIP(hipMemcpy(h->prev_position, out.get(), n_pix * 3 * sizeof(float), hipMemcpyDeviceToHost));
    return rc;
}

} // namespace

extern "C" {

int mipt_render_motion(MiptScene *scene, const MiptCamera *cameras, uint32_t n_views, const MiptOptions *opt,
                       const MiptMotionBuffers *host, MiptStats *stats) {
    MIPT_NO_THROW(motion_host(scene, cameras, n_views, opt, host, stats))
}
int mipt_render_motion_device(MiptScene *scene, const MiptCamera *cameras, uint32_t n_views, const MiptOptions *opt,
                              const MiptMotionBuffers *device, void *hip_stream, MiptStats *stats) {
    MIPT_NO_THROW(motion_device(scene, cameras, n_views, opt, device, hip_stream, stats))
}

} // extern "C"
