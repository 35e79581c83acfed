// mipt_bake.cpp -- the baking entry points of include/mipt.h (mipt_bake_texels, mipt_bake_gather, mipt_bake_surface and their _device forms): argument
// checks, the scene-owned workspace, staging for the host entries and the launches of bake.hip's kernels around the ray kernel of the
// radiance queries (mipt::radiance_launch, mipt_radiance.cpp).  Host C++ only; every device operation is stream-ordered HIP.
#include "../../include/mipt.h"
#include "pt_kernel.h"
#include "mipt_scene.h"                                          // and with it mipt_host_util.h, mipt_internal.h

#include <cstring>

static_assert(sizeof(MiptSurfacePoint) == 16 && sizeof(MiptBakeOptions) == 64, "ABI struct sizes (tests/test_bake_abi.py)");
static_assert(sizeof(MiptBakeTexelOptions) == 32 && sizeof(MiptBakeTexelInfo) == 32, "ABI struct sizes (tests/test_bake_abi.py)");
static_assert(offsetof(MiptSurfacePoint, prim) == offsetof(MiptHit, prim) && offsetof(MiptSurfacePoint, u) == offsetof(MiptHit, u),
              "a MiptHit with a seed in its t word is a point");
static_assert(sizeof(mipt::BakeCtl) == 32, "one memset");
static_assert(sizeof(MiptBakeSurfaceOptions) == 32, "ABI struct sizes (tests/test_lightmap_abi.py)");

namespace {

using mipt::fail;

constexpr uint32_t kHugeCap = 8192;                              // triangles the grid-wide coverage kernel takes (bake.hip)

// ---- texels ------------------------------------------------------------------------------------------------------------------------
int texel_check(const char *who, const MiptScene *scene, uint32_t width, uint32_t height, const MiptBakeTexelOptions *opt, const void *points) {
    if (!scene || !points) return fail(MIPT_ERR_INVALID_ARG, "%s: null scene or points", who);
    if ((uint64_t)width * height >= MIPT_QUERY_MAX_RAYS)
        return fail(MIPT_ERR_INVALID_ARG, "%s: %u x %u texels: width * height must stay below 2^31", who, width, height);
    if (!opt) return MIPT_OK;
    if (opt->flags) return fail(MIPT_ERR_INVALID_ARG, "%s: flags 0x%x: no flag is defined", who, opt->flags);
    return mipt::reserved_check(who, opt->reserved);
}

// the launch, with every argument already checked; d_points in HBM of the scene's device
int texel_launch(MiptScene *scene, uint32_t width, uint32_t height, MiptSurfacePoint *d_points, hipStream_t stream, MiptBakeTexelInfo *info) {
    if (info) memset(info, 0, sizeof *info);
    MIPT_HIP(hipSetDevice(scene->device));
    int rc;
    const size_t n = (size_t)width * height;
    if ((rc = scene->d_bake_owner.grow(n * 8))) return rc;
    if ((rc = scene->d_bake_huge.grow((size_t)kHugeCap * 4))) return rc;
    if ((rc = scene->d_bake_ctl.grow(sizeof(mipt::BakeCtl)))) return rc;
    mipt::BakeCtl ctl;
    MIPT_HIP(hipEventRecord(scene->ev0, stream));
    MIPT_HIP(mipt::launch_bake_texels(scene->dev, scene->d_tri_order, width, height, scene->d_bake_owner, scene->d_bake_huge, kHugeCap,
                                      scene->d_bake_ctl, d_points, scene->n_cu, stream));
    MIPT_HIP(hipEventRecord(scene->ev1, stream));
    MIPT_HIP(hipMemcpyAsync(&ctl, scene->d_bake_ctl, sizeof ctl, hipMemcpyDeviceToHost, stream));
    MIPT_HIP(hipStreamSynchronize(stream));
    if (info) {
        MIPT_HIP(hipEventElapsedTime(&info->kernel_ms, scene->ev0, scene->ev1));
        info->covered_texels = ctl.covered;
        info->degenerate_tris = ctl.degenerate;
    }
    return MIPT_OK;
}

int texels_device(MiptScene *scene, uint32_t width, uint32_t height, const MiptBakeTexelOptions *opt, MiptSurfacePoint *d_points, void *hip_stream,
                  MiptBakeTexelInfo *info) {
    const char *who = "mipt_bake_texels_device";
    int rc = texel_check(who, scene, width, height, opt, d_points);
    if (rc) return rc;
    const mipt::ItemBuffers b{nullptr, nullptr, 0, "d_points", d_points, (uint64_t)width * height * sizeof(MiptSurfacePoint), 16, false, false};
    return mipt::device_call(who, scene, b, width == 0 || height == 0, info,
                             [&] { return texel_launch(scene, width, height, d_points, (hipStream_t)hip_stream, info); });
}

int texels_host(MiptScene *scene, uint32_t width, uint32_t height, const MiptBakeTexelOptions *opt, MiptSurfacePoint *points, MiptBakeTexelInfo *info) {
    int rc = texel_check("mipt_bake_texels", scene, width, height, opt, points);
    if (rc) return rc;
    if (width == 0 || height == 0) { if (info) memset(info, 0, sizeof *info); return MIPT_OK; }
    return mipt::staged_call(scene, nullptr, 0, points, (size_t)width * height * sizeof(MiptSurfacePoint),
                             [&](const void *, void *d_out) { return texel_launch(scene, width, height, (MiptSurfacePoint *)d_out, nullptr, info); });
}

// ---- gather ------------------------------------------------------------------------------------------------------------------------
int gather_check(const char *who, const MiptScene *scene, const void *points, uint64_t n, const MiptBakeOptions *opt, const void *radiance,
                 bool device_entry) {
    return mipt::chunked_entry_check(who, !scene || !points || !opt || !radiance, "null scene, points, options or radiance", "point", n, opt,
                                     device_entry ? nullptr : "mipt_bake_gather_device");
}

int bad_prim(const char *who, uint64_t i, const MiptScene *scene) {
    return fail(MIPT_ERR_INVALID_ARG, "%s: points[%llu].prim names a triangle the scene does not have (%zu triangles)", who, (unsigned long long)i,
                scene->n_tris);
}

// the caller -> record map of the scene (d_bake_inv), made on first use and kept until the tree changes (release_geometry)
int inverse_order(MiptScene *scene, hipStream_t stream) {
    if (scene->d_bake_inv) return MIPT_OK;
    mipt::DevPtr<uint32_t> inv;
    MIPT_HIP(inv.alloc(scene->n_tris ? scene->n_tris : 1));
    MIPT_HIP(hipMemsetAsync(inv.get(), 0, (scene->n_tris ? scene->n_tris : 1) * sizeof(uint32_t), stream));
    MIPT_HIP(mipt::launch_bake_invert_order(scene->dev, scene->d_tri_order, inv.get(), scene->n_cu, stream));
    MIPT_HIP(hipStreamSynchronize(stream));
    scene->d_bake_inv = std::move(inv);
    return MIPT_OK;
}

// the first point of d_points whose triangle the scene does not have, refused as bad_prim; blocks
int check_prims_device(const char *who, MiptScene *scene, const MiptSurfacePoint *d_points, uint64_t n, hipStream_t stream) {
    int rc;
    if ((rc = scene->d_bake_ctl.grow(sizeof(mipt::BakeCtl)))) return rc;
    mipt::BakeCtl ctl;
    MIPT_HIP(mipt::launch_bake_check_points(d_points, n, (uint32_t)scene->n_tris, scene->d_bake_ctl, scene->n_cu, stream));
    MIPT_HIP(hipMemcpyAsync(&ctl, scene->d_bake_ctl, sizeof ctl, hipMemcpyDeviceToHost, stream));
    MIPT_HIP(hipStreamSynchronize(stream));
    if (ctl.bad_point != ~0ull) return bad_prim(who, ctl.bad_point, scene);
    return MIPT_OK;
}
int check_prims_host(const char *who, const MiptScene *scene, const MiptSurfacePoint *points, uint64_t n) {
    for (uint64_t i = 0; i < n; i++)
        if (points[i].prim != MIPT_HIT_NONE && (points[i].prim & 0x01ffffffu) >= scene->n_tris) return bad_prim(who, i, scene);
    return MIPT_OK;
}

// The gather with every argument already checked (the triangle indices too, unless check_prims); d_points / d_radiance in HBM of the
// scene's device, n > 0
int gather_launch(const char *who, MiptScene *scene, const MiptSurfacePoint *d_points, uint64_t n, const MiptBakeOptions *opt, float *d_radiance,
                  hipStream_t stream, bool check_prims, MiptStats *stats) {
    MIPT_HIP(hipSetDevice(scene->device));
    int rc;
    if (check_prims && (rc = check_prims_device(who, scene, d_points, n, stream))) return rc;
    if ((rc = inverse_order(scene, stream))) return rc;
    auto gen = [&](const mipt::PathChunk &c, float4 *d_rays, hipStream_t s) {
        return mipt::launch_bake_rays(scene->dev, d_points, scene->d_bake_inv, c, d_rays, scene->n_cu, s);
    };
    auto fold = [&](const mipt::PathChunk &c, const float4 *, const float *d_path, hipStream_t s) {
        return mipt::launch_bake_reduce(d_points, c, d_path, d_radiance, scene->n_cu, s);
    };
    return mipt::chunked_trace(scene, n, *opt, stream, stats, gen, fold);
}

int gather_device(MiptScene *scene, const MiptSurfacePoint *d_points, uint64_t n, const MiptBakeOptions *opt, float *d_radiance, void *hip_stream,
                  MiptStats *stats) {
    const char *who = "mipt_bake_gather_device";
    int rc = gather_check(who, scene, d_points, n, opt, d_radiance, true);
    if (rc) return rc;
    const mipt::ItemBuffers b{"d_points", d_points, n * sizeof(MiptSurfacePoint), "d_radiance", d_radiance, n * 12, 4, true, true};
    return mipt::device_call(who, scene, b, n == 0, stats,
                             [&] { return gather_launch(who, scene, d_points, n, opt, d_radiance, (hipStream_t)hip_stream, true, stats); });
}

int gather_host(MiptScene *scene, const MiptSurfacePoint *points, uint64_t n, const MiptBakeOptions *opt, float *radiance, MiptStats *stats) {
    const char *who = "mipt_bake_gather";
    int rc = gather_check(who, scene, points, n, opt, radiance, false);
    if (rc) return rc;
    if (stats) memset(stats, 0, sizeof *stats);
    if (n == 0) return MIPT_OK;
    if ((rc = check_prims_host(who, scene, points, n))) return rc;
    return mipt::staged_call(scene, points, (size_t)n * sizeof(MiptSurfacePoint), radiance, (size_t)n * 3 * sizeof(float), [&](const void *d_points, void *d_out) {
        return gather_launch(who, scene, (const MiptSurfacePoint *)d_points, n, opt, (float *)d_out, nullptr, false, stats);
    });
}

// ---- surface -----------------------------------------------------------------------------------------------------------------------
int surface_check(const char *who, const MiptScene *scene, const void *points, uint64_t n, const MiptBakeSurfaceOptions *opt, const void *position,
                  const void *normal) {
    if (!scene || !points || (!position && !normal)) return fail(MIPT_ERR_INVALID_ARG, "%s: null scene or points, or position and normal both null", who);
    int rc;
    if ((rc = mipt::ray_count_check(who, "n", n))) return rc;
    if (!opt) return MIPT_OK;
    if (opt->flags & ~MIPT_BAKE_SURFACE_UNIT_NORMALS)
        return fail(MIPT_ERR_INVALID_ARG, "%s: flags 0x%x: only MIPT_BAKE_SURFACE_UNIT_NORMALS is accepted", who, opt->flags);
    return mipt::reserved_check(who, opt->reserved);
}

// every argument checked, the triangle indices too; the pointers in HBM of the scene's device, n > 0; blocks
int surface_launch(MiptScene *scene, const MiptSurfacePoint *d_points, uint64_t n, const MiptBakeSurfaceOptions *opt, float *d_position,
                   float *d_normal, hipStream_t stream) {
    int rc;
    if ((rc = inverse_order(scene, stream))) return rc;
    const bool unit = opt && (opt->flags & MIPT_BAKE_SURFACE_UNIT_NORMALS);
    MIPT_HIP(mipt::launch_bake_surface(scene->dev, d_points, scene->d_bake_inv, n, unit, d_position, d_normal, scene->n_cu, stream));
    MIPT_HIP(hipStreamSynchronize(stream));
    return MIPT_OK;
}

int surface_device(MiptScene *scene, const MiptSurfacePoint *d_points, uint64_t n, const MiptBakeSurfaceOptions *opt, float *d_position,
                   float *d_normal, void *hip_stream) {
    const char *who = "mipt_bake_surface_device";
    int rc = surface_check(who, scene, d_points, n, opt, d_position, d_normal);
    if (rc) return rc;
    // device_call's order with two result buffers: alignments, the empty call, overlaps, whose memory, the triangles, the launch
    if ((uintptr_t)d_points & 15u) return fail(MIPT_ERR_INVALID_ARG, "%s: d_points must be 16-byte aligned", who);
    if ((uintptr_t)d_position & 3u) return fail(MIPT_ERR_INVALID_ARG, "%s: d_position must be 4-byte aligned", who);
    if ((uintptr_t)d_normal & 3u) return fail(MIPT_ERR_INVALID_ARG, "%s: d_normal must be 4-byte aligned", who);
    if (n == 0) return MIPT_OK;
    const uint64_t in_bytes = n * sizeof(MiptSurfacePoint), out_bytes = n * 12;
    if (d_position && mipt::ranges_overlap(d_points, in_bytes, d_position, out_bytes))
        return fail(MIPT_ERR_INVALID_ARG, "%s: d_points overlaps d_position", who);
    if (d_normal && mipt::ranges_overlap(d_points, in_bytes, d_normal, out_bytes)) return fail(MIPT_ERR_INVALID_ARG, "%s: d_points overlaps d_normal", who);
    if (d_position && d_normal && mipt::ranges_overlap(d_position, out_bytes, d_normal, out_bytes))
        return fail(MIPT_ERR_INVALID_ARG, "%s: d_position overlaps d_normal", who);
    if ((rc = mipt::device_buffer_check(who, d_points, scene->device, "d_points"))) return rc;
    if (d_position && (rc = mipt::device_buffer_check(who, d_position, scene->device, "d_position"))) return rc;
    if (d_normal && (rc = mipt::device_buffer_check(who, d_normal, scene->device, "d_normal"))) return rc;
    MIPT_HIP(hipSetDevice(scene->device));
    if ((rc = check_prims_device(who, scene, d_points, n, (hipStream_t)hip_stream))) return rc;
    return surface_launch(scene, d_points, n, opt, d_position, d_normal, (hipStream_t)hip_stream);
}

int surface_host(MiptScene *scene, const MiptSurfacePoint *points, uint64_t n, const MiptBakeSurfaceOptions *opt, float *position, float *normal) {
    const char *who = "mipt_bake_surface";
    int rc = surface_check(who, scene, points, n, opt, position, normal);
    if (rc) return rc;
    if (n == 0) return MIPT_OK;
    if ((rc = check_prims_host(who, scene, points, n))) return rc;
    // the scene's staging pair holds the points and the first wanted output; a second output is staged beside it
    const size_t out_bytes = (size_t)n * 3 * sizeof(float);
    float *first = position ? position : normal;
    return mipt::staged_call(scene, points, (size_t)n * sizeof(MiptSurfacePoint), first, out_bytes, [&](const void *d_points, void *d_out) -> int {
        mipt::DevPtr<float> d_second;
        if (position && normal) MIPT_HIP(d_second.alloc((size_t)n * 3));
        float *d_position = position ? (float *)d_out : nullptr, *d_normal = !normal ? nullptr : position ? d_second.get() : (float *)d_out;
        int rc2 = surface_launch(scene, (const MiptSurfacePoint *)d_points, n, opt, d_position, d_normal, nullptr);
        if (rc2) return rc2;
        if (position && normal) MIPT_HIP(hipMemcpy(normal, d_second.get(), out_bytes, hipMemcpyDeviceToHost));
        return MIPT_OK;
    });
}

} // namespace

extern "C" {

int mipt_bake_surface(MiptScene *scene, const MiptSurfacePoint *points, uint64_t n, const MiptBakeSurfaceOptions *opt, float *position, float *normal) {
    MIPT_NO_THROW(surface_host(scene, points, n, opt, position, normal))
}
int mipt_bake_surface_device(MiptScene *scene, const MiptSurfacePoint *d_points, uint64_t n, const MiptBakeSurfaceOptions *opt, float *d_position,
                             float *d_normal, void *hip_stream) {
    MIPT_NO_THROW(surface_device(scene, d_points, n, opt, d_position, d_normal, hip_stream))
}

int mipt_bake_texels(MiptScene *scene, uint32_t width, uint32_t height, const MiptBakeTexelOptions *opt, MiptSurfacePoint *points,
                     MiptBakeTexelInfo *info) {
    MIPT_NO_THROW(texels_host(scene, width, height, opt, points, info))
}
int mipt_bake_texels_device(MiptScene *scene, uint32_t width, uint32_t height, const MiptBakeTexelOptions *opt, MiptSurfacePoint *d_points,
                            void *hip_stream, MiptBakeTexelInfo *info) {
    MIPT_NO_THROW(texels_device(scene, width, height, opt, d_points, hip_stream, info))
}
int mipt_bake_gather(MiptScene *scene, const MiptSurfacePoint *points, uint64_t n, const MiptBakeOptions *opt, float *radiance, MiptStats *stats) {
    MIPT_NO_THROW(gather_host(scene, points, n, opt, radiance, stats))
}
int mipt_bake_gather_device(MiptScene *scene, const MiptSurfacePoint *d_points, uint64_t n, const MiptBakeOptions *opt, float *d_radiance,
                            void *hip_stream, MiptStats *stats) {
    MIPT_NO_THROW(gather_device(scene, d_points, n, opt, d_radiance, hip_stream, stats))
}

} // extern "C"
