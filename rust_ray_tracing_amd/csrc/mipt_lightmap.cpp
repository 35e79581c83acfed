// mipt_lightmap.cpp -- the lightmap-finishing entry points of include/mipt.h (mipt_lightmap_filter*, mipt_lightmap_dilate* and their
// *_workspace_bytes): the plane tables, the checks of the operators' own options, the filter constants, the workspace carve-up and
// the launches of lightmap.hip.  The checks every image-space entry makes, the device-entry checks and the host entry's staging are
// mipt_planes.h's and mipt_host_util.h's.  Host C++ only; every device operation is stream-ordered HIP.
#include "../../include/mipt.h"
#include "pt_kernel.h"
#include "mipt_host_util.h"

#include <cmath>
#include <cstring>

static_assert(sizeof(MiptLightmapFilterOptions) == 64 && sizeof(MiptLightmapFilterBuffers) == 64, "ABI struct sizes (tests/test_lightmap_abi.py)");
static_assert(sizeof(MiptLightmapDilateOptions) == 32 && sizeof(MiptLightmapDilateBuffers) == 64, "ABI struct sizes (tests/test_lightmap_abi.py)");

namespace {

using mipt::fail;

constexpr uint64_t kFilterBytesPerTexel = 4 * sizeof(float4);       // two colour planes, position, normal
constexpr uint64_t kDilateBytesPerTexel = 2 * sizeof(float4);       // two state planes

// width * height of an atlas; 0 = an invalid size: a zero side, or not below mipt_bake_texels' limit
uint64_t atlas_texels(uint32_t width, uint32_t height) {
    const uint64_t n = (uint64_t)width * height;
    return n >= MIPT_QUERY_MAX_RAYS ? 0 : n;
}
int atlas_check(const char *who, uint32_t width, uint32_t height, uint64_t *n_tex) {
    int rc;
    if ((rc = mipt::frame_nonzero(who, width, height, 1))) return rc;
    if ((*n_tex = atlas_texels(width, height)) == 0)
        return fail(MIPT_ERR_INVALID_ARG, "%s: %u x %u texels: width * height must stay below 2^31", who, width, height);
    return MIPT_OK;
}

// ---- filter ------------------------------------------------------------------------------------------------------------------------
// in the order of MiptLightmapFilterBuffers
constexpr int kFilterBuffers = 5, kRadiance = 0;
constexpr mipt::Plane kFilterPlanes[kFilterBuffers] = {{"radiance", 12, 4, true, mipt::kPlaneIn, -1}, {"points", 16, 16, true, mipt::kPlaneIn, -1},
                                                       {"position", 12, 4, false, mipt::kPlaneIn, -1}, {"normal", 12, 4, false, mipt::kPlaneIn, -1},
                                                       {"out", 12, 4, true, mipt::kPlaneOut, kRadiance}};

// everything that needs no device: on success d holds the sizes and the filter constants, set the caller's planes
int filter_validate(const char *who, const MiptLightmapFilterOptions *opt, const MiptLightmapFilterBuffers *buf, mipt::DevLightmapFilter &d,
                    mipt::PlaneSet &set, uint64_t &n_tex) {
    int rc;
    if ((rc = mipt::not_null(who, opt, "opt")) || (rc = mipt::not_null(who, buf, "buffers"))) return rc;
    mipt::planes_bind(set, kFilterPlanes, kFilterBuffers, buf);
    if ((rc = mipt::planes_required(who, set)) || (rc = atlas_check(who, opt->width, opt->height, &n_tex))) return rc;
    if (opt->iterations < 1 || opt->iterations > 8) return fail(MIPT_ERR_INVALID_ARG, "%s: iterations %u: must be 1 ... 8", who, opt->iterations);
    if ((rc = mipt::flags_zero(who, opt->flags)) || (rc = mipt::reserved_zero(who, opt->reserved, buf->reserved))) return rc;

    d = mipt::DevLightmapFilter{};
    if (!std::isfinite(opt->sigma_color) || !(opt->sigma_color > 0.0f))
        return fail(MIPT_ERR_INVALID_ARG, "%s: sigma_color must be finite and greater than 0", who);
    for (uint32_t i = 0; i < opt->iterations; i++) {
        const float sc = opt->sigma_color * std::ldexp(1.0f, -(int)i);       // sigma_color * 2^-i
        if (!mipt::inverse_square(sc, &d.kc[i]))
            return fail(MIPT_ERR_INVALID_ARG, "%s: sigma_color %g: 1 / (sigma_color * 2^-%u)^2 is not finite and greater than 0", who, (double)opt->sigma_color, i);
    }
    // a sigma given for an absent term is ignored
    if (buf->normal && !mipt::inverse_square(opt->sigma_normal, &d.kn))
        return fail(MIPT_ERR_INVALID_ARG, "%s: sigma_normal %g: it and 1 / sigma_normal^2 must be finite and greater than 0", who, (double)opt->sigma_normal);
    if (buf->normal && buf->position && !mipt::inverse_square(opt->sigma_plane, &d.kl))
        return fail(MIPT_ERR_INVALID_ARG, "%s: sigma_plane %g: it and 1 / sigma_plane^2 must be finite and greater than 0", who, (double)opt->sigma_plane);
    if (buf->position) {
        if (!std::isfinite(opt->sigma_distance) || !(opt->sigma_distance > 0.0f))
            return fail(MIPT_ERR_INVALID_ARG, "%s: sigma_distance must be finite and greater than 0", who);
        for (uint32_t i = 0; i < opt->iterations; i++) {
            const float sd = opt->sigma_distance * std::ldexp(1.0f, (int)i);  // sigma_distance * 2^i
            if (!mipt::inverse_square(sd, &d.kd[i]))
                return fail(MIPT_ERR_INVALID_ARG, "%s: sigma_distance %g: 1 / (sigma_distance * 2^%u)^2 is not finite and greater than 0", who,
                            (double)opt->sigma_distance, i);
        }
    }
    mipt::planes_size(set, n_tex);
    if ((rc = mipt::planes_disjoint(who, set))) return rc;
    d.width = opt->width; d.height = opt->height; d.iterations = opt->iterations;
    d.tiles_x = mipt::tiles_across(opt->width);
    d.tiles_y = mipt::tiles_down(opt->height);
    return MIPT_OK;
}

// the planes (the caller's, or the host entry's staged copies) and the workspace
void filter_point(mipt::DevLightmapFilter &d, const void *const p[], void *workspace, uint64_t n_tex) {
    d.radiance = (const float *)p[0]; d.points = (const uint4 *)p[1]; d.position = (const float *)p[2]; d.normal = (const float *)p[3];
    d.out = (float *)p[4];
    d.colour[0] = (float4 *)workspace;
    d.colour[1] = d.colour[0] + n_tex;
    d.pos4 = d.colour[0] + 2 * n_tex;
    d.nrm4 = d.colour[0] + 3 * n_tex;
}

int filter_device(const MiptLightmapFilterOptions *opt, const MiptLightmapFilterBuffers *buf, void *d_workspace, uint64_t workspace_bytes, void *hip_stream) {
    const char *who = "mipt_lightmap_filter_device";
    mipt::DevLightmapFilter d;
    mipt::PlaneSet set;
    uint64_t n_tex = 0;
    int rc = filter_validate(who, opt, buf, d, set, n_tex);
    if (rc) return rc;
    const mipt::Workspace ws = {d_workspace, workspace_bytes, n_tex * kFilterBytesPerTexel, "mipt_lightmap_filter_workspace_bytes"};
    if ((rc = mipt::device_entry_check(who, set, &ws))) return rc;
    filter_point(d, set.ptr, d_workspace, n_tex);
    MIPT_HIP(mipt::launch_lightmap_filter(d, (hipStream_t)hip_stream));
    return MIPT_OK;
}

int filter_host(const MiptLightmapFilterOptions *opt, const MiptLightmapFilterBuffers *buf, int device_id) {
    const char *who = "mipt_lightmap_filter";
    mipt::DevLightmapFilter d;
    mipt::PlaneSet set;
    uint64_t n_tex = 0;
    int rc = filter_validate(who, opt, buf, d, set, n_tex);
    if (rc || (rc = mipt::select_device(who, device_id))) return rc;
    mipt::StagedPlanes staged;
    mipt::DevPtr<unsigned char> workspace;
    if ((rc = staged.stage(set))) return rc;
    MIPT_HIP(workspace.alloc(n_tex * kFilterBytesPerTexel));
    filter_point(d, staged.ptr, workspace.get(), n_tex);
    MIPT_HIP(mipt::launch_lightmap_filter(d, nullptr));
    return staged.fetch(set);
}

// ---- dilation ----------------------------------------------------------------------------------------------------------------------
// in the order of MiptLightmapDilateBuffers
constexpr int kDilateBuffers = 4;
constexpr mipt::Plane kDilatePlanes[kDilateBuffers] = {{"radiance", 12, 4, true, mipt::kPlaneIn, -1}, {"points", 16, 16, true, mipt::kPlaneIn, -1},
                                                       {"out", 12, 4, true, mipt::kPlaneOut, kRadiance}, {"level", 4, 4, false, mipt::kPlaneOut, -1}};
static_assert(kFilterBuffers <= mipt::kMaxPlanes && kDilateBuffers <= mipt::kMaxPlanes, "a PlaneSet holds the table");

int dilate_validate(const char *who, const MiptLightmapDilateOptions *opt, const MiptLightmapDilateBuffers *buf, mipt::DevLightmapDilate &d,
                    mipt::PlaneSet &set, uint64_t &n_tex) {
    int rc;
    if ((rc = mipt::not_null(who, opt, "opt")) || (rc = mipt::not_null(who, buf, "buffers"))) return rc;
    mipt::planes_bind(set, kDilatePlanes, kDilateBuffers, buf);
    if ((rc = mipt::planes_required(who, set)) || (rc = atlas_check(who, opt->width, opt->height, &n_tex))) return rc;
    if (opt->radius > MIPT_LIGHTMAP_MAX_RADIUS) return fail(MIPT_ERR_INVALID_ARG, "%s: radius %u: must be 0 ... 64", who, opt->radius);
    if ((rc = mipt::flags_zero(who, opt->flags)) || (rc = mipt::reserved_zero(who, opt->reserved, buf->reserved))) return rc;
    mipt::planes_size(set, n_tex);
    if ((rc = mipt::planes_disjoint(who, set))) return rc;
    d = mipt::DevLightmapDilate{};
    d.width = opt->width; d.height = opt->height; d.radius = opt->radius;
    d.tiles_x = mipt::tiles_across(opt->width);
    d.tiles_y = mipt::tiles_down(opt->height);
    return MIPT_OK;
}

void dilate_point(mipt::DevLightmapDilate &d, const void *const p[], void *workspace, uint64_t n_tex) {
    d.radiance = (const float *)p[0]; d.points = (const uint4 *)p[1]; d.out = (float *)p[2]; d.level = (uint32_t *)p[3];
    d.state[0] = (float4 *)workspace;
    d.state[1] = d.state[0] + n_tex;
}

int dilate_device(const MiptLightmapDilateOptions *opt, const MiptLightmapDilateBuffers *buf, void *d_workspace, uint64_t workspace_bytes, void *hip_stream) {
    const char *who = "mipt_lightmap_dilate_device";
    mipt::DevLightmapDilate d;
    mipt::PlaneSet set;
    uint64_t n_tex = 0;
    int rc = dilate_validate(who, opt, buf, d, set, n_tex);
    if (rc) return rc;
    const mipt::Workspace ws = {d_workspace, workspace_bytes, n_tex * kDilateBytesPerTexel, "mipt_lightmap_dilate_workspace_bytes"};
    if ((rc = mipt::device_entry_check(who, set, &ws))) return rc;
    dilate_point(d, set.ptr, d_workspace, n_tex);
    MIPT_HIP(mipt::launch_lightmap_dilate(d, (hipStream_t)hip_stream));
    return MIPT_OK;
}

int dilate_host(const MiptLightmapDilateOptions *opt, const MiptLightmapDilateBuffers *buf, int device_id) {
    const char *who = "mipt_lightmap_dilate";
    mipt::DevLightmapDilate d;
    mipt::PlaneSet set;
    uint64_t n_tex = 0;
    int rc = dilate_validate(who, opt, buf, d, set, n_tex);
    if (rc || (rc = mipt::select_device(who, device_id))) return rc;
    mipt::StagedPlanes staged;
    mipt::DevPtr<unsigned char> workspace;
    if ((rc = staged.stage(set))) return rc;
    MIPT_HIP(workspace.alloc(n_tex * kDilateBytesPerTexel));
    dilate_point(d, staged.ptr, workspace.get(), n_tex);
    MIPT_HIP(mipt::launch_lightmap_dilate(d, nullptr));
    return staged.fetch(set);
}

} // namespace

extern "C" {

uint64_t mipt_lightmap_filter_workspace_bytes(uint32_t width, uint32_t height) { return atlas_texels(width, height) * kFilterBytesPerTexel; }
int mipt_lightmap_filter(const MiptLightmapFilterOptions *opt, const MiptLightmapFilterBuffers *host, int device_id) {
    MIPT_NO_THROW(filter_host(opt, host, device_id))
}
int mipt_lightmap_filter_device(const MiptLightmapFilterOptions *opt, const MiptLightmapFilterBuffers *device, void *d_workspace,
                                uint64_t workspace_bytes, void *hip_stream) {
    MIPT_NO_THROW(filter_device(opt, device, d_workspace, workspace_bytes, hip_stream))
}
uint64_t mipt_lightmap_dilate_workspace_bytes(uint32_t width, uint32_t height) { return atlas_texels(width, height) * kDilateBytesPerTexel; }
int mipt_lightmap_dilate(const MiptLightmapDilateOptions *opt, const MiptLightmapDilateBuffers *host, int device_id) {
    MIPT_NO_THROW(dilate_host(opt, host, device_id))
}
int mipt_lightmap_dilate_device(const MiptLightmapDilateOptions *opt, const MiptLightmapDilateBuffers *device, void *d_workspace,
                                uint64_t workspace_bytes, void *hip_stream) {
    MIPT_NO_THROW(dilate_device(opt, device, d_workspace, workspace_bytes, hip_stream))
}

} // extern "C"
