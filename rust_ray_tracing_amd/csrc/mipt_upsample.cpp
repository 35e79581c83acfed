// mipt_upsample.cpp -- the entry points of the guided upsampling of include/mipt.h (mipt_upsample_workspace_bytes, mipt_upsample,
// mipt_upsample_device): the plane table, the checks of scale and sigmas, the filter constants, the workspace carve-up and the launches
// of upsample.hip.  The checks every image-space entry makes, the device-entry checks and the host entry's staging are mipt_planes.h's
// and mipt_host_util.h's.  Host C++ only; every device operation is stream-ordered HIP.
#include "../../include/mipt.h"
#include "pt_kernel.h"
#include "mipt_host_util.h"

#include <cmath>
#include <cstring>

static_assert(sizeof(MiptUpsampleOptions) == 64 && sizeof(MiptUpsampleBuffers) == 128, "ABI struct sizes (tests/test_upsample_model.py)");

namespace {

using mipt::fail;

constexpr uint64_t kWorkspaceBytesPerLowPixel = 2 * sizeof(float4);   // the colour plane and the guide plane

// in the order of MiptUpsampleBuffers: the first kLowPlanes at the low resolution (pixel_bytes is per low-resolution pixel there)
constexpr int kBuffers = 11, kLowPlanes = 5;
constexpr mipt::Plane kPlanes[kBuffers] = {{"lo_hdr", 12, 4, true, mipt::kPlaneIn, -1},     {"lo_normal", 12, 4, false, mipt::kPlaneIn, -1},
                                           {"lo_depth", 4, 4, false, mipt::kPlaneIn, -1},   {"lo_albedo", 12, 4, false, mipt::kPlaneIn, -1},
                                           {"lo_material", 4, 4, false, mipt::kPlaneIn, -1}, {"normal", 12, 4, false, mipt::kPlaneIn, -1},
                                           {"depth", 4, 4, false, mipt::kPlaneIn, -1},      {"albedo", 12, 4, false, mipt::kPlaneIn, -1},
                                           {"material", 4, 4, false, mipt::kPlaneIn, -1},   {"out", 12, 4, true, mipt::kPlaneOut, -1},
                                           {"weight", 4, 4, false, mipt::kPlaneOut, -1}};
static_assert(kBuffers <= mipt::kMaxPlanes, "a PlaneSet holds the table");

// everything that needs no device: on success d holds the sizes and the filter constants, set the caller's planes
int validate(const char *who, const MiptUpsampleOptions *opt, const MiptUpsampleBuffers *buf, mipt::DevUpsample &d, mipt::PlaneSet &set, uint64_t &n_lo) {
    int rc;
    if ((rc = mipt::not_null(who, opt, "opt")) || (rc = mipt::not_null(who, buf, "buffers"))) return rc;
    mipt::planes_bind(set, kPlanes, kBuffers, buf);
    if ((rc = mipt::planes_required(who, set)) || (rc = mipt::frame_nonzero(who, opt->width, opt->height, opt->n_views))) return rc;
    if (opt->scale < 2 || opt->scale > 8) return fail(MIPT_ERR_INVALID_ARG, "%s: scale %u: must be 2 ... 8", who, opt->scale);
    if (opt->width % opt->scale) return fail(MIPT_ERR_INVALID_ARG, "%s: width %u is not a multiple of scale %u", who, opt->width, opt->scale);
    if (opt->height % opt->scale) return fail(MIPT_ERR_INVALID_ARG, "%s: height %u is not a multiple of scale %u", who, opt->height, opt->scale);
    uint64_t n_pix = 0;
    if ((rc = mipt::frame_pixels(who, opt->width, opt->height, opt->n_views, &n_pix)) || (rc = mipt::flags_zero(who, opt->flags)) ||
        (rc = mipt::reserved_zero(who, opt->reserved, buf->reserved)))
        return rc;
    n_lo = n_pix / ((uint64_t)opt->scale * opt->scale);

    // a guide is given at both resolutions or at neither
    for (int i = 1; i < kLowPlanes; i++)
        if (!set.ptr[i] != !set.ptr[i + 4])
            return fail(MIPT_ERR_INVALID_ARG, "%s: null %s: %s is given at both resolutions or at neither", who, kPlanes[set.ptr[i] ? i + 4 : i].name,
                        kPlanes[i + 4].name);

    d = mipt::DevUpsample{};
    // a sigma given for an absent guide is ignored
    if (buf->normal && !mipt::inverse_square(opt->sigma_normal, &d.kn))
        return fail(MIPT_ERR_INVALID_ARG, "%s: sigma_normal %g: it and 1 / sigma_normal^2 must be finite and greater than 0", who, (double)opt->sigma_normal);
    if (buf->depth && !mipt::inverse_square(opt->sigma_depth, &d.kz))
        return fail(MIPT_ERR_INVALID_ARG, "%s: sigma_depth %g: it and 1 / sigma_depth^2 must be finite and greater than 0", who, (double)opt->sigma_depth);

    mipt::planes_size(set, n_pix);
    for (int i = 0; i < kLowPlanes; i++) set.bytes[i] = n_lo * kPlanes[i].pixel_bytes;
    if ((rc = mipt::planes_disjoint(who, set))) return rc;                   // nothing may alias
    d.width = opt->width; d.height = opt->height; d.n_views = opt->n_views; d.scale = opt->scale;
    d.lo_width = opt->width / opt->scale; d.lo_height = opt->height / opt->scale;
    d.tiles_x = mipt::tiles_across(d.width); d.tiles_y = mipt::tiles_down(d.height);
    d.lo_tiles_x = mipt::tiles_across(d.lo_width); d.lo_tiles_y = mipt::tiles_down(d.lo_height);
    return MIPT_OK;
}

// the planes (the caller's, or the host entry's staged copies) and the workspace: the colour plane and the guide plane
void point(mipt::DevUpsample &d, const void *const p[], void *workspace, uint64_t n_lo) {
    d.lo_hdr = (const float *)p[0]; d.lo_normal = (const float *)p[1]; d.lo_depth = (const float *)p[2]; d.lo_albedo = (const float *)p[3];
    d.lo_material = (const uint32_t *)p[4];
    d.normal = (const float *)p[5]; d.depth = (const float *)p[6]; d.albedo = (const float *)p[7]; d.material = (const uint32_t *)p[8];
    d.out = (float *)p[9]; d.weight = (float *)p[10];
    d.colour = (float4 *)workspace;
    d.guides = d.colour + n_lo;
}

int upsample_device(const MiptUpsampleOptions *opt, const MiptUpsampleBuffers *buf, void *d_workspace, uint64_t workspace_bytes, void *hip_stream) {
    const char *who = "mipt_upsample_device";
    mipt::DevUpsample d;
    mipt::PlaneSet set;
    uint64_t n_lo = 0;
    int rc = validate(who, opt, buf, d, set, n_lo);
    if (rc) return rc;
    const mipt::Workspace ws = {d_workspace, workspace_bytes, n_lo * kWorkspaceBytesPerLowPixel, "mipt_upsample_workspace_bytes"};
    if ((rc = mipt::device_entry_check(who, set, &ws))) return rc;
    point(d, set.ptr, d_workspace, n_lo);
    MIPT_HIP(mipt::launch_upsample(d, (hipStream_t)hip_stream));
    return MIPT_OK;
}

int upsample_host(const MiptUpsampleOptions *opt, const MiptUpsampleBuffers *buf, int device_id) {
    const char *who = "mipt_upsample";
    mipt::DevUpsample d;
    mipt::PlaneSet set;
    uint64_t n_lo = 0;
    int rc = validate(who, opt, buf, d, set, n_lo);
    if (rc || (rc = mipt::select_device(who, device_id))) return rc;
    mipt::StagedPlanes staged;
    mipt::DevPtr<unsigned char> workspace;
    if ((rc = staged.stage(set))) return rc;
    MIPT_HIP(workspace.alloc(n_lo * kWorkspaceBytesPerLowPixel));
    point(d, staged.ptr, workspace.get(), n_lo);
    MIPT_HIP(mipt::launch_upsample(d, nullptr));
    return staged.fetch(set);
}

} // namespace

extern "C" {

uint64_t mipt_upsample_workspace_bytes(uint32_t width, uint32_t height, uint32_t n_views, uint32_t scale) {
    if (scale < 2 || scale > 8 || width % scale || height % scale) return 0;
    return mipt::batch_pixels(width, height, n_views) / ((uint64_t)scale * scale) * kWorkspaceBytesPerLowPixel;
}
int mipt_upsample(const MiptUpsampleOptions *opt, const MiptUpsampleBuffers *host, int device_id) {
    MIPT_NO_THROW(upsample_host(opt, host, device_id))
}
int mipt_upsample_device(const MiptUpsampleOptions *opt, const MiptUpsampleBuffers *device, void *d_workspace, uint64_t workspace_bytes,
                         void *hip_stream) {
    MIPT_NO_THROW(upsample_device(opt, device, d_workspace, workspace_bytes, hip_stream))
}

} // extern "C"
