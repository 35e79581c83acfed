// mipt_denoise.cpp -- the denoiser entry points of include/mipt.h (mipt_denoise_workspace_bytes, mipt_denoise, mipt_denoise_device):
// the plane table, the checks of the filter's own options, the filter constants, the workspace carve-up and the launches of
// denoise.hip.  The checks every image-space entry makes, the device-entry checks and the host entry's staging are mipt_planes.h's
// and mipt_host_util.h's.  Host C++ only; every device operation is stream-ordered HIP.
#include "../../include/mipt.h"
#include "pt_kernel.h"
#include "mipt_host_util.h"

#include <cmath>
#include <cstring>

static_assert(sizeof(MiptDenoiseOptions) == 64 && sizeof(MiptDenoiseBuffers) == 64, "ABI struct sizes (tests/test_denoise_model.py)");

namespace {

using mipt::fail;

constexpr uint64_t kWorkspaceBytesPerPixel = 3 * sizeof(float4);     // the guide plane and two colour planes

// in the order of MiptDenoiseBuffers
constexpr int kBuffers = 5, kHdr = 0;
constexpr mipt::Plane kPlanes[kBuffers] = {{"hdr", 12, 4, true, mipt::kPlaneIn, -1},    {"normal", 12, 4, false, mipt::kPlaneIn, -1},
                                           {"depth", 4, 4, false, mipt::kPlaneIn, -1},  {"albedo", 12, 4, false, mipt::kPlaneIn, -1},
                                           {"out", 12, 4, true, mipt::kPlaneOut, kHdr}};
static_assert(kBuffers <= mipt::kMaxPlanes, "a PlaneSet holds the table");

// everything that needs no device: on success d holds the sizes and the filter constants, set the caller's planes
int validate(const char *who, const MiptDenoiseOptions *opt, const MiptDenoiseBuffers *buf, mipt::DevDenoise &d, mipt::PlaneSet &set, uint64_t &n_pix) {
    int rc;
    if ((rc = mipt::not_null(who, opt, "opt")) || (rc = mipt::not_null(who, buf, "buffers"))) return rc;
    mipt::planes_bind(set, kPlanes, kBuffers, buf);
    if ((rc = mipt::planes_required(who, set)) || (rc = mipt::frame_nonzero(who, opt->width, opt->height, opt->n_views)) ||
        (rc = mipt::frame_pixels(who, opt->width, opt->height, opt->n_views, &n_pix)))
        return rc;
    if (opt->iterations < 1 || opt->iterations > 8) return fail(MIPT_ERR_INVALID_ARG, "%s: iterations %u: must be 1 ... 8", who, opt->iterations);
    if ((rc = mipt::flags_zero(who, opt->flags)) || (rc = mipt::reserved_zero(who, opt->reserved, buf->reserved))) return rc;

    d = mipt::DevDenoise{};
    if (!std::isfinite(opt->sigma_color) || !(opt->sigma_color > 0.0f))
        return fail(MIPT_ERR_INVALID_ARG, "%s: sigma_color must be finite and greater than 0", who);
    for (uint32_t i = 0; i < opt->iterations; i++) {
        const float sc = opt->sigma_color * std::ldexp(1.0f, -(int)i);       // sigma_color * 2^-i
        if (!mipt::inverse_square(sc, &d.kc[i]))
            return fail(MIPT_ERR_INVALID_ARG, "%s: sigma_color %g: 1 / (sigma_color * 2^-%u)^2 is not finite and greater than 0", who, (double)opt->sigma_color, i);
    }
    // a sigma given for an absent guide is ignored
    if (buf->normal && !mipt::inverse_square(opt->sigma_normal, &d.kn))
        return fail(MIPT_ERR_INVALID_ARG, "%s: sigma_normal %g: it and 1 / sigma_normal^2 must be finite and greater than 0", who, (double)opt->sigma_normal);
    if (buf->depth && !mipt::inverse_square(opt->sigma_depth, &d.kz))
        return fail(MIPT_ERR_INVALID_ARG, "%s: sigma_depth %g: it and 1 / sigma_depth^2 must be finite and greater than 0", who, (double)opt->sigma_depth);

    mipt::planes_size(set, n_pix);
    if ((rc = mipt::planes_disjoint(who, set))) return rc;
    d.width = opt->width; d.height = opt->height; d.n_views = opt->n_views; d.iterations = opt->iterations;
    d.tiles_x = mipt::tiles_across(opt->width);
    d.tiles_y = mipt::tiles_down(opt->height);
    return MIPT_OK;
}

// the planes (the caller's, or the host entry's staged copies) and the workspace: the guide plane and two colour planes
void point(mipt::DevDenoise &d, const void *const p[], void *workspace, uint64_t n_pix) {
    d.hdr = (const float *)p[0]; d.normal = (const float *)p[1]; d.depth = (const float *)p[2]; d.albedo = (const float *)p[3];
    d.out = (float *)p[4];
    d.guides = (float4 *)workspace;
    d.colour[0] = d.guides + n_pix;
    d.colour[1] = d.guides + 2 * n_pix;
}

int denoise_device(const MiptDenoiseOptions *opt, const MiptDenoiseBuffers *buf, void *d_workspace, uint64_t workspace_bytes, void *hip_stream) {
    const char *who = "mipt_denoise_device";
    mipt::DevDenoise d;
    mipt::PlaneSet set;
    uint64_t n_pix = 0;
    int rc = validate(who, opt, buf, d, set, n_pix);
    if (rc) return rc;
    const mipt::Workspace ws = {d_workspace, workspace_bytes, n_pix * kWorkspaceBytesPerPixel, "mipt_denoise_workspace_bytes"};
    if ((rc = mipt::device_entry_check(who, set, &ws))) return rc;
    point(d, set.ptr, d_workspace, n_pix);
    MIPT_HIP(mipt::launch_denoise(d, (hipStream_t)hip_stream));
    return MIPT_OK;
}

int denoise_host(const MiptDenoiseOptions *opt, const MiptDenoiseBuffers *buf, int device_id) {
    const char *who = "mipt_denoise";
    mipt::DevDenoise d;
    mipt::PlaneSet set;
    uint64_t n_pix = 0;
    int rc = validate(who, opt, buf, d, set, n_pix);
    if (rc || (rc = mipt::select_device(who, device_id))) return rc;
    mipt::StagedPlanes staged;
    mipt::DevPtr<unsigned char> workspace;
    if ((rc = staged.stage(set))) return rc;
    MIPT_HIP(workspace.alloc(n_pix * kWorkspaceBytesPerPixel));
    point(d, staged.ptr, workspace.get(), n_pix);
    MIPT_HIP(mipt::launch_denoise(d, nullptr));
    return staged.fetch(set);
}

} // namespace

extern "C" {

uint64_t mipt_denoise_workspace_bytes(uint32_t width, uint32_t height, uint32_t n_views) {
    return mipt::batch_pixels(width, height, n_views) * kWorkspaceBytesPerPixel;
}
int mipt_denoise(const MiptDenoiseOptions *opt, const MiptDenoiseBuffers *host, int device_id) {
    MIPT_NO_THROW(denoise_host(opt, host, device_id))
}
int mipt_denoise_device(const MiptDenoiseOptions *opt, const MiptDenoiseBuffers *device, void *d_workspace, uint64_t workspace_bytes,
                        void *hip_stream) {
    MIPT_NO_THROW(denoise_device(opt, device, d_workspace, workspace_bytes, hip_stream))
}

} // extern "C"
