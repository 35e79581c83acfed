// mipt_denoise.cpp -- the denoiser entry points of include/mipt.h (mipt_denoise_workspace_bytes, mipt_denoise, mipt_denoise_device):
// argument checks, the filter constants, device staging for the host entry and the launches of denoise.hip.  Host C++ only; every
// device operation is stream-ordered HIP.
#include "../../include/mipt.h"
#include "pt_kernel.h"
#include "mipt_host_util.h"

#include <cmath>
#include <cstring>

static_assert(sizeof(MiptDenoiseOptions) == 64 && sizeof(MiptDenoiseBuffers) == 64, "ABI struct sizes (tests/test_denoise_model.py)");

namespace {

using mipt::fail;

constexpr uint64_t kWorkspaceBytesPerPixel = 3 * sizeof(float4);     // the guide plane and two colour planes

constexpr int kBuffers = 5;
struct BufferField { const char *name; uint32_t words; };           // in the order of MiptDenoiseBuffers; every value is 4 bytes
constexpr BufferField kFields[kBuffers] = {{"hdr", 3}, {"normal", 3}, {"depth", 1}, {"albedo", 3}, {"out", 3}};

void unpack(const MiptDenoiseBuffers *b, const void *p[kBuffers]) {
    p[0] = b->hdr; p[1] = b->normal; p[2] = b->depth; p[3] = b->albedo; p[4] = b->out;
}

// 1 / sigma^2 in f32 as include/mipt.h forms it; false unless sigma and the result are finite and greater than 0
bool inverse_square(float sigma, float *k) {
    if (!std::isfinite(sigma) || !(sigma > 0.0f)) return false;
    *k = 1.0f / (sigma * sigma);
    return std::isfinite(*k) && *k > 0.0f;
}

// everything that needs no device: on success d holds the sizes and the filter constants
int validate(const char *who, const MiptDenoiseOptions *opt, const MiptDenoiseBuffers *buf, mipt::DevDenoise &d, uint64_t &n_pix) {
    if (!opt) return fail(MIPT_ERR_INVALID_ARG, "%s: null opt", who);
    if (!buf) return fail(MIPT_ERR_INVALID_ARG, "%s: null buffers", who);
    if (!buf->hdr) return fail(MIPT_ERR_INVALID_ARG, "%s: null hdr", who);
    if (!buf->out) return fail(MIPT_ERR_INVALID_ARG, "%s: null out", who);
    if (opt->width == 0 || opt->height == 0) return fail(MIPT_ERR_INVALID_ARG, "%s: width and height must be greater than 0", who);
    if (opt->n_views == 0) return fail(MIPT_ERR_INVALID_ARG, "%s: n_views == 0", who);
    n_pix = mipt::batch_pixels(opt->width, opt->height, opt->n_views);
    if (n_pix == 0)
        return fail(MIPT_ERR_INVALID_ARG, "%s: %u views of %ux%u: n_views*width*height must stay below 2^32", who, opt->n_views, opt->width, opt->height);
    if (opt->iterations < 1 || opt->iterations > 8) return fail(MIPT_ERR_INVALID_ARG, "%s: iterations %u: must be 1 ... 8", who, opt->iterations);
    if (opt->flags) return fail(MIPT_ERR_INVALID_ARG, "%s: flags 0x%x: must be 0", who, opt->flags);
    for (uint32_t r : opt->reserved)
        if (r) return fail(MIPT_ERR_INVALID_ARG, "%s: reserved option fields must be 0", who);
    for (const void *r : buf->reserved)
        if (r) return fail(MIPT_ERR_INVALID_ARG, "%s: reserved buffer pointers must be NULL", who);

    d = mipt::DevDenoise{};
    if (!std::isfinite(opt->sigma_color) || !(opt->sigma_color > 0.0f))
        return fail(MIPT_ERR_INVALID_ARG, "%s: sigma_color must be finite and greater than 0", who);
    for (uint32_t i = 0; i < opt->iterations; i++) {
        const float sc = opt->sigma_color * std::ldexp(1.0f, -(int)i);       // sigma_color * 2^-i
        if (!inverse_square(sc, &d.kc[i]))
            return fail(MIPT_ERR_INVALID_ARG, "%s: sigma_color %g: 1 / (sigma_color * 2^-%u)^2 is not finite and greater than 0", who, (double)opt->sigma_color, i);
    }
    // a sigma given for an absent guide is ignored
    if (buf->normal && !inverse_square(opt->sigma_normal, &d.kn))
        return fail(MIPT_ERR_INVALID_ARG, "%s: sigma_normal %g: it and 1 / sigma_normal^2 must be finite and greater than 0", who, (double)opt->sigma_normal);
    if (buf->depth && !inverse_square(opt->sigma_depth, &d.kz))
        return fail(MIPT_ERR_INVALID_ARG, "%s: sigma_depth %g: it and 1 / sigma_depth^2 must be finite and greater than 0", who, (double)opt->sigma_depth);

    // out may be hdr itself; nothing else may overlap
    const void *p[kBuffers];
    unpack(buf, p);
    for (int i = 0; i < kBuffers; i++)
        for (int j = i + 1; j < kBuffers; j++) {
            if (!p[i] || !p[j] || (i == 0 && j == 4 && p[i] == p[j])) continue;
            if (mipt::ranges_overlap(p[i], n_pix * kFields[i].words * 4, p[j], n_pix * kFields[j].words * 4))
                return fail(MIPT_ERR_INVALID_ARG, "%s: %s overlaps %s (only out == hdr is allowed)", who, kFields[j].name, kFields[i].name);
        }

    d.hdr = buf->hdr; d.normal = buf->normal; d.depth = buf->depth; d.albedo = buf->albedo; d.out = buf->out;
    d.width = opt->width; d.height = opt->height; d.n_views = opt->n_views; d.iterations = opt->iterations;
    d.tiles_x = (opt->width + 63u) / 64u;
    d.tiles_y = (opt->height + 3u) / 4u;
    return MIPT_OK;
}

void set_workspace(mipt::DevDenoise &d, void *workspace, uint64_t n_pix) {
    d.guides = (float4 *)workspace;
    d.colour[0] = d.guides + n_pix;
    d.colour[1] = d.guides + 2 * n_pix;
}

int denoise_device(const MiptDenoiseOptions *opt, const MiptDenoiseBuffers *buf, void *d_workspace, uint64_t workspace_bytes, void *hip_stream) {
    const char *who = "mipt_denoise_device";
    mipt::DevDenoise d;
    uint64_t n_pix = 0;
    int rc = validate(who, opt, buf, d, n_pix);
    if (rc) return rc;
    const uint64_t need = n_pix * kWorkspaceBytesPerPixel;
    if (!d_workspace) return fail(MIPT_ERR_INVALID_ARG, "%s: null workspace", who);
    if (workspace_bytes < need)
        return fail(MIPT_ERR_INVALID_ARG, "%s: workspace of %llu bytes is too small: mipt_denoise_workspace_bytes() is %llu", who,
                    (unsigned long long)workspace_bytes, (unsigned long long)need);
    if ((uintptr_t)d_workspace & 15u) return fail(MIPT_ERR_INVALID_ARG, "%s: workspace must be 16-byte aligned", who);
    const void *p[kBuffers];
    unpack(buf, p);
    for (int i = 0; i < kBuffers; i++) {
        if ((uintptr_t)p[i] & 3u) return fail(MIPT_ERR_INVALID_ARG, "%s: %s must be 4-byte aligned", who, kFields[i].name);
        if (p[i] && mipt::ranges_overlap(p[i], n_pix * kFields[i].words * 4, d_workspace, need))
            return fail(MIPT_ERR_INVALID_ARG, "%s: %s overlaps the workspace", who, kFields[i].name);
    }
    int device = -1;
    if ((rc = mipt::device_buffer_check(who, buf->hdr, -1, "hdr", "", &device))) return rc;
    for (int i = 1; i < kBuffers; i++)
        if (p[i] && (rc = mipt::device_buffer_check(who, p[i], device, kFields[i].name, "hdr's device"))) return rc;
    if ((rc = mipt::device_buffer_check(who, d_workspace, device, "workspace", "hdr's device"))) return rc;
    MIPT_HIP(hipSetDevice(device));
    set_workspace(d, d_workspace, n_pix);
    MIPT_HIP(mipt::launch_denoise(d, (hipStream_t)hip_stream));
    return MIPT_OK;
}

int denoise_host(const MiptDenoiseOptions *opt, const MiptDenoiseBuffers *buf, int device_id) {
    const char *who = "mipt_denoise";
    mipt::DevDenoise d;
    uint64_t n_pix = 0;
    const int rc = validate(who, opt, buf, d, n_pix);
    if (rc) return rc;
    const hipError_t e = hipSetDevice(device_id);
    if (e != hipSuccess) {
        (void)hipGetLastError();                                  // or the next launch of this thread would report this ordinal's error
        return fail(MIPT_ERR_HIP, "%s: hipSetDevice(device_id = %d) failed: %s", who, device_id, hipGetErrorString(e));
    }
    const void *h[kBuffers];
    unpack(buf, h);
    mipt::DevPtr<float> dev[kBuffers - 1];                       // hdr, normal, depth, albedo; the result replaces hdr's copy (out == hdr)
    mipt::DevPtr<float4> workspace;
    for (int i = 0; i < kBuffers - 1; i++)
        if (h[i]) {
            MIPT_HIP(dev[i].alloc(n_pix * kFields[i].words));
            MIPT_HIP(hipMemcpy(dev[i].get(), h[i], n_pix * kFields[i].words * sizeof(float), hipMemcpyHostToDevice));
        }
    MIPT_HIP(workspace.alloc(n_pix * 3));
    d.hdr = dev[0].get(); d.normal = dev[1].get(); d.depth = dev[2].get(); d.albedo = dev[3].get(); d.out = dev[0].get();
    set_workspace(d, workspace.get(), n_pix);
    MIPT_HIP(mipt::launch_denoise(d, nullptr));
    MIPT_HIP(hipMemcpy(buf->out, dev[0].get(), n_pix * 3 * sizeof(float), hipMemcpyDeviceToHost));   // ordered after the passes: blocks until done
    return MIPT_OK;
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
