// mipt_denoise_variance.cpp -- the entry points of the variance-guided a-trous filter of include/mipt.h
// (mipt_denoise_variance_workspace_bytes, mipt_denoise_variance, mipt_denoise_variance_device): argument checks, the filter constants,
// device staging for the host entry and the launches of denoise_variance.hip.  Host C++ only; every device operation is stream-ordered
// HIP.
#include "../../include/mipt.h"
#include "pt_kernel.h"
#include "mipt_host_util.h"

#include <cmath>
#include <cstring>

static_assert(sizeof(MiptVarianceOptions) == 64 && sizeof(MiptVarianceBuffers) == 128, "ABI struct sizes (tests/test_variance_model.py)");

namespace {

using mipt::fail;

constexpr uint64_t kWorkspaceBytesPerPixel = 3 * sizeof(float4);     // the guide plane and two colour planes

constexpr int kBuffers = 8, kInputs = 6, kHdr = 0, kVariance = 4, kLength = 5, kOut = 6;
struct BufferField { const char *name; uint32_t words; };           // in the order of MiptVarianceBuffers; every value is 4 bytes
constexpr BufferField kFields[kBuffers] = {{"hdr", 3}, {"normal", 3}, {"depth", 1}, {"albedo", 3}, {"variance", 1}, {"length", 1},
                                           {"out", 3}, {"variance_out", 1}};

void unpack(const MiptVarianceBuffers *b, const void *p[kBuffers]) {
    p[0] = b->hdr; p[1] = b->normal; p[2] = b->depth; p[3] = b->albedo; p[4] = b->variance; p[5] = b->length; p[6] = b->out;
    p[7] = b->variance_out;
}

// 1 / sigma^2 in f32 as include/mipt.h forms it; false unless sigma and the result are finite and greater than 0
bool inverse_square(float sigma, float *k) {
    if (!std::isfinite(sigma) || !(sigma > 0.0f)) return false;
    *k = 1.0f / (sigma * sigma);
    return std::isfinite(*k) && *k > 0.0f;
}

// everything that needs no device: on success d holds the sizes and the filter constants
int validate(const char *who, const MiptVarianceOptions *opt, const MiptVarianceBuffers *buf, mipt::DevVariance &d, uint64_t &n_pix) {
    if (!opt) return fail(MIPT_ERR_INVALID_ARG, "%s: null opt", who);
    if (!buf) return fail(MIPT_ERR_INVALID_ARG, "%s: null buffers", who);
    if (!buf->hdr) return fail(MIPT_ERR_INVALID_ARG, "%s: null hdr", who);
    if (!buf->out) return fail(MIPT_ERR_INVALID_ARG, "%s: null out", who);
    if (!buf->variance != !buf->length)
        return fail(MIPT_ERR_INVALID_ARG, "%s: null %s: variance and length are given together or not at all", who, buf->variance ? "length" : "variance");
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

    d = mipt::DevVariance{};
    if (!std::isfinite(opt->sigma_luminance) || !(opt->sigma_luminance > 0.0f))
        return fail(MIPT_ERR_INVALID_ARG, "%s: sigma_luminance must be finite and greater than 0", who);
    if (!std::isfinite(opt->short_history) || !(opt->short_history >= 0.0f))
        return fail(MIPT_ERR_INVALID_ARG, "%s: short_history must be finite and at least 0", who);
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
            if (!p[i] || !p[j] || (i == kHdr && j == kOut && p[i] == p[j])) continue;
            if (mipt::ranges_overlap(p[i], n_pix * kFields[i].words * 4, p[j], n_pix * kFields[j].words * 4))
                return fail(MIPT_ERR_INVALID_ARG, "%s: %s overlaps %s (only out == hdr is allowed)", who, kFields[j].name, kFields[i].name);
        }

    d.hdr = buf->hdr; d.normal = buf->normal; d.depth = buf->depth; d.albedo = buf->albedo; d.variance = buf->variance; d.length = buf->length;
    d.out = buf->out; d.variance_out = buf->variance_out;
    d.width = opt->width; d.height = opt->height; d.n_views = opt->n_views; d.iterations = opt->iterations;
    d.tiles_x = (opt->width + 63u) / 64u;
    d.tiles_y = (opt->height + 3u) / 4u;
    d.sigma_l = opt->sigma_luminance;
    d.short_history = opt->short_history;
    return MIPT_OK;
}

void set_workspace(mipt::DevVariance &d, void *workspace, uint64_t n_pix) {
    d.guides = (float4 *)workspace;
    d.colour[0] = d.guides + n_pix;
    d.colour[1] = d.guides + 2 * n_pix;
}

int variance_device(const MiptVarianceOptions *opt, const MiptVarianceBuffers *buf, void *d_workspace, uint64_t workspace_bytes, void *hip_stream) {
    const char *who = "mipt_denoise_variance_device";
    mipt::DevVariance d;
    uint64_t n_pix = 0;
    int rc = validate(who, opt, buf, d, n_pix);
    if (rc) return rc;
    const uint64_t need = n_pix * kWorkspaceBytesPerPixel;
    if (!d_workspace) return fail(MIPT_ERR_INVALID_ARG, "%s: null workspace", who);
    if (workspace_bytes < need)
        return fail(MIPT_ERR_INVALID_ARG, "%s: workspace of %llu bytes is too small: mipt_denoise_variance_workspace_bytes() is %llu", who,
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
    MIPT_HIP(mipt::launch_denoise_variance(d, (hipStream_t)hip_stream));
    return MIPT_OK;
}

int variance_host(const MiptVarianceOptions *opt, const MiptVarianceBuffers *buf, int device_id) {
    const char *who = "mipt_denoise_variance";
    mipt::DevVariance d;
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
    mipt::DevPtr<float> dev[kInputs];                            // hdr ... length; the result replaces hdr's copy (out == hdr)
    mipt::DevPtr<float> variance_out;
    mipt::DevPtr<float4> workspace;
    for (int i = 0; i < kInputs; i++)
        if (h[i]) {
            MIPT_HIP(dev[i].alloc(n_pix * kFields[i].words));
            MIPT_HIP(hipMemcpy(dev[i].get(), h[i], n_pix * kFields[i].words * sizeof(float), hipMemcpyHostToDevice));
        }
    if (buf->variance_out) MIPT_HIP(variance_out.alloc(n_pix));
    MIPT_HIP(workspace.alloc(n_pix * 3));
    d.hdr = dev[kHdr].get(); d.normal = dev[1].get(); d.depth = dev[2].get(); d.albedo = dev[3].get();
    d.variance = dev[kVariance].get(); d.length = dev[kLength].get();
    d.out = dev[kHdr].get(); d.variance_out = variance_out.get();
    set_workspace(d, workspace.get(), n_pix);
    MIPT_HIP(mipt::launch_denoise_variance(d, nullptr));
    MIPT_HIP(hipMemcpy(buf->out, dev[kHdr].get(), n_pix * 3 * sizeof(float), hipMemcpyDeviceToHost));   // ordered after the passes: blocks until done
    if (buf->variance_out) MIPT_HIP(hipMemcpy(buf->variance_out, variance_out.get(), n_pix * sizeof(float), hipMemcpyDeviceToHost));
    return MIPT_OK;
}

} // namespace

extern "C" {

uint64_t mipt_denoise_variance_workspace_bytes(uint32_t width, uint32_t height, uint32_t n_views) {
    return mipt::batch_pixels(width, height, n_views) * kWorkspaceBytesPerPixel;
}
int mipt_denoise_variance(const MiptVarianceOptions *opt, const MiptVarianceBuffers *host, int device_id) {
    MIPT_NO_THROW(variance_host(opt, host, device_id))
}
int mipt_denoise_variance_device(const MiptVarianceOptions *opt, const MiptVarianceBuffers *device, void *d_workspace,
                                 uint64_t workspace_bytes, void *hip_stream) {
    MIPT_NO_THROW(variance_device(opt, device, d_workspace, workspace_bytes, hip_stream))
}

} // extern "C"
