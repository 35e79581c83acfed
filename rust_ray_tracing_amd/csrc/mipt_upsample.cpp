// mipt_upsample.cpp -- the entry points of the guided upsampling of include/mipt.h (mipt_upsample_workspace_bytes, mipt_upsample,
// mipt_upsample_device): argument checks, the filter constants, device staging for the host entry and the launches of upsample.hip.
// Host C++ only; every device operation is stream-ordered HIP.
#include "../../include/mipt.h"
#include "pt_kernel.h"
#include "mipt_host_util.h"

#include <cmath>
#include <cstring>

static_assert(sizeof(MiptUpsampleOptions) == 64 && sizeof(MiptUpsampleBuffers) == 128, "ABI struct sizes (tests/test_upsample_model.py)");

namespace {

using mipt::fail;

constexpr uint64_t kWorkspaceBytesPerLowPixel = 2 * sizeof(float4);   // the colour plane and the guide plane

constexpr int kBuffers = 11, kInputs = 9, kLowPlanes = 5, kOut = 9, kWeight = 10;
struct BufferField { const char *name; uint32_t words; bool low; };    // in the order of MiptUpsampleBuffers; every value is 4 bytes
constexpr BufferField kFields[kBuffers] = {{"lo_hdr", 3, true}, {"lo_normal", 3, true}, {"lo_depth", 1, true}, {"lo_albedo", 3, true},
                                           {"lo_material", 1, true}, {"normal", 3, false}, {"depth", 1, false}, {"albedo", 3, false},
                                           {"material", 1, false}, {"out", 3, false}, {"weight", 1, false}};

void unpack(const MiptUpsampleBuffers *b, const void *p[kBuffers]) {
    p[0] = b->lo_hdr; p[1] = b->lo_normal; p[2] = b->lo_depth; p[3] = b->lo_albedo; p[4] = b->lo_material;
    p[5] = b->normal; p[6] = b->depth; p[7] = b->albedo; p[8] = b->material; p[9] = b->out; p[10] = b->weight;
}

// 1 / sigma^2 in f32 as include/mipt.h forms it; false unless sigma and the result are finite and greater than 0
bool inverse_square(float sigma, float *k) {
    if (!std::isfinite(sigma) || !(sigma > 0.0f)) return false;
    *k = 1.0f / (sigma * sigma);
    return std::isfinite(*k) && *k > 0.0f;
}

struct Sizes { uint64_t n_pix, n_lo; };
uint64_t bytes_of(int field, const Sizes &s) { return (kFields[field].low ? s.n_lo : s.n_pix) * kFields[field].words * 4; }

// everything that needs no device: on success d holds the sizes, the filter constants and the caller's pointers
int validate(const char *who, const MiptUpsampleOptions *opt, const MiptUpsampleBuffers *buf, mipt::DevUpsample &d, Sizes &s) {
    if (!opt) return fail(MIPT_ERR_INVALID_ARG, "%s: null opt", who);
    if (!buf) return fail(MIPT_ERR_INVALID_ARG, "%s: null buffers", who);
    if (!buf->lo_hdr) return fail(MIPT_ERR_INVALID_ARG, "%s: null lo_hdr", who);
    if (!buf->out) return fail(MIPT_ERR_INVALID_ARG, "%s: null out", who);
    if (opt->width == 0 || opt->height == 0) return fail(MIPT_ERR_INVALID_ARG, "%s: width and height must be greater than 0", who);
    if (opt->n_views == 0) return fail(MIPT_ERR_INVALID_ARG, "%s: n_views == 0", who);
    if (opt->scale < 2 || opt->scale > 8) return fail(MIPT_ERR_INVALID_ARG, "%s: scale %u: must be 2 ... 8", who, opt->scale);
    if (opt->width % opt->scale) return fail(MIPT_ERR_INVALID_ARG, "%s: width %u is not a multiple of scale %u", who, opt->width, opt->scale);
    if (opt->height % opt->scale) return fail(MIPT_ERR_INVALID_ARG, "%s: height %u is not a multiple of scale %u", who, opt->height, opt->scale);
    s.n_pix = mipt::batch_pixels(opt->width, opt->height, opt->n_views);
    if (s.n_pix == 0)
        return fail(MIPT_ERR_INVALID_ARG, "%s: %u views of %ux%u: n_views*width*height must stay below 2^32", who, opt->n_views, opt->width, opt->height);
    s.n_lo = s.n_pix / ((uint64_t)opt->scale * opt->scale);
    if (opt->flags) return fail(MIPT_ERR_INVALID_ARG, "%s: flags 0x%x: must be 0", who, opt->flags);
    for (uint32_t r : opt->reserved)
        if (r) return fail(MIPT_ERR_INVALID_ARG, "%s: reserved option fields must be 0", who);
    for (const void *r : buf->reserved)
        if (r) return fail(MIPT_ERR_INVALID_ARG, "%s: reserved buffer pointers must be NULL", who);

    const void *p[kBuffers];
    unpack(buf, p);
    // a guide is given at both resolutions or at neither
    for (int i = 1; i < kLowPlanes; i++)
        if (!p[i] != !p[i + 4])
            return fail(MIPT_ERR_INVALID_ARG, "%s: null %s: %s is given at both resolutions or at neither", who, kFields[p[i] ? i + 4 : i].name,
                        kFields[i + 4].name);

    d = mipt::DevUpsample{};
    // a sigma given for an absent guide is ignored
    if (buf->normal && !inverse_square(opt->sigma_normal, &d.kn))
        return fail(MIPT_ERR_INVALID_ARG, "%s: sigma_normal %g: it and 1 / sigma_normal^2 must be finite and greater than 0", who, (double)opt->sigma_normal);
    if (buf->depth && !inverse_square(opt->sigma_depth, &d.kz))
        return fail(MIPT_ERR_INVALID_ARG, "%s: sigma_depth %g: it and 1 / sigma_depth^2 must be finite and greater than 0", who, (double)opt->sigma_depth);

    // nothing may alias
    for (int i = 0; i < kBuffers; i++)
        for (int j = i + 1; j < kBuffers; j++) {
            if (!p[i] || !p[j]) continue;
            if (mipt::ranges_overlap(p[i], bytes_of(i, s), p[j], bytes_of(j, s)))
                return fail(MIPT_ERR_INVALID_ARG, "%s: %s overlaps %s", who, kFields[j].name, kFields[i].name);
        }

    d.lo_hdr = buf->lo_hdr; d.lo_normal = buf->lo_normal; d.lo_depth = buf->lo_depth; d.lo_albedo = buf->lo_albedo; d.lo_material = buf->lo_material;
    d.normal = buf->normal; d.depth = buf->depth; d.albedo = buf->albedo; d.material = buf->material;
    d.out = buf->out; d.weight = buf->weight;
    d.width = opt->width; d.height = opt->height; d.n_views = opt->n_views; d.scale = opt->scale;
    d.lo_width = opt->width / opt->scale; d.lo_height = opt->height / opt->scale;
    d.tiles_x = (d.width + 63u) / 64u; d.tiles_y = (d.height + 3u) / 4u;
    d.lo_tiles_x = (d.lo_width + 63u) / 64u; d.lo_tiles_y = (d.lo_height + 3u) / 4u;
    return MIPT_OK;
}

void set_workspace(mipt::DevUpsample &d, void *workspace, uint64_t n_lo) {
    d.colour = (float4 *)workspace;
    d.guides = d.colour + n_lo;
}

int upsample_device(const MiptUpsampleOptions *opt, const MiptUpsampleBuffers *buf, void *d_workspace, uint64_t workspace_bytes, void *hip_stream) {
    const char *who = "mipt_upsample_device";
    mipt::DevUpsample d;
    Sizes s{};
    int rc = validate(who, opt, buf, d, s);
    if (rc) return rc;
    const uint64_t need = s.n_lo * kWorkspaceBytesPerLowPixel;
    if (!d_workspace) return fail(MIPT_ERR_INVALID_ARG, "%s: null workspace", who);
    if (workspace_bytes < need)
        return fail(MIPT_ERR_INVALID_ARG, "%s: workspace of %llu bytes is too small: mipt_upsample_workspace_bytes() is %llu", who,
                    (unsigned long long)workspace_bytes, (unsigned long long)need);
    if ((uintptr_t)d_workspace & 15u) return fail(MIPT_ERR_INVALID_ARG, "%s: workspace must be 16-byte aligned", who);
    const void *p[kBuffers];
    unpack(buf, p);
    for (int i = 0; i < kBuffers; i++) {
        if ((uintptr_t)p[i] & 3u) return fail(MIPT_ERR_INVALID_ARG, "%s: %s must be 4-byte aligned", who, kFields[i].name);
        if (p[i] && mipt::ranges_overlap(p[i], bytes_of(i, s), d_workspace, need))
            return fail(MIPT_ERR_INVALID_ARG, "%s: %s overlaps the workspace", who, kFields[i].name);
    }
    int device = -1;
    if ((rc = mipt::device_buffer_check(who, buf->lo_hdr, -1, "lo_hdr", "", &device))) return rc;
    for (int i = 1; i < kBuffers; i++)
        if (p[i] && (rc = mipt::device_buffer_check(who, p[i], device, kFields[i].name, "lo_hdr's device"))) return rc;
    if ((rc = mipt::device_buffer_check(who, d_workspace, device, "workspace", "lo_hdr's device"))) return rc;
    MIPT_HIP(hipSetDevice(device));
    set_workspace(d, d_workspace, s.n_lo);
    MIPT_HIP(mipt::launch_upsample(d, (hipStream_t)hip_stream));
    return MIPT_OK;
}

int upsample_host(const MiptUpsampleOptions *opt, const MiptUpsampleBuffers *buf, int device_id) {
    const char *who = "mipt_upsample";
    mipt::DevUpsample d;
    Sizes s{};
    const int rc = validate(who, opt, buf, d, s);
    if (rc) return rc;
    const hipError_t e = hipSetDevice(device_id);
    if (e != hipSuccess) {
        (void)hipGetLastError();                                  // or the next launch of this thread would report this ordinal's error
        return fail(MIPT_ERR_HIP, "%s: hipSetDevice(device_id = %d) failed: %s", who, device_id, hipGetErrorString(e));
    }
    const void *h[kBuffers];
    unpack(buf, h);
    mipt::DevPtr<uint32_t> dev[kInputs];                         // lo_hdr ... material: 4-byte words, floats or ids
    mipt::DevPtr<float> out, weight;
    mipt::DevPtr<float4> workspace;
    for (int i = 0; i < kInputs; i++)
        if (h[i]) {
            MIPT_HIP(dev[i].alloc(bytes_of(i, s) / 4));
            MIPT_HIP(hipMemcpy(dev[i].get(), h[i], bytes_of(i, s), hipMemcpyHostToDevice));
        }
    MIPT_HIP(out.alloc(s.n_pix * 3));
    if (buf->weight) MIPT_HIP(weight.alloc(s.n_pix));
    MIPT_HIP(workspace.alloc(s.n_lo * 2));
    d.lo_hdr = (const float *)dev[0].get(); d.lo_normal = (const float *)dev[1].get(); d.lo_depth = (const float *)dev[2].get();
    d.lo_albedo = (const float *)dev[3].get(); d.lo_material = dev[4].get();
    d.normal = (const float *)dev[5].get(); d.depth = (const float *)dev[6].get(); d.albedo = (const float *)dev[7].get(); d.material = dev[8].get();
    d.out = out.get(); d.weight = weight.get();
    set_workspace(d, workspace.get(), s.n_lo);
    MIPT_HIP(mipt::launch_upsample(d, nullptr));
    MIPT_HIP(hipMemcpy(buf->out, out.get(), bytes_of(kOut, s), hipMemcpyDeviceToHost));   // ordered after the passes: blocks until done
    if (buf->weight) MIPT_HIP(hipMemcpy(buf->weight, weight.get(), bytes_of(kWeight, s), hipMemcpyDeviceToHost));
    return MIPT_OK;
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
