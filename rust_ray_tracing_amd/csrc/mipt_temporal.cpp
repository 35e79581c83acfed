// mipt_temporal.cpp -- the temporal-accumulation entry points of include/mipt.h (mipt_temporal_history_bytes, mipt_temporal,
// mipt_temporal_device, mipt_temporal_counts, mipt_temporal_counts_device): argument checks, the camera records, device staging for
// the host entry and the launches of temporal.hip.
// Host C++ only; every device operation is stream-ordered HIP.
#include "../../include/mipt.h"
#include "pt_kernel.h"
#include "mipt_host_util.h"

#include <cmath>
#include <cstring>
#include <vector>

static_assert(sizeof(MiptTemporalOptions) == 64 && sizeof(MiptTemporalBuffers) == 128, "ABI struct sizes (tests/test_temporal_model.py)");

namespace {

using mipt::fail;

constexpr uint64_t kHeaderBytesPerView = 16 * sizeof(float);
constexpr uint64_t kHistoryBytesPerPixel = 3 * sizeof(float4);

// in the order of MiptTemporalBuffers; bytes = per pixel, 0 = a history (its size comes from history_bytes)
constexpr int kBuffers = 11;
constexpr int kHdr = 0, kAlbedo = 5, kHistoryIn = 6, kHistoryOut = 7, kOut = 8, kLength = 9, kVariance = 10;
struct BufferField { const char *name; uint32_t bytes; bool required; };
constexpr BufferField kFields[kBuffers] = {{"hdr", 12, true},       {"position", 12, true},   {"normal", 12, true}, {"depth", 4, true},
                                           {"material", 4, true},   {"albedo", 12, false},    {"history_in", 0, false},
                                           {"history_out", 0, true}, {"out", 12, true},       {"length", 4, false}, {"variance", 4, false}};

void unpack(const MiptTemporalBuffers *b, const void *p[kBuffers]) {
    p[0] = b->hdr; p[1] = b->position; p[2] = b->normal; p[3] = b->depth; p[4] = b->material; p[5] = b->albedo;
    p[6] = b->history_in; p[7] = b->history_out; p[8] = b->out; p[9] = b->length; p[10] = b->variance;
}

uint64_t history_bytes(uint64_t n_pix, uint32_t n_views) { return kHeaderBytesPerView * n_views + kHistoryBytesPerPixel * n_pix; }

// The camera record of include/mipt.h: B = inverse of a[r][c] = look_at[c][r] in binary64 (this file is built with -ffp-contract=off),
// each entry rounded to f32, then the position and four zeros.  false = singular.
bool camera_record(const MiptCamera &cam, float rec[16]) {
    double a[3][3];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) a[r][c] = (double)cam.look_at[c][r];
    double k[3][3];
    k[0][0] = (a[1][1] * a[2][2]) - (a[1][2] * a[2][1]);
    k[0][1] = (a[1][2] * a[2][0]) - (a[1][0] * a[2][2]);
    k[0][2] = (a[1][0] * a[2][1]) - (a[1][1] * a[2][0]);
    k[1][0] = (a[0][2] * a[2][1]) - (a[0][1] * a[2][2]);
    k[1][1] = (a[0][0] * a[2][2]) - (a[0][2] * a[2][0]);
    k[1][2] = (a[0][1] * a[2][0]) - (a[0][0] * a[2][1]);
    k[2][0] = (a[0][1] * a[1][2]) - (a[0][2] * a[1][1]);
    k[2][1] = (a[0][2] * a[1][0]) - (a[0][0] * a[1][2]);
    k[2][2] = (a[0][0] * a[1][1]) - (a[0][1] * a[1][0]);
    const double det = ((a[0][0] * k[0][0]) + (a[0][1] * k[0][1])) + (a[0][2] * k[0][2]);
    if (!std::isfinite(det) || det == 0.0) return false;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            const float b = (float)(k[j][i] / det);
            if (!std::isfinite(b)) return false;
            rec[i * 3 + j] = b;
        }
    rec[9] = cam.position.x; rec[10] = cam.position.y; rec[11] = cam.position.z;
    rec[12] = rec[13] = rec[14] = rec[15] = 0.0f;
    return true;
}

// The count plane of the _counts entries; `counted` false = the plain entries, which have none.
struct Counts { bool counted; const uint32_t *plane; uint32_t cap; };
constexpr Counts kNoCounts = {false, nullptr, 0u};

// everything that needs no device: on success d holds the sizes, the options and the caller's pointers, records the camera records
int validate(const char *who, const MiptTemporalOptions *opt, const MiptCamera *cameras, const MiptTemporalBuffers *buf, const Counts &cnt,
             mipt::DevTemporal &d, std::vector<float> &records) {
    if (!opt) return fail(MIPT_ERR_INVALID_ARG, "%s: null opt", who);
    if (!cameras) return fail(MIPT_ERR_INVALID_ARG, "%s: null cameras", who);
    if (!buf) return fail(MIPT_ERR_INVALID_ARG, "%s: null buffers", who);
    const void *p[kBuffers];
    unpack(buf, p);
    for (int i = 0; i < kBuffers; i++)
        if (kFields[i].required && !p[i]) return fail(MIPT_ERR_INVALID_ARG, "%s: null %s", who, kFields[i].name);
    if (opt->width == 0 || opt->height == 0) return fail(MIPT_ERR_INVALID_ARG, "%s: width and height must be greater than 0", who);
    if (opt->n_views == 0) return fail(MIPT_ERR_INVALID_ARG, "%s: n_views == 0", who);
    const uint64_t n_pix = mipt::batch_pixels(opt->width, opt->height, opt->n_views);
    if (n_pix == 0)
        return fail(MIPT_ERR_INVALID_ARG, "%s: %u views of %ux%u: n_views*width*height must stay below 2^32", who, opt->n_views, opt->width, opt->height);
    if (opt->flags) return fail(MIPT_ERR_INVALID_ARG, "%s: flags 0x%x: must be 0", who, opt->flags);
    if (!(opt->alpha_min >= 0.0f && opt->alpha_min <= 1.0f))
        return fail(MIPT_ERR_INVALID_ARG, "%s: alpha_min %g: must be 0 ... 1", who, (double)opt->alpha_min);
    if (!std::isfinite(opt->max_history) || !(opt->max_history >= 1.0f))
        return fail(MIPT_ERR_INVALID_ARG, "%s: max_history %g: must be finite and at least 1", who, (double)opt->max_history);
    if (!std::isfinite(opt->normal_tol) || !(opt->normal_tol >= 0.0f))
        return fail(MIPT_ERR_INVALID_ARG, "%s: normal_tol %g: must be finite and at least 0", who, (double)opt->normal_tol);
    if (!std::isfinite(opt->depth_tol) || !(opt->depth_tol >= 0.0f))
        return fail(MIPT_ERR_INVALID_ARG, "%s: depth_tol %g: must be finite and at least 0", who, (double)opt->depth_tol);
    for (uint32_t r : opt->reserved)
        if (r) return fail(MIPT_ERR_INVALID_ARG, "%s: reserved option fields must be 0", who);
    for (const void *r : buf->reserved)
        if (r) return fail(MIPT_ERR_INVALID_ARG, "%s: reserved buffer pointers must be NULL", who);
    if (cnt.counted) {
        if (!cnt.plane) return fail(MIPT_ERR_INVALID_ARG, "%s: null counts", who);
        if (cnt.cap < 1 || cnt.cap > 65535) return fail(MIPT_ERR_INVALID_ARG, "%s: samples_cap %u: must be 1 ... 65535", who, cnt.cap);
    }

    records.assign((size_t)opt->n_views * 16, 0.0f);
    for (uint32_t v = 0; v < opt->n_views; v++)
        if (!camera_record(cameras[v], &records[(size_t)v * 16]))
            return fail(MIPT_ERR_INVALID_ARG, "%s: cameras[%u].look_at is singular or not finite: it has no inverse to reproject with", who, v);

    // out may be hdr itself; nothing else may overlap
    uint64_t bytes[kBuffers];
    for (int i = 0; i < kBuffers; i++) bytes[i] = kFields[i].bytes ? n_pix * kFields[i].bytes : history_bytes(n_pix, opt->n_views);
    for (int i = 0; i < kBuffers; i++)
        for (int j = i + 1; j < kBuffers; j++) {
            if (!p[i] || !p[j] || (i == kHdr && j == kOut && p[i] == p[j])) continue;
            if (mipt::ranges_overlap(p[i], bytes[i], p[j], bytes[j]))
                return fail(MIPT_ERR_INVALID_ARG, "%s: %s overlaps %s (only out == hdr is allowed)", who, kFields[j].name, kFields[i].name);
        }

    d = mipt::DevTemporal{};
    d.hdr = buf->hdr; d.position = buf->position; d.normal = buf->normal; d.depth = buf->depth; d.albedo = buf->albedo;
    d.material = buf->material;
    d.out = buf->out; d.length = buf->length; d.variance = buf->variance;
    d.history_in = (const float *)buf->history_in; d.history_out = (float *)buf->history_out;
    d.n_pixels = n_pix;
    d.width = opt->width; d.height = opt->height; d.n_views = opt->n_views;
    d.tiles_x = (opt->width + 63u) / 64u;
    d.tiles_y = (opt->height + 3u) / 4u;
    d.alpha_min = opt->alpha_min; d.max_history = opt->max_history; d.normal_tol = opt->normal_tol; d.depth_tol = opt->depth_tol;
    return MIPT_OK;
}

int temporal_device(const char *who, const MiptTemporalOptions *opt, const MiptCamera *cameras, const MiptTemporalBuffers *buf, const Counts &cnt,
                    void *hip_stream) {
    mipt::DevTemporal d;
    std::vector<float> records;
    int rc = validate(who, opt, cameras, buf, cnt, d, records);
    if (rc) return rc;
    const void *p[kBuffers];
    unpack(buf, p);
    if (cnt.counted) {
        if ((uintptr_t)cnt.plane & 3u) return fail(MIPT_ERR_INVALID_ARG, "%s: counts must be 4-byte aligned", who);
        for (int i = 0; i < kBuffers; i++) {
            const uint64_t bytes = kFields[i].bytes ? d.n_pixels * kFields[i].bytes : history_bytes(d.n_pixels, d.n_views);
            if (p[i] && mipt::ranges_overlap(cnt.plane, d.n_pixels * 4, p[i], bytes))
                return fail(MIPT_ERR_INVALID_ARG, "%s: counts overlaps %s", who, kFields[i].name);
        }
    }
    for (int i = 0; i < kBuffers; i++) {
        const uintptr_t mask = kFields[i].bytes ? 3u : 15u;
        if ((uintptr_t)p[i] & mask) return fail(MIPT_ERR_INVALID_ARG, "%s: %s must be %u-byte aligned", who, kFields[i].name, (unsigned)mask + 1u);
    }
    int device = -1;
    if ((rc = mipt::device_buffer_check(who, buf->hdr, -1, "hdr", "", &device))) return rc;
    for (int i = 1; i < kBuffers; i++)
        if (p[i] && (rc = mipt::device_buffer_check(who, p[i], device, kFields[i].name, "hdr's device"))) return rc;
    if (cnt.counted && (rc = mipt::device_buffer_check(who, cnt.plane, device, "counts", "hdr's device"))) return rc;
    MIPT_HIP(hipSetDevice(device));
    MIPT_HIP(mipt::launch_temporal(d, records.data(), (hipStream_t)hip_stream, cnt.plane, cnt.cap));
    return MIPT_OK;
}

int temporal_host(const char *who, const MiptTemporalOptions *opt, const MiptCamera *cameras, const MiptTemporalBuffers *buf, const Counts &cnt,
                  int device_id) {
    mipt::DevTemporal d;
    std::vector<float> records;
    const int rc = validate(who, opt, cameras, buf, cnt, d, records);
    if (rc) return rc;
    const hipError_t e = hipSetDevice(device_id);
    if (e != hipSuccess) {
        (void)hipGetLastError();                                  // or the next launch of this thread would report this ordinal's error
        return fail(MIPT_ERR_HIP, "%s: hipSetDevice(device_id = %d) failed: %s", who, device_id, hipGetErrorString(e));
    }
    const uint64_t n_pix = d.n_pixels, hist = history_bytes(n_pix, d.n_views);
    const void *h[kBuffers];
    unpack(buf, h);
    mipt::DevPtr<unsigned char> dev[kBuffers];                   // the result replaces hdr's copy (out == hdr); dev[kOut] stays empty
    for (int i = 0; i < kBuffers; i++) {
        if (!h[i] || i == kOut) continue;
        const uint64_t bytes = kFields[i].bytes ? n_pix * kFields[i].bytes : hist;
        MIPT_HIP(dev[i].alloc(bytes));
        if (i < kHistoryOut) MIPT_HIP(hipMemcpy(dev[i].get(), h[i], bytes, hipMemcpyHostToDevice));
    }
    mipt::DevPtr<uint32_t> d_counts;
    if (cnt.counted) {
        MIPT_HIP(d_counts.alloc((size_t)n_pix));
        MIPT_HIP(hipMemcpy(d_counts.get(), cnt.plane, n_pix * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    d.hdr = (const float *)dev[0].get(); d.position = (const float *)dev[1].get(); d.normal = (const float *)dev[2].get();
    d.depth = (const float *)dev[3].get(); d.material = (const uint32_t *)dev[4].get(); d.albedo = (const float *)dev[kAlbedo].get();
    d.history_in = (const float *)dev[kHistoryIn].get(); d.history_out = (float *)dev[kHistoryOut].get();
    d.out = (float *)dev[kHdr].get(); d.length = (float *)dev[kLength].get(); d.variance = (float *)dev[kVariance].get();
    MIPT_HIP(mipt::launch_temporal(d, records.data(), nullptr, d_counts.get(), cnt.cap));
    // ordered after the launches on the null stream: each copy blocks until they are done
    MIPT_HIP(hipMemcpy(buf->history_out, dev[kHistoryOut].get(), hist, hipMemcpyDeviceToHost));
    MIPT_HIP(hipMemcpy(buf->out, dev[kHdr].get(), n_pix * 12, hipMemcpyDeviceToHost));
    if (buf->length) MIPT_HIP(hipMemcpy(buf->length, dev[kLength].get(), n_pix * 4, hipMemcpyDeviceToHost));
    if (buf->variance) MIPT_HIP(hipMemcpy(buf->variance, dev[kVariance].get(), n_pix * 4, hipMemcpyDeviceToHost));
    return MIPT_OK;
}

} // namespace

extern "C" {

uint64_t mipt_temporal_history_bytes(uint32_t width, uint32_t height, uint32_t n_views) {
    const uint64_t n_pix = mipt::batch_pixels(width, height, n_views);
    return n_pix ? history_bytes(n_pix, n_views) : 0;
}
int mipt_temporal(const MiptTemporalOptions *opt, const MiptCamera *cameras, const MiptTemporalBuffers *host, int device_id) {
    MIPT_NO_THROW(temporal_host("mipt_temporal", opt, cameras, host, kNoCounts, device_id))
}
int mipt_temporal_device(const MiptTemporalOptions *opt, const MiptCamera *cameras, const MiptTemporalBuffers *device, void *hip_stream) {
    MIPT_NO_THROW(temporal_device("mipt_temporal_device", opt, cameras, device, kNoCounts, hip_stream))
}
int mipt_temporal_counts(const MiptTemporalOptions *opt, const MiptCamera *cameras, const MiptTemporalBuffers *host, const uint32_t *counts,
                         uint32_t samples_cap, int device_id) {
    const Counts cnt = {true, counts, samples_cap};
    MIPT_NO_THROW(temporal_host("mipt_temporal_counts", opt, cameras, host, cnt, device_id))
}
int mipt_temporal_counts_device(const MiptTemporalOptions *opt, const MiptCamera *cameras, const MiptTemporalBuffers *device,
                                const uint32_t *d_counts, uint32_t samples_cap, void *hip_stream) {
    const Counts cnt = {true, d_counts, samples_cap};
    MIPT_NO_THROW(temporal_device("mipt_temporal_counts_device", opt, cameras, device, cnt, hip_stream))
}

} // extern "C"
