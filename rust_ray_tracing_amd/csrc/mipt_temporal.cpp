// mipt_temporal.cpp -- the temporal-accumulation entry points of include/mipt.h (mipt_temporal_history_bytes, mipt_temporal,
// mipt_temporal_device, mipt_temporal_counts, mipt_temporal_counts_device): the plane table, the checks of the blend's own options,
// the camera records and the launches of temporal.hip.  The checks every image-space entry makes, the device-entry checks and the host
// entry's staging are mipt_planes.h's and mipt_host_util.h's.  Host C++ only; every device operation is stream-ordered HIP.
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

// in the order of MiptTemporalBuffers, then the count plane of the _counts entries, which is an argument of its own; pixel_bytes 0 =
// a history (history_bytes)
constexpr int kBuffers = 11, kHdr = 0, kHistoryIn = 6, kHistoryOut = 7, kCounts = 11;
constexpr mipt::Plane kPlanes[kBuffers + 1] = {
    {"hdr", 12, 4, true, mipt::kPlaneIn, -1},      {"position", 12, 4, true, mipt::kPlaneIn, -1},  {"normal", 12, 4, true, mipt::kPlaneIn, -1},
    {"depth", 4, 4, true, mipt::kPlaneIn, -1},     {"material", 4, 4, true, mipt::kPlaneIn, -1},   {"albedo", 12, 4, false, mipt::kPlaneIn, -1},
    {"history_in", 0, 16, false, mipt::kPlaneIn, -1}, {"history_out", 0, 16, true, mipt::kPlaneOut, -1}, {"out", 12, 4, true, mipt::kPlaneOut, kHdr},
    {"length", 4, 4, false, mipt::kPlaneOut, -1},  {"variance", 4, 4, false, mipt::kPlaneOut, -1}, {"counts", 4, 4, false, mipt::kPlaneIn, -1}};
static_assert(kBuffers + 1 <= mipt::kMaxPlanes, "a PlaneSet holds the table");

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

// everything that needs no device: on success d holds the sizes and the options, set the caller's planes -- the count plane last, which
// the checks here do not hold against the others -- and records the camera records
int validate(const char *who, const MiptTemporalOptions *opt, const MiptCamera *cameras, const MiptTemporalBuffers *buf, const Counts &cnt,
             mipt::DevTemporal &d, mipt::PlaneSet &set, std::vector<float> &records) {
    int rc;
    if ((rc = mipt::not_null(who, opt, "opt")) || (rc = mipt::not_null(who, cameras, "cameras")) || (rc = mipt::not_null(who, buf, "buffers"))) return rc;
    mipt::planes_bind(set, kPlanes, kBuffers, buf);
    uint64_t n_pix = 0;
    if ((rc = mipt::planes_required(who, set)) || (rc = mipt::frame_nonzero(who, opt->width, opt->height, opt->n_views)) ||
        (rc = mipt::frame_pixels(who, opt->width, opt->height, opt->n_views, &n_pix)) || (rc = mipt::flags_zero(who, opt->flags)))
        return rc;
    if (!(opt->alpha_min >= 0.0f && opt->alpha_min <= 1.0f))
        return fail(MIPT_ERR_INVALID_ARG, "%s: alpha_min %g: must be 0 ... 1", who, (double)opt->alpha_min);
    if (!std::isfinite(opt->max_history) || !(opt->max_history >= 1.0f))
        return fail(MIPT_ERR_INVALID_ARG, "%s: max_history %g: must be finite and at least 1", who, (double)opt->max_history);
    if (!std::isfinite(opt->normal_tol) || !(opt->normal_tol >= 0.0f))
        return fail(MIPT_ERR_INVALID_ARG, "%s: normal_tol %g: must be finite and at least 0", who, (double)opt->normal_tol);
    if (!std::isfinite(opt->depth_tol) || !(opt->depth_tol >= 0.0f))
        return fail(MIPT_ERR_INVALID_ARG, "%s: depth_tol %g: must be finite and at least 0", who, (double)opt->depth_tol);
    if ((rc = mipt::reserved_zero(who, opt->reserved, buf->reserved))) return rc;
    if (cnt.counted) {
        if (!cnt.plane) return fail(MIPT_ERR_INVALID_ARG, "%s: null counts", who);
        if (cnt.cap < 1 || cnt.cap > 65535) return fail(MIPT_ERR_INVALID_ARG, "%s: samples_cap %u: must be 1 ... 65535", who, cnt.cap);
    }

    records.assign((size_t)opt->n_views * 16, 0.0f);
    for (uint32_t v = 0; v < opt->n_views; v++)
        if (!camera_record(cameras[v], &records[(size_t)v * 16]))
            return fail(MIPT_ERR_INVALID_ARG, "%s: cameras[%u].look_at is singular or not finite: it has no inverse to reproject with", who, v);

    mipt::planes_size(set, n_pix);
    set.bytes[kHistoryIn] = set.bytes[kHistoryOut] = history_bytes(n_pix, opt->n_views);
    if ((rc = mipt::planes_disjoint(who, set))) return rc;
    set.n = kBuffers + 1;
    set.ptr[kCounts] = cnt.plane;
    set.bytes[kCounts] = n_pix * kPlanes[kCounts].pixel_bytes;

    d = mipt::DevTemporal{};
    d.n_pixels = n_pix;
    d.width = opt->width; d.height = opt->height; d.n_views = opt->n_views;
    d.tiles_x = mipt::tiles_across(opt->width);
    d.tiles_y = mipt::tiles_down(opt->height);
    d.alpha_min = opt->alpha_min; d.max_history = opt->max_history; d.normal_tol = opt->normal_tol; d.depth_tol = opt->depth_tol;
    return MIPT_OK;
}

// the planes: the caller's, or the host entry's staged copies
void point(mipt::DevTemporal &d, const void *const p[]) {
    d.hdr = (const float *)p[0]; d.position = (const float *)p[1]; d.normal = (const float *)p[2]; d.depth = (const float *)p[3];
    d.material = (const uint32_t *)p[4]; d.albedo = (const float *)p[5];
    d.history_in = (const float *)p[kHistoryIn]; d.history_out = (float *)p[kHistoryOut];
    d.out = (float *)p[8]; d.length = (float *)p[9]; d.variance = (float *)p[10];
}

int temporal_device(const char *who, const MiptTemporalOptions *opt, const MiptCamera *cameras, const MiptTemporalBuffers *buf, const Counts &cnt,
                    void *hip_stream) {
    mipt::DevTemporal d;
    mipt::PlaneSet set;
    std::vector<float> records;
    int rc = validate(who, opt, cameras, buf, cnt, d, set, records);
    if (rc) return rc;
    // the count plane against the others, before their own alignment
    if ((rc = mipt::plane_aligned(who, set, kCounts))) return rc;
    for (int i = 0; i < kBuffers; i++)
        if (cnt.plane && set.ptr[i] && mipt::ranges_overlap(cnt.plane, set.bytes[kCounts], set.ptr[i], set.bytes[i]))
            return fail(MIPT_ERR_INVALID_ARG, "%s: counts overlaps %s", who, kPlanes[i].name);
    if ((rc = mipt::device_entry_check(who, set, nullptr))) return rc;
    point(d, set.ptr);
    MIPT_HIP(mipt::launch_temporal(d, records.data(), (hipStream_t)hip_stream, cnt.plane, cnt.cap));
    return MIPT_OK;
}

int temporal_host(const char *who, const MiptTemporalOptions *opt, const MiptCamera *cameras, const MiptTemporalBuffers *buf, const Counts &cnt,
                  int device_id) {
    mipt::DevTemporal d;
    mipt::PlaneSet set;
    std::vector<float> records;
    int rc = validate(who, opt, cameras, buf, cnt, d, set, records);
    if (rc || (rc = mipt::select_device(who, device_id))) return rc;
    mipt::StagedPlanes staged;
    if ((rc = staged.stage(set))) return rc;
    point(d, staged.ptr);
    MIPT_HIP(mipt::launch_temporal(d, records.data(), nullptr, (const uint32_t *)staged.ptr[kCounts], cnt.cap));
    return staged.fetch(set);
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
