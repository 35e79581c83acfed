// mipt_probe.cpp -- the irradiance-probe entry points of include/mipt.h (mipt_probe_bake, mipt_probe_irradiance and their _device
// forms): argument checks and the launches of probe.hip's kernels; the bake traces in chunks through mipt::chunked_trace (mipt_scene.h),
// as the gather of mipt_bake.cpp does.  Host C++ only; every device operation is stream-ordered HIP.
#include "../../include/mipt.h"
#include "pt_kernel.h"
#include "mipt_scene.h"                                          // and with it mipt_host_util.h, mipt_internal.h

#include <cmath>
#include <cstring>

static_assert(sizeof(MiptProbe) == 16 && sizeof(MiptProbeBakeOptions) == 64, "ABI struct sizes (tests/test_probe_abi.py)");
static_assert(sizeof(MiptProbeGrid) == 64 && sizeof(MiptProbeIrradianceBuffers) == 64, "ABI struct sizes (tests/test_probe_abi.py)");
static_assert(sizeof(MiptProbeBakeOptions) == sizeof(MiptBakeOptions) && offsetof(MiptProbeBakeOptions, first_sample) == offsetof(MiptBakeOptions, first_sample) &&
                  offsetof(MiptProbeBakeOptions, sample_stride) == offsetof(MiptBakeOptions, sample_stride) &&
                  offsetof(MiptProbeBakeOptions, reserved) == offsetof(MiptBakeOptions, reserved),
              "field for field MiptBakeOptions");
static_assert(sizeof(MiptProbe) == sizeof(float4), "a probe is one float4 load");

namespace {

using mipt::fail;

constexpr uint64_t kShWords = 27;                                // 9 coefficients x RGB per probe

// ---- bake --------------------------------------------------------------------------------------------------------------------------
int bake_check(const char *who, const MiptScene *scene, const void *probes, uint64_t n, const MiptProbeBakeOptions *opt, const void *sh,
               bool device_entry) {
    return mipt::chunked_entry_check(who, !scene || !probes || !opt || !sh, "null scene, probes, options or sh", "probe", n, opt,
                                     device_entry ? nullptr : "mipt_probe_bake_device");
}

// The bake with every argument already checked; d_probes / d_sh in HBM of the scene's device, n > 0
int bake_launch(MiptScene *scene, const MiptProbe *d_probes, uint64_t n, const MiptProbeBakeOptions *opt, float *d_sh, hipStream_t stream,
                MiptStats *stats) {
    auto gen = [&](const mipt::PathChunk &c, float4 *d_rays, hipStream_t s) { return mipt::launch_probe_rays(d_probes, c, d_rays, scene->n_cu, s); };
    auto fold = [&](const mipt::PathChunk &c, const float4 *d_rays, const float *d_path, hipStream_t s) {
        return mipt::launch_probe_project(c, d_rays, d_path, d_sh, scene->n_cu, s);
    };
    return mipt::chunked_trace(scene, n, *opt, stream, stats, gen, fold);
}

int bake_device(MiptScene *scene, const MiptProbe *d_probes, uint64_t n, const MiptProbeBakeOptions *opt, float *d_sh, void *hip_stream,
                MiptStats *stats) {
    const char *who = "mipt_probe_bake_device";
    int rc = bake_check(who, scene, d_probes, n, opt, d_sh, true);
    if (rc) return rc;
    const mipt::ItemBuffers b{"d_probes", d_probes, n * sizeof(MiptProbe), "d_sh", d_sh, n * kShWords * sizeof(float), 4, true, true};
    return mipt::device_call(who, scene, b, n == 0, stats, [&] { return bake_launch(scene, d_probes, n, opt, d_sh, (hipStream_t)hip_stream, stats); });
}

int bake_host(MiptScene *scene, const MiptProbe *probes, uint64_t n, const MiptProbeBakeOptions *opt, float *sh, MiptStats *stats) {
    const char *who = "mipt_probe_bake";
    int rc = bake_check(who, scene, probes, n, opt, sh, false);
    if (rc) return rc;
    if (stats) memset(stats, 0, sizeof *stats);
    if (n == 0) return MIPT_OK;
    return mipt::staged_call(scene, probes, (size_t)n * sizeof(MiptProbe), sh, (size_t)n * kShWords * sizeof(float), [&](const void *d_probes, void *d_out) {
        return bake_launch(scene, (const MiptProbe *)d_probes, n, opt, (float *)d_out, nullptr, stats);
    });
}

// ---- lookup ------------------------------------------------------------------------------------------------------------------------
// in the order of MiptProbeIrradianceBuffers; sh and valid are sized by the grid, the others by the points (lookup_validate)
constexpr int kLookupBuffers = 5, kIrradiance = 4;
constexpr mipt::Plane kLookupPlanes[kLookupBuffers] = {{"sh", 27 * 4, 4, true, mipt::kPlaneIn, -1}, {"valid", 1, 1, false, mipt::kPlaneIn, -1},
                                                       {"position", 12, 4, true, mipt::kPlaneIn, -1}, {"normal", 12, 4, true, mipt::kPlaneIn, -1},
                                                       {"irradiance", 12, 4, true, mipt::kPlaneOut, -1}};
static_assert(kLookupBuffers <= mipt::kMaxPlanes, "a PlaneSet holds the table");

// everything that needs no device: on success d holds the grid, set the caller's buffers and their sizes
int lookup_validate(const char *who, const MiptProbeGrid *grid, uint64_t n, const MiptProbeIrradianceBuffers *buf, mipt::DevProbeLookup &d,
                    mipt::PlaneSet &set) {
    int rc;
    if ((rc = mipt::not_null(who, grid, "grid")) || (rc = mipt::not_null(who, buf, "buffers"))) return rc;
    if ((rc = mipt::ray_count_check(who, "n", n))) return rc;
    mipt::planes_bind(set, kLookupPlanes, kLookupBuffers, buf);
    if ((rc = mipt::planes_required(who, set))) return rc;
    uint64_t n_probes = 1;
    for (int a = 0; a < 3; a++) {
        if (grid->dims[a] == 0) return fail(MIPT_ERR_INVALID_ARG, "%s: dims %u x %u x %u: every dimension must be greater than 0", who, grid->dims[0], grid->dims[1], grid->dims[2]);
    }
    for (int a = 0; a < 3; a++) {
        n_probes *= grid->dims[a];                                            // each factor < 2^32 and the product checked after every step
        if (n_probes >= MIPT_QUERY_MAX_RAYS)
            return fail(MIPT_ERR_INVALID_ARG, "%s: dims %u x %u x %u: their product must stay below 2^31", who, grid->dims[0], grid->dims[1], grid->dims[2]);
    }
    for (int a = 0; a < 3; a++)
        if (!std::isfinite(grid->spacing[a]) || !(grid->spacing[a] > 0.0f))
            return fail(MIPT_ERR_INVALID_ARG, "%s: spacing[%d] must be finite and greater than 0", who, a);
    if (grid->flags & ~MIPT_PROBE_CLAMP) return fail(MIPT_ERR_INVALID_ARG, "%s: flags 0x%x: only MIPT_PROBE_CLAMP is accepted", who, grid->flags);
    if ((rc = mipt::reserved_zero(who, grid->reserved, buf->reserved))) return rc;
    set.bytes[0] = n_probes * 27 * sizeof(float); set.bytes[1] = n_probes;
    set.bytes[2] = set.bytes[3] = set.bytes[kIrradiance] = n * 12;
    for (int i = 0; i < kIrradiance; i++)
        if (set.ptr[i] && n && mipt::ranges_overlap(set.ptr[i], set.bytes[i], set.ptr[kIrradiance], set.bytes[kIrradiance]))
            return fail(MIPT_ERR_INVALID_ARG, "%s: irradiance overlaps %s", who, set.plane[i].name);
    d = mipt::DevProbeLookup{};
    d.n = n;
    for (int a = 0; a < 3; a++) { d.origin[a] = grid->origin[a]; d.spacing[a] = grid->spacing[a]; d.dims[a] = grid->dims[a]; }
    d.clamp = (grid->flags & MIPT_PROBE_CLAMP) ? 1u : 0u;
    return MIPT_OK;
}

void lookup_point(mipt::DevProbeLookup &d, const void *const p[]) {
    d.sh = (const float *)p[0]; d.valid = (const uint8_t *)p[1]; d.position = (const float *)p[2]; d.normal = (const float *)p[3];
    d.irradiance = (float *)p[4];
}

// on the current device
int lookup_launch(const mipt::DevProbeLookup &d, hipStream_t stream) {
    int device = 0, n_cu = 0;
    MIPT_HIP(hipGetDevice(&device));
    MIPT_HIP(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device));
    MIPT_HIP(mipt::launch_probe_irradiance(d, n_cu, stream));
    return MIPT_OK;
}

int lookup_device(const MiptProbeGrid *grid, uint64_t n, const MiptProbeIrradianceBuffers *buf, void *hip_stream) {
    const char *who = "mipt_probe_irradiance_device";
    mipt::DevProbeLookup d;
    mipt::PlaneSet set;
    int rc = lookup_validate(who, grid, n, buf, d, set);
    if (rc) return rc;
    for (int i = 0; i < set.n; i++)
        if ((rc = mipt::plane_aligned(who, set, i))) return rc;
    if (n == 0) return MIPT_OK;
    if ((rc = mipt::device_entry_check(who, set, nullptr))) return rc;
    lookup_point(d, set.ptr);
    return lookup_launch(d, (hipStream_t)hip_stream);
}

int lookup_host(const MiptProbeGrid *grid, uint64_t n, const MiptProbeIrradianceBuffers *buf, int device_id) {
    const char *who = "mipt_probe_irradiance";
    mipt::DevProbeLookup d;
    mipt::PlaneSet set;
    int rc = lookup_validate(who, grid, n, buf, d, set);
    if (rc || n == 0) return rc;
    if ((rc = mipt::select_device(who, device_id))) return rc;
    mipt::StagedPlanes staged;
    if ((rc = staged.stage(set))) return rc;
    lookup_point(d, staged.ptr);
    if ((rc = lookup_launch(d, nullptr))) return rc;
    return staged.fetch(set);
}

} // namespace

extern "C" {

int mipt_probe_bake(MiptScene *scene, const MiptProbe *probes, uint64_t n, const MiptProbeBakeOptions *opt, float *sh, MiptStats *stats) {
    MIPT_NO_THROW(bake_host(scene, probes, n, opt, sh, stats))
}
int mipt_probe_bake_device(MiptScene *scene, const MiptProbe *d_probes, uint64_t n, const MiptProbeBakeOptions *opt, float *d_sh, void *hip_stream,
                           MiptStats *stats) {
    MIPT_NO_THROW(bake_device(scene, d_probes, n, opt, d_sh, hip_stream, stats))
}
int mipt_probe_irradiance(const MiptProbeGrid *grid, uint64_t n, const MiptProbeIrradianceBuffers *host, int device_id) {
    MIPT_NO_THROW(lookup_host(grid, n, host, device_id))
}
int mipt_probe_irradiance_device(const MiptProbeGrid *grid, uint64_t n, const MiptProbeIrradianceBuffers *device, void *hip_stream) {
    MIPT_NO_THROW(lookup_device(grid, n, device, hip_stream))
}

} // extern "C"
