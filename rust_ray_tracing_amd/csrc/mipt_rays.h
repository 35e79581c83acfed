// mipt_rays.h -- what the entries of include/mipt.h that take a list of work items and a resident scene (ray queries, radiance
// queries, baking) share and that needs no device: the checks of their counts and options.  An entry file keeps its null-argument
// check, its own option checks (sample_stride, the texel limit) and its launch; the order in which it calls the checks below is the
// order in which a caller sees them fire (tests/test_ray_entry_messages.py).  Host C++ only and no HIP type.  What needs HIP -- the
// buffer checks of the device entries -- is at the end of mipt_host_util.h; the staging of the host entries is in mipt_scene.h.
#pragma once
#include "mipt_internal.h"

#include <cmath>
#include <cstddef>
#include <cstdint>

namespace mipt {

// the number of rays or points of a call; `noun` is what the entry's declaration calls it
inline int ray_count_check(const char *who, const char *noun, uint64_t count) {
    if (count >= MIPT_QUERY_MAX_RAYS) return fail(MIPT_ERR_INVALID_ARG, "%s: %s %llu: must stay below 2^31", who, noun, (unsigned long long)count);
    return MIPT_OK;
}

inline int ray_sampling_check(const char *who, uint32_t samples, uint32_t max_ray_depth) {
    if (samples == 0 || max_ray_depth == 0) return fail(MIPT_ERR_INVALID_ARG, "%s: samples and max_ray_depth must be > 0", who);
    return MIPT_OK;
}

template <size_t N> int reserved_check(const char *who, const uint32_t (&reserved)[N]) {
    for (uint32_t r : reserved)
        if (r) return fail(MIPT_ERR_INVALID_ARG, "%s: reserved option fields must be 0", who);
    return MIPT_OK;
}

// What every options struct of these entries has: traversal, shading (null: the entry shades nothing), flags, cull_margin and the
// reserved words, refused in that order.  accepted / accepted_text: the flags the entry takes and how its message lists them
// ("MIPT_FLAG_COUNT is").
template <class Options>
int ray_options_check(const char *who, const Options &opt, const uint32_t *shading, uint32_t accepted, const char *accepted_text) {
    if (opt.traversal > MIPT_TRAVERSAL_CULLED) return fail(MIPT_ERR_INVALID_ARG, "%s: unknown traversal %u", who, opt.traversal);
    if (shading && *shading > MIPT_SHADING_WGPU) return fail(MIPT_ERR_INVALID_ARG, "%s: unknown shading %u", who, *shading);
    if (opt.flags & ~accepted) return fail(MIPT_ERR_INVALID_ARG, "%s: flags 0x%x: only %s accepted", who, opt.flags, accepted_text);
    if (!(opt.cull_margin >= 0.0f) || !std::isfinite(opt.cull_margin))
        return fail(MIPT_ERR_INVALID_ARG, "%s: cull_margin must be finite and >= 0", who);
    return reserved_check(who, opt.reserved);
}

// the options of the entries that trace paths (MiptRadianceOptions, MiptBakeOptions): ray_options_check with their shading and flags
template <class Options> int path_options_check(const char *who, const Options &opt) {
    return ray_options_check(who, opt, &opt.shading, MIPT_FLAG_COUNT | MIPT_FLAG_SUM | MIPT_FLAG_ACCUM,
                             "MIPT_FLAG_COUNT, MIPT_FLAG_SUM and MIPT_FLAG_ACCUM are");
}

// MIPT_FLAG_ACCUM adds to a running sum, and only into memory the caller owns.  device_entry: what a host entry points its caller
// to; null when the caller is that device entry.
inline int accum_check(const char *who, uint32_t flags, const char *device_entry) {
    if (!(flags & MIPT_FLAG_ACCUM)) return MIPT_OK;
    if (!(flags & MIPT_FLAG_SUM))
        return fail(MIPT_ERR_INVALID_ARG, "%s: MIPT_FLAG_ACCUM needs MIPT_FLAG_SUM (a running sum, divided once at the end)", who);
    if (device_entry) return fail(MIPT_ERR_INVALID_ARG, "%s: MIPT_FLAG_ACCUM needs a caller-owned device buffer: use %s", who, device_entry);
    return MIPT_OK;
}

// The entries that trace n items x samples paths in chunks (mipt_bake_gather*: MiptBakeOptions; mipt_probe_bake*: MiptProbeBakeOptions,
// field for field the same): everything that needs neither the scene's contents nor a device.  any_null / null_text: the entry's own
// null test, `opt` among its pointers, and its message; noun: what the entry calls an item; device_entry: as accum_check takes it.
template <class Options>
int chunked_entry_check(const char *who, bool any_null, const char *null_text, const char *noun, uint64_t n, const Options *opt,
                        const char *device_entry) {
    if (any_null) return fail(MIPT_ERR_INVALID_ARG, "%s: %s", who, null_text);
    int rc;
    if ((rc = ray_count_check(who, "n", n)) || (rc = ray_sampling_check(who, opt->samples, opt->max_ray_depth))) return rc;
    if (opt->sample_stride == 0)
        return fail(MIPT_ERR_INVALID_ARG, "%s: sample_stride must be > 0 (every sample of a %s would run on one stream)", who, noun);
    if ((rc = path_options_check(who, *opt))) return rc;
    return accum_check(who, opt->flags, device_entry);
}

} // namespace mipt
