// pt_texel.h -- the nearest-texel lookup of the default shading path, shared by the trace kernels (pt_kernel.hip), the first-hit
// feature pass (first_hit.hip) and the test probe (mipt_diag.hip: mipt_debug_texel).
#pragma once
#include "pt_kernel.h"
#include "pt_device_math.h"

namespace mipt {

// Texture::color_at (texture.rs:33-38) / 255 (vec3.rs:252-260); out-of-range indices (reference: panic) are clamped
// and counted
__device__ __forceinline__ V3 texel_rgb(const DevScene &sc, uint32_t offset, uint32_t width, uint32_t height, float u, float v, DevStats *st) {
    const float fu = u - truncf(u), fv = v - truncf(v);            // f32::fract
    const float fi = fu * (float)width, fj = fv * (float)height;
    // Rust `as i32`: saturating, NaN -> 0
    const long long i = (fi != fi) ? 0ll : (fi >= 2147483648.0f ? 2147483647ll : (fi <= -2147483648.0f ? -2147483648ll : (long long)(int)fi));
    const long long j = (fj != fj) ? 0ll : (fj >= 2147483648.0f ? 2147483647ll : (fj <= -2147483648.0f ? -2147483648ll : (long long)(int)fj));
    long long index = i + j * (long long)width;
    const long long n = (long long)width * (long long)height;
    if (index < 0 || index >= n) {
        index = index < 0 ? 0 : n - 1;
        atomicAdd(&st->tex_clamped, 1ull);
    }
    const uint32_t px = sc.texels[(size_t)offset + (size_t)index];
    return mk(u8_over_255(px & 255u), u8_over_255((px >> 8) & 255u), u8_over_255((px >> 16) & 255u));
}

} // namespace mipt
