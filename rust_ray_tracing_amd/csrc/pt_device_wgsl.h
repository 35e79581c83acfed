// pt_device_wgsl.h -- the building blocks of shading mode 1, the wgpu backend's material model (rt_compute.wgsl:500-569 and
// the Fresnel / reflect / refract step of :158-163): the bilinear repeat sampler, the orthonormal basis, GGX-VNDF and
// cosine-hemisphere sampling.  Included by pt_kernel.hip (shade_wgsl inlines them) and by mipt_diag.hip, whose probe
// evaluates these very functions element-wise for tests/test_gpu_wgsl.py.  One rounded f32 op per WGSL operator,
// transcendentals through the glibc restatement of pt_device_math.h -- operator for operator what the CPU oracle states.
#pragma once

#include "pt_device_math.h"

namespace mipt {

struct V4 { float x, y, z, w; };
__device__ __forceinline__ float w_clamp(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }

__device__ __forceinline__ V4 sample_texture_bilinear(const uint32_t *texels, uint32_t offset, uint32_t width, uint32_t height, float u, float v) {
    const uint32_t W = width, H = height;                                    // textureSampleLevel: linear, repeat (gpu.rs:393-401)
    const float uu = u * (float)W - 0.5f, vv = v * (float)H - 0.5f;
    const float fu = floorf(uu), fv = floorf(vv);
    float a = uu - fu, b = vv - fv;
    const int32_t ic = (fabsf(fu) < 1e9f) ? (int32_t)fu : 0, jc = (fabsf(fv) < 1e9f) ? (int32_t)fv : 0;
    if (!(a == a)) a = 0.0f;
    if (!(b == b)) b = 0.0f;
    const uint32_t i0 = floor_mod(ic, W), j0 = floor_mod(jc, H);             // texel (ic, jc) and its +1 neighbours, wrapped (|ic|, |jc| < 1e9)
    const uint32_t i1 = (i0 + 1u == W) ? 0u : i0 + 1u, j1 = (j0 + 1u == H) ? 0u : j0 + 1u;
    const size_t row0 = (size_t)offset + (size_t)j0 * W, row1 = (size_t)offset + (size_t)j1 * W;
    const uint32_t p00 = texels[row0 + i0], p10 = texels[row0 + i1];
    const uint32_t p01 = texels[row1 + i0], p11 = texels[row1 + i1];
    float out[4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const float t00 = u8_over_255((p00 >> (8 * c)) & 255u), t10 = u8_over_255((p10 >> (8 * c)) & 255u);
        const float t01 = u8_over_255((p01 >> (8 * c)) & 255u), t11 = u8_over_255((p11 >> (8 * c)) & 255u);
        const float top = t00 * (1.0f - a) + t10 * a;
        const float bot = t01 * (1.0f - a) + t11 * a;
        out[c] = top * (1.0f - b) + bot * b;
    }
    V4 r; r.x = out[0]; r.y = out[1]; r.z = out[2]; r.w = out[3];
    return r;
}
__device__ __forceinline__ void build_onb(V3 n, V3 &tangent, V3 &bitangent) {                  // rt_compute.wgsl:565-569
    const V3 up = (fabsf(n.z) < 0.9999999f) ? mk(0.0f, 0.0f, 1.0f) : mk(1.0f, 0.0f, 0.0f);
    tangent = normalized(cross(up, n));
    bitangent = cross(n, tangent);
}
__device__ __forceinline__ V3 to_world(V3 t, V3 b, V3 n, V3 l) {
    return mk((t.x * l.x + b.x * l.y) + n.x * l.z, (t.y * l.x + b.y * l.y) + n.y * l.z, (t.z * l.x + b.z * l.y) + n.z * l.z);
}
__device__ __forceinline__ V3 to_local(V3 t, V3 b, V3 n, V3 w) { return mk(dot(t, w), dot(b, w), dot(n, w)); }

__device__ __forceinline__ V3 sample_ggx_vndf(V3 ve, float ax, float ay, uint32_t &rng) {      // rt_compute.wgsl:503-525
    const float u1 = rand_f32(rng), u2 = rand_f32(rng);
    const V3 Vh = normalized(mk(ax * ve.x, ay * ve.y, ve.z));
    const float lensq = Vh.x * Vh.x + Vh.y * Vh.y;
    V3 T1 = mk(1.0f, 0.0f, 0.0f);
    if (lensq > 0.0f) { const float inv = 1.0f / __builtin_sqrtf(lensq); T1 = mk(-Vh.y * inv, Vh.x * inv, 0.0f * inv); }
    const V3 T2 = cross(Vh, T1);
    const float r = __builtin_sqrtf(u1);
    const float phi = 2.0f * 3.1415926535f * u2;
    const float t1 = r * gl_cosf(phi);
    float t2 = r * gl_sinf(phi);
    const float s = 0.5f * (1.0f + Vh.z);
    t2 = (1.0f - s) * __builtin_sqrtf(1.0f - t1 * t1) + s * t2;
    const float k = __builtin_sqrtf(fmaxf(0.0f, 1.0f - t1 * t1 - t2 * t2));
    const V3 Nh = (T1 * t1 + T2 * t2) + Vh * k;
    return normalized(mk(ax * Nh.x, ay * Nh.y, fmaxf(0.0f, Nh.z)));
}
// cosine_sample_hemisphere (rt_compute.wgsl:527-551), split: the two RNG draws happen where the shader calls the function;
// the direction itself is a pure function of them and is only evaluated on the branch that uses it.
__device__ __forceinline__ V3 cosine_hemisphere_from(float ux, float uy) {
    const float ox = 2.0f * ux - 1.0f, oy = 2.0f * uy - 1.0f;
    float dx, dy;
    if (ox == 0.0f && oy == 0.0f) { dx = 0.0f; dy = 0.0f; }
    else {
        float theta, r;
        if (fabsf(ox) > fabsf(oy)) { r = ox; theta = 0.7853981634f * (oy / ox); }
        else { r = oy; theta = 1.5707963268f - 0.7853981634f * (ox / oy); }
        dx = r * gl_cosf(theta); dy = r * gl_sinf(theta);
    }
    const float z = __builtin_sqrtf(fmaxf(0.0f, 1.0f - dx * dx - dy * dy));
    return mk(dx, dy, z);
}

// rt_compute.wgsl:158-163.  Integer literal exponents = repeated multiplication (same reading as the CPU oracle).
__device__ __forceinline__ V3 wgsl_f0(float ior, float metallic, V3 base) {                     // mix(f0, base_color, metallic)
    const float f0s = ((1.0f - ior) * (1.0f - ior)) / ((1.0f + ior) * (1.0f + ior));
    return mk(f0s * (1.0f - metallic) + base.x * metallic, f0s * (1.0f - metallic) + base.y * metallic, f0s * (1.0f - metallic) + base.z * metallic);
}
__device__ __forceinline__ V3 wgsl_schlick_fresnel(float n_dot_v, V3 f0) {                      // :553-555
    const float p1 = 1.0f - n_dot_v, p2 = p1 * p1;
    const float p5 = (p2 * p2) * p1;
    return mk(f0.x + (1.0f - f0.x) * p5, f0.y + (1.0f - f0.y) * p5, f0.z + (1.0f - f0.z) * p5);
}
__device__ __forceinline__ V3 wgsl_reflect_dir(V3 d, V3 n) {                                    // normalize(reflect(d, n))
    const float two_ndi = 2.0f * dot(n, d);
    return normalized(d - n * two_ndi);
}
__device__ __forceinline__ float wgsl_refract_k(V3 d, V3 n, float ior) {                       // refract's discriminant; < 0 = total internal reflection
    const float ndi = dot(n, d);
    return 1.0f - ior * ior * (1.0f - ndi * ndi);
}
__device__ __forceinline__ V3 wgsl_refract_dir(V3 d, V3 n, float ior) {                         // normalize(refract(d, n, ior)); k < 0 -> normalize(0)
    const float ndi = dot(n, d);
    const float k = 1.0f - ior * ior * (1.0f - ndi * ndi);
    const V3 r = (k < 0.0f) ? mk(0.0f, 0.0f, 0.0f) : (d * ior - n * (ior * ndi + __builtin_sqrtf(k)));
    return normalized(r);
}

} // namespace mipt
