// pt_traverse.h -- the traversal helpers shared by the trace kernels (pt_kernel.hip) and the ray-query kernel (ray_query.hip):
// stack-entry encoding, lane compaction, raw min/max, the exact-division guard, the 16-B geometry load and the slab tests.
// Each including translation unit gets its own internal copy (anonymous namespace), as when they lived in pt_kernel.hip.
#pragma once
#include "pt_kernel.h"
#include "pt_device_math.h"

namespace mipt {

namespace {

constexpr float kMiss = 1e30f;                     // ray.rs:79,217
constexpr uint32_t kNoTri = 0xffffffffu;           // best_tri of a miss; MIPT_HIT_NONE
constexpr uint32_t kFrontBit = 0x80000000u;        // bit 31 of best_tri: the hit is on the front face; MIPT_HIT_FRONT_FACE

// stack entry: inner -> pair index (bit31 = 0);
// leaf -> bit31 | n << 25 | first_tri  (1 <= n <= 63);
// leaf with n >= 64 -> bit31 | (pair*2 + which)  (n field 0: re-read (a, n) from the pair on pop)
__device__ __forceinline__ uint32_t encode_child(uint32_t a, uint32_t n, uint32_t pair, uint32_t which) {
    const uint32_t leaf = 0x80000000u | ((n < 64u) ? ((n << 25) | a) : (pair * 2u + which));
    return (n == 0u) ? a : leaf;
}

__device__ __forceinline__ uint32_t lane_rank(unsigned long long mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// v_min/v_max without the canonicalising v_max(x,x) hipcc puts in front of fminf/fmaxf (it guards against signalling
// NaNs; these operands are FMA results).  Semantics are IEEE minNum/maxNum = Rust f32::min/max.
__device__ __forceinline__ float min_raw(float a, float b) { float r; asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float max_raw(float a, float b) { float r; asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float min3_raw(float a, float b, float c) { float r; asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
__device__ __forceinline__ float max3_raw(float a, float b, float c) { float r; asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }

// Guard of the exact-division fast path (fdiv_ray, pt_device_math.h), evaluated ONCE PER RAY: every |d_c| in [2^-60, 2], every
// |o_c| <= 2^40 and, per axis, |o_c| >= 2^-70 or o_c == 0 -- the latter only on axes where no bounding plane of the scene has a
// coordinate 0 < |p_c| < 2^-76 (DevScene::tiny_axes, found by mipt_scene_create, which also refuses planes beyond 2^40).
// Then for a = fl(p - o): |a| <= 2^41, so |q| = |a/d| <= 2^101 -- no overflow and no NaN (all operands finite, d != 0).  On the small
// side a is exactly 0 or |a| >= 2^-99:  o = 0 gives a = p, which is 0 or >= 2^-76;  |o| >= 2^-70 with |p| < 2^-76 gives
// |a| > 2^-71;  |o| >= 2^-70 with |p| >= 2^-76 makes both multiples of 2^-99, hence their difference too.  So q is normal and both
// residuals a - q*d (multiples of 2^(e_a - 47) >= 2^-146) are representable: fdiv_ray returns RN(a/d).  For a == 0 every term is a
// zero and the quotient is a zero whose sign may differ from IEEE's; a zero only ever meets min/max and ordered comparisons in
// slab_from_t, which do not see its sign.
__device__ __forceinline__ bool origin_safe(float x, bool zero_ok) {
    const uint32_t m = __float_as_uint(x) & 0x7fffffffu;
    return m >= 0x1c800000u /* 2^-70 */ || (m == 0u && zero_ok);
}
__device__ __forceinline__ bool ray_safe(V3 o, V3 d, uint32_t tiny_axes) {
    const float lo = 8.6736174e-19f /* 2^-60 */, hi = 2.0f, omax = 1.0995116e12f /* 2^40 */;
    return (fabsf(d.x) >= lo) && (fabsf(d.x) <= hi) && (fabsf(d.y) >= lo) && (fabsf(d.y) <= hi) &&
           (fabsf(d.z) >= lo) && (fabsf(d.z) <= hi) && (fabsf(o.x) <= omax) && (fabsf(o.y) <= omax) && (fabsf(o.z) <= omax) &&
           origin_safe(o.x, !(tiny_axes & 1u)) && origin_safe(o.y, !(tiny_axes & 2u)) && origin_safe(o.z, !(tiny_axes & 4u));
}

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
template <class R>
__device__ __forceinline__ float4 ldg4(R rsrc, uint32_t byte_off) {
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)byte_off, 0, 0);
    return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}

// ray.rs:69-81 on quotients already computed (+ rt_compute.wgsl:348's t_near < max_distance when CULL)
template <bool CULL>
__device__ __forceinline__ float slab_from_t(float tminx, float tminy, float tminz, float tmaxx, float tmaxy, float tmaxz, float best) {
    float t1x = min_raw(tminx, tmaxx), t1y = min_raw(tminy, tmaxy), t1z = min_raw(tminz, tmaxz);
    float t2x = max_raw(tminx, tmaxx), t2y = max_raw(tminy, tmaxy), t2z = max_raw(tminz, tmaxz);
    float t_near = max3_raw(t1x, t1y, t1z);      // max(max(x, y), z): maxNum is associative, NaNs dropped either way
    float t_far = min3_raw(t2x, t2y, t2z);
    bool ok = (t_near <= t_far) && (t_far > 0.0f);
    if (CULL) ok = ok && (t_near < best);
    return ok ? t_near : kMiss;
}
template <bool CULL>
__device__ __forceinline__ float slab(V3 o, V3 d, float4 lo, float4 hi, float best) {
    return slab_from_t<CULL>((lo.x - o.x) / d.x, (lo.y - o.y) / d.y, (lo.z - o.z) / d.z,
                             (hi.x - o.x) / d.x, (hi.y - o.y) / d.y, (hi.z - o.z) / d.z, best);
}
// both children of a pair: exact quotients by the per-ray reciprocal, computed for every lane (straight-line code in front of
// the only branch, so the first quotients start while the later loads are still in flight; for a ray that failed ray_safe they
// are finite-or-not garbage that traps nothing) and replaced by IEEE divisions for the lanes of such rays
template <bool CULL>
__device__ __forceinline__ void slab_pair(V3 o, V3 d, V3 rd, bool safe, float4 r0, float4 r1, float4 r2, float4 r3,
                                          float best, float &d1, float &d2) {
    const float a0 = r0.x - o.x, a1 = r0.y - o.y, a2 = r0.z - o.z, a3 = r1.x - o.x, a4 = r1.y - o.y, a5 = r1.z - o.z;
    const float b0 = r2.x - o.x, b1 = r2.y - o.y, b2 = r2.z - o.z, b3 = r3.x - o.x, b4 = r3.y - o.y, b5 = r3.z - o.z;
    d1 = slab_from_t<CULL>(fdiv_ray(a0, d.x, rd.x), fdiv_ray(a1, d.y, rd.y), fdiv_ray(a2, d.z, rd.z),
                           fdiv_ray(a3, d.x, rd.x), fdiv_ray(a4, d.y, rd.y), fdiv_ray(a5, d.z, rd.z), best);
    d2 = slab_from_t<CULL>(fdiv_ray(b0, d.x, rd.x), fdiv_ray(b1, d.y, rd.y), fdiv_ray(b2, d.z, rd.z),
                           fdiv_ray(b3, d.x, rd.x), fdiv_ray(b4, d.y, rd.y), fdiv_ray(b5, d.z, rd.z), best);
    if (!safe) {
        d1 = slab<CULL>(o, d, r0, r1, best);
        d2 = slab<CULL>(o, d, r2, r3, best);
    }
}

} // namespace

} // namespace mipt
