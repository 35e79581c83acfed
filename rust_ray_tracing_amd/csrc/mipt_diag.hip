// mipt_diag.hip -- libmipt_diag.so: device-arithmetic probe for the GPU known-answer tests (include/mipt_diag.h).
//
// NOT part of the product library: libmipt.so exports nothing from this file.  The probe evaluates the kernel's own
// arithmetic building blocks (pt_device_math.h: the glibc 2.35 restatement, the exact per-ray division, RNG, sRGB
// quantisation; pt_device_wgsl.h: the sampler, basis, VNDF, hemisphere and Fresnel / reflect / refract of shading mode 1;
// pt_texel.h: the nearest-texel lookup of the default shading path) element-wise, so tests can compare them bit for bit with the
// CPU oracle on millions of arguments.
#include "../../include/mipt_diag.h"
#include "pt_device_math.h"
#include "pt_device_wgsl.h"
#include "pt_texel.h"
#include "mipt_host_util.h"
#include "pt_kernel.h"
#include "mipt_scene.h"

#include <stdio.h>

namespace {

thread_local char g_err[256] = "";

__global__ void debug_eval_kernel(int op, const float *__restrict__ a, const float *__restrict__ b, float b_scalar,
                                  unsigned long long n, float *__restrict__ out) {
    using namespace mipt;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (unsigned long long)gridDim.x * blockDim.x) {
        const float x = a[i], y = b ? b[i] : b_scalar;
        float r = 0.0f;
        switch (op) {
        case 0: r = gl_cosf(x); break;
        case 1: r = gl_log10f(x, GlTabGlobal()); break;
        case 2: r = gl_powf(x, y); break;
        case 3: r = x / y; break;
        case 4: r = __builtin_sqrtf(x); break;
        case 5: r = x * y; break;
        case 6: r = x + y; break;
        case 7: r = fminf(x, y); break;
        case 8: r = fmaxf(x, y); break;
        case 9: { uint32_t s = __float_as_uint(x); r = rand_f32(s); } break;             // xorshift + u32->f32 + /2^32
        case 10: { uint32_t s = __float_as_uint(x); r = rand_f32_nd(s, GlTabGlobal()); } break;
        case 11: { uint32_t s = __float_as_uint(x); V3 v = rand_in_unit_sphere(s, GlTabGlobal()); r = (y == 0.0f) ? v.x : (y == 1.0f ? v.y : v.z); } break;
        case 12: r = __uint_as_float(srgb_quantize(x)); break;
        case 13: r = x - truncf(x); break;
        case 14: r = fdiv_ray(x, y, 1.0f / y); break;
        case 15: r = u8_over_255(__float_as_uint(x)); break;                              // exact-division helper (valid range only)
        case 16: r = gl_sinf(x); break;
        case 17: r = gl_expf(x); break;
        case 18: r = gl_logf(x, GlTabGlobal()); break;
        case 19: r = gl_log10f_unit(x, GlTabGlobal()); break;                              // valid on {0} u [2^-32, 1]
        case 20: r = gl_cosf_2pi(x); break;                                                // valid on [0, 6.2831855]
        case 23: r = __uint_as_float(floor_mod((int32_t)__float_as_uint(x), __float_as_uint(y))); break;   // |i| < 2^30, W >= 1
        default: break;
        }
        out[i] = r;
    }
}

// inputs are the consecutive bit patterns first_bits + i (no input array): the exhaustive sweeps
__global__ void debug_eval_range_kernel(int op, uint32_t first_bits, float y, unsigned long long n, float *__restrict__ out) {
    using namespace mipt;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (unsigned long long)gridDim.x * blockDim.x) {
        const float x = __uint_as_float(first_bits + (uint32_t)i);
        float r = 0.0f;
        switch (op) {
        case 0: r = gl_cosf(x); break;
        case 1: r = gl_log10f(x, GlTabGlobal()); break;
        case 2: r = gl_powf(x, y); break;
        case 16: r = gl_sinf(x); break;
        case 17: r = gl_expf(x); break;
        case 18: r = gl_logf(x, GlTabGlobal()); break;
        case 19: r = gl_log10f_unit(x, GlTabGlobal()); break;
        case 20: r = gl_cosf_2pi(x); break;
        default: break;
        }
        out[i] = r;
    }
}

// shading mode 1's building blocks (pt_device_wgsl.h), one element per row of `in` (kWgslIn[op] floats) -> one row of `out`
// (kWgslOut[op] floats); integers travel as float bit patterns.  The texture of op 0 is texels[0 .. W*H) (checked by the host entry).
constexpr uint32_t kWgslOps = 7;
constexpr uint32_t kWgslIn[kWgslOps] = {2, 3, 6, 6, 6, 2, 11};
constexpr uint32_t kWgslOut[kWgslOps] = {4, 6, 3, 3, 4, 3, 13};
__global__ void debug_wgsl_kernel(int op, const float *__restrict__ in, unsigned long long n, const uint32_t *__restrict__ texels,
                                  uint32_t tex_w, uint32_t tex_h, float *__restrict__ out, uint32_t ni, uint32_t no) {
    using namespace mipt;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (unsigned long long)gridDim.x * blockDim.x) {
        const float *a = in + i * ni;
        float *o = out + i * no;
        switch (op) {
        case 0: { const V4 r = sample_texture_bilinear(texels, 0u, tex_w, tex_h, a[0], a[1]); o[0] = r.x; o[1] = r.y; o[2] = r.z; o[3] = r.w; } break;
        case 1: { V3 t, b; build_onb(mk(a[0], a[1], a[2]), t, b); o[0] = t.x; o[1] = t.y; o[2] = t.z; o[3] = b.x; o[4] = b.y; o[5] = b.z; } break;
        case 2:
        case 3: {
            const V3 nn = mk(a[0], a[1], a[2]), l = mk(a[3], a[4], a[5]);
            V3 t, b; build_onb(nn, t, b);
            const V3 r = (op == 2) ? to_world(t, b, nn, l) : to_local(t, b, nn, l);
            o[0] = r.x; o[1] = r.y; o[2] = r.z;
        } break;
        case 4: {
            uint32_t rng = __float_as_uint(a[5]);
            const V3 r = sample_ggx_vndf(mk(a[0], a[1], a[2]), a[3], a[4], rng);
            o[0] = r.x; o[1] = r.y; o[2] = r.z; o[3] = __uint_as_float(rng);
        } break;
        case 5: { const V3 r = cosine_hemisphere_from(a[0], a[1]); o[0] = r.x; o[1] = r.y; o[2] = r.z; } break;
        case 6: {
            const V3 d = mk(a[0], a[1], a[2]), nn = mk(a[3], a[4], a[5]);
            const V3 f0 = wgsl_f0(a[6], a[7], mk(a[8], a[9], a[10]));
            const V3 fr = wgsl_schlick_fresnel(dot(nn, mk(-d.x, -d.y, -d.z)), f0);
            const V3 sp = wgsl_reflect_dir(d, nn), tr = wgsl_refract_dir(d, nn, a[6]);
            o[0] = f0.x; o[1] = f0.y; o[2] = f0.z; o[3] = fr.x; o[4] = fr.y; o[5] = fr.z; o[6] = sp.x; o[7] = sp.y; o[8] = sp.z;
            o[9] = tr.x; o[10] = tr.y; o[11] = tr.z; o[12] = wgsl_refract_k(d, nn, a[6]);
        } break;
        default: break;
        }
    }
}

// texel_rgb (pt_texel.h) of texture {offset, w, h} in the pool sc.texels at (uv[2i], uv[2i+1]) -> rgb[3i .. 3i+3); the clamp count
// goes where the kernels' goes, into st->tex_clamped
__global__ void debug_texel_kernel(mipt::DevScene sc, const float *__restrict__ uv, unsigned long long n, uint32_t offset, uint32_t w, uint32_t h,
                                   float *__restrict__ rgb, mipt::DevStats *st) {
    using namespace mipt;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (unsigned long long)gridDim.x * blockDim.x) {
        const V3 c = texel_rgb(sc, offset, w, h, uv[2 * i], uv[2 * i + 1], st);
        rgb[3 * i] = c.x; rgb[3 * i + 1] = c.y; rgb[3 * i + 2] = c.z;
    }
}

int fail(hipError_t e, const char *what) {
    snprintf(g_err, sizeof g_err, "%s: %s", what, hipGetErrorString(e));
    return -2;   // MIPT_ERR_HIP
}

} // namespace

extern "C" {

int mipt_debug_eval(int op, const float *a, const float *b, uint64_t n, float *out) {
    if (!a || !out || n == 0) { snprintf(g_err, sizeof g_err, "mipt_debug_eval: bad argument"); return -1; }
    mipt::DevPtr<float> da, db, dout;
    hipError_t e;
    if ((e = da.alloc(n)) != hipSuccess) return fail(e, "hipMalloc");
    if ((e = dout.alloc(n)) != hipSuccess) return fail(e, "hipMalloc");
    if ((e = hipMemcpy(da, a, n * 4, hipMemcpyHostToDevice)) != hipSuccess) return fail(e, "hipMemcpy");
    if (b) {
        if ((e = db.alloc(n)) != hipSuccess) return fail(e, "hipMalloc");
        if ((e = hipMemcpy(db, b, n * 4, hipMemcpyHostToDevice)) != hipSuccess) return fail(e, "hipMemcpy");
    }
    hipLaunchKernelGGL(debug_eval_kernel, dim3(1024), dim3(256), 0, nullptr, op, da.get(), db.get(), 0.0f,
                       (unsigned long long)n, dout.get());
    if ((e = hipGetLastError()) != hipSuccess) return fail(e, "launch");
    if ((e = hipMemcpy(out, dout, n * 4, hipMemcpyDeviceToHost)) != hipSuccess) return fail(e, "hipMemcpy");
    return 0;
}

int mipt_debug_eval_range(int op, uint32_t first_bits, uint64_t n, float y, float *out) {
    if (!out || n == 0 || (uint64_t)first_bits + n > (1ull << 32)) { snprintf(g_err, sizeof g_err, "mipt_debug_eval_range: bad argument"); return -1; }
    mipt::DevPtr<float> dout;
    hipError_t e;
    if ((e = dout.alloc(n)) != hipSuccess) return fail(e, "hipMalloc");
    hipLaunchKernelGGL(debug_eval_range_kernel, dim3(2048), dim3(256), 0, nullptr, op, first_bits, y, (unsigned long long)n, dout.get());
    if ((e = hipGetLastError()) != hipSuccess) return fail(e, "launch");
    if ((e = hipMemcpy(out, dout, n * 4, hipMemcpyDeviceToHost)) != hipSuccess) return fail(e, "hipMemcpy");
    return 0;
}

int mipt_debug_wgsl(int op, const float *in, uint64_t n, const uint32_t *texels, uint32_t tex_w, uint32_t tex_h, float *out) {
    if (op < 0 || op >= (int)kWgslOps || !in || !out || n == 0 || n > (1ull << 26) ||
        (op == 0 && (!texels || tex_w == 0 || tex_h == 0 || (uint64_t)tex_w * tex_h > (1ull << 24)))) {
        snprintf(g_err, sizeof g_err, "mipt_debug_wgsl: bad argument");
        return -1;
    }
    const uint64_t in_bytes = n * kWgslIn[op] * 4, out_bytes = n * kWgslOut[op] * 4;
    mipt::DevPtr<char> din, dtex, dout;
    hipError_t e;
    if ((e = din.alloc(in_bytes)) != hipSuccess) return fail(e, "hipMalloc");
    if ((e = dout.alloc(out_bytes)) != hipSuccess) return fail(e, "hipMalloc");
    if ((e = hipMemcpy(din, in, in_bytes, hipMemcpyHostToDevice)) != hipSuccess) return fail(e, "hipMemcpy");
    if (op == 0) {
        const uint64_t tex_bytes = (uint64_t)tex_w * tex_h * 4;
        if ((e = dtex.alloc(tex_bytes)) != hipSuccess) return fail(e, "hipMalloc");
        if ((e = hipMemcpy(dtex, texels, tex_bytes, hipMemcpyHostToDevice)) != hipSuccess) return fail(e, "hipMemcpy");
    }
    hipLaunchKernelGGL(debug_wgsl_kernel, dim3(1024), dim3(256), 0, nullptr, op, (const float *)din.get(), (unsigned long long)n,
                       (const uint32_t *)dtex.get(), tex_w, tex_h, (float *)dout.get(), kWgslIn[op], kWgslOut[op]);
    if ((e = hipGetLastError()) != hipSuccess) return fail(e, "launch");
    if ((e = hipMemcpy(out, dout, out_bytes, hipMemcpyDeviceToHost)) != hipSuccess) return fail(e, "hipMemcpy");
    return 0;
}

int mipt_debug_texel(const float *uv, uint64_t n, const uint32_t *pool, uint64_t pool_words, uint32_t offset, uint32_t w, uint32_t h,
                     float *rgb_out, uint64_t *clamped_out) {
    if (!uv || !pool || !rgb_out || !clamped_out || n == 0 || n > (1ull << 26) || w == 0 || h == 0 || pool_words == 0 ||
        pool_words > (1ull << 28) || (uint64_t)offset + (uint64_t)w * h > pool_words) {
        snprintf(g_err, sizeof g_err, "mipt_debug_texel: bad argument");
        return -1;
    }
    mipt::DevPtr<float> duv, drgb;
    mipt::DevPtr<uint32_t> dpool;
    mipt::DevPtr<mipt::DevStats> dst;
    hipError_t e;
    if ((e = duv.alloc(n * 2)) != hipSuccess) return fail(e, "hipMalloc");
    if ((e = drgb.alloc(n * 3)) != hipSuccess) return fail(e, "hipMalloc");
    if ((e = dpool.alloc(pool_words)) != hipSuccess) return fail(e, "hipMalloc");
    if ((e = dst.alloc(1)) != hipSuccess) return fail(e, "hipMalloc");
    if ((e = hipMemcpy(duv, uv, n * 8, hipMemcpyHostToDevice)) != hipSuccess) return fail(e, "hipMemcpy");
    if ((e = hipMemcpy(dpool, pool, pool_words * 4, hipMemcpyHostToDevice)) != hipSuccess) return fail(e, "hipMemcpy");
    if ((e = hipMemset(dst, 0, sizeof(mipt::DevStats))) != hipSuccess) return fail(e, "hipMemset");
    mipt::DevScene sc{};
    sc.texels = dpool.get();
    sc.n_texs = 1;
    hipLaunchKernelGGL(debug_texel_kernel, dim3(1024), dim3(256), 0, nullptr, sc, (const float *)duv.get(), (unsigned long long)n, offset, w, h,
                       drgb.get(), dst.get());
    if ((e = hipGetLastError()) != hipSuccess) return fail(e, "launch");
    if ((e = hipMemcpy(rgb_out, drgb, n * 12, hipMemcpyDeviceToHost)) != hipSuccess) return fail(e, "hipMemcpy");
    mipt::DevStats hs;
    if ((e = hipMemcpy(&hs, dst, sizeof hs, hipMemcpyDeviceToHost)) != hipSuccess) return fail(e, "hipMemcpy");
    *clamped_out = hs.tex_clamped;
    return 0;
}

// the frame epilogue's two helpers that have no entry point of their own in include/mipt.h: the product's launchers (pt_kernel.hip,
// linked into this library unchanged) on the caller's device buffers, stream-ordered, no synchronisation
int mipt_debug_divide(float *d_buf, uint64_t n_floats, float divisor, void *stream) {
    if (!d_buf || n_floats == 0) { snprintf(g_err, sizeof g_err, "mipt_debug_divide: bad argument"); return -1; }
    const hipError_t e = mipt::launch_divide(d_buf, (unsigned long long)n_floats, divisor, (hipStream_t)stream);
    return e == hipSuccess ? 0 : fail(e, "launch_divide");
}

int mipt_debug_popcount(const uint32_t *d_bitmap, uint64_t n_words, uint64_t *d_out, void *stream) {
    if (!d_bitmap || !d_out || n_words == 0) { snprintf(g_err, sizeof g_err, "mipt_debug_popcount: bad argument"); return -1; }
    const hipError_t e = mipt::launch_popcount(d_bitmap, (unsigned long long)n_words, (unsigned long long *)d_out, (hipStream_t)stream);
    return e == hipSuccess ? 0 : fail(e, "launch_popcount");
}

// the tile order (pt_kernel.hip "tile order"): the product's sort on host arrays, and the state a scene handle keeps
int mipt_debug_tile_order(const uint32_t *cost, uint32_t n_tiles, uint32_t samples, uint32_t *order_out) {
    if (!cost || !order_out || n_tiles == 0 || samples == 0) { snprintf(g_err, sizeof g_err, "mipt_debug_tile_order: bad argument"); return -1; }
    mipt::DevPtr<uint32_t> dcost, dorder;
    hipError_t e;
    if ((e = dcost.alloc(n_tiles)) != hipSuccess) return fail(e, "hipMalloc");
    if ((e = dorder.alloc(n_tiles)) != hipSuccess) return fail(e, "hipMalloc");
    if ((e = hipMemcpy(dcost, cost, (size_t)n_tiles * 4, hipMemcpyHostToDevice)) != hipSuccess) return fail(e, "hipMemcpy");
    if ((e = hipMemset(dorder, 0xff, (size_t)n_tiles * 4)) != hipSuccess) return fail(e, "hipMemset");
    if ((e = mipt::launch_tile_order(dcost, n_tiles, samples, dorder, nullptr)) != hipSuccess) return fail(e, "launch_tile_order");
    if ((e = hipMemcpy(order_out, dorder, (size_t)n_tiles * 4, hipMemcpyDeviceToHost)) != hipSuccess) return fail(e, "hipMemcpy");
    return 0;
}

int mipt_diag_scene_tile_order(const void *scene, uint32_t *cost_out, uint32_t *order_out, uint32_t cap, uint32_t info_out[3]) {
    const MiptScene *s = (const MiptScene *)scene;
    if (!s || !info_out) { snprintf(g_err, sizeof g_err, "mipt_diag_scene_tile_order: bad argument"); return -1; }
    const uint32_t n = s->tile_order_valid ? s->tile_key[4] : 0u;
    info_out[0] = n; info_out[1] = s->tile_order_valid ? 1u : 0u; info_out[2] = s->tile_order_used ? 1u : 0u;
    if (n == 0u || !cost_out || !order_out) return 0;
    if (cap < n) { snprintf(g_err, sizeof g_err, "mipt_diag_scene_tile_order: cap %u < %u tiles", cap, n); return -1; }
    hipError_t e;
    if ((e = hipSetDevice(s->device)) != hipSuccess) return fail(e, "hipSetDevice");
    if ((e = hipMemcpy(cost_out, s->d_tile_cost, (size_t)n * 4, hipMemcpyDeviceToHost)) != hipSuccess) return fail(e, "hipMemcpy");
    // a launch whose list holds every slot queues no sort (mipt_api.cpp): the order of its tile costs is made here, by the same
    // kernel, into a buffer of this call's own -- the handle is only read
    mipt::DevPtr<uint32_t> dorder;
    const uint32_t *order = s->d_tile_order;
    if (!s->tile_order_sorted) {
        if ((e = dorder.alloc(n)) != hipSuccess) return fail(e, "hipMalloc");
        if ((e = mipt::launch_tile_order(s->d_tile_cost, n, s->tile_key[6], dorder, nullptr)) != hipSuccess) return fail(e, "launch_tile_order");
        order = dorder;
    }
    if ((e = hipMemcpy(order_out, order, (size_t)n * 4, hipMemcpyDeviceToHost)) != hipSuccess) return fail(e, "hipMemcpy");
    return 0;
}

// hot pixels (pt_kernel.hip "hot pixels"): the product's selection on host arrays, and the state a scene handle keeps
int mipt_debug_hot_select(const uint32_t *cost, uint32_t n_slots, uint32_t samples, uint32_t n_hot, uint32_t *hot_out, uint32_t *bits_out) {
    if (!cost || !hot_out || !bits_out || n_slots == 0 || samples == 0 || n_hot == 0 || n_hot > n_slots) {
        snprintf(g_err, sizeof g_err, "mipt_debug_hot_select: bad argument");
        return -1;
    }
    const size_t bit_words = ((size_t)n_slots + 63) / 64 * 2;
    mipt::DevPtr<uint32_t> dcost, dwork, dhot, dbits;
    hipError_t e;
    if ((e = dcost.alloc(n_slots)) != hipSuccess) return fail(e, "hipMalloc");
    if ((e = dwork.alloc(mipt::hot_work_words(n_slots))) != hipSuccess) return fail(e, "hipMalloc");
    if ((e = dhot.alloc(n_hot)) != hipSuccess) return fail(e, "hipMalloc");
    if ((e = dbits.alloc(bit_words)) != hipSuccess) return fail(e, "hipMalloc");
    if ((e = hipMemcpy(dcost, cost, (size_t)n_slots * 4, hipMemcpyHostToDevice)) != hipSuccess) return fail(e, "hipMemcpy");
    if ((e = hipMemset(dhot, 0xff, (size_t)n_hot * 4)) != hipSuccess) return fail(e, "hipMemset");
    if ((e = hipMemset(dbits, 0xff, bit_words * 4)) != hipSuccess) return fail(e, "hipMemset");
    if ((e = mipt::launch_pixel_reduce(dcost, n_slots, samples, nullptr, dwork, nullptr)) != hipSuccess) return fail(e, "launch_pixel_reduce");
    if ((e = mipt::launch_hot_select(dcost, n_slots, samples, n_hot, dwork, dhot, dbits, nullptr)) != hipSuccess) return fail(e, "launch_hot_select");
    if ((e = hipMemcpy(hot_out, dhot, (size_t)n_hot * 4, hipMemcpyDeviceToHost)) != hipSuccess) return fail(e, "hipMemcpy");
    if ((e = hipMemcpy(bits_out, dbits, bit_words * 4, hipMemcpyDeviceToHost)) != hipSuccess) return fail(e, "hipMemcpy");
    return 0;
}

int mipt_diag_scene_hot_pixels(const void *scene, uint32_t *pixel_cost_out, uint32_t cap_slots, uint32_t *hot_out, uint32_t cap_hot, uint32_t info_out[3]) {
    const MiptScene *s = (const MiptScene *)scene;
    if (!s || !info_out) { snprintf(g_err, sizeof g_err, "mipt_diag_scene_hot_pixels: bad argument"); return -1; }
    const uint32_t n = s->tile_order_valid ? s->tile_key[4] * 64u : 0u, h = s->tile_order_valid ? s->hot_n : 0u;
    info_out[0] = n; info_out[1] = h; info_out[2] = s->tile_order_valid ? s->hot_used : 0u;
    if (n == 0u || !pixel_cost_out || !hot_out) return 0;
    if (cap_slots < n || cap_hot < h) { snprintf(g_err, sizeof g_err, "mipt_diag_scene_hot_pixels: cap %u / %u < %u slots / %u hot", cap_slots, cap_hot, n, h); return -1; }
    hipError_t e;
    if ((e = hipSetDevice(s->device)) != hipSuccess) return fail(e, "hipSetDevice");
    if ((e = hipMemcpy(pixel_cost_out, s->d_pixel_cost, (size_t)n * 4, hipMemcpyDeviceToHost)) != hipSuccess) return fail(e, "hipMemcpy");
    if (h != 0u && (e = hipMemcpy(hot_out, s->d_hot, (size_t)h * 4, hipMemcpyDeviceToHost)) != hipSuccess) return fail(e, "hipMemcpy");
    return 0;
}

int mipt_diag_scene_hot_bits(const void *scene, uint32_t *bits_out, uint32_t cap_words) {
    const MiptScene *s = (const MiptScene *)scene;
    const uint32_t n = (s && s->tile_order_valid && s->list_n != 0u) ? s->tile_key[4] * 2u : 0u;
    if (!s || !bits_out || n == 0u || cap_words < n) { snprintf(g_err, sizeof g_err, "mipt_diag_scene_hot_bits: bad argument, no list, or cap < %u words", n); return -1; }
    hipError_t e;
    if ((e = hipSetDevice(s->device)) != hipSuccess) return fail(e, "hipSetDevice");
    if ((e = hipMemcpy(bits_out, s->d_hot_bits, (size_t)n * 4, hipMemcpyDeviceToHost)) != hipSuccess) return fail(e, "hipMemcpy");
    return 0;
}

int mipt_diag_scene_cost_atomics(void *scene, int on) {
    MiptScene *s = (MiptScene *)scene;
    if (!s) { snprintf(g_err, sizeof g_err, "mipt_diag_scene_cost_atomics: bad argument"); return -1; }
    s->cost_atomics = on != 0;
    return 0;
}

int mipt_diag_scene_list(const void *scene, uint32_t *list_out, uint32_t cap, uint32_t info_out[2]) {
    const MiptScene *s = (const MiptScene *)scene;
    if (!s || !info_out) { snprintf(g_err, sizeof g_err, "mipt_diag_scene_list: bad argument"); return -1; }
    const uint32_t n = s->tile_order_valid ? s->list_n : 0u;
    info_out[0] = n; info_out[1] = s->tile_order_valid ? s->list_used : 0u;
    if (n == 0u || !list_out) return 0;
    if (cap < n) { snprintf(g_err, sizeof g_err, "mipt_diag_scene_list: cap %u < %u entries", cap, n); return -1; }
    hipError_t e;
    if ((e = hipSetDevice(s->device)) != hipSuccess) return fail(e, "hipSetDevice");
    if ((e = hipMemcpy(list_out, s->d_hot, (size_t)n * 4, hipMemcpyDeviceToHost)) != hipSuccess) return fail(e, "hipMemcpy");
    return 0;
}

// payload, not allocation: the pool is n_texels words, a table one record per material (both allocations are padded when tiny).
// tests/cpp/scene_hooks.hip copies the three to the host (mipt_diag_scene_read, which = 2 / 3 / 4).
int mipt_diag_scene_tables(const void *scene, uint64_t out[3]) {
    const MiptScene *s = (const MiptScene *)scene;
    if (!s || !out) { snprintf(g_err, sizeof g_err, "mipt_diag_scene_tables: bad argument"); return -1; }
    out[0] = s->n_texels * 4; out[1] = (uint64_t)s->dev.n_mats * sizeof(mipt::DevMaterial); out[2] = (uint64_t)s->dev.n_mats * sizeof(mipt::DevMaterialFull);
    return 0;
}

const char *mipt_diag_last_error(void) { return g_err; }

} // extern "C"
