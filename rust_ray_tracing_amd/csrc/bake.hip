// bake.hip -- the kernels of include/mipt.h "baking": which triangle owns a lightmap texel and where on it the texel's centre lies
// (mipt_bake_texels*), and the rays a surface point gathers light along with the ordered sum of what they bring back
// (mipt_bake_gather*; the paths themselves run in pt_kernel.hip's ray kernel, untouched), and where a surface point lies and which
// way its surface faces (mipt_bake_surface*).  Every operator is one rounded f32 operation
// (-ffp-contract=off, correctly rounded division and square root): tests/tools/bake_model.py restates the arithmetic in numpy.
#include "pt_kernel.h"
#include "chunk_paths.h"
#include "pt_device_math.h"
#include "../../include/mipt.h"

namespace mipt {

namespace {

constexpr uint32_t kT = 256;
constexpr unsigned long long kNoOwner = ~0ull;

// ---- texels ------------------------------------------------------------------------------------------------------------------------
// One triangle's UV corners as tri_attr holds them (words 9 ... 14 of the 64-B record) and what the test needs of them.
struct UvTri {
    float ax, ay, bx, by, cx, cy, d;                // a; b - a; c - a; the determinant
    float lo_x, hi_x, lo_y, hi_y;                   // the bounding box of a, b, c
    bool usable;                                    // d finite and != 0
};
__device__ __forceinline__ UvTri load_uv(const float4 *tri_attr, uint32_t t) {
    const float4 a2 = tri_attr[(size_t)t * 4 + 2], a3 = tri_attr[(size_t)t * 4 + 3];
    UvTri r;
    r.ax = a2.y; r.ay = a2.z;
    const float bx = a2.w, by = a3.x, cx = a3.y, cy = a3.z;
    r.lo_x = fminf(r.ax, fminf(bx, cx)); r.hi_x = fmaxf(r.ax, fmaxf(bx, cx));
    r.lo_y = fminf(r.ay, fminf(by, cy)); r.hi_y = fmaxf(r.ay, fmaxf(by, cy));
    r.bx = bx - r.ax; r.by = by - r.ay; r.cx = cx - r.ax; r.cy = cy - r.ay;
    r.d = (r.bx * r.cy) - (r.cx * r.by);
    r.usable = (r.d != 0.0f) && (fabsf(r.d) < __builtin_inff());      // a NaN fails the second comparison
    return r;
}
// the texel centre (include/mipt.h): one conversion, one addition, one division per coordinate
__device__ __forceinline__ float centre(uint32_t x, float size_f) { return ((float)x + 0.5f) / size_f; }
// include/mipt.h "covered": the box comparisons are exact, the rest is the header's expression tree
__device__ __forceinline__ bool covers(const UvTri &k, float s, float t, float &u, float &v) {
    const float px = s - k.ax, py = t - k.ay;
    u = ((px * k.cy) - (k.cx * py)) / k.d;
    v = ((k.bx * py) - (px * k.by)) / k.d;
    return s >= k.lo_x && s <= k.hi_x && t >= k.lo_y && t <= k.hi_y && u >= 0.0f && v >= 0.0f && (u + v) <= 1.0f;
}
// Texel columns (rows) [first, first + count) that hold every centre inside [lo, hi]: in exact arithmetic ceil(lo * size - 0.5) ...
// floor(hi * size - 0.5); the float estimate of the two ends and the centre's own rounding are each off by at most size * 2^-23 texels,
// so the range is widened by `pad` = 1 + size / 2^19 texels, then clipped to the atlas.  count == 0: none.
__device__ __forceinline__ void span(float lo, float hi, uint32_t size, float size_f, float pad, uint32_t &first, uint32_t &count) {
    float a = ceilf(lo * size_f - 0.5f) - pad, b = floorf(hi * size_f - 0.5f) + pad;
    a = fminf(fmaxf(a, 0.0f), size_f);                               // into [0, size] before the conversion: no overflow, and lo, hi are finite
    b = fminf(fmaxf(b, -1.0f), size_f - 1.0f);
    if (!(b >= a)) { first = 0u; count = 0u; return; }
    first = (uint32_t)a;
    uint32_t last = (uint32_t)b;
    if (last > size - 1u) last = size - 1u;
    count = first <= last ? last - first + 1u : 0u;
}

struct TexelArgs {
    const float4 *tri_attr;
    const uint32_t *tri_order;                      // tree order -> the caller's order; NULL = the same
    unsigned long long *owner;                      // width * height words, all ones before the coverage pass
    uint32_t *huge;                                 // tree indices of the triangles left to cover_huge_kernel
    BakeCtl *ctl;
    uint32_t n_tris, width, height, huge_cap;
    float width_f, height_f, pad_x, pad_y;
};

__device__ __forceinline__ void claim(const TexelArgs &a, const UvTri &k, unsigned long long key, uint32_t x, uint32_t y) {
    float u, v;
    // the atomic returns nothing, so the lane does not wait for it.  (Reading the word first and skipping the atomic when it is at
    // or below the key already was tried: 19.7 ms against 9.7 ms on the 10 M-triangle scene at 2048 x 2048 -- the lane waits for the load.)
    if (covers(k, centre(x, a.width_f), centre(y, a.height_f), u, v)) atomicMin(&a.owner[(size_t)y * a.width + x], key);
}

// The coverage pass.  A lane takes one triangle of the tree order.  A box of at most kLaneTexels texels is that lane's own loop; a
// larger one is walked by the whole wave, 64 texels a step, one such triangle after the other; one above kWaveTexels goes to the
// list of cover_huge_kernel, where the whole grid walks it (a full list leaves it to the wave).  The thresholds: a lane's loop of 64
// steps is what the wave spends on 64 steps of one triangle, so below 64 texels cooperation cannot win; 2^16 texels are 1 024 wave
// steps, about the time the rest of the launch takes on a scene of a few million triangles.
constexpr uint32_t kLaneTexels = 64u, kWaveTexels = 1u << 16;
__global__ __launch_bounds__(kT) void cover_kernel(TexelArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_round = (a.n_tris + 63u) & ~63u;                // whole waves stay together for the ballots
    for (uint32_t t = blockIdx.x * kT + threadIdx.x; t < n_round; t += gridDim.x * kT) {
        UvTri k{};
        uint32_t x0 = 0, nx = 0, y0 = 0, ny = 0;
        bool degenerate = false;
        if (t < a.n_tris) {
            k = load_uv(a.tri_attr, t);
            degenerate = !k.usable;
            if (k.usable) {
                span(k.lo_x, k.hi_x, a.width, a.width_f, a.pad_x, x0, nx);
                span(k.lo_y, k.hi_y, a.height, a.height_f, a.pad_y, y0, ny);
            }
        }
        const unsigned long long m_deg = __ballot(degenerate);
        if (m_deg != 0ull && lane == (uint32_t)__ffsll((long long)m_deg) - 1u) atomicAdd(&a.ctl->degenerate, (uint32_t)__popcll(m_deg));
        const uint32_t texels = nx * ny;                             // < 2^31: the atlas is
        const unsigned long long key = ((unsigned long long)(a.tri_order && t < a.n_tris ? a.tri_order[t] : t) << 32) | t;
        if (texels != 0u && texels <= kLaneTexels) {
            for (uint32_t j = 0; j < texels; j++) claim(a, k, key, x0 + j % nx, y0 + j / nx);
        }
        unsigned long long m_big = __ballot(texels > kLaneTexels);
        while (m_big != 0ull) {                                      // wave-uniform
            const int src = __ffsll((long long)m_big) - 1;
            m_big &= m_big - 1ull;
            const uint32_t b_texels = __shfl(texels, src);
            const uint32_t b_t = __shfl(t, src);
            if (b_texels > kWaveTexels) {
                uint32_t slot = 0;
                if (lane == 0u) slot = atomicAdd(&a.ctl->n_huge, 1u);
                slot = __shfl(slot, 0);
                if (slot < a.huge_cap) {
                    if (lane == 0u) a.huge[slot] = b_t;
                    continue;
                }
            }
            UvTri b;
            b.ax = __shfl(k.ax, src); b.ay = __shfl(k.ay, src); b.bx = __shfl(k.bx, src); b.by = __shfl(k.by, src);
            b.cx = __shfl(k.cx, src); b.cy = __shfl(k.cy, src); b.d = __shfl(k.d, src);
            b.lo_x = __shfl(k.lo_x, src); b.hi_x = __shfl(k.hi_x, src); b.lo_y = __shfl(k.lo_y, src); b.hi_y = __shfl(k.hi_y, src);
            b.usable = true;
            const uint32_t b_x0 = __shfl(x0, src), b_nx = __shfl(nx, src), b_y0 = __shfl(y0, src);
            const unsigned long long b_key = ((unsigned long long)__shfl((uint32_t)(key >> 32), src) << 32) | b_t;
            for (uint32_t j = lane; j < b_texels; j += 64u) claim(a, b, b_key, b_x0 + j % b_nx, b_y0 + j / b_nx);
        }
    }
}
// the triangles of the list, one after the other, each walked by the whole grid
__global__ __launch_bounds__(kT) void cover_huge_kernel(TexelArgs a) {
    const uint32_t n = a.ctl->n_huge < a.huge_cap ? a.ctl->n_huge : a.huge_cap;
    for (uint32_t e = 0; e < n; e++) {
        const uint32_t t = a.huge[e];
        const UvTri k = load_uv(a.tri_attr, t);
        uint32_t x0, nx, y0, ny;
        span(k.lo_x, k.hi_x, a.width, a.width_f, a.pad_x, x0, nx);
        span(k.lo_y, k.hi_y, a.height, a.height_f, a.pad_y, y0, ny);
        const uint32_t texels = nx * ny;
        const unsigned long long key = ((unsigned long long)(a.tri_order ? a.tri_order[t] : t) << 32) | t;
        for (uint32_t j = blockIdx.x * kT + threadIdx.x; j < texels; j += gridDim.x * kT) claim(a, k, key, x0 + j % nx, y0 + j / nx);
    }
}
// The resolve pass: a lane per texel; u, v of the owner computed again (the same operations on the same operands: the same bits)
__global__ __launch_bounds__(kT) void resolve_kernel(TexelArgs a, uint4 *points) {
    const uint32_t n = a.width * a.height;
    const uint32_t n_round = (n + 63u) & ~63u;
    uint32_t covered = 0;
    for (uint32_t i = blockIdx.x * kT + threadIdx.x; i < n_round; i += gridDim.x * kT) {
        bool has = false;
        if (i < n) {
            const unsigned long long w = a.owner[i];
            uint4 rec = make_uint4(i, 0u, 0u, MIPT_HIT_NONE);
            if (w != kNoOwner) {
                const UvTri k = load_uv(a.tri_attr, (uint32_t)w);
                float u, v;
                (void)covers(k, centre(i % a.width, a.width_f), centre(i / a.width, a.height_f), u, v);
                rec = make_uint4(i, __float_as_uint(u), __float_as_uint(v), (uint32_t)(w >> 32) | MIPT_HIT_FRONT_FACE);
                has = true;
            }
            points[i] = rec;
        }
        covered += (uint32_t)__popcll(__ballot(has));
    }
    if ((threadIdx.x & 63u) == 0u && covered != 0u) atomicAdd(&a.ctl->covered, (unsigned long long)covered);
}

// ---- gather ------------------------------------------------------------------------------------------------------------------------
// The caller's index -> the record of the intersection stream.  tri_pos is laid out by leaf (scene_device.hip "slots"), not in tree
// order; record q carries its triangle's tree index t in its tenth word, and tri_order[t] is the caller's index of t.
__global__ __launch_bounds__(kT) void invert_order_kernel(const float4 *tri_pos, const uint32_t *tri_order, uint32_t n_tris, uint32_t *inv) {
    for (uint32_t q = blockIdx.x * kT + threadIdx.x; q < n_tris; q += gridDim.x * kT) {
        const uint32_t t = __float_as_uint(tri_pos[(size_t)q * 4 + 2].y);
        if (t < n_tris) inv[tri_order ? tri_order[t] : t] = q;
    }
}
// the first point whose triangle the scene does not have
__global__ __launch_bounds__(kT) void check_points_kernel(const uint4 *points, unsigned long long n, uint32_t n_tris, BakeCtl *ctl) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * kT + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * kT) {
        const uint32_t prim = points[i].w;
        if (prim != MIPT_HIT_NONE && (prim & 0x01ffffffu) >= n_tris) atomicMin(&ctl->bad_point, i);
    }
}

// P and N of a surface point (include/mipt.h "mipt_bake_gather"), N turned round for a back face; false: no point, P and N untouched.
// The one statement of them: the gather's rays and mipt_bake_surface start from the same bits.
__device__ __forceinline__ bool surface_point(const DevScene &sc, const uint32_t *inv_order, const uint4 &pt, V3 &P, V3 &N) {
    const uint32_t k = pt.w & 0x01ffffffu;
    if (pt.w == MIPT_HIT_NONE || k >= sc.n_tris) return false;                            // (the entry has refused any other triangle)
    const float4 *tp = sc.tri_pos + (size_t)inv_order[k] * 4;
    const float4 p0 = tp[0], p1 = tp[1], p2 = tp[2];
    const uint32_t t = __float_as_uint(p2.y);                                              // the record's triangle in tree order: tri_attr's index
    if (t >= sc.n_tris) return false;                                                     // (cannot be: the map was made from these records)
    const float4 a0 = sc.tri_attr[(size_t)t * 4 + 0], a1 = sc.tri_attr[(size_t)t * 4 + 1], a2 = sc.tri_attr[(size_t)t * 4 + 2];
    const float u = __uint_as_float(pt.y), v = __uint_as_float(pt.z);
    P = (mk(p0.x, p0.y, p0.z) + mk(p0.w, p1.x, p1.y) * u) + mk(p1.z, p1.w, p2.x) * v;
    const float w = (1.0f - u) - v;                                                       // ray.rs:45
    N = (mk(a0.x, a0.y, a0.z) * w + mk(a0.w, a1.x, a1.y) * u) + mk(a1.z, a1.w, a2.x) * v;
    if (!(pt.w & MIPT_HIT_FRONT_FACE)) N = mk(-N.x, -N.y, -N.z);                          // ray.rs:46-48
    return true;
}
// no point: a ray whose slab tests all fail (every quotient a NaN), so it costs one step; the reduce kernel never reads it
__device__ __forceinline__ void no_point_ray(float4 *ray) {
    const float qnan = __uint_as_float(0x7fc00000u);
    ray[0] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    ray[1] = make_float4(qnan, qnan, qnan, __uint_as_float(1u));
}

// Ray generation: a lane per path of the chunk.
__global__ __launch_bounds__(kT) void bake_rays_kernel(DevScene sc, const uint4 *points, const uint32_t *inv_order, PathChunk c, float4 *rays) {
    for (unsigned long long j = (unsigned long long)blockIdx.x * kT + threadIdx.x; j < c.n_paths; j += (unsigned long long)gridDim.x * kT) {
        const PathOf at = path_of(c.first_path, c.samples, j);
        const uint4 pt = points[at.p];
        V3 P, N;
        if (!surface_point(sc, inv_order, pt, P, N)) { no_point_ray(rays + j * 2); continue; }
        uint32_t rng = path_rng(pt.x, c.first_sample, c.sample_stride, at.s);
        const V3 rs = rand_in_unit_sphere(rng, GlTabGlobal());
        const V3 dir = normalized(N + rs);                                                // ray.rs:179-180
        const V3 o = P + dir * 0.0001f;                                                   // ray.rs:181
        rays[j * 2] = make_float4(o.x, o.y, o.z, 0.0f);
        rays[j * 2 + 1] = make_float4(dir.x, dir.y, dir.z, __uint_as_float(rng));
    }
}

// The ordered sum: a lane per point that has a path in the chunk (chunk_paths.h: its span, and when it goes on from carry_in or
// leaves its sum in carry_out).
__global__ __launch_bounds__(kT) void bake_reduce_kernel(const uint4 *points, PathChunk c, const float *path, float *radiance) {
    const ChunkItems items = chunk_items(c.first_path, c.n_paths, c.samples);
    for (unsigned long long j = (unsigned long long)blockIdx.x * kT + threadIdx.x; j < items.count; j += (unsigned long long)gridDim.x * kT) {
        const unsigned long long p = items.p_first + j;
        const ItemSpan sp = item_span(c.first_path, c.n_paths, c.samples, p);
        const bool none = points[p].w == MIPT_HIT_NONE;
        float *dst = radiance + p * 3;
        if (none && c.accumulate) continue;                                               // left untouched
        float r = 0.0f, gr = 0.0f, b = 0.0f;
        if (sp.q0 != sp.begin) { r = c.carry_in[0]; gr = c.carry_in[1]; b = c.carry_in[2]; }
        else if (c.accumulate) { r = dst[0]; gr = dst[1]; b = dst[2]; }                   // the running sum goes on
        if (!none) {
            for (unsigned long long q = sp.q0; q < sp.q1; q++) {
                const float *src = path + (q - c.first_path) * 3;
                r = r + src[0]; gr = gr + src[1]; b = b + src[2];                        // cpu.rs:52
            }
        }
        if (sp.q1 != sp.end) { c.carry_out[0] = r; c.carry_out[1] = gr; c.carry_out[2] = b; continue; }
        if (!c.sum_only && !none) {
            r = r / c.samples_f; gr = gr / c.samples_f; b = b / c.samples_f;             // cpu.rs:60
        }
        dst[0] = r; dst[1] = gr; dst[2] = b;
    }
}

// ---- surface -----------------------------------------------------------------------------------------------------------------------
// A lane per point: P and N of surface_point, N normalized on request.  No point: +0.  Either output may be null.
__global__ __launch_bounds__(kT) void bake_surface_kernel(DevScene sc, const uint4 *points, const uint32_t *inv_order, unsigned long long n,
                                                          uint32_t unit, float *position, float *normal) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * kT + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * kT) {
        const uint4 pt = points[i];
        V3 P = mk(0.0f, 0.0f, 0.0f), N = mk(0.0f, 0.0f, 0.0f);
        if (surface_point(sc, inv_order, pt, P, N) && unit) N = normalized(N);
        if (position) { float *o = position + i * 3; o[0] = P.x; o[1] = P.y; o[2] = P.z; }
        if (normal) { float *o = normal + i * 3; o[0] = N.x; o[1] = N.y; o[2] = N.z; }
    }
}

} // namespace

hipError_t launch_bake_texels(const DevScene &sc, const uint32_t *tri_order, uint32_t width, uint32_t height, unsigned long long *owner,
                              uint32_t *huge, uint32_t huge_cap, BakeCtl *ctl, void *points, int n_cu, hipStream_t stream) {
    const size_t n = (size_t)width * height;
    hipError_t e = hipMemsetAsync(owner, 0xff, n * sizeof(unsigned long long), stream);
    if (e != hipSuccess) return e;
    if ((e = hipMemsetAsync(ctl, 0, sizeof(BakeCtl), stream)) != hipSuccess) return e;
    TexelArgs a{};
    a.tri_attr = sc.tri_attr; a.tri_order = tri_order; a.owner = owner; a.huge = huge; a.ctl = ctl;
    a.n_tris = sc.n_tris; a.width = width; a.height = height; a.huge_cap = huge_cap;
    a.width_f = (float)width; a.height_f = (float)height;
    a.pad_x = 1.0f + (float)(width >> 19); a.pad_y = 1.0f + (float)(height >> 19);          // span()
    if (sc.n_tris) {
        hipLaunchKernelGGL(cover_kernel, dim3(grid_for(sc.n_tris, n_cu, kT)), dim3(kT), 0, stream, a);
        hipLaunchKernelGGL(cover_huge_kernel, dim3((uint32_t)(n_cu > 0 ? n_cu : 1) * 4u), dim3(kT), 0, stream, a);
    }
    hipLaunchKernelGGL(resolve_kernel, dim3(grid_for(n, n_cu, kT)), dim3(kT), 0, stream, a, reinterpret_cast<uint4 *>(points));
    return hipGetLastError();
}

hipError_t launch_bake_invert_order(const DevScene &sc, const uint32_t *tri_order, uint32_t *inv, int n_cu, hipStream_t stream) {
    hipLaunchKernelGGL(invert_order_kernel, dim3(grid_for(sc.n_tris, n_cu, kT)), dim3(kT), 0, stream, sc.tri_pos, tri_order, sc.n_tris, inv);
    return hipGetLastError();
}

hipError_t launch_bake_check_points(const void *points, unsigned long long n, uint32_t n_tris, BakeCtl *ctl, int n_cu, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(ctl, 0, sizeof(BakeCtl), stream);
    if (e != hipSuccess) return e;
    if ((e = hipMemsetAsync(&ctl->bad_point, 0xff, sizeof(unsigned long long), stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(check_points_kernel, dim3(grid_for(n, n_cu, kT)), dim3(kT), 0, stream, reinterpret_cast<const uint4 *>(points), n, n_tris, ctl);
    return hipGetLastError();
}

hipError_t launch_bake_rays(const DevScene &sc, const void *points, const uint32_t *inv_order, const PathChunk &c, float4 *rays, int n_cu,
                            hipStream_t stream) {
    hipLaunchKernelGGL(bake_rays_kernel, dim3(grid_for(c.n_paths, n_cu, kT)), dim3(kT), 0, stream, sc, reinterpret_cast<const uint4 *>(points), inv_order, c,
                       rays);
    return hipGetLastError();
}

hipError_t launch_bake_surface(const DevScene &sc, const void *points, const uint32_t *inv_order, unsigned long long n, bool unit,
                               float *position, float *normal, int n_cu, hipStream_t stream) {
    hipLaunchKernelGGL(bake_surface_kernel, dim3(grid_for(n, n_cu, kT)), dim3(kT), 0, stream, sc, reinterpret_cast<const uint4 *>(points), inv_order, n,
                       unit ? 1u : 0u, position, normal);
    return hipGetLastError();
}

hipError_t launch_bake_reduce(const void *points, const PathChunk &c, const float *path, float *radiance, int n_cu, hipStream_t stream) {
    hipLaunchKernelGGL(bake_reduce_kernel, dim3(grid_for(chunk_items(c.first_path, c.n_paths, c.samples).count, n_cu, kT)), dim3(kT), 0, stream,
                       reinterpret_cast<const uint4 *>(points), c, path, radiance);
    return hipGetLastError();
}

} // namespace mipt
