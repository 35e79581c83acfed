// probe.hip -- the kernels of include/mipt.h "irradiance probes": the rays a probe sends over the whole sphere and the ordered
// projection of what they bring back onto real spherical harmonics up to band 2 (mipt_probe_bake*; the paths themselves run in
// pt_kernel.hip's ray kernel, untouched), and the lookup that blends a grid of such probes at a point and convolves with the clamped
// cosine (mipt_probe_irradiance*).  Every operator is one rounded f32 operation (-ffp-contract=off, correctly rounded division):
// tests/tools/probe_model.py restates the arithmetic in numpy.
#include "pt_kernel.h"
#include "chunk_paths.h"
#include "pt_device_math.h"
#include "../../include/mipt.h"

namespace mipt {

namespace {

constexpr uint32_t kT = 256;

// the basis of include/mipt.h, one function at a time: k is uniform per wave of the projection kernel
__device__ __forceinline__ float sh_basis(uint32_t k, float x, float y, float z) {
    switch (k) {
    case 0: return 0.2820948f;
    case 1: return 0.48860252f * y;
    case 2: return 0.48860252f * z;
    case 3: return 0.48860252f * x;
    case 4: return 1.0925485f * (x * y);
    case 5: return 1.0925485f * (y * z);
    case 6: return 0.31539157f * ((3.0f * (z * z)) - 1.0f);
    case 7: return 1.0925485f * (x * z);
    default: return 0.54627424f * ((x * x) - (y * y));
    }
}

// Ray generation: a lane per path of the chunk (include/mipt.h "mipt_probe_bake").
__global__ __launch_bounds__(kT) void probe_rays_kernel(const float4 *probes, PathChunk c, float4 *rays) {
    for (unsigned long long j = (unsigned long long)blockIdx.x * kT + threadIdx.x; j < c.n_paths; j += (unsigned long long)gridDim.x * kT) {
        const PathOf at = path_of(c.first_path, c.samples, j);
        const float4 pr = probes[at.p];
        uint32_t rng = path_rng(__float_as_uint(pr.w), c.first_sample, c.sample_stride, at.s);
        const V3 d = rand_in_unit_sphere(rng, GlTabGlobal());                             // vec3.rs:66-68: a unit vector, used as given
        rays[j * 2] = make_float4(pr.x, pr.y, pr.z, 0.0f);                                // the origin is the probe: no offset
        rays[j * 2 + 1] = make_float4(d.x, d.y, d.z, __uint_as_float(rng));
    }
}

// The ordered projection: a lane per (probe that has a path in the chunk, coefficient k), three running sums each -- the 27 sums of
// a probe are independent of each other, so nine lanes walk the probe's samples side by side.  Lanes are handed out as
// [group of 64 probes][k][probe of the group]: k is the same for a whole wave, so the basis function is a scalar branch.  The walk
// itself is serial -- the sum is ordered -- and bound by the latency of its loads: kBatch samples are fetched before they are added,
// in order.  chunk_paths.h: a probe's span, and when it goes on from carry_in or leaves its sums in carry_out.
constexpr int kBatch = 16;
__host__ __device__ inline unsigned long long project_lanes(unsigned long long n_probes) { return ((n_probes + 63ull) / 64ull) * (9ull * 64ull); }   // kernel and launcher
__global__ __launch_bounds__(kT) void probe_project_kernel(PathChunk c, const float4 *rays, const float *path, float *sh) {
    const ChunkItems items = chunk_items(c.first_path, c.n_paths, c.samples);
    const unsigned long long n = project_lanes(items.count);
    for (unsigned long long j = (unsigned long long)blockIdx.x * kT + threadIdx.x; j < n; j += (unsigned long long)gridDim.x * kT) {
        const unsigned long long local = (j / (9ull * 64ull)) * 64ull + (j & 63ull);
        const uint32_t k = (uint32_t)((j / 64ull) % 9ull);                                // wave-uniform: kT and the stride are multiples of 64
        if (local >= items.count) continue;
        const unsigned long long p = items.p_first + local;
        const ItemSpan sp = item_span(c.first_path, c.n_paths, c.samples, p);
        float *dst = sh + p * 27ull + k * 3u;
        float r = 0.0f, gr = 0.0f, b = 0.0f;
        if (sp.q0 != sp.begin) { r = c.carry_in[k * 3u]; gr = c.carry_in[k * 3u + 1u]; b = c.carry_in[k * 3u + 2u]; }
        else if (c.accumulate) { r = dst[0]; gr = dst[1]; b = dst[2]; }                   // the running sums go on
        const float4 *ray = rays + (sp.q0 - c.first_path) * 2ull + 1ull;                  // the direction half of the record
        const float *src = path + (sp.q0 - c.first_path) * 3ull;
        unsigned long long left = sp.q1 - sp.q0;
        for (; left >= (unsigned long long)kBatch; left -= kBatch, ray += 2 * kBatch, src += 3 * kBatch) {
            float4 d[kBatch];
            float l[kBatch][3];
#pragma unroll
            for (int u = 0; u < kBatch; u++) { d[u] = ray[2 * u]; l[u][0] = src[3 * u]; l[u][1] = src[3 * u + 1]; l[u][2] = src[3 * u + 2]; }
#pragma unroll
            for (int u = 0; u < kBatch; u++) {
                const float y = sh_basis(k, d[u].x, d[u].y, d[u].z);
                r = r + (l[u][0] * y); gr = gr + (l[u][1] * y); b = b + (l[u][2] * y);
            }
        }
        for (; left != 0ull; left--, ray += 2, src += 3) {
            const float4 d = ray[0];
            const float y = sh_basis(k, d.x, d.y, d.z);
            r = r + (src[0] * y); gr = gr + (src[1] * y); b = b + (src[2] * y);
        }
        if (sp.q1 != sp.end) { c.carry_out[k * 3u] = r; c.carry_out[k * 3u + 1u] = gr; c.carry_out[k * 3u + 2u] = b; continue; }
        if (!c.sum_only) {
            r = (r / c.samples_f) * 12.566371f; gr = (gr / c.samples_f) * 12.566371f; b = (b / c.samples_f) * 12.566371f;
        }
        dst[0] = r; dst[1] = gr; dst[2] = b;
    }
}

// ---- lookup --------------------------------------------------------------------------------------------------------------------------
// one axis of the cell a point lies in: the lower probe i0 and the weights of the two
__device__ __forceinline__ void cell_axis(float p, float origin, float spacing, uint32_t dim, uint32_t &i0, float &w0, float &w1) {
    float gq = (p - origin) / spacing;
    if (!(gq >= 0.0f)) gq = 0.0f;                                                         // a NaN too
    gq = fminf(gq, (float)(dim - 1u));
    float f = 0.0f;
    i0 = 0u;
    if (dim != 1u) {
        const uint32_t i = (uint32_t)gq;
        i0 = i < dim - 2u ? i : dim - 2u;
        f = gq - (float)i0;
    }
    w0 = 1.0f - f; w1 = f;
}

// A lane per point.
__global__ __launch_bounds__(kT) void probe_irradiance_kernel(DevProbeLookup a) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * kT + threadIdx.x; i < a.n; i += (unsigned long long)gridDim.x * kT) {
        const float *pp = a.position + i * 3ull, *pn = a.normal + i * 3ull;
        uint32_t i0[3];
        float w[3][2];
        for (int ax = 0; ax < 3; ax++) cell_axis(pp[ax], a.origin[ax], a.spacing[ax], a.dims[ax], i0[ax], w[ax][0], w[ax][1]);
        float b[9][3];
        for (int k = 0; k < 9; k++) b[k][0] = b[k][1] = b[k][2] = 0.0f;
        float wsum = 0.0f;
#pragma unroll
        for (uint32_t c8 = 0; c8 < 8u; c8++) {
            const uint32_t dx = c8 & 1u, dy = (c8 >> 1) & 1u, dz = c8 >> 2;
            const float wt = (w[0][dx] * w[1][dy]) * w[2][dz];
            if (wt == 0.0f) continue;                                                     // skipped, never read (a corner beyond a one-probe axis is here)
            const uint32_t ix = i0[0] + dx, iy = i0[1] + dy, iz = i0[2] + dz;
            if (ix >= a.dims[0] || iy >= a.dims[1] || iz >= a.dims[2]) continue;          // (cannot be: its weight is 0)
            const unsigned long long probe = ((unsigned long long)iz * a.dims[1] + iy) * a.dims[0] + ix;
            if (a.valid && a.valid[probe] == 0) continue;
            const float *s = a.sh + probe * 27ull;
#pragma unroll
            for (int k = 0; k < 9; k++) {
                b[k][0] = b[k][0] + (wt * s[k * 3]); b[k][1] = b[k][1] + (wt * s[k * 3 + 1]); b[k][2] = b[k][2] + (wt * s[k * 3 + 2]);
            }
            wsum = wsum + wt;
        }
        const float x = pn[0], y = pn[1], z = pn[2];
        float Y[9];
#pragma unroll
        for (int k = 0; k < 9; k++) Y[k] = sh_basis((uint32_t)k, x, y, z);
        float *out = a.irradiance + i * 3ull;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float band1 = ((Y[1] * b[1][c]) + (Y[2] * b[2][c])) + (Y[3] * b[3][c]);
            const float band2 = ((((Y[4] * b[4][c]) + (Y[5] * b[5][c])) + (Y[6] * b[6][c])) + (Y[7] * b[7][c])) + (Y[8] * b[8][c]);
            float e = ((3.1415927f * (Y[0] * b[0][c])) + (2.0943952f * band1)) + (0.7853982f * band2);
            if (a.valid) e = wsum == 0.0f ? 0.0f : e / wsum;
            if (a.clamp) e = e > 0.0f ? e : 0.0f;
            out[c] = e;
        }
    }
}

} // namespace

hipError_t launch_probe_rays(const void *probes, const PathChunk &c, float4 *rays, int n_cu, hipStream_t stream) {
    hipLaunchKernelGGL(probe_rays_kernel, dim3(grid_for(c.n_paths, n_cu, kT)), dim3(kT), 0, stream, reinterpret_cast<const float4 *>(probes), c, rays);
    return hipGetLastError();
}

hipError_t launch_probe_project(const PathChunk &c, const float4 *rays, const float *path, float *sh, int n_cu, hipStream_t stream) {
    const unsigned long long lanes = project_lanes(chunk_items(c.first_path, c.n_paths, c.samples).count);
    hipLaunchKernelGGL(probe_project_kernel, dim3(grid_for(lanes, n_cu, kT)), dim3(kT), 0, stream, c, rays, path, sh);
    return hipGetLastError();
}

hipError_t launch_probe_irradiance(const DevProbeLookup &d, int n_cu, hipStream_t stream) {
    hipLaunchKernelGGL(probe_irradiance_kernel, dim3(grid_for(d.n, n_cu, kT)), dim3(kT), 0, stream, d);
    return hipGetLastError();
}

} // namespace mipt
