// denoise_variance.hip -- the variance-guided a-trous filter of include/mipt.h ("variance-guided a-trous filter"):
// mipt_denoise_variance*.  The second half of the SVGF-style pipeline whose first half is temporal.hip.
//
// A pack pass, a spatial-estimate pass (skipped when short_history == 0), then one launch per iteration.  The shape is denoise.hip's,
// for the reasons given there: one pixel per lane, a 256-thread block covers 64x4 pixels, the planar inputs are packed into one float4
// of guides {n.x, n.y, n.z, z} and one of colour per pixel so that a tap costs two 16-byte loads, and which guides exist and whether a
// pass is the last are template arguments.  The colour's fourth word, which denoise.hip leaves 0, carries the pixel's variance.
//
// The estimate pass reads colour plane 0 and writes whole float4s into plane 1, so no lane reads a word another lane is writing; the
// iterations then ping-pong from the plane that was written last.  An iteration reads 9 variances at distance 1 (the prefilter) and
// the 25 taps at its step; the reuse between neighbouring pixels is left to the vector L1 and L2.
//
// Every operator below is one rounded f32 operation in the order the header gives (the translation unit is built with
// -ffp-contract=off); expf is gl_expf of pt_device_math.h on [-128, -0], sqrtf the correctly rounded expansion of __builtin_sqrtf.
#include "pt_kernel.h"
#include "pt_device_math.h"

namespace mipt {

namespace {

constexpr uint32_t kTileW = 64, kTileH = 4;                  // pixels a block covers: one wave per row
constexpr uint32_t kMaxGrid = 1u << 20;                      // blocks per launch; a block walks the tiles with this stride
static_assert(kTileW * kTileH == (uint32_t)kBlockThreads, "one pixel per lane");

constexpr float kAlbedoFloor = 1.0f / 256.0f;

// The pixel of this lane in tile `t` of the launch: tiles run over (view, tile row, tile column).  false = outside the frame (a ragged
// edge tile).  idx < 2^32 (MIPT_BATCH_MAX_PIXELS).
__device__ __forceinline__ bool lane_pixel(const DevVariance &d, unsigned long long t, uint32_t &x, uint32_t &y, size_t &view_base) {
    const uint32_t per_view = d.tiles_x * d.tiles_y;
    const uint32_t view = (uint32_t)(t / per_view), r = (uint32_t)(t % per_view);
    x = (r % d.tiles_x) * kTileW + (threadIdx.x & (kTileW - 1u));
    y = (r / d.tiles_x) * kTileH + (threadIdx.x / kTileW);
    view_base = (size_t)view * d.width * d.height;
    return x < d.width && y < d.height;
}

__device__ __forceinline__ float floored(float albedo) { return albedo > kAlbedoFloor ? albedo : kAlbedoFloor; }   // a NaN gives the floor

__device__ __forceinline__ float luminance(const float4 &c) { return ((0.2126f * c.x) + (0.7152f * c.y)) + (0.0722f * c.z); }

// (dn * kn) of two packed guides
__device__ __forceinline__ float normal_term(const float4 &gp, const float4 &gq, float kn) {
    const float nx = gp.x - gq.x, ny = gp.y - gq.y, nz = gp.z - gq.z;
    return (((nx * nx) + (ny * ny)) + (nz * nz)) * kn;
}
// (dz * kz)
__device__ __forceinline__ float depth_term(const float4 &gp, const float4 &gq, float kz) {
    const float dz = (gp.w - gq.w) * (gp.w - gq.w);
    return dz * kz;
}

template <bool NORMAL, bool DEPTH, bool ALBEDO>
__global__ __launch_bounds__(kBlockThreads) void variance_pack_kernel(DevVariance d, unsigned long long n_tiles) {
    for (unsigned long long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        uint32_t x, y;
        size_t base;
        if (!lane_pixel(d, t, x, y, base)) continue;
        const size_t i = base + ((size_t)y * d.width + x);
        const float *h = d.hdr + i * 3;
        float r = h[0], g = h[1], b = h[2];
        if (ALBEDO) {
            const float *a = d.albedo + i * 3;
            r = r / floored(a[0]); g = g / floored(a[1]); b = b / floored(a[2]);
        }
        float var = 0.0f;
        if (d.variance) {                                     // the same for every lane of the launch
            const float v = d.variance[i];
            var = v > 0.0f ? v : 0.0f;                        // a NaN gives 0
        }
        d.colour[0][i] = make_float4(r, g, b, var);
        if (NORMAL || DEPTH) {
            float4 gd = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (NORMAL) { const float *n = d.normal + i * 3; gd.x = n[0]; gd.y = n[1]; gd.z = n[2]; }
            if (DEPTH) gd.w = d.depth[i];
            d.guides[i] = gd;
        }
    }
}

// The variance of a pixel whose history is shorter than short_history, from the luminances of its 5x5 neighbourhood; every other
// pixel is copied.  colour[0] -> colour[1].
template <bool NORMAL, bool DEPTH>
__global__ __launch_bounds__(kBlockThreads) void variance_estimate_kernel(DevVariance d, unsigned long long n_tiles) {
    const float4 *__restrict__ src = d.colour[0];
    float4 *__restrict__ dst = d.colour[1];
    for (unsigned long long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        uint32_t x, y;
        size_t base;
        if (!lane_pixel(d, t, x, y, base)) continue;
        const size_t i = base + ((size_t)y * d.width + x);
        float4 cp = src[i];
        const float len = d.length ? d.length[i] : 1.0f;
        if (!(len >= d.short_history)) {                      // a NaN length takes this side
            float4 gp = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (NORMAL || DEPTH) gp = d.guides[i];
            float s1 = 0.0f, s2 = 0.0f, ws = 0.0f;
#pragma unroll
            for (int dy = -2; dy <= 2; dy++) {
                const long long qy = (long long)y + dy;
                if (qy < 0 || qy >= (long long)d.height) continue;
#pragma unroll
                for (int dx = -2; dx <= 2; dx++) {
                    const long long qx = (long long)x + dx;
                    if (qx < 0 || qx >= (long long)d.width) continue;
                    float w = 1.0f, lq;                       // the centre, or no guide at all: 1 without evaluation
                    if (dy == 0 && dx == 0) {
                        lq = luminance(cp);
                    } else {
                        const size_t q = base + ((size_t)qy * d.width + (size_t)qx);
                        lq = luminance(src[q]);
                        if (NORMAL || DEPTH) {
                            const float4 gq = d.guides[q];
                            float eg;
                            if (NORMAL && DEPTH) eg = normal_term(gp, gq, d.kn) + depth_term(gp, gq, d.kz);
                            else if (NORMAL) eg = normal_term(gp, gq, d.kn);
                            else eg = depth_term(gp, gq, d.kz);
                            eg = eg < 128.0f ? eg : 128.0f;   // a NaN gives 128
                            w = gl_expf(-eg);
                        }
                    }
                    s1 = s1 + (w * lq);
                    s2 = s2 + (w * (lq * lq));
                    ws = ws + w;
                }
            }
            const float mu = s1 / ws;
            float v = (s2 / ws) - (mu * mu);
            v = v > 0.0f ? v : 0.0f;
            const float lc = len > 1.0f ? len : 1.0f;
            cp.w = v * (d.short_history / lc);
        }
        dst[i] = cp;
    }
}

// MODE 0: a middle iteration, colour plane to colour plane; 1: the last, to the planar outputs; 2: the last, re-modulated by the albedo
template <bool NORMAL, bool DEPTH, int MODE>
__global__ __launch_bounds__(kBlockThreads) void variance_pass_kernel(DevVariance d, unsigned long long n_tiles, const float4 *__restrict__ src,
                                                                      float4 *__restrict__ dst, uint32_t step) {
    constexpr float h[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    constexpr float g3[3] = {1.0f / 4.0f, 1.0f / 2.0f, 1.0f / 4.0f};
    for (unsigned long long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        uint32_t x, y;
        size_t base;
        if (!lane_pixel(d, t, x, y, base)) continue;
        const size_t i = base + ((size_t)y * d.width + x);
        const float4 cp = src[i];
        float4 gp = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (NORMAL || DEPTH) gp = d.guides[i];
        // the 3x3 prefilter of the variance: at distance 1 whatever the step, a neighbour outside the frame skipped
        float gs = 0.0f, gw = 0.0f;
#pragma unroll
        for (int dy = -1; dy <= 1; dy++) {
            const long long qy = (long long)y + dy;
            if (qy < 0 || qy >= (long long)d.height) continue;
#pragma unroll
            for (int dx = -1; dx <= 1; dx++) {
                const long long qx = (long long)x + dx;
                if (qx < 0 || qx >= (long long)d.width) continue;
                const float gk = g3[dy + 1] * g3[dx + 1];                // exact: a constant after unrolling
                const float vq = (dy == 0 && dx == 0) ? cp.w : src[base + ((size_t)qy * d.width + (size_t)qx)].w;
                gs = gs + (gk * vq);
                gw = gw + gk;
            }
        }
        const float gv = gs / gw;
        const float kl = 1.0f / ((d.sigma_l * __builtin_sqrtf(gv)) + 1e-8f);
        const float lp = luminance(cp);
        float sr = 0.0f, sg = 0.0f, sb = 0.0f, sv = 0.0f, wsum = 0.0f;
#pragma unroll
        for (int dy = -2; dy <= 2; dy++) {
            // a tap outside the frame is skipped: neither weighted nor added (signed 64-bit: step * 2 may pass the frame's size)
            const long long qy = (long long)y + (long long)dy * (long long)step;
            if (qy < 0 || qy >= (long long)d.height) continue;
#pragma unroll
            for (int dx = -2; dx <= 2; dx++) {
                const long long qx = (long long)x + (long long)dx * (long long)step;
                if (qx < 0 || qx >= (long long)d.width) continue;
                const float hk = h[dy + 2] * h[dx + 2];                  // exact: a constant after unrolling
                float w;
                float4 cq;
                if (dy == 0 && dx == 0) {
                    cq = cp;
                    w = hk;                                               // the centre: 9/64 without evaluation
                } else {
                    const size_t q = base + ((size_t)qy * d.width + (size_t)qx);
                    cq = src[q];
                    float e = fabsf(lp - luminance(cq)) * kl;
                    if (NORMAL || DEPTH) {
                        const float4 gq = d.guides[q];
                        if (NORMAL) e = e + normal_term(gp, gq, d.kn);
                        if (DEPTH) e = e + depth_term(gp, gq, d.kz);
                    }
                    e = e < 128.0f ? e : 128.0f;                          // a NaN gives 128
                    w = hk * gl_expf(-e);
                }
                sr = sr + (w * cq.x); sg = sg + (w * cq.y); sb = sb + (w * cq.z);
                sv = sv + ((w * w) * cq.w);
                wsum = wsum + w;
            }
        }
        float r = cp.x, g = cp.y, b = cp.z, var = cp.w;
        if (wsum > 0.0f) { r = sr / wsum; g = sg / wsum; b = sb / wsum; var = sv / (wsum * wsum); }
        if (MODE == 0) {
            dst[i] = make_float4(r, g, b, var);
        } else {
            if (MODE == 2) {
                const float *a = d.albedo + i * 3;
                r = r * floored(a[0]); g = g * floored(a[1]); b = b * floored(a[2]);
            }
            float *o = d.out + i * 3;
            o[0] = r; o[1] = g; o[2] = b;
            if (d.variance_out) d.variance_out[i] = var;
        }
    }
}

template <bool NORMAL, bool DEPTH>
hipError_t launch_passes(const DevVariance &d, unsigned long long n_tiles, uint32_t grid, hipStream_t stream) {
    hipError_t e;
    if (d.albedo) hipLaunchKernelGGL((variance_pack_kernel<NORMAL, DEPTH, true>), dim3(grid), dim3(kBlockThreads), 0, stream, d, n_tiles);
    else hipLaunchKernelGGL((variance_pack_kernel<NORMAL, DEPTH, false>), dim3(grid), dim3(kBlockThreads), 0, stream, d, n_tiles);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    uint32_t first = 0;                                       // the plane the first iteration reads
    if (d.short_history > 0.0f) {
        hipLaunchKernelGGL((variance_estimate_kernel<NORMAL, DEPTH>), dim3(grid), dim3(kBlockThreads), 0, stream, d, n_tiles);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        first = 1;
    }
    for (uint32_t i = 0; i < d.iterations; i++) {
        const float4 *src = d.colour[(first + i) & 1u];
        float4 *dst = d.colour[(first + i + 1u) & 1u];
        const uint32_t step = 1u << i;
        if (i + 1u < d.iterations)
            hipLaunchKernelGGL((variance_pass_kernel<NORMAL, DEPTH, 0>), dim3(grid), dim3(kBlockThreads), 0, stream, d, n_tiles, src, dst, step);
        else if (!d.albedo)
            hipLaunchKernelGGL((variance_pass_kernel<NORMAL, DEPTH, 1>), dim3(grid), dim3(kBlockThreads), 0, stream, d, n_tiles, src, dst, step);
        else
            hipLaunchKernelGGL((variance_pass_kernel<NORMAL, DEPTH, 2>), dim3(grid), dim3(kBlockThreads), 0, stream, d, n_tiles, src, dst, step);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

} // namespace

// instantiations: {normal} x {depth} x ({pack with / without albedo} + {estimate} + {middle, last, last with albedo})
hipError_t launch_denoise_variance(const DevVariance &d, hipStream_t stream) {
    const unsigned long long n_tiles = (unsigned long long)d.tiles_x * d.tiles_y * d.n_views;
    const uint32_t grid = n_tiles < kMaxGrid ? (uint32_t)n_tiles : kMaxGrid;
    if (d.normal) return d.depth ? launch_passes<true, true>(d, n_tiles, grid, stream) : launch_passes<true, false>(d, n_tiles, grid, stream);
    return d.depth ? launch_passes<false, true>(d, n_tiles, grid, stream) : launch_passes<false, false>(d, n_tiles, grid, stream);
}

} // namespace mipt
