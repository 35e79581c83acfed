// denoise.hip -- the edge-avoiding a-trous wavelet filter of include/mipt.h ("a-trous denoiser"): mipt_denoise*.
//
// A pack pass, then one launch per iteration.  The pack pass turns the planar inputs into one float4 of (demodulated) colour and one
// float4 {n.x, n.y, n.z, z} of guides per pixel, so that a tap costs two 16-byte loads instead of seven 4-byte ones.  An iteration
// reads one colour plane and writes the other; the last one re-modulates and writes the planar output, so `out` may be `hdr`.
//
// One pixel per lane.  A 256-thread block covers 64x4 pixels: the 64 lanes of a wave are 64 neighbours of one row, and a tap load at
// any step s is one contiguous 1 KB run of a row.  The 25 taps of neighbouring pixels overlap; that reuse is left to the vector L1
// and L2.  Which guides exist and whether a pass is the last are template arguments, so no lane ever branches on them.
//
// Every operator below is one rounded f32 operation in the order the header gives (the translation unit is built with
// -ffp-contract=off); expf is gl_expf of pt_device_math.h, glibc 2.35's, on the domain [-128, -0] the clamp leaves.
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
__device__ __forceinline__ bool lane_pixel(const DevDenoise &d, unsigned long long t, uint32_t &x, uint32_t &y, size_t &view_base) {
    const uint32_t per_view = d.tiles_x * d.tiles_y;
    const uint32_t view = (uint32_t)(t / per_view), r = (uint32_t)(t % per_view);
    x = (r % d.tiles_x) * kTileW + (threadIdx.x & (kTileW - 1u));
    y = (r / d.tiles_x) * kTileH + (threadIdx.x / kTileW);
    view_base = (size_t)view * d.width * d.height;
    return x < d.width && y < d.height;
}

__device__ __forceinline__ float floored(float albedo) { return albedo > kAlbedoFloor ? albedo : kAlbedoFloor; }   // a NaN gives the floor

template <bool NORMAL, bool DEPTH, bool ALBEDO>
__global__ __launch_bounds__(kBlockThreads) void denoise_pack_kernel(DevDenoise d, unsigned long long n_tiles) {
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
        d.colour[0][i] = make_float4(r, g, b, 0.0f);
        if (NORMAL || DEPTH) {
            float4 gd = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (NORMAL) { const float *n = d.normal + i * 3; gd.x = n[0]; gd.y = n[1]; gd.z = n[2]; }
            if (DEPTH) gd.w = d.depth[i];
            d.guides[i] = gd;
        }
    }
}

// MODE 0: a middle iteration, colour plane to colour plane; 1: the last, to the planar output; 2: the last, re-modulated by the albedo
template <bool NORMAL, bool DEPTH, int MODE>
__global__ __launch_bounds__(kBlockThreads) void denoise_pass_kernel(DevDenoise d, unsigned long long n_tiles, const float4 *__restrict__ src,
                                                                     float4 *__restrict__ dst, uint32_t step, float kc) {
    constexpr float h[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    for (unsigned long long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        uint32_t x, y;
        size_t base;
        if (!lane_pixel(d, t, x, y, base)) continue;
        const size_t i = base + ((size_t)y * d.width + x);
        const float4 cp = src[i];
        float4 gp = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (NORMAL || DEPTH) gp = d.guides[i];
        float sr = 0.0f, sg = 0.0f, sb = 0.0f, wsum = 0.0f;
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
                    const float dr = cp.x - cq.x, dg = cp.y - cq.y, db = cp.z - cq.z;
                    float e = (((dr * dr) + (dg * dg)) + (db * db)) * kc;
                    if (NORMAL || DEPTH) {
                        const float4 gq = d.guides[q];
                        if (NORMAL) {
                            const float nx = gp.x - gq.x, ny = gp.y - gq.y, nz = gp.z - gq.z;
                            e = e + ((((nx * nx) + (ny * ny)) + (nz * nz)) * d.kn);
                        }
                        if (DEPTH) {
                            const float dz = (gp.w - gq.w) * (gp.w - gq.w);
                            e = e + (dz * d.kz);
                        }
                    }
                    e = e < 128.0f ? e : 128.0f;                          // a NaN gives 128
                    w = hk * gl_expf(-e);
                }
                sr = sr + (w * cq.x); sg = sg + (w * cq.y); sb = sb + (w * cq.z);
                wsum = wsum + w;
            }
        }
        float r = cp.x, g = cp.y, b = cp.z;
        if (wsum > 0.0f) { r = sr / wsum; g = sg / wsum; b = sb / wsum; }
        if (MODE == 0) {
            dst[i] = make_float4(r, g, b, 0.0f);
        } else {
            if (MODE == 2) {
                const float *a = d.albedo + i * 3;
                r = r * floored(a[0]); g = g * floored(a[1]); b = b * floored(a[2]);
            }
            float *o = d.out + i * 3;
            o[0] = r; o[1] = g; o[2] = b;
        }
    }
}

template <bool NORMAL, bool DEPTH>
hipError_t launch_passes(const DevDenoise &d, unsigned long long n_tiles, uint32_t grid, hipStream_t stream) {
    hipError_t e;
    if (d.albedo) hipLaunchKernelGGL((denoise_pack_kernel<NORMAL, DEPTH, true>), dim3(grid), dim3(kBlockThreads), 0, stream, d, n_tiles);
    else hipLaunchKernelGGL((denoise_pack_kernel<NORMAL, DEPTH, false>), dim3(grid), dim3(kBlockThreads), 0, stream, d, n_tiles);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    for (uint32_t i = 0; i < d.iterations; i++) {
        const float4 *src = d.colour[i & 1u];
        float4 *dst = d.colour[(i + 1u) & 1u];
        const uint32_t step = 1u << i;
        if (i + 1u < d.iterations)
            hipLaunchKernelGGL((denoise_pass_kernel<NORMAL, DEPTH, 0>), dim3(grid), dim3(kBlockThreads), 0, stream, d, n_tiles, src, dst, step, d.kc[i]);
        else if (!d.albedo)
            hipLaunchKernelGGL((denoise_pass_kernel<NORMAL, DEPTH, 1>), dim3(grid), dim3(kBlockThreads), 0, stream, d, n_tiles, src, dst, step, d.kc[i]);
        else
            hipLaunchKernelGGL((denoise_pass_kernel<NORMAL, DEPTH, 2>), dim3(grid), dim3(kBlockThreads), 0, stream, d, n_tiles, src, dst, step, d.kc[i]);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

} // namespace

// instantiations: {normal} x {depth} x ({pack with / without albedo} + {middle, last, last with albedo})
hipError_t launch_denoise(const DevDenoise &d, hipStream_t stream) {
    const unsigned long long n_tiles = (unsigned long long)d.tiles_x * d.tiles_y * d.n_views;
    const uint32_t grid = n_tiles < kMaxGrid ? (uint32_t)n_tiles : kMaxGrid;
    if (d.normal) return d.depth ? launch_passes<true, true>(d, n_tiles, grid, stream) : launch_passes<true, false>(d, n_tiles, grid, stream);
    return d.depth ? launch_passes<false, true>(d, n_tiles, grid, stream) : launch_passes<false, false>(d, n_tiles, grid, stream);
}

} // namespace mipt
