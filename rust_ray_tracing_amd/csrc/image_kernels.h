// image_kernels.h -- what the image-space kernels share on the device: denoise.hip, denoise_variance.hip,
// upsample.hip, temporal.hip and lightmap.hip; sample_map.hip takes the colour helpers alone.  The tiles themselves are tile_shape.h.
//
// One pixel per lane.  A 256-thread block covers 64x4 pixels: the 64 lanes of a wave are 64 neighbours of one row, and a tap load at
// any step s is one contiguous 1 KB run of a row.  The taps of neighbouring pixels overlap; that reuse is left to the vector L1 and
// L2.  A pack pass turns planar inputs into one float4 of colour and one of guides {n.x, n.y, n.z, z} per pixel, so that a tap costs
// two 16-byte loads instead of seven 4-byte ones.  What a filter has and which pass it is in are template arguments of its kernels, so
// no lane ever branches on them.
//
// Every operator below is one rounded f32 operation in the order include/mipt.h gives (the translation units are built with
// -ffp-contract=off); expf is gl_expf of pt_device_math.h, glibc 2.35's, on the domain [-128, -0] the clamp leaves.
#pragma once
#include "pt_kernel.h"
#include "pt_device_math.h"
#include "tile_shape.h"

namespace mipt {

static_assert(kTileW * kTileH == (uint32_t)kBlockThreads, "one pixel per lane");

// ---- the tile walk: for (t = blockIdx.x; t < n_tiles; t += gridDim.x) over tile_count() tiles, on a grid of tile_grid() blocks ----
// The pixel of this lane in tile `t` of a launch over views of width x height.  false = outside the frame (a ragged edge tile).
// The pixel's index is (size_t)view * width * height + ((size_t)y * width + x), below 2^32 (MIPT_BATCH_MAX_PIXELS).
__device__ __forceinline__ bool lane_pixel(uint32_t width, uint32_t height, uint32_t tiles_x, uint32_t tiles_y, unsigned long long t,
                                           uint32_t &x, uint32_t &y, uint32_t &view) {
    const TilePixel p = tile_pixel(tiles_x, tiles_y, t, threadIdx.x);
    x = p.x; y = p.y; view = p.view;
    return x < width && y < height;
}
// The same over an atlas, which is one view; its index (size_t)y * width + x stays below 2^31.
__device__ __forceinline__ bool lane_texel(uint32_t width, uint32_t height, uint32_t tiles_x, uint32_t t, uint32_t &x, uint32_t &y) {
    const TilePixel p = tile_texel(tiles_x, t, threadIdx.x);
    x = p.x; y = p.y;
    return x < width && y < height;
}

// ---- colour ----
constexpr float kAlbedoFloor = 1.0f / 256.0f;
__device__ __forceinline__ float floored(float albedo) { return albedo > kAlbedoFloor ? albedo : kAlbedoFloor; }   // a NaN gives the floor

__device__ __forceinline__ float luminance(float r, float g, float b) { return ((0.2126f * r) + (0.7152f * g)) + (0.0722f * b); }   // Rec. 709
__device__ __forceinline__ float luminance(const float4 &c) { return luminance(c.x, c.y, c.z); }

// ---- a tap's weight ----
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
// the guide terms without a colour term in front: a single one is itself, not 0 + itself.  At least one of the two exists.
template <bool NORMAL, bool DEPTH>
__device__ __forceinline__ float guide_energy(const float4 &gp, const float4 &gq, float kn, float kz) {
    if (NORMAL && DEPTH) return normal_term(gp, gq, kn) + depth_term(gp, gq, kz);
    return NORMAL ? normal_term(gp, gq, kn) : depth_term(gp, gq, kz);
}
// hk * exp(-min(e, 128)).  The NaN rule: the comparison is written so that a NaN energy gives 128, a weight of hk * exp(-128) > 0.
__device__ __forceinline__ float tap_weight(float hk, float e) {
    e = e < 128.0f ? e : 128.0f;
    return hk * gl_expf(-e);
}

// ---- the pack pass of a frame filter ----
// Pixel i's planar inputs as colour[i] = {hdr / floored(albedo), w} and guides[i] = {n.x, n.y, n.z, z}; an absent guide's words are 0,
// and guides is not written when both are absent.
template <bool NORMAL, bool DEPTH, bool ALBEDO>
__device__ __forceinline__ void pack_pixel(const float *hdr, const float *albedo, const float *normal, const float *depth, size_t i, float w,
                                           float4 *colour, float4 *guides) {
    const float *h = hdr + i * 3;
    float r = h[0], g = h[1], b = h[2];
    if (ALBEDO) {
        const float *a = albedo + i * 3;
        r = r / floored(a[0]); g = g / floored(a[1]); b = b / floored(a[2]);
    }
    colour[i] = make_float4(r, g, b, w);
    if (NORMAL || DEPTH) {
        float4 gd = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (NORMAL) { const float *n = normal + i * 3; gd.x = n[0]; gd.y = n[1]; gd.z = n[2]; }
        if (DEPTH) gd.w = depth[i];
        guides[i] = gd;
    }
}

// ---- the taps of a pixel ----
// The 1D kernels: the B3 spline of the a-trous taps (radius 2) and the 3-tap binomial of the variance prefilter (radius 1).
constexpr float tap_kernel(int radius, int k) {
    constexpr float h[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    constexpr float g[3] = {1.0f / 4.0f, 1.0f / 2.0f, 1.0f / 4.0f};
    return radius == 2 ? h[k] : g[k];
}
// f(hk, centre, q) for each of the (2R + 1)^2 taps of pixel (x, y) at distance `step` that lie inside the frame, row by row.  The
// bounds rule: a tap outside is skipped, neither weighted nor added; it is tested in signed 64 bits, since step * 2 may pass the
// frame's size.  hk, the product of the two 1D kernels, is exact and a constant after unrolling; so is `centre`, and a caller takes
// the centre from the registers it holds instead of loading q, which is then base + its own index.
template <int R, typename F>
__device__ __forceinline__ void grid_taps(uint32_t x, uint32_t y, uint32_t width, uint32_t height, uint32_t step, size_t base, F &&f) {
    static_assert(R == 1 || R == 2, "tap_kernel has a kernel for these two radii");
#pragma unroll
    for (int dy = -R; dy <= R; dy++) {
        const long long qy = (long long)y + (long long)dy * (long long)step;
        if (qy < 0 || qy >= (long long)height) continue;
#pragma unroll
        for (int dx = -R; dx <= R; dx++) {
            const long long qx = (long long)x + (long long)dx * (long long)step;
            if (qx < 0 || qx >= (long long)width) continue;
            f(tap_kernel(R, dy + R) * tap_kernel(R, dx + R), dy == 0 && dx == 0, base + ((size_t)qy * width + (size_t)qx));
        }
    }
}
// the 25 a-trous taps, and the 3x3 neighbourhood at distance 1
template <typename F>
__device__ __forceinline__ void atrous_taps(uint32_t x, uint32_t y, uint32_t width, uint32_t height, uint32_t step, size_t base, F &&f) {
    grid_taps<2>(x, y, width, height, step, base, f);
}
template <typename F>
__device__ __forceinline__ void taps_3x3(uint32_t x, uint32_t y, uint32_t width, uint32_t height, size_t base, F &&f) {
    grid_taps<1>(x, y, width, height, 1u, base, f);
}

// ---- the launch ladder of an iterated filter (host) ----
// pack() -- the pack pass and whatever else goes before the iterations -- then pass(i, src, dst, mode) for i = 0 ... iterations - 1
// at step 2^i: iteration i reads colour[(first + i) & 1] and writes the other plane.  mode 0: a middle iteration, colour plane to colour
// plane; 1: the last, to the planar output; 2: the last, re-modulated by the albedo.  Both return hipGetLastError() of their launch.
template <typename Pack, typename Pass>
hipError_t launch_ladder(float4 *const (&colour)[2], uint32_t first, uint32_t iterations, bool remodulate, Pack &&pack, Pass &&pass) {
    hipError_t e = pack();
    for (uint32_t i = 0; i < iterations && e == hipSuccess; i++)
        e = pass(i, (const float4 *)colour[(first + i) & 1u], colour[(first + i + 1u) & 1u], i + 1u < iterations ? 0 : remodulate ? 2 : 1);
    return e;
}

} // namespace mipt
