// denoise.hip -- the edge-avoiding a-trous wavelet filter of include/mipt.h ("a-trous denoiser"): mipt_denoise*.
//
// A pack pass, then one launch per iteration (image_kernels.h: the tile walk, the pack, the taps, the ladder).  An iteration reads one
// colour plane and writes the other; the last one re-modulates and writes the planar output, so `out` may be `hdr`.  Which guides
// exist and whether a pass is the last are template arguments.
#include "image_kernels.h"

namespace mipt {

namespace {

template <bool NORMAL, bool DEPTH, bool ALBEDO>
__global__ __launch_bounds__(kBlockThreads) void denoise_pack_kernel(DevDenoise d, unsigned long long n_tiles) {
    for (unsigned long long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        uint32_t x, y, view;
        if (!lane_pixel(d.width, d.height, d.tiles_x, d.tiles_y, t, x, y, view)) continue;
        const size_t i = (size_t)view * d.width * d.height + ((size_t)y * d.width + x);
        pack_pixel<NORMAL, DEPTH, ALBEDO>(d.hdr, d.albedo, d.normal, d.depth, i, 0.0f, d.colour[0], d.guides);
    }
}

// MODE: launch_ladder's
template <bool NORMAL, bool DEPTH, int MODE>
__global__ __launch_bounds__(kBlockThreads) void denoise_pass_kernel(DevDenoise d, unsigned long long n_tiles, const float4 *__restrict__ src,
                                                                     float4 *__restrict__ dst, uint32_t step, float kc) {
    for (unsigned long long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        uint32_t x, y, view;
        if (!lane_pixel(d.width, d.height, d.tiles_x, d.tiles_y, t, x, y, view)) continue;
        const size_t base = (size_t)view * d.width * d.height, i = base + ((size_t)y * d.width + x);
        const float4 cp = src[i];
        float4 gp = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (NORMAL || DEPTH) gp = d.guides[i];
        float sr = 0.0f, sg = 0.0f, sb = 0.0f, wsum = 0.0f;
        const auto tap = [&](float hk, bool centre, size_t q) {
            const float4 cq = centre ? cp : src[q];
            float w = hk;                                                 // the centre: 9/64 without evaluation
            if (!centre) {
                const float dr = cp.x - cq.x, dg = cp.y - cq.y, db = cp.z - cq.z;
                float e = (((dr * dr) + (dg * dg)) + (db * db)) * kc;
                if (NORMAL || DEPTH) {
                    const float4 gq = d.guides[q];
                    if (NORMAL) e = e + normal_term(gp, gq, d.kn);
                    if (DEPTH) e = e + depth_term(gp, gq, d.kz);
                }
                w = tap_weight(hk, e);
            }
            sr = sr + (w * cq.x); sg = sg + (w * cq.y); sb = sb + (w * cq.z);
            wsum = wsum + w;
        };
        // atrous_taps of image_kernels.h spelled out: the same taps, bounds rule and kernel.  Written in the kernel, the compiler keeps
        // gl_expf's rare branch out of a tap's straight path; through the shared loop a pass was 4 % slower.
#pragma unroll
        for (int dy = -2; dy <= 2; dy++) {
            const long long qy = (long long)y + (long long)dy * (long long)step;
            if (qy < 0 || qy >= (long long)d.height) continue;
#pragma unroll
            for (int dx = -2; dx <= 2; dx++) {
                const long long qx = (long long)x + (long long)dx * (long long)step;
                if (qx < 0 || qx >= (long long)d.width) continue;
                tap(tap_kernel(2, dy + 2) * tap_kernel(2, dx + 2), dy == 0 && dx == 0, base + ((size_t)qy * d.width + (size_t)qx));
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
hipError_t launch_passes(const DevDenoise &d, hipStream_t stream) {
    const unsigned long long n_tiles = tile_count(d.tiles_x, d.tiles_y, d.n_views);
    const dim3 grid(tile_grid(n_tiles, kFrameMaxGrid)), block(kBlockThreads);
    return launch_ladder(
        d.colour, 0u, d.iterations, d.albedo != nullptr,
        [&] {
            const auto pack = d.albedo ? denoise_pack_kernel<NORMAL, DEPTH, true> : denoise_pack_kernel<NORMAL, DEPTH, false>;
            hipLaunchKernelGGL(pack, grid, block, 0, stream, d, n_tiles);
            return hipGetLastError();
        },
        [&](uint32_t i, const float4 *src, float4 *dst, int mode) {
            const auto pass = mode == 0 ? denoise_pass_kernel<NORMAL, DEPTH, 0> : mode == 1 ? denoise_pass_kernel<NORMAL, DEPTH, 1> : denoise_pass_kernel<NORMAL, DEPTH, 2>;
            hipLaunchKernelGGL(pass, grid, block, 0, stream, d, n_tiles, src, dst, 1u << i, d.kc[i]);
            return hipGetLastError();
        });
}

} // namespace

// instantiations: {normal} x {depth} x ({pack with / without albedo} + {middle, last, last with albedo})
hipError_t launch_denoise(const DevDenoise &d, hipStream_t stream) {
    if (d.normal) return d.depth ? launch_passes<true, true>(d, stream) : launch_passes<true, false>(d, stream);
    return d.depth ? launch_passes<false, true>(d, stream) : launch_passes<false, false>(d, stream);
}

} // namespace mipt
