// denoise_variance.hip -- the variance-guided a-trous filter of include/mipt.h ("variance-guided a-trous filter"):
// mipt_denoise_variance*.  The second half of the SVGF-style pipeline whose first half is temporal.hip.
//
// A pack pass, a spatial-estimate pass (skipped when short_history == 0), then one launch per iteration (image_kernels.h: the tile
// walk, the pack, the taps, the ladder).  The colour's fourth word, which denoise.hip leaves 0, carries the pixel's variance.
//
// The estimate pass reads colour plane 0 and writes whole float4s into plane 1, so no lane reads a word another lane is writing; the
// iterations then ping-pong from the plane that was written last.  An iteration reads 9 variances at distance 1 (the prefilter) and
// the 25 taps at its step.  sqrtf is the correctly rounded expansion of __builtin_sqrtf.
#include "image_kernels.h"

namespace mipt {

namespace {

template <bool NORMAL, bool DEPTH, bool ALBEDO>
__global__ __launch_bounds__(kBlockThreads) void variance_pack_kernel(DevVariance d, unsigned long long n_tiles) {
    for (unsigned long long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        uint32_t x, y, view;
        if (!lane_pixel(d.width, d.height, d.tiles_x, d.tiles_y, t, x, y, view)) continue;
        const size_t i = (size_t)view * d.width * d.height + ((size_t)y * d.width + x);
        float var = 0.0f;
        if (d.variance) {                                     // the same for every lane of the launch
            const float v = d.variance[i];
            var = v > 0.0f ? v : 0.0f;                        // a NaN gives 0
        }
        pack_pixel<NORMAL, DEPTH, ALBEDO>(d.hdr, d.albedo, d.normal, d.depth, i, var, d.colour[0], d.guides);
    }
}

// The variance of a pixel whose history is shorter than short_history, from the luminances of its 5x5 neighbourhood; every other
// pixel is copied.  colour[0] -> colour[1].
template <bool NORMAL, bool DEPTH>
__global__ __launch_bounds__(kBlockThreads) void variance_estimate_kernel(DevVariance d, unsigned long long n_tiles) {
    const float4 *__restrict__ src = d.colour[0];
    float4 *__restrict__ dst = d.colour[1];
    for (unsigned long long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        uint32_t x, y, view;
        if (!lane_pixel(d.width, d.height, d.tiles_x, d.tiles_y, t, x, y, view)) continue;
        const size_t base = (size_t)view * d.width * d.height, i = base + ((size_t)y * d.width + x);
        float4 cp = src[i];
        const float len = d.length ? d.length[i] : 1.0f;
        if (!(len >= d.short_history)) {                      // a NaN length takes this side
            float4 gp = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (NORMAL || DEPTH) gp = d.guides[i];
            float s1 = 0.0f, s2 = 0.0f, ws = 0.0f;
            atrous_taps(x, y, d.width, d.height, 1u, base, [&](float, bool centre, size_t q) {   // the taps' places, not their kernel
                const float lq = luminance(centre ? cp : src[q]);
                float w = 1.0f;                               // the centre, or no guide at all: 1 without evaluation
                if (!centre && (NORMAL || DEPTH)) w = tap_weight(1.0f, guide_energy<NORMAL, DEPTH>(gp, d.guides[q], d.kn, d.kz));   // 1 * v is v, bit for bit
                s1 = s1 + (w * lq);
                s2 = s2 + (w * (lq * lq));
                ws = ws + w;
            });
            const float mu = s1 / ws;
            float v = (s2 / ws) - (mu * mu);
            v = v > 0.0f ? v : 0.0f;
            const float lc = len > 1.0f ? len : 1.0f;
            cp.w = v * (d.short_history / lc);
        }
        dst[i] = cp;
    }
}

// MODE: launch_ladder's
template <bool NORMAL, bool DEPTH, int MODE>
__global__ __launch_bounds__(kBlockThreads) void variance_pass_kernel(DevVariance d, unsigned long long n_tiles, const float4 *__restrict__ src,
                                                                      float4 *__restrict__ dst, uint32_t step) {
    for (unsigned long long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        uint32_t x, y, view;
        if (!lane_pixel(d.width, d.height, d.tiles_x, d.tiles_y, t, x, y, view)) continue;
        const size_t base = (size_t)view * d.width * d.height, i = base + ((size_t)y * d.width + x);
        const float4 cp = src[i];
        float4 gp = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (NORMAL || DEPTH) gp = d.guides[i];
        // the 3x3 prefilter of the variance: at distance 1 whatever the step
        float gs = 0.0f, gw = 0.0f;
        taps_3x3(x, y, d.width, d.height, base, [&](float gk, bool centre, size_t q) {
            const float vq = centre ? cp.w : src[q].w;
            gs = gs + (gk * vq);
            gw = gw + gk;
        });
        const float gv = gs / gw;
        const float kl = 1.0f / ((d.sigma_l * __builtin_sqrtf(gv)) + 1e-8f);
        const float lp = luminance(cp);
        float sr = 0.0f, sg = 0.0f, sb = 0.0f, sv = 0.0f, wsum = 0.0f;
        const auto tap = [&](float hk, bool centre, size_t q) {
            const float4 cq = centre ? cp : src[q];
            float w = hk;                                                 // the centre: 9/64 without evaluation
            if (!centre) {
                float e = fabsf(lp - luminance(cq)) * kl;
                if (NORMAL || DEPTH) {
                    const float4 gq = d.guides[q];
                    if (NORMAL) e = e + normal_term(gp, gq, d.kn);
                    if (DEPTH) e = e + depth_term(gp, gq, d.kz);
                }
                w = tap_weight(hk, e);
            }
            sr = sr + (w * cq.x); sg = sg + (w * cq.y); sb = sb + (w * cq.z);
            sv = sv + ((w * w) * cq.w);
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
hipError_t launch_passes(const DevVariance &d, hipStream_t stream) {
    const unsigned long long n_tiles = tile_count(d.tiles_x, d.tiles_y, d.n_views);
    const dim3 grid(tile_grid(n_tiles, kFrameMaxGrid)), block(kBlockThreads);
    const bool estimate = d.short_history > 0.0f;             // its pass leaves the colour in plane 1: the first iteration reads that
    return launch_ladder(
        d.colour, estimate ? 1u : 0u, d.iterations, d.albedo != nullptr,
        [&] {
            const auto pack = d.albedo ? variance_pack_kernel<NORMAL, DEPTH, true> : variance_pack_kernel<NORMAL, DEPTH, false>;
            hipLaunchKernelGGL(pack, grid, block, 0, stream, d, n_tiles);
            hipError_t e = hipGetLastError();
            if (e != hipSuccess || !estimate) return e;
            hipLaunchKernelGGL((variance_estimate_kernel<NORMAL, DEPTH>), grid, block, 0, stream, d, n_tiles);
            return hipGetLastError();
        },
        [&](uint32_t i, const float4 *src, float4 *dst, int mode) {
            const auto pass = mode == 0 ? variance_pass_kernel<NORMAL, DEPTH, 0> : mode == 1 ? variance_pass_kernel<NORMAL, DEPTH, 1> : variance_pass_kernel<NORMAL, DEPTH, 2>;
            hipLaunchKernelGGL(pass, grid, block, 0, stream, d, n_tiles, src, dst, 1u << i);
            return hipGetLastError();
        });
}

} // namespace

// instantiations: {normal} x {depth} x ({pack with / without albedo} + {estimate} + {middle, last, last with albedo})
hipError_t launch_denoise_variance(const DevVariance &d, hipStream_t stream) {
    if (d.normal) return d.depth ? launch_passes<true, true>(d, stream) : launch_passes<true, false>(d, stream);
    return d.depth ? launch_passes<false, true>(d, stream) : launch_passes<false, false>(d, stream);
}

} // namespace mipt
