// lightmap.hip -- the kernels of include/mipt.h "lightmap finishing": the edge-avoiding a-trous filter over the covered texels of an
// atlas (mipt_lightmap_filter*) and the dilation into its gutters (mipt_lightmap_dilate*).
//
// Both are a pack pass, then one launch per iteration or pass (image_kernels.h: the tile walk over the atlas's one view, the taps, the
// ladder).  The filter's pack pass writes one float4 of colour per texel with the covered flag in w, and one float4 each of position
// and normal where those guides exist: a tap is then 16-byte loads, and a tap whose colour word says "uncovered" fetches no guide.
// An iteration reads one colour plane and writes the other; the last one writes the planar output, so `out` may be `radiance`.
// Which guides exist and whether a pass is the last are template arguments.  The dilation keeps {r, g, b, level} per texel in two
// planes; a pass reads one and writes the other, so it sees only the state of the pass before it.
//
// An uncovered texel's words travel through the planes as loaded: no arithmetic touches them.
#include "image_kernels.h"
#include "../../include/mipt.h"

namespace mipt {

namespace {

// ---- filter ------------------------------------------------------------------------------------------------------------------------
template <bool POS, bool NRM>
__global__ __launch_bounds__(kBlockThreads) void lightmap_pack_kernel(DevLightmapFilter d, uint32_t n_tiles) {
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        uint32_t x, y;
        if (!lane_texel(d.width, d.height, d.tiles_x, t, x, y)) continue;
        const size_t i = (size_t)y * d.width + x;
        const float *c = d.radiance + i * 3;
        const bool covered = d.points[i].w != MIPT_HIT_NONE;
        d.colour[0][i] = make_float4(c[0], c[1], c[2], covered ? 1.0f : 0.0f);
        if (POS) { const float *p = d.position + i * 3; d.pos4[i] = make_float4(p[0], p[1], p[2], 0.0f); }
        if (NRM) { const float *n = d.normal + i * 3; d.nrm4[i] = make_float4(n[0], n[1], n[2], 0.0f); }
    }
}

template <bool POS, bool NRM, bool LAST>
__global__ __launch_bounds__(kBlockThreads) void lightmap_pass_kernel(DevLightmapFilter d, uint32_t n_tiles, const float4 *__restrict__ src,
                                                                      float4 *__restrict__ dst, uint32_t step, float kc, float kd) {
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        uint32_t x, y;
        if (!lane_texel(d.width, d.height, d.tiles_x, t, x, y)) continue;
        const size_t i = (size_t)y * d.width + x;
        const float4 cp = src[i];
        float r = cp.x, g = cp.y, b = cp.z;
        if (cp.w != 0.0f) {                                              // an uncovered texel keeps its words
            float4 pp = make_float4(0.0f, 0.0f, 0.0f, 0.0f), np = pp;
            if (POS) pp = d.pos4[i];
            if (NRM) np = d.nrm4[i];
            float sr = 0.0f, sg = 0.0f, sb = 0.0f, wsum = 0.0f;
            const auto tap = [&](float hk, bool centre, size_t q) {
                const float4 cq = centre ? cp : src[q];                  // one whole load, then the test of its w
                float w = hk;                                             // the centre: 9/64 without evaluation
                if (!centre) {
                    if (cq.w == 0.0f) return;                             // an uncovered tap: skipped like one outside, no guide fetched
                    const float dr = cp.x - cq.x, dg = cp.y - cq.y, db = cp.z - cq.z;
                    float e = (((dr * dr) + (dg * dg)) + (db * db)) * kc;
                    float4 nq = make_float4(0.0f, 0.0f, 0.0f, 0.0f), pq = nq;
                    if (NRM) nq = d.nrm4[q];
                    if (POS) pq = d.pos4[q];
                    if (NRM) e = e + normal_term(np, nq, d.kn);
                    if (POS) {
                        const float Dx = pq.x - pp.x, Dy = pq.y - pp.y, Dz = pq.z - pp.z;   // tap minus centre: l below has a sign
                        if (NRM) {
                            const float l = ((np.x * Dx) + (np.y * Dy)) + (np.z * Dz);
                            e = e + ((l * l) * d.kl);
                        }
                        e = e + ((((Dx * Dx) + (Dy * Dy)) + (Dz * Dz)) * kd);
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
                    tap(tap_kernel(2, dy + 2) * tap_kernel(2, dx + 2), dy == 0 && dx == 0, ((size_t)qy * d.width + (size_t)qx));
                }
            }
            if (wsum > 0.0f) { r = sr / wsum; g = sg / wsum; b = sb / wsum; }
        }
        if (!LAST) {
            dst[i] = make_float4(r, g, b, cp.w);
        } else {
            float *o = d.out + i * 3;
            o[0] = r; o[1] = g; o[2] = b;
        }
    }
}

template <bool POS, bool NRM>
hipError_t launch_filter_passes(const DevLightmapFilter &d, hipStream_t stream) {
    const uint32_t n_tiles = (uint32_t)tile_count(d.tiles_x, d.tiles_y, 1u);   // at most 2^30 (tile_shape.h)
    const dim3 grid(tile_grid(n_tiles, kAtlasMaxGrid)), block(kBlockThreads);
    return launch_ladder(
        d.colour, 0u, d.iterations, false,
        [&] {
            hipLaunchKernelGGL((lightmap_pack_kernel<POS, NRM>), grid, block, 0, stream, d, n_tiles);
            return hipGetLastError();
        },
        [&](uint32_t i, const float4 *src, float4 *dst, int mode) {
            const auto pass = mode == 0 ? lightmap_pass_kernel<POS, NRM, false> : lightmap_pass_kernel<POS, NRM, true>;
            hipLaunchKernelGGL(pass, grid, block, 0, stream, d, n_tiles, src, dst, 1u << i, d.kc[i], d.kd[i]);
            return hipGetLastError();
        });
}

// ---- dilation ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlockThreads) void dilate_pack_kernel(DevLightmapDilate d, uint32_t n_tiles) {
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        uint32_t x, y;
        if (!lane_texel(d.width, d.height, d.tiles_x, t, x, y)) continue;
        const size_t i = (size_t)y * d.width + x;
        const float *c = d.radiance + i * 3;
        d.state[0][i] = make_float4(c[0], c[1], c[2], __uint_as_float(d.points[i].w != MIPT_HIT_NONE ? 1u : 0u));
    }
}

// pass k: a texel of level 0 with a neighbour of non-zero level takes the neighbours' mean and level k + 1
__global__ __launch_bounds__(kBlockThreads) void dilate_pass_kernel(DevLightmapDilate d, uint32_t n_tiles, const float4 *__restrict__ src,
                                                                    float4 *__restrict__ dst, uint32_t k) {
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        uint32_t x, y;
        if (!lane_texel(d.width, d.height, d.tiles_x, t, x, y)) continue;
        const size_t i = (size_t)y * d.width + x;
        float4 s = src[i];
        if (__float_as_uint(s.w) == 0u) {
            float sr = 0.0f, sg = 0.0f, sb = 0.0f;
            uint32_t count = 0;
            taps_3x3(x, y, d.width, d.height, 0, [&](float, bool centre, size_t qi) {   // the eight neighbours, unweighted
                if (centre) return;
                const float4 q = src[qi];
                if (__float_as_uint(q.w) == 0u) return;
                sr = sr + q.x; sg = sg + q.y; sb = sb + q.z;
                count++;
            });
            if (count != 0u) {
                const float cf = (float)count;
                s = make_float4(sr / cf, sg / cf, sb / cf, __uint_as_float(k + 1u));
            }
        }
        dst[i] = s;
    }
}

__global__ __launch_bounds__(kBlockThreads) void dilate_unpack_kernel(DevLightmapDilate d, uint32_t n_tiles, const float4 *__restrict__ src) {
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        uint32_t x, y;
        if (!lane_texel(d.width, d.height, d.tiles_x, t, x, y)) continue;
        const size_t i = (size_t)y * d.width + x;
        const float4 s = src[i];
        float *o = d.out + i * 3;
        o[0] = s.x; o[1] = s.y; o[2] = s.z;
        if (d.level) d.level[i] = __float_as_uint(s.w);
    }
}

} // namespace

// instantiations: {position} x {normal} x ({pack} + {middle, last})
hipError_t launch_lightmap_filter(const DevLightmapFilter &d, hipStream_t stream) {
    if (d.position) return d.normal ? launch_filter_passes<true, true>(d, stream) : launch_filter_passes<true, false>(d, stream);
    return d.normal ? launch_filter_passes<false, true>(d, stream) : launch_filter_passes<false, false>(d, stream);
}

hipError_t launch_lightmap_dilate(const DevLightmapDilate &d, hipStream_t stream) {
    const uint32_t n_tiles = (uint32_t)tile_count(d.tiles_x, d.tiles_y, 1u);
    const uint32_t grid = tile_grid(n_tiles, kAtlasMaxGrid);
    hipError_t e;
    hipLaunchKernelGGL(dilate_pack_kernel, dim3(grid), dim3(kBlockThreads), 0, stream, d, n_tiles);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    for (uint32_t k = 1; k <= d.radius; k++) {
        hipLaunchKernelGGL(dilate_pass_kernel, dim3(grid), dim3(kBlockThreads), 0, stream, d, n_tiles, d.state[(k - 1u) & 1u], d.state[k & 1u], k);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(dilate_unpack_kernel, dim3(grid), dim3(kBlockThreads), 0, stream, d, n_tiles, d.state[d.radius & 1u]);
    return hipGetLastError();
}

} // namespace mipt
