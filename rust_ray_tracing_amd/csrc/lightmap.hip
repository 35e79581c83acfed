// lightmap.hip -- the kernels of include/mipt.h "lightmap finishing": the edge-avoiding a-trous filter over the covered texels of an
// atlas (mipt_lightmap_filter*) and the dilation into its gutters (mipt_lightmap_dilate*).
//
// Both are a pack pass, then one launch per iteration or pass, in the shape of denoise.hip: one texel per lane, a 256-thread block
// covers 64x4 texels, so a tap load at any step is one contiguous run of a row, and the reuse between neighbouring texels' taps is
// left to the vector L1 and L2.  The filter's pack pass writes one float4 of colour per texel with the covered flag in w, and one
// float4 each of position and normal where those guides exist: a tap is then 16-byte loads, and a tap whose colour word says
// "uncovered" fetches no guide.  An iteration reads one colour plane and writes the other; the last one writes the planar output, so
// `out` may be `radiance`.  Which guides exist and whether a pass is the last are template arguments.  The dilation keeps {r, g, b,
// level} per texel in two planes; a pass reads one and writes the other, so it sees only the state of the pass before it.
//
// Every operator below is one rounded f32 operation in the order the header gives (the translation unit is built with
// -ffp-contract=off); expf is gl_expf of pt_device_math.h, glibc 2.35's, on the domain [-128, -0] the clamp leaves.  An uncovered
// texel's words travel through the planes as loaded: no arithmetic touches them.
#include "pt_kernel.h"
#include "pt_device_math.h"
#include "../../include/mipt.h"

namespace mipt {

namespace {

constexpr uint32_t kTileW = 64, kTileH = 4;                  // texels a block covers: one wave per row
constexpr uint32_t kMaxGrid = 1u << 16;                      // blocks per launch; a block walks the tiles with this stride
static_assert(kTileW * kTileH == (uint32_t)kBlockThreads, "one texel per lane");

// The texel of this lane in tile `t`; false = outside the atlas (a ragged edge tile).  The index stays below 2^31.
__device__ __forceinline__ bool lane_texel(uint32_t width, uint32_t height, uint32_t tiles_x, uint32_t t, uint32_t &x, uint32_t &y) {
    x = (t % tiles_x) * kTileW + (threadIdx.x & (kTileW - 1u));
    y = (t / tiles_x) * kTileH + (threadIdx.x / kTileW);
    return x < width && y < height;
}

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
    constexpr float h[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
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
#pragma unroll
            for (int dy = -2; dy <= 2; dy++) {
                // a tap outside the atlas is skipped: neither weighted nor added (signed 64-bit: step * 2 may pass the atlas's size)
                const long long qy = (long long)y + (long long)dy * (long long)step;
                if (qy < 0 || qy >= (long long)d.height) continue;
#pragma unroll
                for (int dx = -2; dx <= 2; dx++) {
                    const long long qx = (long long)x + (long long)dx * (long long)step;
                    if (qx < 0 || qx >= (long long)d.width) continue;
                    const float hk = h[dy + 2] * h[dx + 2];              // exact: a constant after unrolling
                    float w;
                    float4 cq;
                    if (dy == 0 && dx == 0) {
                        cq = cp;
                        w = hk;                                           // the centre: 9/64 without evaluation
                    } else {
                        const size_t q = (size_t)qy * d.width + (size_t)qx;
                        cq = src[q];
                        if (cq.w == 0.0f) continue;                       // an uncovered tap: skipped like one outside, no guide fetched
                        const float dr = cp.x - cq.x, dg = cp.y - cq.y, db = cp.z - cq.z;
                        float e = (((dr * dr) + (dg * dg)) + (db * db)) * kc;
                        float4 nq = make_float4(0.0f, 0.0f, 0.0f, 0.0f), pq = nq;
                        if (NRM) nq = d.nrm4[q];
                        if (POS) pq = d.pos4[q];
                        if (NRM) {
                            const float nx = np.x - nq.x, ny = np.y - nq.y, nz = np.z - nq.z;
                            e = e + ((((nx * nx) + (ny * ny)) + (nz * nz)) * d.kn);
                        }
                        if (POS) {
                            const float Dx = pq.x - pp.x, Dy = pq.y - pp.y, Dz = pq.z - pp.z;
                            if (NRM) {
                                const float l = ((np.x * Dx) + (np.y * Dy)) + (np.z * Dz);
                                e = e + ((l * l) * d.kl);
                            }
                            e = e + ((((Dx * Dx) + (Dy * Dy)) + (Dz * Dz)) * kd);
                        }
                        e = e < 128.0f ? e : 128.0f;                      // a NaN gives 128
                        w = hk * gl_expf(-e);
                    }
                    sr = sr + (w * cq.x); sg = sg + (w * cq.y); sb = sb + (w * cq.z);
                    wsum = wsum + w;
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
hipError_t launch_filter_passes(const DevLightmapFilter &d, uint32_t n_tiles, uint32_t grid, hipStream_t stream) {
    hipError_t e;
    hipLaunchKernelGGL((lightmap_pack_kernel<POS, NRM>), dim3(grid), dim3(kBlockThreads), 0, stream, d, n_tiles);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    for (uint32_t i = 0; i < d.iterations; i++) {
        const float4 *src = d.colour[i & 1u];
        float4 *dst = d.colour[(i + 1u) & 1u];
        const uint32_t step = 1u << i;
        if (i + 1u < d.iterations)
            hipLaunchKernelGGL((lightmap_pass_kernel<POS, NRM, false>), dim3(grid), dim3(kBlockThreads), 0, stream, d, n_tiles, src, dst, step, d.kc[i], d.kd[i]);
        else
            hipLaunchKernelGGL((lightmap_pass_kernel<POS, NRM, true>), dim3(grid), dim3(kBlockThreads), 0, stream, d, n_tiles, src, dst, step, d.kc[i], d.kd[i]);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
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
#pragma unroll
            for (int dy = -1; dy <= 1; dy++) {
                const long long qy = (long long)y + dy;
                if (qy < 0 || qy >= (long long)d.height) continue;
#pragma unroll
                for (int dx = -1; dx <= 1; dx++) {
                    const long long qx = (long long)x + dx;
                    if ((dy == 0 && dx == 0) || qx < 0 || qx >= (long long)d.width) continue;
                    const float4 q = src[(size_t)qy * d.width + (size_t)qx];
                    if (__float_as_uint(q.w) == 0u) continue;
                    sr = sr + q.x; sg = sg + q.y; sb = sb + q.z;
                    count++;
                }
            }
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
    const uint32_t n_tiles = d.tiles_x * d.tiles_y;                      // < 2^31: one tile holds at least one texel
    const uint32_t grid = n_tiles < kMaxGrid ? n_tiles : kMaxGrid;
    if (d.position) return d.normal ? launch_filter_passes<true, true>(d, n_tiles, grid, stream) : launch_filter_passes<true, false>(d, n_tiles, grid, stream);
    return d.normal ? launch_filter_passes<false, true>(d, n_tiles, grid, stream) : launch_filter_passes<false, false>(d, n_tiles, grid, stream);
}

hipError_t launch_lightmap_dilate(const DevLightmapDilate &d, hipStream_t stream) {
    const uint32_t n_tiles = d.tiles_x * d.tiles_y;
    const uint32_t grid = n_tiles < kMaxGrid ? n_tiles : kMaxGrid;
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
