// temporal.hip -- the temporal accumulation of include/mipt.h ("temporal accumulation"): mipt_temporal*.
//
// One gather kernel.  Every pixel projects its first hit's world position through the camera record the previous history carries,
// gathers that history with four bilinear taps that must agree with it in material, normal and depth, blends this frame's sample in
// and writes the new history, the output frame and the optional length / variance planes.  A history keeps three float4 per pixel
// ({colour, length}, {normal, depth}, {moments, material}), so a tap costs three 16-byte loads.
//
// The tile walk and the colour helpers are image_kernels.h's; the four bilinear taps are this file's own.  Whether there is an albedo
// plane and whether this is the first frame are template arguments: the absent branches do not exist in the code; neither does
// anything of the count plane (mipt_temporal_counts*, COUNTS) in the plain kernels, whose argument stays DevTemporal.  The camera
// records of this frame travel as kernel arguments, eight views to a launch, and the first tile of each view writes its record into
// history_out's header, so the entry neither allocates nor copies.
//
// Every comparison is written so that a NaN takes the reject / reset side.
#include "image_kernels.h"

namespace mipt {

namespace {

constexpr float kMinWeight = 1.0f / 64.0f;
constexpr float kMiss = 1e30f;

struct Sums { float w, r, g, b, len, m1, m2; };

// One tap of view `base` of the previous history: added to `s` if it lies inside the frame and agrees with the pixel.  q < 2^32.
// COUNTS: a tap without a sample behind it (len_q > 0 fails; a NaN too) is rejected as well.
template <bool COUNTS>
__device__ __forceinline__ void tap(const DevTemporal &d, const float4 *h0, const float4 *h1, const float4 *h2, size_t base, long long qx,
                                    long long qy, float w, uint32_t material, float nx, float ny, float nz, float d2, Sums &s) {
    if (qx < 0 || qx >= (long long)d.width || qy < 0 || qy >= (long long)d.height) return;
    const size_t q = base + ((size_t)qy * d.width + (size_t)qx);
    const float4 c = h0[q], g = h1[q], m = h2[q];
    const float dx = nx - g.x, dy = ny - g.y, dz = nz - g.z;
    const float dn = ((dx * dx) + (dy * dy)) + (dz * dz);
    const bool ok = __float_as_uint(m.z) == material && dn <= d.normal_tol && fabsf(d2 - (g.w * g.w)) <= d.depth_tol * d2;
    if (!ok) return;
    if (COUNTS && !(c.w > 0.0f)) return;
    s.w = s.w + w;
    s.r = s.r + (w * c.x); s.g = s.g + (w * c.y); s.b = s.b + (w * c.z);
    s.len = s.len + (w * c.w);
    s.m1 = s.m1 + (w * m.x); s.m2 = s.m2 + (w * m.y);
}

template <bool COUNTS> struct KernelArgs { using type = DevTemporal; };
template <> struct KernelArgs<true> { using type = DevTemporalCounts; };
__device__ __forceinline__ const DevTemporal &plain(const DevTemporal &a) { return a; }
__device__ __forceinline__ const DevTemporal &plain(const DevTemporalCounts &a) { return a.t; }
__device__ __forceinline__ uint32_t samples_of(const DevTemporal &, size_t) { return 1u; }
__device__ __forceinline__ uint32_t samples_of(const DevTemporalCounts &a, size_t i) {
    const uint32_t k = a.counts[i];
    return k < a.samples_cap ? k : a.samples_cap;
}

template <bool ALBEDO, bool FIRST, bool COUNTS>
__global__ __launch_bounds__(kBlockThreads) void temporal_kernel(typename KernelArgs<COUNTS>::type args, unsigned long long n_tiles) {
    const DevTemporal &d = plain(args);
    const size_t header = (size_t)d.n_views * 16;            // f32 in front of the planes
    const float4 *in0 = nullptr, *in1 = nullptr, *in2 = nullptr;
    if (!FIRST) {
        in0 = (const float4 *)(d.history_in + header);
        in1 = in0 + d.n_pixels;
        in2 = in1 + d.n_pixels;
    }
    float4 *out0 = (float4 *)(d.history_out + header), *out1 = out0 + d.n_pixels, *out2 = out1 + d.n_pixels;
    const float wf = (float)d.width, hf = (float)d.height;
    const float aspect = wf / hf;
    for (unsigned long long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        uint32_t x, y, local;                                 // local < view_count <= kTemporalGroupViews
        const bool inside = lane_pixel(d.width, d.height, d.tiles_x, d.tiles_y, t, x, y, local);
        const uint32_t view = d.view_begin + local;
        // the camera record: lanes 0 ... 15 of the view's first tile -- row 0, x == lane -- and before the test, since a frame narrower
        // than 16 pixels has them outside
        static_assert(kTileW >= 16u, "the 16 words of a record lie in one tile row");
        if (y == 0u && x < 16u) d.history_out[(size_t)view * 16 + x] = d.camera[local][x];
        if (!inside) continue;                                // a ragged edge tile
        const size_t base = (size_t)view * d.width * d.height;
        const size_t i = base + ((size_t)y * d.width + x);   // < 2^32 (MIPT_BATCH_MAX_PIXELS)

        const uint32_t ns = samples_of(args, i);              // the pixel's samples in this frame: 1 without a count plane
        const float nf = (float)ns;
        float ccr = 0.0f, ccg = 0.0f, ccb = 0.0f;             // ns == 0: hdr holds nothing of this frame and is not read
        if (!COUNTS || ns > 0u) {
            const float *h = d.hdr + i * 3;
            ccr = h[0]; ccg = h[1]; ccb = h[2];
        }
        float ar = 1.0f, ag = 1.0f, ab = 1.0f;
        if (ALBEDO) {
            const float *a = d.albedo + i * 3;
            ar = floored(a[0]); ag = floored(a[1]); ab = floored(a[2]);
            ccr = ccr / ar; ccg = ccg / ag; ccb = ccb / ab;
        }
        const float l = luminance(ccr, ccg, ccb);
        const float *n = d.normal + i * 3;
        const float nx = n[0], ny = n[1], nz = n[2];
        const float depth = d.depth[i];
        const uint32_t material = d.material[i];

        float cr = ccr, cg = ccg, cb = ccb, len = 1.0f, m1 = l, m2 = l * l;      // RESET
        if (COUNTS) {                                                            // ns == 0: cc and l are +0, and so is all of it
            len = nf < d.max_history ? nf : d.max_history;
            if (ns == 0u) { cr = cg = cb = 0.0f; m1 = m2 = 0.0f; }
        }
        if (!FIRST && depth < kMiss) {
            const float *rec = d.history_in + (size_t)view * 16;                 // B[3][3], C[3]: the same for the whole block
            const float *p = d.position + i * 3;
            const float dx = p[0] - rec[9], dy = p[1] - rec[10], dz = p[2] - rec[11];
            const float vx = ((rec[0] * dx) + (rec[1] * dy)) + (rec[2] * dz);
            const float vy = ((rec[3] * dx) + (rec[4] * dy)) + (rec[5] * dz);
            const float vz = ((rec[6] * dx) + (rec[7] * dy)) + (rec[8] * dz);
            if (vz > 0.0f) {
                const float sx = -(vx / vz), sy = vy / vz;
                const float fx = (((sx / aspect) + 1.0f) * 0.5f) * wf;
                const float fy = hf - (((sy + 1.0f) * 0.5f) * hf);
                if (fx >= -1.0f && fx < wf && fy >= -1.0f && fy < hf) {
                    const float flx = floorf(fx), fly = floorf(fy);
                    const long long x0 = (long long)flx, y0 = (long long)fly;
                    const float wx = fx - flx, wy = fy - fly;
                    const float ox = 1.0f - wx, oy = 1.0f - wy;
                    const float d2 = ((dx * dx) + (dy * dy)) + (dz * dz);
                    Sums s = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
                    tap<COUNTS>(d, in0, in1, in2, base, x0, y0, ox * oy, material, nx, ny, nz, d2, s);
                    tap<COUNTS>(d, in0, in1, in2, base, x0 + 1, y0, wx * oy, material, nx, ny, nz, d2, s);
                    tap<COUNTS>(d, in0, in1, in2, base, x0, y0 + 1, ox * wy, material, nx, ny, nz, d2, s);
                    tap<COUNTS>(d, in0, in1, in2, base, x0 + 1, y0 + 1, wx * wy, material, nx, ny, nz, d2, s);
                    if (s.w > kMinWeight) {
                        const float pr = s.r / s.w, pg = s.g / s.w, pb = s.b / s.w, lp = s.len / s.w;
                        const float p1 = s.m1 / s.w, p2 = s.m2 / s.w;
                        if (COUNTS && ns == 0u) {                                // pure reprojection; sl / sw may round past the cap
                            cr = pr; cg = pg; cb = pb; len = lp < d.max_history ? lp : d.max_history; m1 = p1; m2 = p2;
                        } else {
                            float ln = lp + nf;
                            ln = ln < d.max_history ? ln : d.max_history;
                            float al = nf / ln;
                            al = al > d.alpha_min ? al : d.alpha_min;
                            if (COUNTS) al = al < 1.0f ? al : 1.0f;
                            cr = pr + ((ccr - pr) * al); cg = pg + ((ccg - pg) * al); cb = pb + ((ccb - pb) * al);
                            m1 = p1 + ((l - p1) * al);
                            m2 = p2 + (((l * l) - p2) * al);
                            len = ln;
                        }
                    }
                }
            }
        }

        out0[i] = make_float4(cr, cg, cb, len);
        out1[i] = make_float4(nx, ny, nz, depth);
        out2[i] = make_float4(m1, m2, __uint_as_float(material), 0.0f);
        float *o = d.out + i * 3;
        if (ALBEDO) { o[0] = cr * ar; o[1] = cg * ag; o[2] = cb * ab; }
        else { o[0] = cr; o[1] = cg; o[2] = cb; }
        if (d.length) d.length[i] = len;
        if (d.variance) {
            const float var = m2 - (m1 * m1);
            d.variance[i] = var > 0.0f ? var : 0.0f;
        }
    }
}

template <bool ALBEDO, bool FIRST>
hipError_t launch_group(const DevTemporal &d, const uint32_t *counts, uint32_t samples_cap, hipStream_t stream) {
    const unsigned long long n_tiles = tile_count(d.tiles_x, d.tiles_y, d.view_count);
    const uint32_t grid = tile_grid(n_tiles, kFrameMaxGrid);
    if (counts) {
        const DevTemporalCounts c = {d, counts, samples_cap};
        hipLaunchKernelGGL((temporal_kernel<ALBEDO, FIRST, true>), dim3(grid), dim3(kBlockThreads), 0, stream, c, n_tiles);
    } else {
        hipLaunchKernelGGL((temporal_kernel<ALBEDO, FIRST, false>), dim3(grid), dim3(kBlockThreads), 0, stream, d, n_tiles);
    }
    return hipGetLastError();
}

} // namespace

hipError_t launch_temporal(DevTemporal d, const float *records, hipStream_t stream, const uint32_t *counts, uint32_t samples_cap) {
    for (uint32_t v = 0; v < d.n_views; v += kTemporalGroupViews) {
        d.view_begin = v;
        d.view_count = d.n_views - v < kTemporalGroupViews ? d.n_views - v : kTemporalGroupViews;
        for (uint32_t k = 0; k < d.view_count; k++)
            for (int j = 0; j < 16; j++) d.camera[k][j] = records[(size_t)(v + k) * 16 + j];
        hipError_t e;
        if (d.albedo) e = d.history_in ? launch_group<true, false>(d, counts, samples_cap, stream) : launch_group<true, true>(d, counts, samples_cap, stream);
        else e = d.history_in ? launch_group<false, false>(d, counts, samples_cap, stream) : launch_group<false, true>(d, counts, samples_cap, stream);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

} // namespace mipt
