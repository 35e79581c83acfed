// upsample.hip -- the joint-bilateral upsampling of include/mipt.h ("guided upsampling"): mipt_upsample*.  The step that closes the
// pipeline of first_hit.hip, temporal.hip and denoise_variance.hip: a frame traced and filtered at W/k x H/k comes back at W x H, its
// edges and textures taken from the full-resolution guides.
//
// A pack pass over the low frame, then one pass over the full frame (image_kernels.h: the tile walk, the pack, the guide terms).  The
// low frame's planar inputs are packed into one float4 of colour {c.r, c.g, c.b, bits(material)} and one of guides {n.x, n.y, n.z, z}
// per low pixel, so that a tap costs at most two 16-byte loads.  Which guides exist is a template argument; the scale is a kernel
// argument, uniform over the launch.  The 64 lanes of a tile row share 64/k + 1 low texels per low row; that reuse is left to the
// vector L1 and L2.
//
// A tap that does not take part (outside the low frame, or with a bilinear weight of 0) is predicated off: it is not loaded.  A tap
// whose material differs has loaded its colour -- the plain bilinear sums need it -- but not its guides.
#include "image_kernels.h"

namespace mipt {

namespace {

template <bool NORMAL, bool DEPTH, bool ALBEDO, bool MATERIAL>
__global__ __launch_bounds__(kBlockThreads) void upsample_pack_kernel(DevUpsample d, unsigned long long n_tiles) {
    for (unsigned long long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        uint32_t x, y, view;
        if (!lane_pixel(d.lo_width, d.lo_height, d.lo_tiles_x, d.lo_tiles_y, t, x, y, view)) continue;
        const size_t i = (size_t)view * d.lo_width * d.lo_height + ((size_t)y * d.lo_width + x);
        pack_pixel<NORMAL, DEPTH, ALBEDO>(d.lo_hdr, d.lo_albedo, d.lo_normal, d.lo_depth, i, MATERIAL ? __uint_as_float(d.lo_material[i]) : 0.0f,
                                          d.colour, d.guides);
    }
}

template <bool NORMAL, bool DEPTH, bool ALBEDO, bool MATERIAL>
__global__ __launch_bounds__(kBlockThreads) void upsample_kernel(DevUpsample d, unsigned long long n_tiles) {
    const float4 *__restrict__ colour = d.colour;
    const float4 *__restrict__ guides = d.guides;
    const uint32_t k = d.scale, lw = d.lo_width, lh = d.lo_height;
    const float fk = (float)k;
    for (unsigned long long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        uint32_t X, Y, view;
        if (!lane_pixel(d.width, d.height, d.tiles_x, d.tiles_y, t, X, Y, view)) continue;
        const size_t i = (size_t)view * d.width * d.height + ((size_t)Y * d.width + X);
        const size_t lo_base = (size_t)view * lw * lh;
        const uint32_t x0 = X / k, y0 = Y / k;               // < lw, < lh: width = k * lw, height = k * lh
        const uint32_t rx = X - x0 * k, ry = Y - y0 * k;
        const float wx = (float)rx / fk, ux = 1.0f - wx;
        const float wy = (float)ry / fk, uy = 1.0f - wy;
        float4 gp = make_float4(0.0f, 0.0f, 0.0f, 0.0f);     // the pixel's own guides, as the pack pass lays out a low pixel's
        uint32_t mp = 0;
        if (NORMAL) { const float *n = d.normal + i * 3; gp.x = n[0]; gp.y = n[1]; gp.z = n[2]; }
        if (DEPTH) gp.w = d.depth[i];
        if (MATERIAL) mp = d.material[i];
        float br = 0.0f, bg = 0.0f, bb = 0.0f, bsum = 0.0f;  // the plain bilinear sums
        float sr = 0.0f, sg = 0.0f, sb = 0.0f, wsum = 0.0f;  // the guided sums
#pragma unroll
        for (uint32_t ty = 0; ty < 2; ty++) {
            // skipped: outside the low frame, or a bilinear weight of 0
            if (ty && (ry == 0 || y0 + 1u >= lh)) continue;
#pragma unroll
            for (uint32_t tx = 0; tx < 2; tx++) {
                if (tx && (rx == 0 || x0 + 1u >= lw)) continue;
                const float b = (tx ? wx : ux) * (ty ? wy : uy);
                const size_t q = lo_base + ((size_t)(y0 + ty) * lw + (x0 + tx));
                const float4 cq = colour[q];
                br = br + (b * cq.x); bg = bg + (b * cq.y); bb = bb + (b * cq.z);
                bsum = bsum + b;
                if (MATERIAL && __float_as_uint(cq.w) != mp) continue;
                float w = b;                                  // neither normal nor depth: b without evaluation
                if (NORMAL || DEPTH) w = tap_weight(b, guide_energy<NORMAL, DEPTH>(gp, guides[q], d.kn, d.kz));
                sr = sr + (w * cq.x); sg = sg + (w * cq.y); sb = sb + (w * cq.z);
                wsum = wsum + w;
            }
        }
        // bsum > 0: tap (x0, y0) is never skipped
        float r, g, b;
        if (wsum > 0.0f) { r = sr / wsum; g = sg / wsum; b = sb / wsum; }
        else { r = br / bsum; g = bg / bsum; b = bb / bsum; }
        if (ALBEDO) {
            const float *a = d.albedo + i * 3;
            r = r * floored(a[0]); g = g * floored(a[1]); b = b * floored(a[2]);
        }
        float *o = d.out + i * 3;
        o[0] = r; o[1] = g; o[2] = b;
        if (d.weight) d.weight[i] = wsum;                     // the same for every lane of the launch
    }
}

template <bool NORMAL, bool DEPTH, bool ALBEDO, bool MATERIAL>
hipError_t launch_both(const DevUpsample &d, hipStream_t stream) {
    const unsigned long long lo_tiles = tile_count(d.lo_tiles_x, d.lo_tiles_y, d.n_views), n_tiles = tile_count(d.tiles_x, d.tiles_y, d.n_views);
    const uint32_t lo_grid = tile_grid(lo_tiles, kFrameMaxGrid), grid = tile_grid(n_tiles, kFrameMaxGrid);
    hipError_t e;
    hipLaunchKernelGGL((upsample_pack_kernel<NORMAL, DEPTH, ALBEDO, MATERIAL>), dim3(lo_grid), dim3(kBlockThreads), 0, stream, d, lo_tiles);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL((upsample_kernel<NORMAL, DEPTH, ALBEDO, MATERIAL>), dim3(grid), dim3(kBlockThreads), 0, stream, d, n_tiles);
    return hipGetLastError();
}

template <bool NORMAL, bool DEPTH>
hipError_t launch_guides(const DevUpsample &d, hipStream_t stream) {
    if (d.albedo) return d.material ? launch_both<NORMAL, DEPTH, true, true>(d, stream) : launch_both<NORMAL, DEPTH, true, false>(d, stream);
    return d.material ? launch_both<NORMAL, DEPTH, false, true>(d, stream) : launch_both<NORMAL, DEPTH, false, false>(d, stream);
}

} // namespace

// instantiations: {normal} x {depth} x {albedo} x {material} x {pack, upsample}
hipError_t launch_upsample(const DevUpsample &d, hipStream_t stream) {
    if (d.normal) return d.depth ? launch_guides<true, true>(d, stream) : launch_guides<true, false>(d, stream);
    return d.depth ? launch_guides<false, true>(d, stream) : launch_guides<false, false>(d, stream);
}

} // namespace mipt
