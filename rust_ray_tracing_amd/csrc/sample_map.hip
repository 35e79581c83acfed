// sample_map.hip -- the sample map of include/mipt.h ("adaptive sampling"): mipt_sample_map*.  The variance plane the temporal and
// variance passes leave in HBM becomes a per-pixel sample count for mipt_render_adaptive*, under a budget on the frame's mean.
//
// mipt_sample_map: two launches.  sample_map_reduce_kernel forms every pixel's weight qi, an integer, and adds them up: per lane in 64 bits, per wave
// by shuffles, per block through LDS, one atomic per block.  An integer sum is exact in any order, so the result is the model's S
// whatever the grid.  The last block to finish (a ticket in the workspace) forms the ratio r = E / S once, in binary64, and leaves
// it beside S.  sample_map_assign_kernel forms qi again -- the same function on the same operands, the same bits; 16 or 28 B read per
// pixel are cheaper than a plane of weights written and read back -- and writes the count.
//
// Every f32 operator below is one rounded operation in the order the header gives (the translation unit is built with
// -ffp-contract=off and correctly rounded f32 divide and sqrt); the binary64 divide is the compiler's IEEE expansion (v_div_scale,
// v_rcp, the Newton steps in FMAs, v_div_fmas, v_div_fixup), which is correctly rounded.
//
// mipt_sample_map_fill: the same reduction, then one launch per round (sample_map_fill_kernel below): rounds + 1 launches, since each
// round's pass also forms the two sums of the round after it.
#include "image_kernels.h"                                  // floored, luminance

#include <cstddef>

namespace mipt {

namespace {

constexpr uint32_t kMapThreads = 256, kMapWaves = kMapThreads / 64;
constexpr uint32_t kMapMaxGrid = 2048;                       // blocks per launch; a block walks the pixels with this stride

// qi of pixel i.  MODE 0: variance alone; 1: relative to hdr's luminance; 2: to the luminance of hdr / albedo.
template <int MODE>
__device__ __forceinline__ uint32_t pixel_weight(const DevSampleMap &d, unsigned long long i) {
    const float var = d.variance[i];
    const float v = var > 0.0f ? var : 0.0f;
    const float s = sqrtf(v);
    float w = s;
    if (MODE != 0) {
        const float *h = d.hdr + i * 3;
        float r = h[0], g = h[1], b = h[2];
        if (MODE == 2) {
            const float *a = d.albedo + i * 3;
            r = r / floored(a[0]); g = g / floored(a[1]); b = b / floored(a[2]);
        }
        float l = luminance(r, g, b);
        l = l > 0.0f ? l : 0.0f;
        w = s / (l + 0.00390625f);
    }
    const float q = w * 4096.0f;
    return q > 0.0f ? (q < 16777215.0f ? (uint32_t)q : 16777215u) : 0u;
}

template <int MODE>
__global__ __launch_bounds__(kMapThreads) void sample_map_reduce_kernel(DevSampleMap d) {
    __shared__ unsigned long long s_part[kMapWaves];
    unsigned long long acc = 0ull;
    for (unsigned long long i = (unsigned long long)blockIdx.x * kMapThreads + threadIdx.x; i < d.n_pixels;
         i += (unsigned long long)gridDim.x * kMapThreads)
        acc += (unsigned long long)pixel_weight<MODE>(d, i);
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o);
    if ((threadIdx.x & 63u) == 0u) s_part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0u) {
        unsigned long long block = 0ull;
        for (uint32_t w = 0; w < kMapWaves; w++) block += s_part[w];
        if (block) atomicAdd(&d.work->sum, block);
        __threadfence();                                      // the sum before the ticket
        if (atomicAdd(&d.work->done, 1u) == gridDim.x - 1u) {
            const unsigned long long sum = atomicAdd(&d.work->sum, 0ull);
            d.work->ratio = sum ? (double)d.extra / (double)sum : 0.0;
        }
    }
}

template <int MODE>
__global__ __launch_bounds__(kMapThreads) void sample_map_assign_kernel(DevSampleMap d) {
    const unsigned long long sum = d.work->sum;
    const double r = d.work->ratio;
    for (unsigned long long i = (unsigned long long)blockIdx.x * kMapThreads + threadIdx.x; i < d.n_pixels;
         i += (unsigned long long)gridDim.x * kMapThreads) {
        uint32_t e = d.uniform_extra;                         // S == 0: nothing to tell the pixels apart
        if (sum != 0ull) {
            const double x = (double)pixel_weight<MODE>(d, i) * r;
            e = x < (double)d.span ? (uint32_t)x : d.span;
        }
        d.counts[i] = d.min_samples + e;
    }
}

template <int MODE>
hipError_t launch_mode(const DevSampleMap &d, uint32_t grid, hipStream_t stream) {
    hipLaunchKernelGGL(sample_map_reduce_kernel<MODE>, dim3(grid), dim3(kMapThreads), 0, stream, d);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(sample_map_assign_kernel<MODE>, dim3(grid), dim3(kMapThreads), 0, stream, d);
    return hipGetLastError();
}

// ---- mipt_sample_map_fill*: what the clamp cuts off goes to the pixels that can still take it ----
// Round k's pass.  `cur` is slot k - 1: S_k and r_k (round 1: the reduction's S and r; later rounds: `active`, left by the pass before).
// The running e lives in counts: every pixel is read and written by the one lane that owns it, so a pass needs no order among its
// lanes.  Unless LAST, the pass also adds up what round k + 1 needs -- A over all pixels, S over those below the span -- into `next`
// (slot k), and its last block forms r_{k+1}: integer sums, exact in any order, and one binary64 divide.  The LAST pass adds
// min_samples.
template <int MODE, bool FIRST_ROUND, bool LAST>
__global__ __launch_bounds__(kMapThreads) void sample_map_fill_kernel(DevSampleMap d, const SampleMapFillWork *cur, SampleMapFillWork *next) {
    __shared__ unsigned long long s_sum[kMapWaves], s_assigned[kMapWaves];
    const unsigned long long sum = cur->sum;
    const double r = cur->ratio;
    const bool active = FIRST_ROUND ? true : cur->active != 0u;
    unsigned long long acc_s = 0ull, acc_a = 0ull;
    for (unsigned long long i = (unsigned long long)blockIdx.x * kMapThreads + threadIdx.x; i < d.n_pixels;
         i += (unsigned long long)gridDim.x * kMapThreads) {
        uint32_t qi = 0u, e;
        if (FIRST_ROUND) {
            e = d.uniform_extra;                              // S == 0: nothing to tell the pixels apart
            if (!LAST || sum != 0ull) qi = pixel_weight<MODE>(d, i);
            if (sum != 0ull) {
                const double x = (double)qi * r;
                e = x < (double)d.span ? (uint32_t)x : d.span;
            }
        } else {
            e = d.counts[i];
            if (e < d.span && (active || !LAST)) {
                qi = pixel_weight<MODE>(d, i);
                if (active) {
                    const double x = (double)qi * r;
                    const uint32_t room = d.span - e;
                    const uint32_t add = x < (double)room ? (uint32_t)x : room;
                    e = e + add;
                }
            }
        }
        d.counts[i] = LAST ? d.min_samples + e : e;
        if (!LAST) {
            acc_a += (unsigned long long)e;
            if (e < d.span) acc_s += (unsigned long long)qi;
        }
    }
    if (LAST) return;
    for (int o = 32; o > 0; o >>= 1) { acc_s += __shfl_down(acc_s, o); acc_a += __shfl_down(acc_a, o); }
    if ((threadIdx.x & 63u) == 0u) { s_sum[threadIdx.x >> 6] = acc_s; s_assigned[threadIdx.x >> 6] = acc_a; }
    __syncthreads();
    if (threadIdx.x == 0u) {
        unsigned long long bs = 0ull, ba = 0ull;
        for (uint32_t w = 0; w < kMapWaves; w++) { bs += s_sum[w]; ba += s_assigned[w]; }
        if (bs) atomicAdd(&next->sum, bs);
        if (ba) atomicAdd(&next->assigned, ba);
        __threadfence();                                      // the sums before the ticket
        if (atomicAdd(&next->done, 1u) == gridDim.x - 1u) {
            const unsigned long long s_next = atomicAdd(&next->sum, 0ull), a = atomicAdd(&next->assigned, 0ull);
            const unsigned long long left = a < d.extra ? d.extra - a : 0ull;
            const bool on = s_next != 0ull && left != 0ull;
            next->ratio = on ? (double)left / (double)s_next : 0.0;
            next->active = on ? 1u : 0u;
        }
    }
}

template <int MODE, bool FIRST_ROUND>
void launch_fill_round(const DevSampleMap &d, const SampleMapFillWork *cur, SampleMapFillWork *next, bool last, uint32_t grid, hipStream_t stream) {
    if (last) hipLaunchKernelGGL((sample_map_fill_kernel<MODE, FIRST_ROUND, true>), dim3(grid), dim3(kMapThreads), 0, stream, d, cur, next);
    else hipLaunchKernelGGL((sample_map_fill_kernel<MODE, FIRST_ROUND, false>), dim3(grid), dim3(kMapThreads), 0, stream, d, cur, next);
}

template <int MODE>
hipError_t launch_fill_mode(DevSampleMap d, SampleMapFillWork *slots, uint32_t rounds, uint32_t grid, hipStream_t stream) {
    d.work = (SampleMapWork *)slots;                          // slot 0 begins like SampleMapWork: round 1's S and r are the plain map's
    hipLaunchKernelGGL(sample_map_reduce_kernel<MODE>, dim3(grid), dim3(kMapThreads), 0, stream, d);
    hipError_t e = hipGetLastError();
    for (uint32_t k = 1; k <= rounds && e == hipSuccess; k++) {
        SampleMapFillWork *next = k == rounds ? nullptr : slots + k;   // the last pass adds nothing up
        if (k == 1) launch_fill_round<MODE, true>(d, slots, next, k == rounds, grid, stream);
        else launch_fill_round<MODE, false>(d, slots + (k - 1), next, k == rounds, grid, stream);
        e = hipGetLastError();
    }
    return e;
}

static_assert(sizeof(SampleMapFillWork) == 32 && offsetof(SampleMapFillWork, sum) == offsetof(SampleMapWork, sum) &&
                  offsetof(SampleMapFillWork, ratio) == offsetof(SampleMapWork, ratio) && offsetof(SampleMapFillWork, done) == offsetof(SampleMapWork, done),
              "slot 0 is written by sample_map_reduce_kernel");

} // namespace

hipError_t launch_sample_map_fill(const DevSampleMap &d, SampleMapFillWork *slots, uint32_t rounds, hipStream_t stream) {
    const unsigned long long blocks = (d.n_pixels + kMapThreads - 1u) / kMapThreads;
    const uint32_t grid = (uint32_t)(blocks < kMapMaxGrid ? blocks : kMapMaxGrid);
    hipError_t e = hipMemsetAsync(slots, 0, sizeof(SampleMapFillWork) * rounds, stream);
    if (e != hipSuccess) return e;
    if (d.hdr && d.albedo) return launch_fill_mode<2>(d, slots, rounds, grid, stream);
    if (d.hdr) return launch_fill_mode<1>(d, slots, rounds, grid, stream);
    return launch_fill_mode<0>(d, slots, rounds, grid, stream);
}

hipError_t launch_sample_map(const DevSampleMap &d, hipStream_t stream) {
    const unsigned long long blocks = (d.n_pixels + kMapThreads - 1u) / kMapThreads;
    const uint32_t grid = (uint32_t)(blocks < kMapMaxGrid ? blocks : kMapMaxGrid);
    hipError_t e = hipMemsetAsync(d.work, 0, sizeof(SampleMapWork), stream);
    if (e != hipSuccess) return e;
    if (d.hdr && d.albedo) return launch_mode<2>(d, grid, stream);
    if (d.hdr) return launch_mode<1>(d, grid, stream);
    return launch_mode<0>(d, grid, stream);
}

} // namespace mipt
