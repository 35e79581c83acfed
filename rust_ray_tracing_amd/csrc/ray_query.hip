// ray_query.hip -- batched ray queries on a resident scene: closest hit and occlusion for caller-supplied rays.
//
// The traversal is the trace kernel's (pt_kernel.hip), i.e. Ray::traverse_bvh (reference src/renderer/backend/cpu/ray.rs:84-139)
// step for step over the same [pairs | tri_pos] records, through the helpers of pt_traverse.h: same visit order, same strict-<
// closest hit, one rounded f32 operation per operator.  What differs is what surrounds it: a lane's work item is a RAY read from the
// caller's array instead of a pixel, hit_info.distance starts at the ray's t_max instead of 1e30, and a finished lane writes a
// MiptHit (or one occlusion byte) instead of shading.
//
// One persistent wave64 = 64 rays in flight, one per lane.  Finished lanes wait until a quarter of the wave's live lanes are idle
// (or none traverses), then write their results and take new rays from the global counter with one wave-aggregated atomic.
#include "pt_kernel.h"
#include "pt_device_math.h"
#include "pt_traverse.h"

namespace mipt {

namespace {

// refill when idle lanes / live lanes >= kRefillNum / kRefillDen: the refill pass is two 16-B loads, three divisions and one store
// per lane, far lighter than the trace kernel's service pass (3/8 there)
constexpr uint32_t kRefillNum = 1, kRefillDen = 4;

enum : uint32_t {
    QS_T = 0,   // traversing
    QS_D = 1,   // traversal finished: result to write, then a new ray
    QS_N = 2,   // needs a ray (nothing to write)
    QS_X = 3    // queue exhausted, lane retired
};

} // namespace

template <bool COUNT, bool CULL, bool ANYHIT>
__global__ __launch_bounds__(kBlockThreads) void ray_query_kernel(DevScene sc, DevQuery q) {
    __shared__ uint32_t s_stack[kWavesPerBlock][kStackLds + 1][64];   // row kStackLds: scratch target of the branch-free push

    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wib = threadIdx.x >> 6;
    uint32_t(*stk)[64] = s_stack[wib];
    uint32_t *ovf = q.ovf + ((size_t)blockIdx.x * kWavesPerBlock + wib) * (size_t)(kStackOvf * 64) + lane;

    const auto geom = __builtin_amdgcn_make_buffer_rsrc((void *)sc.pairs, 0, (int)sc.geom_bytes, 0x00020000);

    uint32_t state = QS_N;
    unsigned long long ray_i = 0;
    V3 o = mk(0, 0, 0), d = mk(0, 0, 1), rd = mk(0, 0, 1);
    bool dir_safe = false;
    float best_t = kMiss, best_u = 0, best_v = 0;
    uint32_t best_tri = kNoTri;
    uint32_t tri_cur = 0, tri_end = 0, pair = 0, sp = 0;
    unsigned long long c_rays = 0, c_inner = 0, c_tris = 0, c_hits = 0;
    uint32_t c_maxsp = 0;

    for (;;) {
        const unsigned long long m_t = __ballot(state == QS_T);
        const unsigned long long m_need = __ballot(state == QS_D || state == QS_N);
        const uint32_t n_t = (uint32_t)__popcll(m_t), n_need = (uint32_t)__popcll(m_need);
        if ((n_t | n_need) == 0u) break;

        // ---------------- refill: write results, fetch rays ------------------------------------------
        if (n_need != 0u && (n_t == 0u || n_need * kRefillDen >= (n_t + n_need) * kRefillNum)) {
            if (state == QS_D) {
                if (ANYHIT) {
                    reinterpret_cast<uint8_t *>(q.out)[ray_i] = best_tri != kNoTri ? (uint8_t)1 : (uint8_t)0;
                } else {
                    uint4 h;
                    if (best_tri != kNoTri) {
                        // the record carries its triangle's index in the tree's order; the caller's order goes through the
                        // permutation BVH::build applied (null: the caller passed the tree order)
                        const uint32_t t = best_tri & ~kFrontBit;
                        const uint32_t prim = q.tri_order ? q.tri_order[t] : t;
                        h = make_uint4(__float_as_uint(best_t), __float_as_uint(best_u), __float_as_uint(best_v), prim | (best_tri & kFrontBit));
                    } else {
                        h = make_uint4(__float_as_uint(kMiss), 0u, 0u, kNoTri);      // HitInfo::default, ray.rs:214-226
                    }
                    reinterpret_cast<uint4 *>(q.out)[ray_i] = h;
                }
                if (COUNT && best_tri != kNoTri) c_hits++;
                state = QS_N;
            }
            // one atomic per wave, compacted over the lanes that need a ray
            const unsigned long long m_n = __ballot(state == QS_N);
            unsigned long long base = 0;
            const uint32_t leader = (uint32_t)__ffsll((long long)m_n) - 1u;
            if (lane == leader) base = atomicAdd(&q.stats->queue, (unsigned long long)__popcll(m_n));
            base = __shfl(base, (int)leader);
            if (state == QS_N) {
                ray_i = base + lane_rank(m_n);
                if (ray_i >= q.n_rays) {
                    state = QS_X;
                } else {
                    const float4 r0 = q.rays[2ull * ray_i], r1 = q.rays[2ull * ray_i + 1ull];   // {origin, t_max}, {direction, reserved}
                    o = mk(r0.x, r0.y, r0.z); d = mk(r1.x, r1.y, r1.z);
                    // ---- start traverse_bvh (ray.rs:84-88) with hit_info.distance = t_max ----
                    best_t = r0.w; best_u = 0.0f; best_v = 0.0f; best_tri = kNoTri;
                    rd = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
                    dir_safe = ray_safe(o, d, sc.tiny_axes);
                    sp = 0; pair = 0u;
                    tri_cur = sc.root_a; tri_end = sc.root_a + sc.root_n;   // root leaf (root_n > 0) or inner (empty range)
                    if (COUNT) c_rays++;
                    state = QS_T;
                }
            }
            continue;   // re-evaluate the ballots
        }

        // ---------------- one traversal step per traversing lane ---------------------------------
        if (state == QS_T) {
            const bool leaf = tri_cur < tri_end;
            // one buffer descriptor over [pairs | tri_pos], 32-bit byte offset per lane (no 64-bit address math)
            const uint32_t voff = leaf ? (sc.tri_off_bytes + tri_cur * kTriPosStride) : (pair * 64u);
            // top of the stack, read now so that its LDS latency hides under the global loads: a step that pops never pushes
            const uint32_t top_e = stk[(sp - 1u) & (uint32_t)(kStackLds - 1)][lane];
            float4 r0, r1, r2, r3;
            r0 = ldg4(geom, voff); r1 = ldg4(geom, voff + 16u); r2 = ldg4(geom, voff + 32u);
            r3 = ldg4(geom, voff + 48u);                                 // tri_pos is padded by one float4
            // all four 16-B loads stay in front of the inner/leaf branch (pt_kernel.hip: LLVM otherwise sinks the last two)
            asm volatile("" ::: "memory");
            bool need_pop = false, finished = false;
            if (leaf) {                                                              // ray.rs:19-67, 90-99
                const V3 v0 = mk(r0.x, r0.y, r0.z), e1 = mk(r0.w, r1.x, r1.y), e2 = mk(r1.z, r1.w, r2.x);
                const V3 rce2 = cross(d, e2);
                const float det = dot(e1, rce2);
                const float inv_det = 1.0f / det;
                const V3 s = o - v0;
                const float u = inv_det * dot(s, rce2);
                const V3 sce1 = cross(s, e1);
                const float v = inv_det * dot(d, sce1);
                const float t = inv_det * dot(e2, sce1);
                // ray.rs:56-59 verbatim boolean form: NaN u/v pass, NaN t fails
                const bool has_hit = (t > 0.0f) && !(u < 0.0f || u > 1.0f) && !(v < 0.0f || u + v > 1.0f);
                if (COUNT) c_tris++;
                if (has_hit && t < best_t) {                                         // ray.rs:96 (strict <)
                    best_tri = __float_as_uint(r2.y) | ((det > 0.0f) ? kFrontBit : 0u);   // ray.rs:39
                    if (ANYHIT) {
                        finished = true;                                             // occluded: the bound stays at t_max, the ray ends here
                    } else {
                        best_t = t; best_u = u; best_v = v;
                    }
                }
                tri_cur += 1;
                need_pop = (tri_cur == tri_end);
            } else {                                                                 // ray.rs:108-137
                const float max_d = best_t * q.cull_scale;
                float d1, d2;
                slab_pair<CULL>(o, d, rd, dir_safe, r0, r1, r2, r3, max_d, d1, d2);
                uint32_t a1 = __float_as_uint(r0.w), n1 = __float_as_uint(r1.w);
                uint32_t a2 = __float_as_uint(r2.w), n2 = __float_as_uint(r3.w);
                uint32_t w2 = 1u;
                if (COUNT) c_inner++;
                if (d1 > d2) {                                                       // ray.rs:120-123
                    float td = d1; d1 = d2; d2 = td;
                    uint32_t ta = a1; a1 = a2; a2 = ta;
                    uint32_t tn = n1; n1 = n2; n2 = tn;
                    w2 = 0u;
                }
                if (d1 == kMiss) {                                                   // ray.rs:124-130
                    need_pop = true;
                } else {
                    const bool push = d2 < kMiss;                                    // ray.rs:133-136
                    const uint32_t e = encode_child(a2, n2, pair, w2);
                    const bool in_lds = sp < (uint32_t)kStackLds;
                    stk[(push && in_lds) ? sp : (uint32_t)kStackLds][lane] = e;      // no branch: non-pushing lanes hit the scratch row
                    if (push && !in_lds) {                                           // rare: spill region / overflow
                        if (sp < (uint32_t)(kStackLds + kStackOvf)) ovf[(size_t)(sp - kStackLds) * 64] = e;
                        else atomicAdd(&q.stats->stack_overflows, 1ull);              // reference: panic (ray.rs:85)
                    }
                    sp += (push && sp < (uint32_t)(kStackLds + kStackOvf)) ? 1u : 0u;
                    if (COUNT) c_maxsp = sp > c_maxsp ? sp : c_maxsp;
                    if (n1 > 0u) { tri_cur = a1; tri_end = a1 + n1; }                // ray.rs:131 node = child_1
                    else { pair = a1; }
                }
            }
            if (finished) {
                state = QS_D;
            } else if (need_pop) {                                                   // ray.rs:100-105, 125-129
                if (sp == 0u) {
                    state = QS_D;
                } else {
                    sp -= 1;
                    uint32_t e = top_e;
                    if (sp >= (uint32_t)kStackLds) e = ovf[(size_t)(sp - kStackLds) * 64];  // rare
                    if (e & 0x80000000u) {
                        uint32_t n = (e >> 25) & 63u, a = e & 0x01ffffffu;
                        if (n == 0u) {                                               // big leaf: child-ref form
                            const uint32_t ref = e & 0x7fffffffu;
                            const float4 *p = sc.pairs + (size_t)(ref >> 1) * 4 + (ref & 1u) * 2;
                            a = __float_as_uint(p[0].w); n = __float_as_uint(p[1].w);
                        }
                        tri_cur = a; tri_end = a + n;
                    } else {
                        pair = e; tri_cur = 0; tri_end = 0;
                    }
                }
            }
        }
    }

    if (COUNT) {
        atomicAdd(&q.stats->rays, c_rays);
        atomicAdd(&q.stats->inner_steps, c_inner);
        atomicAdd(&q.stats->tri_tests, c_tris);
        atomicAdd(&q.stats->hits, c_hits);
        atomicMax(&q.stats->max_stack, (unsigned long long)c_maxsp);
    }
}

template <bool COUNT, bool CULL, bool ANYHIT>
static hipError_t launch_q(const DevScene &sc, const DevQuery &q, int grid, hipStream_t stream) {
    hipLaunchKernelGGL((ray_query_kernel<COUNT, CULL, ANYHIT>), dim3(grid), dim3(kBlockThreads), 0, stream, sc, q);
    return hipGetLastError();
}
template <bool COUNT, bool CULL, bool ANYHIT>
static int occ_q() {
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, ray_query_kernel<COUNT, CULL, ANYHIT>, kBlockThreads, 0) != hipSuccess) n = 1;
    return n;
}
// instantiations: {count} x {cull} x {closest, any hit}
#define MIPT_QUERY_DISPATCH(FN, ...)                                                                                    \
    do {                                                                                                                \
        if (anyhit) {                                                                                                   \
            if (count) return cull ? FN<true, true, true>(__VA_ARGS__) : FN<true, false, true>(__VA_ARGS__);            \
            return cull ? FN<false, true, true>(__VA_ARGS__) : FN<false, false, true>(__VA_ARGS__);                     \
        }                                                                                                               \
        if (count) return cull ? FN<true, true, false>(__VA_ARGS__) : FN<true, false, false>(__VA_ARGS__);              \
        return cull ? FN<false, true, false>(__VA_ARGS__) : FN<false, false, false>(__VA_ARGS__);                       \
    } while (0)

hipError_t launch_ray_query(const DevScene &sc, const DevQuery &q, bool count, bool cull, bool anyhit, int grid, hipStream_t stream) {
    MIPT_QUERY_DISPATCH(launch_q, sc, q, grid, stream);
}
static int occ_query_dispatch(bool count, bool cull, bool anyhit) { MIPT_QUERY_DISPATCH(occ_q); }
int query_blocks_per_cu(bool count, bool cull, bool anyhit) {
    int n = occ_query_dispatch(count, cull, anyhit);
    if (n < 1) n = 1;
    if (n > 8) n = 8;
    return n;
}

} // namespace mipt
