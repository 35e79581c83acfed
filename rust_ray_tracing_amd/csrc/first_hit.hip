// first_hit.hip -- first-hit feature buffers: what the camera ray of every pixel hits and what the surface looks like there
// (depth, primitive and material ids, position, uv, interpolated normal, albedo, emission) -- mipt_render_features*.
//
// The camera ray of (view, pixel, sample) is the trace kernel's (pt_kernel.hip: cpu.rs:28-50, reseeded per sample by
// rt_compute.wgsl:102 in MIPT_SEED_PER_SAMPLE mode), the traversal is Ray::traverse_bvh (reference src/renderer/backend/cpu/ray.rs:84-139)
// through the helpers of pt_traverse.h exactly as ray_query.hip runs it, and the values of a hit are the fields intersect_tri
// (ray.rs:45-60) and the first iteration of trace (ray.rs:153-176) compute for the winner.  Nothing scatters: a lane's sample ends at
// its first hit.
//
// One persistent wave64 = 64 pixels in flight, one per lane.  The work index runs over (view, 8x8 tile, pixel) as in
// pt_trace_batch_kernel, so a wave's primary rays are neighbours.  Finished lanes wait until a quarter of the wave's live lanes are
// idle (or none traverses), then read their hit's attributes, store or add them into their pixel's output slots and either start their
// pixel's next sample or take a new pixel from the global counter with one wave-aggregated atomic.
//
// The motion pass (mipt_render_motion*, include/mipt.h "previous positions") is the same kernel with MOTION != 0: the first sample's
// traversal, and in the finished-lane step, instead of the attributes, the hit triangle's three corners in the PREVIOUS geometry --
// from the caller's triangle array (kMotionExplicit) or from the scene's previous mesh generation through the expansion rule
// (kMotionTracked) -- interpolated with the hit's barycentrics.
#include "pt_kernel.h"
#include "pt_device_math.h"
#include "pt_texel.h"
#include "pt_traverse.h"
#include "pt_mesh_rule.h"

namespace mipt {

namespace {

// refill when idle lanes / live lanes >= kRefillNum / kRefillDen (ray_query.hip's rule and ratio)
#ifndef MIPT_FIRST_HIT_REFILL_NUM
#define MIPT_FIRST_HIT_REFILL_NUM 1
#define MIPT_FIRST_HIT_REFILL_DEN 4
#endif
constexpr uint32_t kRefillNum = MIPT_FIRST_HIT_REFILL_NUM, kRefillDen = MIPT_FIRST_HIT_REFILL_DEN;

enum : uint32_t {
    FS_T = 0,   // traversing
    FS_D = 1,   // traversal finished: attributes to read, then the next sample or the pixel's stores
    FS_N = 2,   // needs a pixel
    FS_X = 3    // queue exhausted, lane retired
};

// One step of a pixel's mean, formed as final_color is (cpu.rs:30,52,60): the sum starts at +0, takes the samples in order and is
// divided by the sample count once, after the last -- also when that is the only one.  The running sum lives in the pixel's output
// slot, which is its lane's alone until the pixel is done, and not in nine registers per lane, which would cost occupancy.
__device__ __forceinline__ void accumulate(float *p, V3 v, bool first, bool last, float samples_f) {
    V3 acc = mk(0.0f, 0.0f, 0.0f);
    if (!first) acc = mk(p[0], p[1], p[2]);
    acc = acc + v;
    if (last) acc = acc / samples_f;
    p[0] = acc.x; p[1] = acc.y; p[2] = acc.z;
}

} // namespace

// waves per SIMD the register allocation is held to: the query kernel's 8 (64 VGPRs: 63 used, no scratch); the counting twin carries five
// 64-bit counters per lane and keeps its natural 5 (at 8 it would spill 16 VGPRs to scratch)
#ifndef MIPT_FIRST_HIT_WAVES
#define MIPT_FIRST_HIT_WAVES 8
#endif
// the tracked motion pass (MOTION == 2) holds a part's matrix next to three corners: 7 waves (72 VGPRs) keep it out of scratch, which 8 do not
#define MIPT_FIRST_HIT_BOUNDS(COUNT, MOTION) __launch_bounds__(kBlockThreads, COUNT ? 5 : (MOTION == 2 ? 7 : MIPT_FIRST_HIT_WAVES))

enum : int { kMotionNone = 0, kMotionExplicit = 1, kMotionTracked = 2 };

// corner c of triangle T (the caller's order) in the previous geometry.  Explicit: a 12-byte run of the fat triangle array, 112 T +
// 32 c.  Tracked: the expansion rule (pt_mesh_rule.h) on the previous position array with the previous matrix of T's part, `part`.
template <int MOTION>
__device__ __forceinline__ V3 prev_corner(const DevFeatures &f, uint32_t T, uint32_t c, uint32_t part) {
    float p[3] = {0.0f, 0.0f, 0.0f};
    if constexpr (MOTION == kMotionExplicit) {
        const float *q = f.prev_tris + ((size_t)T * 28u + c * 8u);
        p[0] = q[0]; p[1] = q[1]; p[2] = q[2];
    } else {
        const uint32_t ip = f.prev_idx[(size_t)T * 3u + c];
        if (ip < f.prev_n_pos) {                                          // as expand_corner: an index out of range leaves zero
            const float *q = f.prev_pos + (size_t)ip * 3u;
            p[0] = q[0]; p[1] = q[1]; p[2] = q[2];
        }
        const PartRec &r = f.prev_rec[part];
        if (r.has_xf) xf_position(r, p);
    }
    return mk(p[0], p[1], p[2]);
}

template <bool COUNT, bool CULL, int MOTION = kMotionNone>
__global__ MIPT_FIRST_HIT_BOUNDS(COUNT, MOTION) void first_hit_kernel(DevScene sc, DevFeatures f) {
    __shared__ uint32_t s_stack[kWavesPerBlock][kStackLds + 1][64];   // row kStackLds: scratch target of the branch-free push

    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wib = threadIdx.x >> 6;
    uint32_t(*stk)[64] = s_stack[wib];
    uint32_t *ovf = f.ovf + ((size_t)blockIdx.x * kWavesPerBlock + wib) * (size_t)(kStackOvf * 64) + lane;

    const auto geom = __builtin_amdgcn_make_buffer_rsrc((void *)sc.pairs, 0, (int)sc.geom_bytes, 0x00020000);

    // wave-uniform: a finished lane reads its hit's tri_attr record for any of these
    const bool want_attr = f.material || f.uv || f.normal || f.albedo || f.emission;

    uint32_t state = FS_N;
    uint32_t px = 0, py = 0, view = 0, sample = 0;
    V3 o = mk(0, 0, 0), d = mk(0, 0, 1), rd = mk(0, 0, 1);
    bool dir_safe = false;
    float best_t = kMiss, best_u = 0, best_v = 0;
    uint32_t best_tri = kNoTri;
    uint32_t tri_cur = 0, tri_end = 0, pair = 0, sp = 0;
    unsigned long long c_rays = 0, c_inner = 0, c_tris = 0, c_hits = 0, c_tex = 0;
    uint32_t c_maxsp = 0;
    uint32_t w_pixels = 0;                                                // wave-uniform: pixels this wave has written

    for (;;) {
        const unsigned long long m_t = __ballot(state == FS_T);
        const unsigned long long m_need = __ballot(state == FS_D || state == FS_N);
        const uint32_t n_t = (uint32_t)__popcll(m_t), n_need = (uint32_t)__popcll(m_need);
        if ((n_t | n_need) == 0u) break;

        // ---------------- refill: finish samples, write pixels, fetch pixels, camera rays ------------
        if (n_need != 0u && (n_t == 0u || n_need * kRefillDen >= (n_t + n_need) * kRefillNum)) {
            bool gen = false, wrote = false;                              // this lane starts a camera ray / has written its pixel in this pass
            if constexpr (MOTION != kMotionNone) {
                if (state == FS_D) {                                      // one sample per pixel: the lane's pixel is done here
                    const size_t slot = (size_t)view * f.view_pixels + ((size_t)py * f.width + px);
                    V3 prev = mk(0.0f, 0.0f, 0.0f);                       // a miss, as `position`
                    if (best_tri != kNoTri) {
                        const uint32_t tri = best_tri & ~kFrontBit;
                        const uint32_t T = f.tri_order ? f.tri_order[tri] : tri;             // the `prim` store's mapping
                        uint32_t part = 0u;
                        if constexpr (MOTION == kMotionTracked) part = part_of(f.prev_rec, f.prev_n_parts, T);
                        const float u = best_u, v = best_v;
                        const float w = (1.0f - u) - v;
                        prev = prev_corner<MOTION>(f, T, 0u, part) * w;
                        prev = prev + prev_corner<MOTION>(f, T, 1u, part) * u;
                        prev = prev + prev_corner<MOTION>(f, T, 2u, part) * v;
                    }
                    float *p = f.prev_position + slot * 3; p[0] = prev.x; p[1] = prev.y; p[2] = prev.z;
                    wrote = true; state = FS_N;
                }
            } else
            if (state == FS_D) {
                const bool hit = best_tri != kNoTri;
                const size_t slot = (size_t)view * f.view_pixels + ((size_t)py * f.width + px);
                const bool first = sample == 0u;                       // the first sample of the call: depth, ids, position, uv
                sample += 1;
                const bool last = !(sample < f.samples);
                // A miss leaves HitInfo::default (ray.rs:214-226) and takes the sky's colour and strength (ray.rs:184-193).  Each value
                // is stored as soon as it is known, so that few of them are live at once.
                if (first) {
                    if (f.depth) f.depth[slot] = best_t;
                    if (f.prim) {
                        const uint32_t tri = best_tri & ~kFrontBit;
                        f.prim[slot] = hit ? ((f.tri_order ? f.tri_order[tri] : tri) | (best_tri & kFrontBit)) : kNoTri;
                    }
                    if (f.position) {
                        const V3 point = hit ? o + d * best_t : mk(0.0f, 0.0f, 0.0f);          // ray.rs:60
                        float *p = f.position + slot * 3; p[0] = point.x; p[1] = point.y; p[2] = point.z;
                    }
                }
                uint32_t material = 0xffffffffu;
                float uvx = 0.0f, uvy = 0.0f;
                if (want_attr) {
                    V3 normal = mk(0.0f, 0.0f, 0.0f);
                    if (hit) {
                        const float4 *at = sc.tri_attr + (size_t)(best_tri & ~kFrontBit) * 4;
                        const float4 a0 = at[0], a1 = at[1], a2 = at[2], a3 = at[3];
                        const float u = best_u, v = best_v;
                        const float w = 1.0f - u - v;                                        // ray.rs:45
                        normal = mk(a0.x, a0.y, a0.z) * w + mk(a0.w, a1.x, a1.y) * u + mk(a1.z, a1.w, a2.x) * v;
                        if (!(best_tri & kFrontBit)) normal = mk(-normal.x, -normal.y, -normal.z);   // ray.rs:46-48
                        uvx = ((a2.y * w) + (a2.w * u)) + (a3.y * v);                        // ray.rs:50-53
                        uvy = ((a2.z * w) + (a3.x * u)) + (a3.z * v);
                        material = __float_as_uint(a3.w);
                    }
                    // the means are formed as final_color is (cpu.rs:30,52,60): see accumulate
                    if (f.normal) accumulate(f.normal + slot * 3, normal, first, last, f.samples_f);
                    if (first) {
                        if (f.material) f.material[slot] = material;
                        if (f.uv) { float *p = f.uv + slot * 2; p[0] = uvx; p[1] = uvy; }
                    }
                }
                if (f.albedo) {                                                              // ray.rs:162-169
                    V3 albedo = mk(1.0f, 1.0f, 1.0f);
                    if (hit) {
                        const DevMaterial *m = sc.mats + material;                           // ray.rs:153-154
                        const uint32_t tw = m->base_w;
                        if (tw != 0u) {
                            albedo = texel_rgb(sc, m->base_off, tw, m->base_h, uvx, uvy, f.stats);
                            if (COUNT) c_tex++;
                        } else {
                            albedo = mk(m->base[0], m->base[1], m->base[2]);
                        }
                    }
                    accumulate(f.albedo + slot * 3, albedo, first, last, f.samples_f);
                }
                if (f.emission) {                                                            // ray.rs:170-176
                    V3 emission = mk(1.0f, 1.0f, 1.0f);
                    if (hit) {
                        const DevMaterial *m = sc.mats + material;
                        const uint32_t tw = m->emis_w;
                        if (tw != 0u) {
                            emission = texel_rgb(sc, m->emis_off, tw, m->emis_h, uvx, uvy, f.stats);
                            if (COUNT) c_tex++;
                        } else {
                            emission = mk(m->emis[0], m->emis[1], m->emis[2]);
                        }
                    }
                    accumulate(f.emission + slot * 3, emission, first, last, f.samples_f);
                }
                if (COUNT && hit) c_hits++;
                if (last) { wrote = true; state = FS_N; }
                else gen = true;
            }
            w_pixels += (uint32_t)__popcll(__ballot(wrote));
            // ---- fetch a pixel: one atomic per wave, compacted over the lanes that need one ----
            const unsigned long long m_n = __ballot(state == FS_N);
            if (m_n != 0ull) {
                unsigned long long base = 0;
                const uint32_t leader = (uint32_t)__ffsll((long long)m_n) - 1u;
                if (lane == leader) base = atomicAdd(&f.stats->queue, (unsigned long long)__popcll(m_n));
                base = __shfl(base, (int)leader);
                if (state == FS_N) {
                    const unsigned long long wi = base + lane_rank(m_n);
                    if (wi >= f.total_work) {
                        state = FS_X;
                    } else {
                        // work index -> view, 8x8 tile within the view, pixel within the tile (pt_trace_batch_kernel's decode)
                        uint32_t lt = (uint32_t)(wi >> 6);
                        const uint32_t p = (uint32_t)wi & 63u;
                        const uint32_t n = f.n_tiles;
                        uint32_t q = __umulhi(lt, f.tiles_recip), r = lt - q * n;
                        if (r >= n) { q += 1u; r -= n; }
                        if (r >= n) { q += 1u; r -= n; }
                        const uint32_t x = (r % f.tiles_x) * 8u + (p & 7u);
                        const uint32_t y = (r / f.tiles_x) * 8u + (p >> 3);
                        if (x < f.width && y < f.height) {                // ragged edge tiles: skip, stay FS_N
                            view = q; px = x; py = y;
                            sample = 0;
                            gen = true;
                        }
                    }
                }
            }
            // ---- camera ray of (pixel, sample): cpu.rs:28-50 ----
            if (gen) {
                uint32_t rng;
                if (f.seed_mode != 0u) rng = (f.sample_begin + sample) * 6023u + (757283u * px + 872653746u * py);   // rt_compute.wgsl:102
                else rng = 987612486u * ((py * f.width + px) + 87636354u);                // cpu.rs:28-29 (one sample: the stream's first)
                const uint32_t y = f.height - py;                                         // cpu.rs:32
                const float screen_x = ((((float)px / (float)f.width) * 2.0f) - 1.0f) * f.aspect;   // cpu.rs:33-34
                const float screen_y = (((float)y / (float)f.height) * 2.0f) - 1.0f;     // cpu.rs:35
                const float jx = (rand_f32(rng) * 2.0f - 1.0f) * 0.0005f;                 // cpu.rs:38-42
                const float jy = (rand_f32(rng) * 2.0f - 1.0f) * 0.0005f;
                const float rx = -screen_x + jx, ry = screen_y + jy, rz = 1.0f;
                // Mat4f * Vec3f, upper-left 3x3, data[col][row] (mat4.rs:143-152)
                const float4 *cr = f.cams + (size_t)view * 4;
                const float4 c0 = cr[0], c1 = cr[1], c2 = cr[2], c3 = cr[3];
                const V3 dir = mk(c0.x * rx + c1.x * ry + c2.x * rz,
                                  c0.y * rx + c1.y * ry + c2.y * rz,
                                  c0.z * rx + c1.z * ry + c2.z * rz);
                d = normalized(dir);
                o = mk(c3.x, c3.y, c3.z);
                // ---- start traverse_bvh (ray.rs:84-88, HitInfo::default :214-226) ----
                best_t = kMiss; best_u = 0.0f; best_v = 0.0f; best_tri = kNoTri;
                rd = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
                dir_safe = ray_safe(o, d, sc.tiny_axes);
                sp = 0; pair = 0u;
                tri_cur = sc.root_a; tri_end = sc.root_a + sc.root_n;     // root leaf (root_n > 0) or inner (empty range)
                if (COUNT) c_rays++;
                state = FS_T;
            }
            continue;   // re-evaluate the ballots
        }

        // ---------------- one traversal step per traversing lane (ray_query.hip's, closest hit) ----------
        if (state == FS_T) {
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
            bool need_pop = false;
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
                    best_t = t; best_u = u; best_v = v;
                    best_tri = __float_as_uint(r2.y) | ((det > 0.0f) ? kFrontBit : 0u);   // ray.rs:39
                }
                tri_cur += 1;
                need_pop = (tri_cur == tri_end);
            } else {                                                                 // ray.rs:108-137
                const float max_d = best_t * f.cull_scale;
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
                        else atomicAdd(&f.stats->stack_overflows, 1ull);              // reference: panic (ray.rs:85)
                    }
                    sp += (push && sp < (uint32_t)(kStackLds + kStackOvf)) ? 1u : 0u;
                    if (COUNT) c_maxsp = sp > c_maxsp ? sp : c_maxsp;
                    if (n1 > 0u) { tri_cur = a1; tri_end = a1 + n1; }                // ray.rs:131 node = child_1
                    else { pair = a1; }
                }
            }
            if (need_pop) {                                                          // ray.rs:100-105, 125-129
                if (sp == 0u) {
                    state = FS_D;
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
        atomicAdd(&f.stats->rays, c_rays);
        atomicAdd(&f.stats->inner_steps, c_inner);
        atomicAdd(&f.stats->tri_tests, c_tris);
        atomicAdd(&f.stats->hits, c_hits);
        atomicAdd(&f.stats->texel_fetches, c_tex);
        atomicMax(&f.stats->max_stack, (unsigned long long)c_maxsp);
    }
    if (lane == 0u && w_pixels) atomicAdd(&f.stats->pixels, (unsigned long long)w_pixels);
}

template <bool COUNT, bool CULL, int MOTION = kMotionNone>
static hipError_t launch_f(const DevScene &sc, const DevFeatures &f, int grid, hipStream_t stream) {
    hipLaunchKernelGGL((first_hit_kernel<COUNT, CULL, MOTION>), dim3(grid), dim3(kBlockThreads), 0, stream, sc, f);
    return hipGetLastError();
}
template <bool COUNT, bool CULL, int MOTION = kMotionNone>
static int occ_f() {
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, first_hit_kernel<COUNT, CULL, MOTION>, kBlockThreads, 0) != hipSuccess) n = 1;
    return n;
}

// instantiations: {count} x {cull}
hipError_t launch_first_hit(const DevScene &sc, const DevFeatures &f, bool count, bool cull, int grid, hipStream_t stream) {
    if (count) return cull ? launch_f<true, true>(sc, f, grid, stream) : launch_f<true, false>(sc, f, grid, stream);
    return cull ? launch_f<false, true>(sc, f, grid, stream) : launch_f<false, false>(sc, f, grid, stream);
}
int first_hit_blocks_per_cu(bool count, bool cull) {
    int n = count ? (cull ? occ_f<true, true>() : occ_f<true, false>()) : (cull ? occ_f<false, true>() : occ_f<false, false>());
    if (n < 1) n = 1;
    if (n > 8) n = 8;
    return n;
}

// the motion pass: {cull} x {explicit, tracked}; tracked = f.prev_tris is null
hipError_t launch_motion(const DevScene &sc, const DevFeatures &f, bool cull, int grid, hipStream_t stream) {
    if (f.prev_tris) return cull ? launch_f<false, true, kMotionExplicit>(sc, f, grid, stream) : launch_f<false, false, kMotionExplicit>(sc, f, grid, stream);
    return cull ? launch_f<false, true, kMotionTracked>(sc, f, grid, stream) : launch_f<false, false, kMotionTracked>(sc, f, grid, stream);
}
int motion_blocks_per_cu(bool explicit_source, bool cull) {
    int n = explicit_source ? (cull ? occ_f<false, true, kMotionExplicit>() : occ_f<false, false, kMotionExplicit>())
                            : (cull ? occ_f<false, true, kMotionTracked>() : occ_f<false, false, kMotionTracked>());
    if (n < 1) n = 1;
    if (n > 8) n = 8;
    return n;
}

} // namespace mipt
