// scene_update.hip -- new geometry in a resident scene: mipt_scene_update_triangles{,_device} (include/mipt.h).
//
// The reference's realtime loop edits its Rc<RefCell<Scene>> (src/main.rs:46, window.rs:349-389); here the edit reaches the HBM layout
// of pt_kernel.h without touching the materials, the texel pool or the workspace, in one of two ways:
//   REFIT   the tree, the order of the 64-B pair records and the triangle slots stay.  Every bound becomes the fold of Node::grow_by_tri
//           (bvh.rs:185-193) over the node's triangles: a leaf child folds the exact vertex positions of its slots [a, a+n) (each slot's
//           record names its triangle), an inner child is the union of the two bounds in its child record.  One launch per tree level,
//           deepest first: a level only reads records of deeper levels, and the kernel boundary makes them visible -- nothing is handed
//           between workgroups inside a launch.  The results go into a SCRATCH copy of the records, are checked as mipt_scene_create
//           checks a node array (bound limits, tiny plane coordinates), and only a clean result is committed: the records, then both
//           triangle streams by slot, then the kept node array's bounds, then DevScene::tiny_axes.
//   REBUILD the geometry half of mipt_scene_create_from_triangles (scene_device.hip mipt::build_geometry) on the new triangles, into new
//           allocations; the old geometry is freed only after that succeeded.
// Both run from triangles in HBM: the host entry stages its array into HBM first (one path, not two).
#include "../../include/mipt.h"
#include "mipt_scene.h"                                          // and with it mipt_host_util.h, mipt_internal.h

#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

namespace {

constexpr int kT = 256;
constexpr uint32_t kSerialLeaf = 16;            // a leaf child with more triangles goes to the workgroup-per-leaf pass
constexpr uint32_t kMaxLevels = 8192 + 64;      // mipt_scene_create refuses trees deeper than 8192 (+ one batch) levels

using mipt::fail;
double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct Box { float lo[3], hi[3]; };
__device__ __forceinline__ void box_empty(Box *b) {                // Node::default (bvh.rs:174-181)
    for (int k = 0; k < 3; k++) { b->lo[k] = 3.40282347e38f; b->hi[k] = -3.40282347e38f; }
}
__device__ __forceinline__ void box_grow(Box *b, const Box &o) {
    for (int k = 0; k < 3; k++) { b->lo[k] = fminf(b->lo[k], o.lo[k]); b->hi[k] = fmaxf(b->hi[k], o.hi[k]); }
}
// grow_by_tri with the triangle of intersection-stream slot `slot`: its record names the (tree-order) triangle t, the new positions are
// tris[tri_order ? tri_order[t] : t] -- exact vertices, not v0 + e1 of the stream (rounded)
__device__ __forceinline__ void box_grow_slot(Box *b, const float4 *tri_pos, uint32_t slot, const MiptTriangle *tris, const uint32_t *tri_order) {
    const uint32_t t = reinterpret_cast<const uint32_t *>(tri_pos)[(size_t)slot * 16 + 9];     // tri_pos[4*slot+2].y
    const MiptTriangle *tr = tris + (tri_order ? tri_order[t] : t);
    for (int v = 0; v < 3; v++) {
        const float p[3] = {tr->vertices[v].position.x, tr->vertices[v].position.y, tr->vertices[v].position.z};
        for (int k = 0; k < 3; k++) { b->lo[k] = fminf(b->lo[k], p[k]); b->hi[k] = fmaxf(b->hi[k], p[k]); }
    }
}
__device__ __forceinline__ void store_child(float4 *rec, uint32_t w, const Box &b) {               // bounds only: a / n stay
    const float4 lo = rec[w * 2u], hi = rec[w * 2u + 1u];
    rec[w * 2u] = make_float4(b.lo[0], b.lo[1], b.lo[2], lo.w);
    rec[w * 2u + 1u] = make_float4(b.hi[0], b.hi[1], b.hi[2], hi.w);
}

struct Ctl {
    uint32_t bad_tri, bad_bound, tiny_axes, n_big;
    uint32_t overflow, pad[3];
    Box root;
};

// ---- the plan: records grouped by depth, breadth-first from record 0 (= pair 0, the root's children: the tree top of the pair
// order is breadth-first, mipt_internal.h).  lv[d] = records at depth d, lv[kMaxLevels + d] = where they start in `plan`. ----
__global__ void plan_level(const float4 *pairs, const MiptNode *nodes, uint32_t *plan, uint32_t *pair_of, uint32_t cap, uint32_t *lv, uint32_t d, Ctl *ctl) {
    const uint32_t cnt = lv[d], off = lv[kMaxLevels + d], next = off + cnt;
    if (blockIdx.x == 0 && threadIdx.x == 0) lv[kMaxLevels + d + 1u] = next;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < cnt; i += gridDim.x * blockDim.x) {
        const uint32_t j = plan[off + i];
        for (uint32_t w = 0; w < 2u; w++) {
            const float4 lo = pairs[(size_t)j * 4 + w * 2u], hi = pairs[(size_t)j * 4 + w * 2u + 1u];
            if (__float_as_uint(hi.w) != 0u) continue;                             // a leaf child
            const uint32_t pos = next + atomicAdd(&lv[d + 1u], 1u);
            if (pos >= cap) { atomicOr(&ctl->overflow, 1u); continue; }
            const uint32_t c = __float_as_uint(lo.w);
            plan[pos] = c;
            if (pair_of) pair_of[c] = (nodes[2u * pair_of[j] + 1u + w].first_tri_or_child - 1u) / 2u;
        }
    }
}

// ---- refit ----
// material ids of the new triangles (the reference indexes materials[material_id], mipt_scene_create refuses it): lowest offender
__global__ void check_materials(const MiptTriangle *tris, uint32_t n_tris, uint32_t n_materials, Ctl *ctl) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_tris; i += gridDim.x * blockDim.x)
        if (tris[i].material_id >= n_materials) atomicMin(&ctl->bad_tri, i);
}
// every leaf child of every record; big leaves are listed for refit_big_leaves (pad records: two zero children, skipped as inner)
__global__ void refit_leaves(const float4 *pairs, float4 *scratch, uint32_t n_records, const float4 *tri_pos, const MiptTriangle *tris,
                             const uint32_t *tri_order, uint32_t *big, Ctl *ctl) {
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n_records; j += gridDim.x * blockDim.x) {
        for (uint32_t w = 0; w < 2u; w++) {
            const float4 lo = pairs[(size_t)j * 4 + w * 2u], hi = pairs[(size_t)j * 4 + w * 2u + 1u];
            const uint32_t n = __float_as_uint(hi.w), a = __float_as_uint(lo.w);
            if (n == 0u) continue;
            if (n > kSerialLeaf) { big[atomicAdd(&ctl->n_big, 1u)] = 2u * j + w; continue; }
            Box b;
            box_empty(&b);
            for (uint32_t s = a; s < a + n; s++) box_grow_slot(&b, tri_pos, s, tris, tri_order);
            store_child(scratch + (size_t)j * 4, w, b);
        }
    }
}
// the fold of slots [a, a+n) by one workgroup (f32 min / max are exact: only the sign of a zero can depend on the order)
__device__ Box block_fold(uint32_t a, uint32_t n, const float4 *tri_pos, const MiptTriangle *tris, const uint32_t *tri_order) {
    __shared__ Box s_box[kT / 64];
    Box b;
    box_empty(&b);
    for (uint32_t s = a + threadIdx.x; s < a + n; s += kT) box_grow_slot(&b, tri_pos, s, tris, tri_order);
    for (int o = 32; o > 0; o >>= 1)
        for (int k = 0; k < 3; k++) { b.lo[k] = fminf(b.lo[k], __shfl_xor(b.lo[k], o)); b.hi[k] = fmaxf(b.hi[k], __shfl_xor(b.hi[k], o)); }
    if ((threadIdx.x & 63u) == 0u) s_box[threadIdx.x >> 6] = b;
    __syncthreads();
    Box r;
    box_empty(&r);
    for (int i = 0; i < kT / 64; i++) box_grow(&r, s_box[i]);
    __syncthreads();
    return r;
}
__global__ __launch_bounds__(kT) void refit_big_leaves(const float4 *pairs, float4 *scratch, const float4 *tri_pos, const MiptTriangle *tris,
                                                       const uint32_t *tri_order, const uint32_t *big, const Ctl *ctl) {
    const uint32_t n_big = ctl->n_big;
    for (uint32_t e = blockIdx.x; e < n_big; e += gridDim.x) {
        const uint32_t j = big[e] >> 1, w = big[e] & 1u;
        const uint32_t a = __float_as_uint(pairs[(size_t)j * 4 + w * 2u].w), n = __float_as_uint(pairs[(size_t)j * 4 + w * 2u + 1u].w);
        const Box b = block_fold(a, n, tri_pos, tris, tri_order);
        if (threadIdx.x == 0) store_child(scratch + (size_t)j * 4, w, b);
    }
}
__device__ __forceinline__ Box record_union(const float4 *rec) {
    Box b;
    const float4 l0 = rec[0], h0 = rec[1], l1 = rec[2], h1 = rec[3];
    b.lo[0] = fminf(l0.x, l1.x); b.lo[1] = fminf(l0.y, l1.y); b.lo[2] = fminf(l0.z, l1.z);
    b.hi[0] = fmaxf(h0.x, h1.x); b.hi[1] = fmaxf(h0.y, h1.y); b.hi[2] = fmaxf(h0.z, h1.z);
    return b;
}
// one tree level: the inner children of its records become the union of their child records (one level deeper: already final)
__global__ void refit_level(const uint32_t *plan, uint32_t off, uint32_t cnt, float4 *scratch) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < cnt; i += gridDim.x * blockDim.x) {
        const uint32_t j = plan[off + i];
        float4 *rec = scratch + (size_t)j * 4;
        for (uint32_t w = 0; w < 2u; w++) {
            const float4 lo = rec[w * 2u], hi = rec[w * 2u + 1u];
            if (__float_as_uint(hi.w) != 0u) continue;
            store_child(rec, w, record_union(scratch + (size_t)__float_as_uint(lo.w) * 4));
        }
    }
}
// the root's bound: the union of record 0, or the fold of a root leaf's triangles
__global__ __launch_bounds__(kT) void refit_root(const float4 *scratch, uint32_t has_pairs, uint32_t root_a, uint32_t root_n, const float4 *tri_pos,
                                                 const MiptTriangle *tris, const uint32_t *tri_order, Ctl *ctl) {
    if (has_pairs) { if (threadIdx.x == 0) ctl->root = record_union(scratch); return; }
    const Box b = block_fold(root_a, root_n, tri_pos, tris, tri_order);
    if (threadIdx.x == 0) ctl->root = b;
}
// check_nodes of scene_device.hip over the refit bounds: every child of every record, and the root
__device__ __forceinline__ void check_plane(float v, uint32_t k, uint32_t *bad, uint32_t *tiny_axes) {
    const float lim = 1.0995116e12f, tiny = 1.3234890e-23f /* 2^-76 */;
    if (!(fabsf(v) <= lim)) *bad = 1u;
    if (v != 0.0f && fabsf(v) < tiny) *tiny_axes |= 1u << k;
}
__global__ void check_bounds(const float4 *scratch, uint32_t n_records, Ctl *ctl) {
    uint32_t bad = 0, tiny_axes = 0;
    const uint32_t n = 2u * n_records + 1u;                           // record children, then the root
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        float p[6];
        if (i < 2u * n_records) {
            const float4 lo = scratch[(size_t)i * 2], hi = scratch[(size_t)i * 2 + 1];
            p[0] = lo.x; p[1] = lo.y; p[2] = lo.z; p[3] = hi.x; p[4] = hi.y; p[5] = hi.z;
        } else {
            for (int k = 0; k < 3; k++) { p[k] = ctl->root.lo[k]; p[3 + k] = ctl->root.hi[k]; }
        }
        for (uint32_t k = 0; k < 3u; k++) { check_plane(p[k], k, &bad, &tiny_axes); check_plane(p[3 + k], k, &bad, &tiny_axes); }
    }
    for (int o = 32; o > 0; o >>= 1) { tiny_axes |= __shfl_xor(tiny_axes, o); bad |= __shfl_xor(bad, o); }
    if ((threadIdx.x & 63u) == 0u) {
        if (tiny_axes) atomicOr(&ctl->tiny_axes, tiny_axes);
        if (bad) atomicOr(&ctl->bad_bound, 1u);
    }
}
// commit: both triangle streams by slot -- the slot-driven form of write_tris (scene_device.hip): slot s holds tree-order triangle t
// (its record says which), whose attributes live at t; the edges are one rounded f32 subtraction each (ray.rs:24-25; -ffp-contract=off)
__global__ void rewrite_tris(const MiptTriangle *tris, const uint32_t *tri_order, uint32_t n_tris, float4 *tri_pos, float4 *tri_attr) {
    for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < n_tris; s += gridDim.x * blockDim.x) {
        const uint32_t t = reinterpret_cast<const uint32_t *>(tri_pos)[(size_t)s * 16 + 9];
        const float4 *src = reinterpret_cast<const float4 *>(tris + (tri_order ? tri_order[t] : t));
        const float4 a0 = src[0], a1 = src[1], a2 = src[2], a3 = src[3], a4 = src[4], a5 = src[5], a6 = src[6];
        const float e1x = a2.x - a0.x, e1y = a2.y - a0.y, e1z = a2.z - a0.z;
        const float e2x = a4.x - a0.x, e2y = a4.y - a0.y, e2z = a4.z - a0.z;
        const size_t q = (size_t)s * 4;
        tri_pos[q + 0] = make_float4(a0.x, a0.y, a0.z, e1x);
        tri_pos[q + 1] = make_float4(e1y, e1z, e2x, e2y);
        tri_pos[q + 2] = make_float4(e2z, __uint_as_float(t), 0.0f, 0.0f);
        tri_pos[q + 3] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        tri_attr[(size_t)t * 4 + 0] = make_float4(a1.x, a1.y, a1.z, a3.x);
        tri_attr[(size_t)t * 4 + 1] = make_float4(a3.y, a3.z, a5.x, a5.y);
        tri_attr[(size_t)t * 4 + 2] = make_float4(a5.z, a0.w, a1.w, a2.w);
        tri_attr[(size_t)t * 4 + 3] = make_float4(a3.w, a4.w, a5.w, a6.x);
    }
}
// commit: the kept node array (mipt_scene_get_bvh) -- record j holds nodes 2k+1, 2k+2 of reference pair k = pair_of[j]
__device__ __forceinline__ void node_bounds(MiptNode *n, const float lo[3], const float hi[3]) {
    n->bounds_min.x = lo[0]; n->bounds_min.y = lo[1]; n->bounds_min.z = lo[2];
    n->bounds_max.x = hi[0]; n->bounds_max.y = hi[1]; n->bounds_max.z = hi[2];
}
__global__ void refit_nodes(const float4 *scratch, const uint32_t *plan, uint32_t n_plan, const uint32_t *pair_of, MiptNode *nodes, const Ctl *ctl) {
    const uint32_t i0 = blockIdx.x * blockDim.x + threadIdx.x;
    if (i0 == 0) node_bounds(nodes, ctl->root.lo, ctl->root.hi);
    for (uint32_t i = i0; i < n_plan; i += gridDim.x * blockDim.x) {
        const uint32_t j = plan[i], k = pair_of[j];
        for (uint32_t w = 0; w < 2u; w++) {
            const float4 lo = scratch[(size_t)j * 4 + w * 2u], hi = scratch[(size_t)j * 4 + w * 2u + 1u];
            const float l[3] = {lo.x, lo.y, lo.z}, h[3] = {hi.x, hi.y, hi.z};
            node_bounds(nodes + 2u * k + 1u + w, l, h);
        }
    }
}

uint32_t grid_for(size_t n, uint32_t cap) {
    const size_t g = (n + kT - 1) / kT;
    return g < 1 ? 1u : (g > cap ? cap : (uint32_t)g);
}

// the REFIT plan of `s`, made once per tree (see MiptScene::refit_level_off)
int ensure_plan(MiptScene *s, hipStream_t st) {
    if (!s->refit_level_off.empty() || s->dev.n_pairs == 0) return MIPT_OK;
    const uint32_t cap = s->dev.n_pairs;
    mipt::DevPtr<uint32_t> plan, pair_of, lv;
    mipt::DevPtr<Ctl> ctl;
    mipt::SyncOnExit sync(st);                                           // a failure waits for the queued kernels before the buffers go
    MIPT_HIP(plan.alloc(cap));
    if (s->d_nodes) MIPT_HIP(pair_of.alloc(cap));
    MIPT_HIP(lv.alloc(2 * kMaxLevels + 1));
    MIPT_HIP(ctl.alloc(1));
    MIPT_HIP(hipMemsetAsync(lv, 0, (size_t)(2 * kMaxLevels + 1) * 4, st));
    MIPT_HIP(hipMemsetAsync(ctl, 0, sizeof(Ctl), st));
    MIPT_HIP(hipMemsetAsync(plan, 0, 4, st));                             // level 0 = { record 0 } (pair 0)
    if (pair_of) MIPT_HIP(hipMemsetAsync(pair_of, 0, 4, st));
    {
        const uint32_t one = 1;
        MIPT_HIP(hipMemcpyAsync(lv, &one, 4, hipMemcpyHostToDevice, st));
        MIPT_HIP(hipStreamSynchronize(st));
    }
    std::vector<uint32_t> h_lv(2 * kMaxLevels + 1);
    uint32_t depth = 0;
    for (;;) {                                                          // batches of levels, then one look at the next level's size
        for (int b = 0; b < 16 && depth + 1 < kMaxLevels; b++, depth++)
            hipLaunchKernelGGL(plan_level, dim3(1024), dim3(kT), 0, st, (const float4 *)s->dev.pairs, s->d_nodes, plan, pair_of, cap, lv, depth, ctl);
        MIPT_HIP(hipGetLastError());
        MIPT_HIP(hipMemcpyAsync(h_lv.data(), lv, h_lv.size() * 4, hipMemcpyDeviceToHost, st));
        MIPT_HIP(hipStreamSynchronize(st));
        if (h_lv[depth] == 0u) break;
        if (depth + 1 >= kMaxLevels) return fail(MIPT_ERR_BVH, "refit plan: tree deeper than %u levels", kMaxLevels);
    }
    Ctl hc;
    MIPT_HIP(hipMemcpy(&hc, ctl, sizeof hc, hipMemcpyDeviceToHost));
    if (hc.overflow) return fail(MIPT_ERR_BVH, "refit plan: more records reached than the scene holds (internal)");
    lv.reset();
    ctl.reset();
    std::vector<uint32_t> off(depth + 1);                               // levels 0 .. depth-1 and the end
    for (uint32_t d = 0; d <= depth; d++) off[d] = h_lv[kMaxLevels + d];
    s->d_refit_plan = std::move(plan);
    s->d_refit_pair = std::move(pair_of);
    s->refit_level_off = std::move(off);
    sync.dismiss();
    return MIPT_OK;
}

int refit(MiptScene *s, const MiptTriangle *d_tris, hipStream_t st, MiptUpdateInfo *inf) {
    const uint32_t n_tris = (uint32_t)s->n_tris, n_records = s->dev.n_pairs;
    { const int rc = ensure_plan(s, st); if (rc) return rc; }
    mipt::Event e0, e1;
    mipt::DevPtr<float4> scratch;
    mipt::DevPtr<uint32_t> big;
    mipt::DevPtr<Ctl> ctl;
    mipt::SyncOnExit sync(st);                                           // on every way out, success included: `st` is idle before the buffers go
    MIPT_HIP(hipEventCreate(e0.put()));
    MIPT_HIP(hipEventCreate(e1.put()));
    MIPT_HIP(ctl.alloc(1));
    if (n_records) {
        MIPT_HIP(scratch.alloc((size_t)n_records * 4));
        MIPT_HIP(big.alloc((size_t)n_records * 2));
    }
    {
        Ctl h;
        memset(&h, 0, sizeof h);
        h.bad_tri = 0xffffffffu;
        MIPT_HIP(hipMemcpyAsync(ctl, &h, sizeof h, hipMemcpyHostToDevice, st));
    }
    const float4 *pairs = s->dev.pairs, *tri_pos = s->dev.tri_pos;
    const uint32_t *order = s->d_tri_order;
    MIPT_HIP(hipEventRecord(e0, st));
    hipLaunchKernelGGL(check_materials, dim3(grid_for(n_tris, 4096)), dim3(kT), 0, st, d_tris, n_tris, s->dev.n_mats, ctl);
    if (n_records) {
        MIPT_HIP(hipMemcpyAsync(scratch, pairs, (size_t)n_records * 64, hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL(refit_leaves, dim3(grid_for(n_records, 4096)), dim3(kT), 0, st, pairs, scratch, n_records, tri_pos, d_tris, order, big, ctl);
        hipLaunchKernelGGL(refit_big_leaves, dim3(1024), dim3(kT), 0, st, pairs, scratch, tri_pos, d_tris, order, big, ctl);
        const std::vector<uint32_t> &off = s->refit_level_off;
        for (size_t d = off.size() - 1; d-- > 0;) {                      // deepest level first
            const uint32_t cnt = off[d + 1] - off[d];
            if (cnt) hipLaunchKernelGGL(refit_level, dim3(grid_for(cnt, 4096)), dim3(kT), 0, st, s->d_refit_plan, off[d], cnt, scratch);
        }
    }
    hipLaunchKernelGGL(refit_root, dim3(1), dim3(kT), 0, st, scratch, n_records ? 1u : 0u, s->dev.root_a, s->dev.root_n, tri_pos, d_tris, order, ctl);
    hipLaunchKernelGGL(check_bounds, dim3(grid_for(2 * (size_t)n_records + 1, 2048)), dim3(kT), 0, st, scratch, n_records, ctl);
    MIPT_HIP(hipGetLastError());
    MIPT_HIP(hipEventRecord(e1, st));
    Ctl hc;
    MIPT_HIP(hipMemcpyAsync(&hc, ctl, sizeof hc, hipMemcpyDeviceToHost, st));
    MIPT_HIP(hipStreamSynchronize(st));
    float build_ms = 0.0f;
    (void)hipEventElapsedTime(&build_ms, e0, e1);
    if (hc.bad_bound) return fail(MIPT_ERR_SCENE_LIMIT, "a node has a non-finite bound or one beyond 2^40");
    if (hc.bad_tri != 0xffffffffu) {
        MiptTriangle t;
        const hipError_t e = hipMemcpy(&t, d_tris + hc.bad_tri, sizeof t, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return fail(MIPT_ERR_HIP, "reading a triangle back: %s", hipGetErrorString(e));
        return fail(MIPT_ERR_INVALID_ARG, "triangle %u has material_id %u >= n_materials %u", hc.bad_tri, t.material_id, s->dev.n_mats);
    }
    // ---- commit: nothing below can fail on the data, only on the runtime ----
    const double t_commit = now_ms();
    if (n_records) MIPT_HIP(hipMemcpyAsync((void *)pairs, scratch, (size_t)n_records * 64, hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(rewrite_tris, dim3(grid_for(n_tris, 4096)), dim3(kT), 0, st, d_tris, order, n_tris, (float4 *)tri_pos, (float4 *)s->dev.tri_attr);
    if (s->d_nodes) {
        const uint32_t n_plan = s->refit_level_off.empty() ? 0u : s->refit_level_off.back();
        hipLaunchKernelGGL(refit_nodes, dim3(grid_for(n_plan, 2048)), dim3(kT), 0, st, scratch, s->d_refit_plan, n_plan, s->d_refit_pair, s->d_nodes, ctl);
    }
    MIPT_HIP(hipGetLastError());
    MIPT_HIP(hipStreamSynchronize(st));
    s->dev.tiny_axes = hc.tiny_axes;
    inf->build_ms = build_ms;
    inf->layout_ms = now_ms() - t_commit;
    return MIPT_OK;
}

int rebuild(MiptScene *s, const MiptTriangle *d_tris, uint32_t n_tris, MiptUpdateInfo *inf) {
    mipt::ResidentBvh bvh;
    mipt::SceneGeometry geo;
    const int rc = mipt::build_geometry(d_tris, n_tris, s->dev.n_mats, s->device, false, &bvh, &geo);
    if (rc) return rc;                                                // with what the build left in `bvh`
    const double t_build = geo.t_build;
    inf->build_ms = geo.build_ms;
    mipt::release_geometry(s);
    mipt::attach_geometry(s, std::move(geo));
    s->info.built_on_device = 1u;
    inf->layout_ms = now_ms() - t_build;
    return MIPT_OK;
}

int check_args(const char *who, const MiptScene *s, const void *tris, uint32_t n_tris, uint32_t mode) {
    if (!s || !tris) return fail(MIPT_ERR_INVALID_ARG, "%s: null argument", who);
    if (mode != MIPT_UPDATE_REFIT && mode != MIPT_UPDATE_REBUILD) return fail(MIPT_ERR_INVALID_ARG, "%s: mode %u is neither MIPT_UPDATE_REFIT nor MIPT_UPDATE_REBUILD", who, mode);
    if (n_tris == 0) return fail(MIPT_ERR_INVALID_ARG, "%s: no triangles (the reference panics in BVH::build)", who);
    if (mode == MIPT_UPDATE_REFIT && n_tris != s->n_tris)
        return fail(MIPT_ERR_INVALID_ARG, "%s: REFIT keeps the tree: %u triangles given, the scene has %zu", who, n_tris, s->n_tris);
    if (n_tris > mipt::kMaxTris) return fail(MIPT_ERR_SCENE_LIMIT, "%u triangles exceed the 2^25 device-format limit", n_tris);
    return MIPT_OK;
}

void finish_info(const MiptScene *s, MiptUpdateInfo *inf, double t0) {
    inf->total_ms = now_ms() - t0;
    inf->n_tris = (uint32_t)s->n_tris; inf->n_nodes = s->info.n_nodes; inf->n_pair_records = s->info.n_pair_records; inf->reserved = 0;
}

} // namespace

void mipt::release_geometry(MiptScene *s) {
    (void)hipSetDevice(s->device);
    s->d_geom.reset(); s->d_tri_attr.reset(); s->d_nodes.reset(); s->d_tri_order.reset();
    s->d_touched.reset(); s->d_refit_plan.reset(); s->d_refit_pair.reset();
    s->d_bake_inv.reset();                                                // the caller -> tree map of mipt_bake_gather: the tree it was made for is gone
    s->refit_level_off.clear();
}

int mipt::scene_update_device(MiptScene *s, const MiptTriangle *d_tris, uint32_t n_tris, uint32_t mode, hipStream_t st, MiptUpdateInfo *info,
                              bool expanded_mesh) {
    const double t0 = now_ms();
    { const int rc = check_args("mipt_scene_update_triangles_device", s, d_tris, n_tris, mode); if (rc) return rc; }
    if (s->mesh && !expanded_mesh)
        return fail(MIPT_ERR_INVALID_ARG, "mipt_scene_update_triangles_device: scene owns a mesh (use mipt_scene_set_transforms / mipt_scene_update_mesh_device)");
    MiptUpdateInfo inf{};
    hipError_t e = hipSetDevice(s->device);
    if (e == hipSuccess) e = hipStreamSynchronize(st);                   // ordered after the caller's earlier work on `st`
    if (e != hipSuccess) return fail(MIPT_ERR_HIP, "mipt_scene_update_triangles_device: %s", hipGetErrorString(e));
    const int rc = mode == MIPT_UPDATE_REFIT ? refit(s, d_tris, st, &inf) : rebuild(s, d_tris, n_tris, &inf);
    if (rc) return rc;
    finish_info(s, &inf, t0);
    if (info) *info = inf;
    return MIPT_OK;
}

int mipt::scene_update_host(MiptScene *s, const MiptTriangle *tris, uint32_t n_tris, uint32_t mode, MiptUpdateInfo *info) {
    const double t0 = now_ms();
    { const int rc = check_args("mipt_scene_update_triangles", s, tris, n_tris, mode); if (rc) return rc; }
    if (s->mesh) return fail(MIPT_ERR_INVALID_ARG, "mipt_scene_update_triangles: scene owns a mesh (use mipt_scene_set_transforms / mipt_scene_update_mesh_device)");
    hipError_t e = hipSetDevice(s->device);
    mipt::DevPtr<MiptTriangle> d_tris;
    if (e == hipSuccess) e = d_tris.alloc(n_tris);
    if (e != hipSuccess) return fail(MIPT_ERR_HIP, "mipt_scene_update_triangles: %s", hipGetErrorString(e));
    int rc = mipt::upload_staged(d_tris, tris, (size_t)n_tris * sizeof(MiptTriangle));
    const double t_up = now_ms();
    MiptUpdateInfo inf{};
    if (rc == MIPT_OK) rc = mipt::scene_update_device(s, d_tris, n_tris, mode, nullptr, &inf, false);
    (void)hipSetDevice(s->device);
    d_tris.reset();
    if (rc) return rc;
    inf.upload_ms = t_up - t0;
    finish_info(s, &inf, t0);
    if (info) *info = inf;
    return MIPT_OK;
}

// dst := src's geometry by device-to-device copies, into new allocations first (the replica keeps rendering its old geometry if a copy
// fails); the mechanism of clone_issue / clone_finish (mipt_api.cpp)
int mipt::replica_refresh(const MiptScene *src, MiptScene *dst) {
    const int device = dst->device;
    SceneGeometry g;
    mipt::SyncOnExit sync(nullptr, device);                              // a failed copy: the others are waited for before g's buffers go
    MIPT_HIP(hipSetDevice(device));
    if (device != src->device) {
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, device, src->device) == hipSuccess && can) {
            const hipError_t pe = hipDeviceEnablePeerAccess(src->device, 0);
            if (pe != hipSuccess) (void)hipGetLastError();                // hipErrorPeerAccessAlreadyEnabled included
        }
    }
    struct Part { void **dst; const void *from; size_t alloc, copy; };
    const Part parts[] = {{(void **)g.d_geom.put(), src->d_geom, src->geom_alloc, (size_t)src->dev.geom_bytes},
                          {(void **)g.d_tri_attr.put(), src->d_tri_attr, src->attr_bytes < 16 ? 16 : src->attr_bytes, src->attr_bytes},
                          {(void **)g.d_nodes.put(), src->d_nodes, (size_t)src->n_nodes * sizeof(MiptNode), (size_t)src->n_nodes * sizeof(MiptNode)},
                          {(void **)g.d_tri_order.put(), src->d_tri_order, src->n_tris * 4, src->n_tris * 4}};
    for (const Part &p : parts) {
        if (!p.from) continue;
        MIPT_HIP(hipMalloc(p.dst, p.alloc ? p.alloc : 16));
        if (p.copy) MIPT_HIP(hipMemcpyPeerAsync(*p.dst, device, p.from, src->device, p.copy, nullptr));
    }
    MIPT_HIP(hipStreamSynchronize(nullptr));
    release_geometry(dst);
    dst->n_tris = src->n_tris; dst->n_nodes = src->n_nodes; dst->max_leaf = src->max_leaf;
    dst->geom_alloc = src->geom_alloc; dst->attr_bytes = src->attr_bytes;
    dst->d_geom = std::move(g.d_geom); dst->d_tri_attr = std::move(g.d_tri_attr); dst->d_nodes = std::move(g.d_nodes); dst->d_tri_order = std::move(g.d_tri_order);
    sync.dismiss();
    mipt::DevScene d = src->dev;                                          // sizes, root, tiny_axes; this replica's own buffers
    d.pairs = (const float4 *)dst->d_geom.get();
    d.tri_pos = (const float4 *)(dst->d_geom.get() + src->dev.tri_off_bytes);
    d.tri_attr = (const float4 *)dst->d_tri_attr.get();
    d.mats = dst->dev.mats; d.mats_full = dst->dev.mats_full; d.texels = dst->dev.texels;
    dst->dev = d;
    dst->info.n_tris = src->info.n_tris; dst->info.n_nodes = src->info.n_nodes; dst->info.n_pair_records = src->info.n_pair_records;
    dst->info.max_leaf = src->info.max_leaf; dst->info.geometry_bytes = src->info.geometry_bytes; dst->info.built_on_device = src->info.built_on_device;
    return MIPT_OK;
}

extern "C" {

int mipt_scene_update_triangles(MiptScene *scene, const MiptTriangle *tris, uint32_t n_tris, uint32_t mode, MiptUpdateInfo *info) {
    MIPT_NO_THROW(mipt::scene_update_host(scene, tris, n_tris, mode, info))
}

int mipt_scene_update_triangles_device(MiptScene *scene, const MiptTriangle *d_tris, uint32_t n_tris, uint32_t mode, void *hip_stream,
                                       MiptUpdateInfo *info) {
    MIPT_NO_THROW(mipt::scene_update_device(scene, d_tris, n_tris, mode, (hipStream_t)hip_stream, info))
}

} // extern "C"
