// scene_mesh.hip -- resident indexed meshes: mipt_mesh_expand, mipt_scene_create_from_mesh, mipt_scene_set_transforms,
// mipt_scene_update_mesh_device, mipt_scene_mesh_info (include/mipt.h, "resident indexed meshes") and the previous generation a
// mesh keeps for the motion pass, mipt_scene_track_motion ("previous positions").
//
// The reference expands its OBJ's vertex buffer + index triples into 112-byte fat triangles on the host (scene.rs:48-76) and every
// other geometry entry of this library takes that fat array.  Here the indexed arrays stay in HBM and the expansion is a kernel:
//   mesh_prepare_parts  one lane per part: the part's matrix columns and their cofactor columns (computed once per part), its
//                       material and first triangle, as one 96-byte PartRec
//   mesh_expand         one lane per triangle: binary search of the part over PartRec::first_tri, 3-9 index loads, three gathers of
//                       (12 + 12 + 8) B, the optional transform, and the 112-byte triangle as seven float4 into LDS at a 7-slot
//                       stride (odd: conflict-free); after a barrier the workgroup's 256 triangles (28 672 B) leave as consecutive
//                       float4 per lane, so every store instruction of a wave covers 1 KiB of whole 128-byte lines
// The expanded array (scene-owned, kept between updates: no allocation per frame) is handed to mipt::build_geometry at create time
// and to mipt::scene_update_device afterwards; nothing downstream knows about meshes.  The arithmetic of a vertex is ONE function
// compiled for host and device (xf_position / xf_normal below) under the file-wide -ffp-contract=off and correctly rounded
// divide / sqrt, so mipt_mesh_expand is the byte-for-byte yardstick of the kernel.
//
// Nothing resident is replaced before an update has succeeded: new transforms are prepared into a spare PartRec table, new vertex
// arrays are read from the caller's buffers by the expansion, and only after the REFIT / REBUILD committed are the tables swapped
// and the arrays copied over the resident ones.
#include "../../include/mipt.h"
#include "mipt_scene.h"                                          // and with it mipt_host_util.h, mipt_internal.h
#include "pt_mesh_rule.h"                                        // PartRec, xf_position, part_of: shared with the motion pass

#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>
#include <new>

static_assert(sizeof(MiptMeshPart) == 16 && sizeof(MiptMeshInfo) == 56 && sizeof(MiptMeshDesc) == 104, "mesh ABI structs (rust_ray_tracing_amd/_lib.py)");
static_assert(sizeof(MiptTriangle) == 112, "Triangle");

namespace mipt {

struct SceneMesh {
    float *d_pos = nullptr, *d_nrm = nullptr, *d_tex = nullptr;
    uint32_t *d_idx[3] = {nullptr, nullptr, nullptr};     // position / normal / tex-coord stream; [1], [2] may alias [0]
    MiptMeshPart *d_parts = nullptr;
    PartRec *d_rec[3] = {nullptr, nullptr, nullptr};      // [cur] = the table of the resident geometry; a table that is neither [cur]
    int cur = 0;                                          // nor [prev] is a spare.  [2] exists only while motion is tracked
    // mipt_scene_track_motion: the generation before the last successful update = d_prev_pos + d_rec[prev] (prev == cur: the
    // update kept the table, or there was none yet)
    bool track = false, prev_pos_same = false;            // prev_pos_same: d_prev_pos holds what d_pos holds
    int prev = 0;
    float *d_prev_pos = nullptr;
    uint64_t track_bytes = 0;                             // what tracking holds; part of array_bytes while it is on
    float *d_xf_stage = nullptr;                          // n_parts x 16 f32: where mipt_scene_set_transforms puts the host matrices
    uint32_t *d_flag = nullptr;                           // first position index entry out of range (0xffffffff = none)
    MiptTriangle *d_expanded = nullptr;
    uint32_t n_pos = 0, n_nrm = 0, n_tex = 0, n_idx = 0, n_tris = 0, n_parts = 0, has_xf = 0, streams = 1;
    uint64_t array_bytes = 0;
};

} // namespace mipt

namespace {

using mipt::PartRec;
using mipt::SceneMesh;
using mipt::xf_position;

constexpr int kT = 256;                                   // lanes = triangles of a workgroup of mesh_expand
constexpr uint32_t kNoIndex = 0xffffffffu;

using mipt::fail;
double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// ---- the expansion rule: one function for the host and the device -------------------------------------------------------------
__host__ __device__ inline void cross3(const float *a, const float *b, float *o) {      // vec3.rs:137-143
    o[0] = (a[1] * b[2]) - (a[2] * b[1]);
    o[1] = (a[2] * b[0]) - (a[0] * b[2]);
    o[2] = (a[0] * b[1]) - (a[1] * b[0]);
}
__host__ __device__ inline float length3(const float *v) {                              // vec3.rs:94-96
    return __builtin_sqrtf(((v[0] * v[0]) + (v[1] * v[1])) + (v[2] * v[2]));
}
// m: 16 f32, Mat4f data[col][row]; null = no transform
__host__ __device__ inline void part_record(const float *m, uint32_t first_tri, uint32_t material_id, PartRec *r) {
    r->first_tri = first_tri; r->material_id = material_id; r->has_xf = m ? 1u : 0u;
    for (int col = 0; col < 4; col++)
        for (int row = 0; row < 3; row++) r->a[col][row] = m ? m[col * 4 + row] : (col == row ? 1.0f : 0.0f);
    cross3(r->a[1], r->a[2], r->c[0]);
    cross3(r->a[2], r->a[0], r->c[1]);
    cross3(r->a[0], r->a[1], r->c[2]);
}
__host__ __device__ inline void xf_normal(const PartRec &r, float *n) {
    const float l0 = length3(n);
    float c[3];
    for (int k = 0; k < 3; k++) c[k] = ((r.c[0][k] * n[0]) + (r.c[1][k] * n[1])) + (r.c[2][k] * n[2]);
    const float l1 = length3(c);
    if (l1 > 0.0f && l1 < INFINITY) {
        const float s = l0 / l1;
        for (int k = 0; k < 3; k++) c[k] = c[k] * s;
    }
    for (int k = 0; k < 3; k++) n[k] = c[k];
}

struct MeshView {
    const float *pos, *nrm, *tex;
    const uint32_t *ip, *in, *it;
    uint32_t n_pos, n_nrm, n_tex, n_tris;
};

// corner `e` (= 3*t + c) as the eight words of a Vertex; false: its position index is out of range (the vertex is left at zero)
__host__ __device__ inline bool expand_corner(const MeshView &m, const PartRec &r, uint32_t e, uint32_t *v) {
    const uint32_t ip = m.ip[e], in = m.in[e], it = m.it[e];
    float p[3] = {0.0f, 0.0f, 0.0f}, n[3] = {0.0f, 0.0f, 0.0f};
    uint32_t tx = 0u, ty = 0u;
    const bool ok = ip < m.n_pos;
    uint32_t *pw = reinterpret_cast<uint32_t *>(p), *nw = reinterpret_cast<uint32_t *>(n);
    if (ok) { const uint32_t *s = reinterpret_cast<const uint32_t *>(m.pos) + (size_t)ip * 3; pw[0] = s[0]; pw[1] = s[1]; pw[2] = s[2]; }
    if (in < m.n_nrm) { const uint32_t *s = reinterpret_cast<const uint32_t *>(m.nrm) + (size_t)in * 3; nw[0] = s[0]; nw[1] = s[1]; nw[2] = s[2]; }
    if (it < m.n_tex) { const uint32_t *s = reinterpret_cast<const uint32_t *>(m.tex) + (size_t)it * 2; tx = s[0]; ty = s[1]; }
    if (r.has_xf) { xf_position(r, p); xf_normal(r, n); }
    v[0] = pw[0]; v[1] = pw[1]; v[2] = pw[2]; v[3] = tx;
    v[4] = nw[0]; v[5] = nw[1]; v[6] = nw[2]; v[7] = ty;
    return ok;
}

// ---- kernels --------------------------------------------------------------------------------------------------------------------
__global__ void mesh_prepare_parts(const MiptMeshPart *parts, uint32_t n_parts, const float *xf, PartRec *out) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_parts) return;
    PartRec r;
    part_record(xf ? xf + (size_t)p * 16 : nullptr, parts[p].first_tri, parts[p].material_id, &r);
    out[p] = r;
}

__global__ __launch_bounds__(kT) void mesh_expand(MeshView m, const PartRec *parts, uint32_t n_parts, float4 *out, uint32_t *flag) {
    __shared__ float4 stage[kT * 7];
    const uint32_t base = blockIdx.x * (uint32_t)kT, t = base + threadIdx.x;
    if (t < m.n_tris) {
        const PartRec r = parts[mipt::part_of(parts, n_parts, t)];
        float4 *dst = stage + threadIdx.x * 7u;
#pragma unroll
        for (uint32_t c = 0; c < 3u; c++) {
            uint32_t v[8];
            if (!expand_corner(m, r, 3u * t + c, v)) atomicMin(flag, 3u * t + c);
            dst[2u * c] = make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3]));
            dst[2u * c + 1u] = make_float4(__uint_as_float(v[4]), __uint_as_float(v[5]), __uint_as_float(v[6]), __uint_as_float(v[7]));
        }
        dst[6] = make_float4(__uint_as_float(r.material_id), 0.0f, 0.0f, 0.0f);
    }
    __syncthreads();
    const size_t first = (size_t)base * 7u, end = (size_t)m.n_tris * 7u;
#pragma unroll
    for (uint32_t i = 0; i < 7u; i++) {
        const uint32_t q = i * (uint32_t)kT + threadIdx.x;
        if (first + q < end) out[first + q] = stage[q];
    }
}

// ---- host-visible checks (before any device call) -------------------------------------------------------------------------------
// n_materials < 0: not checked (mipt_mesh_expand has no material table)
int check_mesh(const char *who, const MiptMeshDesc *m, int64_t n_materials) {
    if (!m->positions || !m->indices || !m->parts) return fail(MIPT_ERR_INVALID_ARG, "%s: null positions, indices or parts", who);
    if (m->n_indices % 3u) return fail(MIPT_ERR_INVALID_ARG, "%s: n_indices %u is not a multiple of 3", who, m->n_indices);
    const uint32_t n_tris = m->n_indices / 3u;
    if (n_tris == 0u) return fail(MIPT_ERR_INVALID_ARG, "%s: no triangles (the reference panics in BVH::build)", who);
    if (n_tris > mipt::kMaxTris) return fail(MIPT_ERR_SCENE_LIMIT, "%u triangles exceed the 2^25 device-format limit", n_tris);
    uint64_t next = 0;
    for (uint32_t p = 0; p < m->n_parts; p++) {
        const MiptMeshPart &q = m->parts[p];
        if (q.reserved != 0u) return fail(MIPT_ERR_INVALID_ARG, "%s: part %u: reserved must be 0", who, p);
        if (q.first_tri != next)
            return fail(MIPT_ERR_INVALID_ARG, "%s: parts must tile the triangles in order: part %u starts at %u, expected %llu", who, p, q.first_tri, (unsigned long long)next);
        next += q.n_tris;
        if (next > n_tris)
            return fail(MIPT_ERR_INVALID_ARG, "%s: parts must tile the triangles in order: part %u ends at %llu of %u triangles", who, p, (unsigned long long)next, n_tris);
        if (n_materials >= 0 && (int64_t)q.material_id >= n_materials)
            return fail(MIPT_ERR_INVALID_ARG, "%s: part %u has material_id %u >= n_materials %lld", who, p, q.material_id, (long long)n_materials);
    }
    if (next != n_tris)
        return fail(MIPT_ERR_INVALID_ARG, "%s: parts must tile the triangles in order: %u parts cover %llu of %u triangles", who, m->n_parts, (unsigned long long)next, n_tris);
    return MIPT_OK;
}

int check_mode(const char *who, uint32_t mode) {
    if (mode != MIPT_UPDATE_REFIT && mode != MIPT_UPDATE_REBUILD)
        return fail(MIPT_ERR_INVALID_ARG, "%s: mode %u is neither MIPT_UPDATE_REFIT nor MIPT_UPDATE_REBUILD", who, mode);
    return MIPT_OK;
}

int bad_position_index(uint32_t entry, uint32_t value, uint32_t n_pos) {
    return fail(MIPT_ERR_INVALID_ARG, "position index %u at index entry %u (triangle %u, corner %u) is out of range: %u positions", value, entry, entry / 3u, entry % 3u, n_pos);
}

int mesh_expand_host(const MiptMeshDesc *m, MiptTriangle *out, uint32_t cap, uint32_t *n_out) {
    if (!m) return fail(MIPT_ERR_INVALID_ARG, "mipt_mesh_expand: null argument");
    { const int rc = check_mesh("mipt_mesh_expand", m, -1); if (rc) return rc; }
    const uint32_t n_tris = m->n_indices / 3u;
    if (n_out) *n_out = n_tris;
    if (!out || cap < n_tris) return fail(MIPT_ERR_INVALID_ARG, "mipt_mesh_expand: room for %u triangles, the mesh has %u", out ? cap : 0u, n_tris);
    const MeshView v{m->positions, m->normals, m->tex_coords, m->indices, m->normal_indices ? m->normal_indices : m->indices,
                     m->tex_coord_indices ? m->tex_coord_indices : m->indices, m->n_positions, m->normals ? m->n_normals : 0u,
                     m->tex_coords ? m->n_tex_coords : 0u, n_tris};
    for (uint32_t p = 0; p < m->n_parts; p++) {
        const MiptMeshPart &q = m->parts[p];
        PartRec r;
        part_record(m->transforms ? m->transforms + (size_t)p * 16 : nullptr, q.first_tri, q.material_id, &r);
        for (uint32_t t = q.first_tri; t < q.first_tri + q.n_tris; t++) {
            uint32_t w[28];
            for (uint32_t c = 0; c < 3u; c++)
                if (!expand_corner(v, r, 3u * t + c, w + 8u * c)) return bad_position_index(3u * t + c, m->indices[3u * t + c], m->n_positions);
            w[24] = r.material_id; w[25] = w[26] = w[27] = 0u;
            memcpy(out + t, w, sizeof w);
        }
    }
    return MIPT_OK;
}

// ---- the resident mesh ----------------------------------------------------------------------------------------------------------
void free_mesh_buffers(SceneMesh *m) {
    if (!m) return;
    void *ptrs[] = {m->d_pos, m->d_nrm, m->d_tex, m->d_idx[0], m->d_idx[1] != m->d_idx[0] ? m->d_idx[1] : nullptr,
                    m->d_idx[2] != m->d_idx[0] ? m->d_idx[2] : nullptr, m->d_parts, m->d_rec[0], m->d_rec[1], m->d_rec[2], m->d_prev_pos, m->d_xf_stage,
                    m->d_flag, m->d_expanded};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    delete m;
}

uint32_t grid_for(size_t n, uint32_t per_block) { return (uint32_t)((n + per_block - 1) / per_block); }

// expansion of the resident mesh -- with `pos` / `nrm` in place of the resident arrays where given -- through PartRec table `rec` into
// d_expanded, queued on `st`; e0 ... e1 = HIP-event time of the kernels once the caller has synchronised on e1
hipError_t queue_expand(const SceneMesh *m, const float *pos, const float *nrm, const float *d_xf, bool new_records, int rec, hipStream_t st, mipt::Event &e0, mipt::Event &e1) {
    hipError_t e = hipEventCreate(e0.put());
    if (e == hipSuccess) e = hipEventCreate(e1.put());
    if (e == hipSuccess) e = hipEventRecord(e0, st);
    if (e != hipSuccess) return e;
    if (new_records) hipLaunchKernelGGL(mesh_prepare_parts, dim3(grid_for(m->n_parts, 64)), dim3(64), 0, st, m->d_parts, m->n_parts, d_xf, m->d_rec[rec]);
    const MeshView v{pos ? pos : m->d_pos, nrm ? nrm : m->d_nrm, m->d_tex, m->d_idx[0], m->d_idx[1], m->d_idx[2], m->n_pos, m->n_nrm, m->n_tex, m->n_tris};
    hipLaunchKernelGGL(mesh_expand, dim3(grid_for(m->n_tris, kT)), dim3(kT), 0, st, v, m->d_rec[rec], m->n_parts, (float4 *)m->d_expanded, m->d_flag);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipEventRecord(e1, st);
    return e;
}

int create_from_mesh(const MiptSceneDesc *desc, const MiptMeshDesc *mesh, int device_id, MiptScene **out) {
    if (!desc || !mesh || !out) return fail(MIPT_ERR_INVALID_ARG, "mipt_scene_create_from_mesh: null argument");
    *out = nullptr;
    { const int rc = check_mesh("mipt_scene_create_from_mesh", mesh, (int64_t)desc->n_materials); if (rc) return rc; }
    {   // the material / texture references, as mipt_scene_create_from_triangles checks them first
        mipt::MaterialTables tables;
        const int rc = mipt::build_material_tables(desc, &tables, false);
        if (rc) return rc;
    }
    const double t_begin = now_ms();
    int ndev = 0;
    {
        const hipError_t e = hipGetDeviceCount(&ndev);
        if (e != hipSuccess) return fail(MIPT_ERR_HIP, "hipGetDeviceCount failed: %s", hipGetErrorString(e));
        if (device_id < 0 || device_id >= ndev) return fail(MIPT_ERR_HIP, "HIP device %d not available (%d visible)", device_id, ndev);
    }
    std::unique_ptr<SceneMesh, void (*)(SceneMesh *)> mesh_owner(new (std::nothrow) SceneMesh(), free_mesh_buffers);
    SceneMesh *const m = mesh_owner.get();
    if (!m) return fail(MIPT_ERR_INVALID_ARG, "out of host memory");
    // Holds the scene only from its creation to the hand-over below, three assignments that cannot fail: it is here so that an exception
    // or a later edit in that window still detaches the mesh from the half-made scene before both go (the mesh once, by its own owner).
    std::unique_ptr<MiptScene, void (*)(MiptScene *)> scene_owner(nullptr, [](MiptScene *p) { p->mesh = nullptr; mipt::free_scene(p); });
    mipt::SyncOnExit sync(mipt::SyncOnExit::kWholeDevice);              // a failure waits for the device, then the scene goes, then the mesh
    MIPT_HIP(hipSetDevice(device_id));
    m->n_pos = mesh->n_positions;
    m->n_nrm = mesh->normals ? mesh->n_normals : 0u;
    m->n_tex = mesh->tex_coords ? mesh->n_tex_coords : 0u;
    m->n_idx = mesh->n_indices; m->n_tris = mesh->n_indices / 3u; m->n_parts = mesh->n_parts;
    m->has_xf = mesh->transforms ? 1u : 0u;
    const size_t pos_b = (size_t)m->n_pos * 12, nrm_b = (size_t)m->n_nrm * 12, tex_b = (size_t)m->n_tex * 8, idx_b = (size_t)m->n_idx * 4,
                 parts_b = (size_t)m->n_parts * sizeof(MiptMeshPart), rec_b = (size_t)m->n_parts * sizeof(PartRec), xf_b = (size_t)m->n_parts * 64,
                 exp_b = (size_t)m->n_tris * sizeof(MiptTriangle);
    // ---- the mesh crosses PCIe once ----
    struct Up { void **dst; const void *src; size_t bytes; };
    const uint32_t *in_idx = mesh->normal_indices && mesh->normal_indices != mesh->indices ? mesh->normal_indices : nullptr;
    const uint32_t *it_idx = mesh->tex_coord_indices && mesh->tex_coord_indices != mesh->indices ? mesh->tex_coord_indices : nullptr;
    const Up ups[] = {{(void **)&m->d_pos, mesh->positions, pos_b}, {(void **)&m->d_nrm, mesh->normals, nrm_b}, {(void **)&m->d_tex, mesh->tex_coords, tex_b},
                      {(void **)&m->d_idx[0], mesh->indices, idx_b}, {(void **)&m->d_idx[1], in_idx, in_idx ? idx_b : 0}, {(void **)&m->d_idx[2], it_idx, it_idx ? idx_b : 0},
                      {(void **)&m->d_parts, mesh->parts, parts_b}, {(void **)&m->d_xf_stage, mesh->transforms, xf_b}};
    for (const Up &u : ups) {
        const bool stage = u.dst == (void **)&m->d_xf_stage;              // allocated even without transforms: mipt_scene_set_transforms fills it
        if (!u.bytes || (!u.src && !stage)) continue;
        MIPT_HIP(hipMalloc(u.dst, u.bytes));
        m->array_bytes += u.bytes;
        if (u.src) { const int rc = mipt::upload_staged(*u.dst, u.src, u.bytes); if (rc) return rc; }
    }
    m->streams = 1u + (m->d_idx[1] ? 1u : 0u) + (m->d_idx[2] ? 1u : 0u);
    if (!m->d_idx[1]) m->d_idx[1] = m->d_idx[0];
    if (!m->d_idx[2]) m->d_idx[2] = m->d_idx[0];
    MIPT_HIP(hipMalloc((void **)&m->d_rec[0], rec_b));
    MIPT_HIP(hipMalloc((void **)&m->d_rec[1], rec_b));
    MIPT_HIP(hipMalloc((void **)&m->d_flag, 4));
    m->array_bytes += 2 * rec_b + 4;
    MIPT_HIP(hipMalloc((void **)&m->d_expanded, exp_b));
    const double t_up = now_ms();
    // ---- expansion; a position index out of range ends the call here ----
    MIPT_HIP(hipMemset(m->d_flag, 0xff, 4));
    float expand_ms = 0.0f;
    {
        mipt::Event e0, e1;
        MIPT_HIP(queue_expand(m, nullptr, nullptr, mesh->transforms ? m->d_xf_stage : nullptr, true, 0, nullptr, e0, e1));
        uint32_t bad = kNoIndex;
        MIPT_HIP(hipMemcpy(&bad, m->d_flag, 4, hipMemcpyDeviceToHost));      // null stream: after the kernels
        (void)hipEventElapsedTime(&expand_ms, e0, e1);
        if (bad != kNoIndex) {
            uint32_t value = 0;
            MIPT_HIP(hipMemcpy(&value, m->d_idx[0] + bad, 4, hipMemcpyDeviceToHost));
            return bad_position_index(bad, value, mesh->n_positions);
        }
    }
    // ---- from here on it is mipt_scene_create_from_triangles with the triangles already in HBM ----
    MiptScene *s = nullptr;
    { const int rc = mipt::scene_create_from_resident_triangles(desc, m->d_expanded, m->n_tris, device_id, &s); if (rc) return rc; }
    scene_owner.reset(s);
    s->mesh = m;
    s->info.upload_ms += t_up - t_begin;
    s->info.build_ms += expand_ms;
    s->info.total_ms = now_ms() - t_begin;
    sync.dismiss();
    mesh_owner.release();                                                // the scene's from here on
    *out = scene_owner.release();
    return MIPT_OK;
}

// One update of a mesh scene: the expansion (from the caller's arrays where given, through new PartRecs where the transforms change),
// the REFIT / REBUILD, and only then the commit.  xf_change: 0 = keep the table, 1 = d_xf holds new matrices, 2 = back to none.
int apply(MiptScene *s, const float *d_pos, const float *d_nrm, const float *d_xf, int xf_change, uint32_t mode, hipStream_t st, MiptUpdateInfo *inf) {
    SceneMesh *m = s->mesh;
    mipt::SyncOnExit sync(st);                                                            // a failure leaves nothing of this update queued on `st`
    MIPT_HIP(hipStreamSynchronize(st));                                                    // ordered after the caller's earlier work on `st`
    int rec = m->cur;                                                                      // new matrices go into a spare table
    if (xf_change) for (rec = 0; rec == m->cur || (m->track && rec == m->prev); rec++) {}
    float expand_ms = 0.0f;
    {
        mipt::Event e0, e1;
        MIPT_HIP(queue_expand(m, d_pos, d_nrm, xf_change == 1 ? d_xf : nullptr, xf_change != 0, rec, st, e0, e1));
        MIPT_HIP(hipStreamSynchronize(st));
        (void)hipEventElapsedTime(&expand_ms, e0, e1);
    }
    { const int rc = mipt::scene_update_device(s, m->d_expanded, m->n_tris, mode, st, inf, true); if (rc) return rc; }
    // ---- commit: with motion tracked, what is resident becomes the previous generation first (its positions are copied unless the
    // copy already holds them; its part table changes roles below) ----
    if (m->track && !m->prev_pos_same)
        MIPT_HIP(hipMemcpyAsync(m->d_prev_pos, m->d_pos, (size_t)m->n_pos * 12, hipMemcpyDeviceToDevice, st));
    if (d_pos) MIPT_HIP(hipMemcpyAsync(m->d_pos, d_pos, (size_t)m->n_pos * 12, hipMemcpyDeviceToDevice, st));
    if (d_nrm) MIPT_HIP(hipMemcpyAsync(m->d_nrm, d_nrm, (size_t)m->n_nrm * 12, hipMemcpyDeviceToDevice, st));
    MIPT_HIP(hipStreamSynchronize(st));
    if (m->track) { m->prev = m->cur; m->prev_pos_same = !d_pos; }
    m->cur = rec;
    if (xf_change) m->has_xf = xf_change == 1 ? 1u : 0u;
    inf->build_ms += expand_ms;
    sync.dismiss();
    return MIPT_OK;
}

int set_transforms(MiptScene *s, const float *xf, uint32_t n_parts, uint32_t mode, MiptUpdateInfo *info) {
    const double t0 = now_ms();
    if (!s) return fail(MIPT_ERR_INVALID_ARG, "mipt_scene_set_transforms: null scene");
    { const int rc = check_mode("mipt_scene_set_transforms", mode); if (rc) return rc; }
    if (!s->mesh) return fail(MIPT_ERR_INVALID_ARG, "mipt_scene_set_transforms: the scene has no mesh (it was not made by mipt_scene_create_from_mesh)");
    SceneMesh *m = s->mesh;
    if (n_parts != m->n_parts)
        return fail(MIPT_ERR_INVALID_ARG, "mipt_scene_set_transforms: %u transforms given, the mesh has %u parts", n_parts, m->n_parts);
    MIPT_HIP(hipSetDevice(s->device));
    if (xf) MIPT_HIP(hipMemcpy(m->d_xf_stage, xf, (size_t)n_parts * 64, hipMemcpyHostToDevice));
    const double t_up = now_ms();
    MiptUpdateInfo inf{};
    { const int rc = apply(s, nullptr, nullptr, m->d_xf_stage, xf ? 1 : 2, mode, nullptr, &inf); if (rc) return rc; }
    inf.upload_ms = t_up - t0;
    inf.total_ms = now_ms() - t0;
    if (info) *info = inf;
    return MIPT_OK;
}

int update_mesh_device(MiptScene *s, const float *d_pos, const float *d_nrm, const float *d_xf, uint32_t mode, hipStream_t st, MiptUpdateInfo *info) {
    const double t0 = now_ms();
    if (!s) return fail(MIPT_ERR_INVALID_ARG, "mipt_scene_update_mesh_device: null scene");
    { const int rc = check_mode("mipt_scene_update_mesh_device", mode); if (rc) return rc; }
    if (!s->mesh) return fail(MIPT_ERR_INVALID_ARG, "mipt_scene_update_mesh_device: the scene has no mesh (it was not made by mipt_scene_create_from_mesh)");
    if (d_nrm && s->mesh->n_nrm == 0u) return fail(MIPT_ERR_INVALID_ARG, "mipt_scene_update_mesh_device: the mesh has no normals to replace");
    MIPT_HIP(hipSetDevice(s->device));
    MiptUpdateInfo inf{};
    { const int rc = apply(s, d_pos, d_nrm, d_xf, d_xf ? 1 : 0, mode, st, &inf); if (rc) return rc; }
    inf.upload_ms = 0.0;
    inf.total_ms = now_ms() - t0;
    if (info) *info = inf;
    return MIPT_OK;
}

int mesh_info(const MiptScene *s, MiptMeshInfo *out) {
    if (!s || !out) return fail(MIPT_ERR_INVALID_ARG, "mipt_scene_mesh_info: null argument");
    if (!s->mesh) return fail(MIPT_ERR_INVALID_ARG, "mipt_scene_mesh_info: the scene has no mesh (it was not made by mipt_scene_create_from_mesh)");
    const SceneMesh *m = s->mesh;
    MiptMeshInfo i{};
    i.n_positions = m->n_pos; i.n_normals = m->n_nrm; i.n_tex_coords = m->n_tex; i.n_indices = m->n_idx;
    i.n_tris = m->n_tris; i.n_parts = m->n_parts; i.has_transforms = m->has_xf; i.index_streams = m->streams;
    i.array_bytes = m->array_bytes + m->track_bytes;
    i.expanded_bytes = (uint64_t)m->n_tris * sizeof(MiptTriangle);
    i.hbm_bytes = i.array_bytes + i.expanded_bytes;
    *out = i;
    return MIPT_OK;
}

int track_motion(MiptScene *s, uint32_t enable) {
    if (!s) return fail(MIPT_ERR_INVALID_ARG, "mipt_scene_track_motion: null scene");
    if (!s->mesh) return fail(MIPT_ERR_INVALID_ARG, "mipt_scene_track_motion: the scene has no mesh (it was not made by mipt_scene_create_from_mesh)");
    SceneMesh *m = s->mesh;
    if ((enable != 0u) == m->track) return MIPT_OK;
    MIPT_HIP(hipSetDevice(s->device));
    const size_t pos_b = (size_t)m->n_pos * 12, rec_b = (size_t)m->n_parts * sizeof(PartRec);
    if (enable) {
        mipt::DevPtr<PartRec> rec;
        mipt::DevPtr<float> pos;
        MIPT_HIP(rec.alloc(m->n_parts));
        MIPT_HIP(pos.alloc((size_t)m->n_pos * 3));
        MIPT_HIP(hipMemcpy(pos.get(), m->d_pos, pos_b, hipMemcpyDeviceToDevice));       // the previous generation = the current one
        m->d_rec[2] = rec.release(); m->d_prev_pos = pos.release();
        m->prev = m->cur; m->prev_pos_same = true;
        m->track_bytes = pos_b + rec_b;
        m->track = true;
    } else {
        MIPT_HIP(hipDeviceSynchronize());                                                // nothing in flight reads what goes
        if (m->cur == 2) { PartRec *t = m->d_rec[0]; m->d_rec[0] = m->d_rec[2]; m->d_rec[2] = t; m->cur = 0; }
        (void)hipFree(m->d_rec[2]); m->d_rec[2] = nullptr;
        (void)hipFree(m->d_prev_pos); m->d_prev_pos = nullptr;
        m->prev = m->cur; m->track_bytes = 0; m->track = false;
    }
    return MIPT_OK;
}

} // namespace

bool mipt::mesh_motion_source(const MiptScene *s, MeshMotionSource *out) {
    if (!s || !s->mesh || !s->mesh->track) return false;
    const SceneMesh *m = s->mesh;
    out->prev_rec = m->d_rec[m->prev]; out->n_parts = m->n_parts;
    out->prev_pos = m->d_prev_pos; out->n_pos = m->n_pos;
    out->idx = m->d_idx[0];
    return true;
}

void mipt::free_mesh(MiptScene *s) {
    if (!s || !s->mesh) return;
    free_mesh_buffers(s->mesh);
    s->mesh = nullptr;
}

extern "C" {

int mipt_mesh_expand(const MiptMeshDesc *mesh, MiptTriangle *out, uint32_t cap, uint32_t *n_out) { MIPT_NO_THROW(mesh_expand_host(mesh, out, cap, n_out)) }

int mipt_scene_create_from_mesh(const MiptSceneDesc *desc, const MiptMeshDesc *mesh, int device_id, MiptScene **out) {
    MIPT_NO_THROW(create_from_mesh(desc, mesh, device_id, out))
}

int mipt_scene_set_transforms(MiptScene *scene, const float *transforms, uint32_t n_parts, uint32_t mode, MiptUpdateInfo *info) {
    MIPT_NO_THROW(set_transforms(scene, transforms, n_parts, mode, info))
}

int mipt_scene_update_mesh_device(MiptScene *scene, const float *d_positions, const float *d_normals, const float *d_transforms, uint32_t mode,
                                  void *hip_stream, MiptUpdateInfo *info) {
    MIPT_NO_THROW(update_mesh_device(scene, d_positions, d_normals, d_transforms, mode, (hipStream_t)hip_stream, info))
}

int mipt_scene_mesh_info(const MiptScene *scene, MiptMeshInfo *out) { MIPT_NO_THROW(mesh_info(scene, out)) }

int mipt_scene_track_motion(MiptScene *scene, uint32_t enable) { MIPT_NO_THROW(track_motion(scene, enable)) }

} // extern "C"
