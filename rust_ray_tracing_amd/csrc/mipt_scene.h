// mipt_scene.h -- the device-resident scene behind the opaque MiptScene handle, shared by the translation units that build, change
// and use it -- mipt_api.cpp (host checks, materials, replicas, renders), scene_device.hip (tree and layout built on the GPU),
// bvh_build_device.hip (the builder), scene_update.hip (refit / rebuild), scene_mesh.hip (the resident mesh), mipt_query.cpp (ray
// queries), mipt_features.cpp (first-hit feature buffers), mipt_multi.cpp (one replica per GPU) -- and by the test library's checksum hook (tests/cpp/scene_hooks.hip,
// libmipt_diag.so).  Internal: HIP types, not part of include/mipt.h.  At the end, the launch scaffold of the traversal kernels, which
// works on a scene's workspace.
#pragma once
#include "../../include/mipt.h"
#include "chunk_paths.h"
#include "mipt_host_util.h"
#include "pt_kernel.h"

#include <stddef.h>

#include <memory>
#include <vector>

namespace mipt { struct SceneMesh; }

struct MiptScene {
    int device = 0;
    mipt::DevScene dev{};
    // Every device array, buffer and event below is owned by its member and goes with the scene (mipt::free_scene is `delete`):
    // DevPtr, a fixed array; DevBuf, workspace that grows on demand and knows its size.
    mipt::DevPtr<char> d_geom, d_tri_attr;
    mipt::DevPtr<mipt::DevMaterial> d_mats;
    mipt::DevPtr<mipt::DevMaterialFull> d_mats_full;
    mipt::DevPtr<uint32_t> d_texels;
    // Sizes a replica allocates and copies (clone_issue, replica_refresh): every one is at most what its buffer was allocated with.
    // geom_alloc is the allocation (the payload, dev.geom_bytes, is copied); attr_bytes is allocation and payload; mats_bytes,
    // mats_full_bytes and texel_bytes are the allocations -- the payload, or one record / 16 bytes when that is more.
    size_t geom_alloc = 0, attr_bytes = 0, mats_bytes = 0, mats_full_bytes = 0, texel_bytes = 0;
    uint64_t n_texels = 0;                  // texels in the pool (its payload is n_texels * 4 bytes)
    // a scene whose BVH was built on the device keeps the tree for mipt_scene_get_bvh: nodes in the reference's order and the
    // triangle permutation BVH::build applied (reordered[t] = original[tri_order[t]])
    mipt::DevPtr<MiptNode> d_nodes;
    uint32_t n_nodes = 0;
    mipt::DevPtr<uint32_t> d_tri_order;
    MiptSceneInfo info{};
    // workspace
    mipt::DevPtr<mipt::DevStats> d_stats;
    mipt::DevBuf<uint32_t> d_ovf;           // spill slots of the traversal stack, one set per wave of the largest grid launched so far:
                                            // sized and grown by mipt::traversal_grid (below) and by nothing else
    mipt::DevPtr<uint32_t> d_touched;       // MIPT_FLAG_TOUCHED: line bitmap, allocated on first use
    size_t n_tris = 0;
    mipt::DevBuf<float> d_hdr;
    mipt::DevBuf<uint8_t> d_rgba;
    mipt::DevBuf<float4> d_cams;            // mipt_render_batch*: the camera table (DevBatch::cams), grown on demand
    std::vector<float4> h_cams;             // its host staging copy (outlives the stream-ordered upload)
    // tile order (mipt_api.cpp render_launch, pt_kernel.hip): rays per local tile as the last plain single-view launch measured them,
    // the tiles sorted by that cost, and what that launch was -- {width, height, tile world, tile rank, local tiles, seed mode,
    // samples} and its camera.  A launch with the same key and camera hands its tiles out in that order; any other runs in the plain
    // order and measures.
    mipt::DevBuf<uint32_t> d_tile_cost, d_tile_order;
    uint32_t tile_key[7] = {0, 0, 0, 0, 0, 0, 0};
    float tile_cam[12] = {0};               // DevParams::cam of that launch, compared bit for bit
    bool tile_order_valid = false;          // d_tile_order is the order of d_tile_cost, both of the launch tile_key describes
    bool tile_order_used = false;           // that launch itself handed its tiles out by the order before it (read by the test hook)
    bool tile_order_sorted = false;         // d_tile_order really holds that order: the sort is queued only where a launch can read it
                                            // (a list of every slot leaves the tiles no walk), else the test hook sorts d_tile_cost itself
    // hot pixels, part of the same state (one key, one valid flag): rays per slot (local tile * 64 + pixel of the tile) of that launch,
    // the tile costs being their sums; the hot_n slots of highest cost, which the next launch with the key and camera hands out first,
    // their bitmap (2 words per tile) and the scratch of the selection kernels (mipt::hot_work_words)
    mipt::DevBuf<uint32_t> d_pixel_cost, d_hot, d_hot_bits, d_hot_work;
    bool pixel_cost_clean = false;          // the slots of d_pixel_cost that are no pixels of tile_key's image read 0 (a launch that packs
                                            // its costs writes the pixels' slots alone and zeroes the buffer only where this is false)
    bool cost_atomics = false;              // test hook (mipt_diag_scene_cost_atomics): never pack, one atomic per path as before
    uint32_t hot_n = 0;                     // entries of d_hot (0 = the launch was too large for 32-bit slots: no hot list)
    uint32_t hot_used = 0;                  // entries that launch itself took from the list made before it (0 = it ran without)
    // the list goes on behind its first hot_n entries, in the same cost order: list_n >= hot_n entries of d_hot, all local slots where
    // the compiled-in ratio says so (mipt_api.cpp MIPT_LIST_NUM / DEN); a launch hands out all of them before it walks the tiles
    uint32_t list_n = 0;                    // entries of d_hot in cost order (0 exactly when hot_n is 0)
    uint32_t list_used = 0;                 // entries that launch itself took, hot_used of them as "the hot pixels"
    mipt::DevBuf<void> d_qrays, d_qout;     // the host entries of the queries, radiance queries and bake: staging for items and results (mipt::staged_call)
    // baking (mipt_bake.cpp, bake.hip): the owner word per texel and the list of triangles the whole grid covers (mipt_bake_texels);
    // the counters of a call; the map from the caller's triangle index to its tri_pos record, made on first use and dropped with the tree
    // (release_geometry).  Grown on demand.
    mipt::DevBuf<unsigned long long> d_bake_owner;
    mipt::DevBuf<uint32_t> d_bake_huge;
    mipt::DevBuf<mipt::BakeCtl> d_bake_ctl;
    mipt::DevPtr<uint32_t> d_bake_inv;
    // the entries that trace in chunks (mipt_bake_gather*, mipt_probe_bake*), sized and handed out by mipt::chunked_trace (below) and
    // by nothing else: the ray and radiance staging of one chunk, 32 and 12 B per path, and the two carry slots of an item that spans
    // chunks, kCarrySlotWords each -- a point's 3 running sums or a probe's 27 in the first words of a slot
    mipt::DevBuf<float4> d_bake_rays;
    mipt::DevBuf<float> d_bake_path;
    mipt::DevBuf<float> d_chunk_carry;
    mipt::Event ev0, ev1;
    int n_cu = 0;
    uint32_t max_leaf = 0;
    // REFIT plan of mipt_scene_update_triangles (scene_update.hip), made on the first REFIT and kept until the tree changes: the
    // pair records grouped by depth (record indices, level after level from the root) and, for a scene that keeps its tree
    // (d_nodes), the reference pair index of every record
    mipt::DevPtr<uint32_t> d_refit_plan, d_refit_pair;
    std::vector<uint32_t> refit_level_off;  // level d = plan[off[d], off[d+1]); empty = no plan yet
    // the resident indexed mesh of a scene made by mipt_scene_create_from_mesh (scene_mesh.hip); null for a plain scene
    mipt::SceneMesh *mesh = nullptr;
};

namespace mipt {

void free_scene(MiptScene *s);
struct SceneDeleter { void operator()(MiptScene *s) const { free_scene(s); } };
using ScenePtr = std::unique_ptr<MiptScene, SceneDeleter>;      // a scene under construction: freed unless release()d to the caller
// the resident mesh of `s` (if any) freed, on the current device (scene_mesh.hip); geometry, materials and workspace stay
void free_mesh(MiptScene *s);
// The previous generation of a mesh scene that tracks motion (mipt_scene_track_motion), as the motion pass reads it: the part table
// and the position array of the geometry before the last successful update, and the position index stream.  false: `s` is no
// tracked mesh.
struct PartRec;
struct MeshMotionSource { const PartRec *prev_rec; const float *prev_pos; const uint32_t *idx; uint32_t n_parts, n_pos; };
bool mesh_motion_source(const MiptScene *s, MeshMotionSource *out);
// stats buffer, events, CU count: everything a scene needs besides its geometry.  On failure the scene is left for free_scene.
int scene_finish_workspace(MiptScene *s);
// A replica of `src` in the memory of `device` by device-to-device copies (xGMI between GPUs of a node; a plain copy on the same
// device), queued on `stream` of... the current device is left at `device`.  No host staging.
int scene_clone_to(const MiptScene *src, int device, MiptScene **out);
// outs[1 .. n_dev) = replicas of `src` on device_ids[1 .. n_dev), every copy queued before the first is waited for (seven pulls from
// one GPU run on seven xGMI links at once); all-or-nothing.
int scene_clone_many(const MiptScene *src, const int *device_ids, int n_dev, MiptScene **outs);

// Host tables of a scene's materials and textures (mipt_api.cpp): the 64-B CPU-shading record, the 128-B record of the wgpu
// material model and the texel pool.
struct MaterialTables {
    std::vector<DevMaterial> mats;
    std::vector<DevMaterialFull> mats_full;
    std::vector<uint32_t> texels;             // the pool, when build_material_tables was asked to gather it
    std::vector<uint32_t> tex_offset;         // first texel of texture i in the pool
    uint64_t n_texels = 0;
};
// validates the texture references; gather_texels = false leaves `texels` empty (the caller moves the textures into the pool itself)
int build_material_tables(const MiptSceneDesc *desc, MaterialTables *out, bool gather_texels = true);
// on the current device.  With an empty `texels` the pool is allocated (n_texels) but not filled.
int upload_material_tables(MiptScene *s, const MaterialTables &t);

// ---- who frees what: ResidentBvh and SceneGeometry own their device arrays.  They are move-only, what one still holds when it goes
// out of scope is freed on every outcome, and arrays change hands by a move or release(), never by copying a pointer.  The members of
// MiptScene are owners of the same kind that live as long as the handle: attach_geometry moves a SceneGeometry's arrays into them,
// release_geometry resets those of the geometry, and deleting the scene frees whatever is left (free_scene names none of them).  The
// one exception is MiptScene::mesh, whose arrays scene_mesh.hip still frees by hand (free_mesh). ----
// BVH::build (bvh.rs:13-161) on the GPU with everything staying in HBM (bvh_build_device.hip): `d_tris` in, the node array in the
// reference's order and the triangle permutation out (reordered[t] = original[d_tri_order[t]]).
struct ResidentBvh {
    DevPtr<MiptNode> d_nodes;
    uint32_t n_nodes = 0;
    DevPtr<uint32_t> d_tri_order;
    uint32_t levels = 0;                  // levels the level-synchronous part ran
    double build_ms = 0.0;                // HIP events around the build kernels
};
int bvh_build_resident(const MiptTriangle *d_tris, uint32_t n_tris, int device_id, ResidentBvh *out);
// optional: what the first launch of each builder kernel would pay, up front (call with the device set)
void bvh_builder_resolve_kernels();

// The geometry half of a device-built scene (scene_device.hip): the tree and the layout kernels, from triangles already in HBM --
// what mipt_scene_create_from_triangles / mipt_scene_create run after their upload, and what REBUILD runs on a live scene.
struct SceneGeometry {
    DevPtr<char> d_geom, d_tri_attr;
    size_t geom_alloc = 0, attr_bytes = 0, pairs_bytes = 0, pos_bytes = 0;
    DevPtr<MiptNode> d_nodes;               // the tree and the triangle permutation (BVH::build only; host nodes: null)
    DevPtr<uint32_t> d_tri_order;
    uint32_t n_tris = 0, n_nodes = 0, n_records_padded = 0, max_leaf = 0, tiny_axes = 0, root_a = 0, root_n = 0;
    double build_ms = 0.0, t_build = 0.0;
};
// `bvh` in: with host_nodes, the caller's (validated) node array already in HBM; else empty, filled by the build.  On success `out`
// holds the geometry and, unless host_nodes, the tree (the caller's uploaded nodes are freed: the caller has them on the host).
// No scene is touched; on failure `out` is as it was and `bvh` still holds what the caller put there, or what the build made.
int build_geometry(const MiptTriangle *d_tris, uint32_t n_tris, uint32_t n_materials, int device_id, bool host_nodes, ResidentBvh *bvh,
                   SceneGeometry *out);
// g's buffers become s's (whose own geometry must be freed or moved out first), and the dev / info geometry fields are set
void attach_geometry(MiptScene *s, SceneGeometry &&g);
// the geometry, tree and refit plan of `s` (not its materials or workspace) freed; the MIPT_FLAG_TOUCHED bitmap too (sized by geometry)
void release_geometry(MiptScene *s);
// host -> device copy of a large pageable array through a ring of pinned buffers (scene_device.hip); blocks until it has arrived
int upload_staged(void *d_dst, const void *h_src, size_t bytes);
// mipt_scene_update_triangles_device without the exception fence (scene_update.hip; the host entry: mipt_internal.h)
// expanded_mesh: the call comes from scene_mesh.hip with the expansion of the scene's own mesh (any other caller is refused on a
// scene that owns a mesh: its resident mesh and the triangles would disagree)
int scene_update_device(MiptScene *s, const MiptTriangle *d_tris, uint32_t n_tris, uint32_t mode, hipStream_t stream, MiptUpdateInfo *info,
                        bool expanded_mesh = false);

// ---- the launch scaffold of the traversal kernels (mipt_api.cpp: the trace kernels; mipt_query.cpp: the ray queries;
// mipt_features.cpp: the first-hit feature pass) ----
// Renders, queries and feature passes of one scene share its workspace: d_stats, the events and the spill slots of the traversal stack (d_ovf, one
// set per wave of the grid).  These two functions are the only code that sizes, grows and hands out that workspace.
//
// The grid of a launch: n_cu x blocks_per_cu blocks, at most ceil(work / kBlockThreads), at least 1; the scene's spill slots are
// grown to the grid's wave count (the current device is the scene's).
inline int traversal_grid(MiptScene *scene, int blocks_per_cu, unsigned long long work, int *grid_out) {
    long long grid = (long long)scene->n_cu * blocks_per_cu;
    const long long need_blocks = (long long)((work + kBlockThreads - 1) / kBlockThreads);
    if (grid > need_blocks) grid = need_blocks;
    if (grid < 1) grid = 1;
    const size_t waves = (size_t)grid * kWavesPerBlock;
    *grid_out = (int)grid;
    return scene->d_ovf.grow(waves * (size_t)mipt::kStackOvf * 64 * sizeof(uint32_t));
}

// MIPT_ERR_STACK with the one text every launch that traces reports it in (traversal_launch; chunked_trace over its chunks)
inline int stack_overflow_fail(unsigned long long count) {
    return fail(MIPT_ERR_STACK, "traversal stack overflowed %llu times (capacity %d; the reference panics at 32, ray.rs:85)", count,
                kStackLds + kStackOvf);
}

// One timed launch on `stream`: d_stats zeroed, ev0, launch(), ev1, after_ev1(), the counters copied to `hs`, the stream
// synchronised, `ms` = ev0 ... ev1 (the kernel alone).  `launch` and `after_ev1` queue their work on `stream` and return a status.
// MIPT_ERR_STACK (hs and ms are valid, the results are written) when a traversal stack overflowed.
template <class Launch, class After>
int traversal_launch(MiptScene *scene, hipStream_t stream, Launch launch, After after_ev1, DevStats &hs, float &ms) {
    int rc;
    MIPT_HIP(hipMemsetAsync(scene->d_stats, 0, sizeof(mipt::DevStats), stream));
    MIPT_HIP(hipEventRecord(scene->ev0, stream));
    if ((rc = launch())) return rc;
    MIPT_HIP(hipEventRecord(scene->ev1, stream));
    if ((rc = after_ev1())) return rc;
    MIPT_HIP(hipMemcpyAsync(&hs, scene->d_stats, sizeof hs, hipMemcpyDeviceToHost, stream));
    MIPT_HIP(hipStreamSynchronize(stream));
    MIPT_HIP(hipEventElapsedTime(&ms, scene->ev0, scene->ev1));
    if (hs.stack_overflows) return stack_overflow_fail(hs.stack_overflows);
    return MIPT_OK;
}

// ---- the entries that take a list of work items (mipt_query.cpp, mipt_radiance.cpp, mipt_bake.cpp; their option checks:
// mipt_rays.h) ----
// The buffers of a device entry: the items (`in` null: the entry has none -- the texels), always 16-byte aligned, and the results.
struct ItemBuffers {
    const char *in_name; const void *in; uint64_t in_bytes;
    const char *out_name; const void *out; uint64_t out_bytes; uint32_t out_align;      // out_align 1: any address
    bool refuse_overlap;
    bool zero_first;                    // mipt_bake_gather_device zeroes its stats as soon as both buffers are aligned
};
// A device entry after its argument and option checks, in the order its caller sees: the alignment of the items, then of the results,
// also of an empty list; an empty call is done, with *results (the caller's MiptStats or info, may be null) zeroed; no overlap, where
// the entry refuses it; both buffers memory of the scene's device, which is the first use of the scene; then launch().
template <class Results, class Launch>
int device_call(const char *who, const MiptScene *scene, const ItemBuffers &b, bool no_items, Results *results, Launch launch) {
    if (b.in && ((uintptr_t)b.in & 15u)) return fail(MIPT_ERR_INVALID_ARG, "%s: %s must be 16-byte aligned", who, b.in_name);
    if ((uintptr_t)b.out & (b.out_align - 1u)) return fail(MIPT_ERR_INVALID_ARG, "%s: %s must be %u-byte aligned", who, b.out_name, b.out_align);
    if (results && (no_items || b.zero_first)) memset(results, 0, sizeof *results);
    if (no_items) return MIPT_OK;                                 // no device work
    if (b.refuse_overlap && ranges_overlap(b.in, b.in_bytes, b.out, b.out_bytes))
        return fail(MIPT_ERR_INVALID_ARG, "%s: %s overlaps %s", who, b.in_name, b.out_name);
    int rc;
    if (b.in && (rc = device_buffer_check(who, b.in, scene->device, b.in_name))) return rc;
    if ((rc = device_buffer_check(who, b.out, scene->device, b.out_name))) return rc;
    return launch();
}

// A host entry on the scene's staging pair: d_qrays and d_qout grown, the items (`in` null: none) copied in, launch(d_in, d_out) on the
// null stream, the results copied out.  Both copies block.  MIPT_ERR_STACK from the launch means that the results are there: they are
// fetched and the status is passed on.
template <class Launch>
int staged_call(MiptScene *scene, const void *in, size_t in_bytes, void *out, size_t out_bytes, Launch launch) {
    int rc;
    MIPT_HIP(hipSetDevice(scene->device));
    if (in && (rc = scene->d_qrays.grow(in_bytes))) return rc;
    if ((rc = scene->d_qout.grow(out_bytes < 16 ? 16 : out_bytes))) return rc;
    if (in) MIPT_HIP(hipMemcpy(scene->d_qrays, in, in_bytes, hipMemcpyHostToDevice));
    rc = launch(scene->d_qrays.get(), scene->d_qout.get());
    if (rc && rc != MIPT_ERR_STACK) return rc;
    MIPT_HIP(hipMemcpy(out, scene->d_qout, out_bytes, hipMemcpyDeviceToHost));
    return rc;
}

// The camera table of a launch over `n_views` views: one 64-B record per view {look_at column 0, 1, 2, position} in scene->h_cams,
// scene->d_cams grown to hold it and the copy queued on `stream` (the current device is the scene's).
inline int upload_camera_table(MiptScene *scene, const MiptCamera *cameras, uint32_t n_views, hipStream_t stream) {
    scene->h_cams.assign((size_t)n_views * 4, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    for (uint32_t v = 0; v < n_views; v++) {
        const MiptCamera &c = cameras[v];
        for (int col = 0; col < 3; col++) scene->h_cams[(size_t)v * 4 + col] = make_float4(c.look_at[col][0], c.look_at[col][1], c.look_at[col][2], 0.0f);
        scene->h_cams[(size_t)v * 4 + 3] = make_float4(c.position.x, c.position.y, c.position.z, 0.0f);
    }
    const size_t bytes = scene->h_cams.size() * sizeof(float4);
    const int rc = scene->d_cams.grow(bytes);
    if (rc) return rc;
    MIPT_HIP(hipMemcpyAsync(scene->d_cams, scene->h_cams.data(), bytes, hipMemcpyHostToDevice, stream));
    return MIPT_OK;
}

// *stats = the counters of a trace launch and its kernel time; every other field 0 (touched_lines: mipt_api.cpp adds them)
inline void stats_from_device(const DevStats &hs, float kernel_ms, MiptStats *stats) {
    memset(stats, 0, sizeof *stats);
    stats->kernel_ms = kernel_ms;
    stats->rays = hs.rays; stats->inner_steps = hs.inner_steps; stats->tri_tests = hs.tri_tests;
    stats->hits = hs.hits; stats->texel_fetches = hs.texel_fetches; stats->stack_overflows = hs.stack_overflows;
    stats->tex_clamped = hs.tex_clamped; stats->max_stack = hs.max_stack; stats->pixels = hs.pixels;
    stats->diag[0] = hs.d_iters; stats->diag[1] = hs.d_inner_lanes; stats->diag[2] = hs.d_leaf_lanes;
    stats->diag[3] = hs.d_iters_inner; stats->diag[4] = hs.d_iters_leaf; stats->diag[5] = hs.d_services;
    stats->diag[6] = hs.d_service_lanes; stats->diag[7] = hs.d_cycles_service; stats->diag[8] = hs.d_cycles_total; stats->diag[9] = hs.d_cycles_mem; stats->diag[10] = hs.d_cycles_tail;
}

// The trace launch of mipt_query_radiance_device with every argument already checked (mipt_radiance.cpp); chunked_trace runs it per
// chunk.  d_rays / d_radiance in HBM of the scene's device; blocks until done; MIPT_ERR_STACK with results and stats delivered.
int radiance_launch(MiptScene *scene, const MiptRay *d_rays, uint64_t n_rays, const MiptRadianceOptions *opt, float *d_radiance, hipStream_t stream,
                    MiptStats *stats);

// ---- the entries that trace in chunks (mipt_bake.cpp: the gather; mipt_probe.cpp: the probe bake) ----
// The paths of one trace launch -- 32 + 12 B of staging each -- and the sum of the chunks' counters (max_stack: their maximum;
// kernel_ms is chunked_trace's).
constexpr uint64_t kChunkPaths = 1ull << 22;
inline void add_stats(MiptStats *sum, const MiptStats &c) {
    sum->rays += c.rays; sum->inner_steps += c.inner_steps; sum->tri_tests += c.tri_tests; sum->hits += c.hits;
    sum->texel_fetches += c.texel_fetches; sum->stack_overflows += c.stack_overflows; sum->tex_clamped += c.tex_clamped;
    sum->pixels += c.pixels;
    if (c.max_stack > sum->max_stack) sum->max_stack = c.max_stack;
    for (size_t k = 0; k < sizeof sum->diag / sizeof sum->diag[0]; k++) sum->diag[k] += c.diag[k];
}

// n items x opt.samples paths, n > 0 and every option checked (MiptBakeOptions or MiptProbeBakeOptions), in chunks of at most
// kChunkPaths on `stream`: per chunk gen(chunk, d_rays, stream) writes the chunk's rays, radiance_launch traces them one sample
// each, and fold(chunk, d_rays, d_path, stream) adds the traced radiance to the caller's result per item in sample order; both
// return a hipError_t.  An item that straddles a chunk edge passes its running sums on through the scene's two carry slots
// (chunk_paths.h: carry_slots).  Blocks until done; *stats (may be null) = the chunks' counters and the time from the first kernel
// to the last; MIPT_ERR_STACK with results and stats delivered.
template <class Options, class Gen, class Fold>
int chunked_trace(MiptScene *scene, uint64_t n, const Options &opt, hipStream_t stream, MiptStats *stats, Gen gen, Fold fold) {
    MIPT_HIP(hipSetDevice(scene->device));
    int rc;
    const uint64_t total = n * opt.samples;                               // < 2^63: n < 2^31, samples < 2^32
    const uint64_t chunk = total < kChunkPaths ? total : kChunkPaths;
    if ((rc = scene->d_bake_rays.grow((size_t)chunk * sizeof(MiptRay)))) return rc;
    if ((rc = scene->d_bake_path.grow((size_t)chunk * 12))) return rc;
    if ((rc = scene->d_chunk_carry.grow(2 * kCarrySlotWords * sizeof(float)))) return rc;
    Event ev0, ev1;
    MIPT_HIP(hipEventCreate(ev0.put()));
    MIPT_HIP(hipEventCreate(ev1.put()));
    MIPT_HIP(hipEventRecord(ev0.get(), stream));

    MiptRadianceOptions ro{};
    ro.samples = 1; ro.max_ray_depth = opt.max_ray_depth; ro.traversal = opt.traversal; ro.cull_margin = opt.cull_margin;
    ro.shading = opt.shading; ro.flags = (opt.flags & MIPT_FLAG_COUNT) | MIPT_FLAG_SUM;
    float4 *d_rays = scene->d_bake_rays;
    float *d_path = scene->d_bake_path, *d_carry = scene->d_chunk_carry;
    PathChunk c{};
    c.samples = opt.samples; c.first_sample = opt.first_sample; c.sample_stride = opt.sample_stride;
    c.sum_only = (opt.flags & MIPT_FLAG_SUM) ? 1u : 0u; c.accumulate = (opt.flags & MIPT_FLAG_ACCUM) ? 1u : 0u;
    c.samples_f = (float)opt.samples;                                     // cpu.rs:60
    MiptStats sum{};
    bool stack = false;
    uint64_t index = 0;
    for (uint64_t first = 0; first < total; first += chunk, index++) {
        c.first_path = first; c.n_paths = total - first < chunk ? total - first : chunk;
        const CarrySlots slots = carry_slots(index);                      // chunk_paths.h
        c.carry_in = d_carry + kCarrySlotWords * slots.in; c.carry_out = d_carry + kCarrySlotWords * slots.out;
        MIPT_HIP(gen(c, d_rays, stream));
        MiptStats st;
        rc = radiance_launch(scene, (const MiptRay *)d_rays, c.n_paths, &ro, d_path, stream, &st);
        if (rc && rc != MIPT_ERR_STACK) return rc;
        stack = stack || rc == MIPT_ERR_STACK;
        add_stats(&sum, st);
        MIPT_HIP(fold(c, d_rays, d_path, stream));
    }
    MIPT_HIP(hipEventRecord(ev1.get(), stream));
    MIPT_HIP(hipStreamSynchronize(stream));
    float ms = 0.0f;
    MIPT_HIP(hipEventElapsedTime(&ms, ev0.get(), ev1.get()));
    sum.kernel_ms = ms;
    if (stats) *stats = sum;
    if (stack) return stack_overflow_fail(sum.stack_overflows);
    return MIPT_OK;
}

// ---- the first-hit passes (mipt_features.cpp: the feature buffers; mipt_motion.cpp: previous positions) ----
// the checks that concern neither the buffers nor a device; `buffers` is only tested for null.  count_allowed: MIPT_FLAG_COUNT passes
int first_hit_check(const char *who, const MiptScene *scene, const MiptCamera *cameras, uint32_t n_views, const MiptOptions *opt,
                    const void *buffers, bool count_allowed);
// the frame constants, the grid and the camera table of a launch, on `stream`; the output pointers of `f` are the caller's to set
int first_hit_setup(MiptScene *scene, const MiptCamera *cameras, uint32_t n_views, const MiptOptions *opt, int blocks_per_cu,
                    hipStream_t stream, DevFeatures *f, int *grid_out);

} // namespace mipt
