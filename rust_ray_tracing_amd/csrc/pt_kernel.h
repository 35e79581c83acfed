// pt_kernel.h -- device-side scene layout and launch interface (internal to libmipt.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mipt {

// ---- HBM layout (see DESIGN.md "Data layout") ------------------------------------------
// pairs    : n_pairs x 64 B.  pair k = { nodes[2k+1], nodes[2k+2] } of the reference array
//            (children are always pushed adjacently at odd indices, bvh.rs:121,131-132), each
//            child kept in the reference's Node layout {min.xyz, a, max.xyz, n}: n = num_tris;
//            a = first triangle (leaf) or the PAIR index of its own children (inner).
// tri_pos  : n_tris x 64 B intersection stream {v0.xyz, e1.xyz, e2.xyz, 7 pad words} (a 48-B stride straddles 128-B lines:
//            1.41 memory requests per record instead of 1),
//            e1 = v1 - v0, e2 = v2 - v0 rounded once on the host exactly as ray.rs:24-25 does.
// tri_attr : n_tris x 64 B shading stream {n0,n1,n2 (9 f32), uv0,uv1,uv2 (6 f32), material_id}.
// mats     : n_materials x 64 B {base_color.xyz, emission.xyz} -- the only Material fields cpu/ray.rs:162-176 reads --
//            plus the two textures' {texel offset into `texels`, width, height} inlined; texels = RGBA8 as u32.
// 64 B: the texture descriptors (texel offset, width, height) ride in the material record, so a textured hit costs
// attr -> material -> texel (three dependent fetches) instead of four.  tex_w == 0 means "no texture" (u32::MAX id).
struct DevMaterial {
    float base[3]; uint32_t base_off;
    float emis[3]; uint32_t emis_off;
    uint32_t base_w, base_h, emis_w, emis_h;
    uint32_t pad[4];
};

// 128 B: every Material field the wgpu backend's shader reads (rt_compute.wgsl:41-56) + the six textures' descriptors
// {texel offset, width, height}; width == 0 = no texture.  Order: base, transparency, roughness, metallic, emission, normal.
struct DevMaterialFull {
    float base[3]; float transmission;
    float emission[3]; float ior;
    float roughness, metallic, transparency, pad0;
    uint32_t tex[6][3];
    uint32_t pad1[2];
};

struct DevScene {
    const float4 *pairs;          // = geom: [pairs | tri_pos] live in ONE allocation so the traversal step can address either
    const float4 *tri_pos;        //   through one buffer descriptor with a 32-bit byte offset (tri_off_bytes = n_pairs * 64)
    uint32_t tri_off_bytes, geom_bytes;
    uint32_t tiny_axes;           // bit c: some bounding plane has a coordinate 0 < |p_c| < 2^-76 on axis c (see ray_safe, pt_traverse.h)
    const float4 *tri_attr;
    const DevMaterial *mats;
    const DevMaterialFull *mats_full;   // shading mode 1 (rt_compute.wgsl material model)
    const uint32_t *texels;
    uint32_t n_pairs, n_tris, n_mats, n_texs;
    uint32_t root_a, root_n;      // root node: leaf (root_n > 0: tris [root_a, root_a+root_n)) or inner (pair 0)
};

struct DevStats {                 // zeroed before every launch
    unsigned long long queue;     // next work index
    unsigned long long rays, inner_steps, tri_tests, hits, texel_fetches;
    unsigned long long stack_overflows, tex_clamped, max_stack, pixels;
    // wave-level occupancy diagnostics (COUNT build): traversal iterations, lanes doing inner / leaf work,
    // iterations that ran the inner / leaf branch, service passes, lanes serviced
    unsigned long long d_iters, d_inner_lanes, d_leaf_lanes, d_iters_inner, d_iters_leaf, d_services, d_service_lanes;
    unsigned long long d_cycles_service, d_cycles_total, d_cycles_mem, d_cycles_tail;   // per-wave s_memtime cycles spent in service passes / alive
    unsigned long long touched_geom, touched_attr;                                     // distinct 128-B lines read (MIPT_FLAG_TOUCHED)
};

struct DevParams {
    uint32_t width, height, samples, max_depth;
    uint32_t seed_mode, sample_begin, sum_only, packed;
    uint32_t accumulate;                    // hdr += this call's result (progressive rendering)
    uint32_t cost_packed;                   // pixel_cost != NULL: 1 = a pixel's rays ride in its lane's sample counter and are stored once
                                            // (cost_packs()), 0 = one atomic per path into pixel_cost, which the host has zeroed
    uint32_t tile_rank, tile_world, tiles_x, tiles_y;
    uint32_t n_local_tiles;
    uint32_t n_list;                        // work indices [0, n_list) take slot hot[wi] (0 = no list); pt_kernel.hip "hot pixels"
    unsigned long long total_work;          // n_local_tiles * 64 + n_list, or n_list alone when the list holds every slot
    float aspect;                           // width as f32 / height as f32 (cpu.rs:34)
    float samples_f;
    float cull_scale;                       // 1 + cull_margin
    uint32_t reverse_tiles;                 // hand out the tile list back to front (bottom rows first)
    uint32_t service_num, service_den;      // run the service pass when need/live >= num/den
    uint32_t leaf_period, leaf_den;         // triangle tests run when leaf_period iterations have passed since the last ones or
                                            // 1/leaf_den of the traversing lanes wait for one (pt_kernel.hip "leaf phases"); period 1 = always
    float cam[12];                          // look_at columns 0..2 (xyz each), position
    float *hdr;                             // full-frame or rank-packed, 3 f32 per pixel
    uint32_t *ovf;                          // traversal-stack overflow area [wave][entry][lane]
    DevStats *stats;
    const uint32_t *tile_order;             // local tile handed out at queue position i (NULL = plain order); pt_kernel.hip "tile order"
    uint32_t *pixel_cost;                   // rays traced per slot (local tile * 64 + pixel of the tile), added up by this launch (NULL = not measured)
    const uint32_t *hot;                    // n_list != 0: the n_list most expensive slots of the frame before, in cost order, handed out first ...
    const uint32_t *hot_bits;               // ... and one bit per slot, set for those: the pass over tile_order skips them
    uint32_t *touched;                      // COUNT build + MIPT_FLAG_TOUCHED: one bit per 128-B line of [geom | tri_attr] (else NULL)
    uint32_t touched_attr_base;             // first bit of the tri_attr stream in `touched`
};

// A batch of views (pt_trace_batch_kernel): a separate kernel argument, so the single-view kernels' arguments stay as they are.
struct DevBatch {
    const float4 *cams;                     // n_views x 64 B: {look_at column 0, column 1, column 2, position}, xyz each (w unused)
    uint32_t view_pixels;                   // width * height: the output slots of one view
    uint32_t tiles_recip;                   // floor((2^32 - 1) / n_local_tiles): umulhi(lt, it) is lt / n_local_tiles or up to 2 below
};

// A pixel's cost in its lane's sample counter: the samples done in the low kCostShift bits, the rays of its paths above them.  A
// path traces at most max(max_depth, 1) rays, so neither field overflows where this holds.
constexpr uint32_t kCostShift = 12, kCostSampleMask = (1u << kCostShift) - 1u;
inline bool cost_packs(uint32_t samples, uint32_t max_depth) {
    return samples <= kCostSampleMask && (unsigned long long)samples * ((unsigned long long)max_depth + 1ull) <= (0xffffffffu >> kCostShift);
}
constexpr int kStackLds = 16;               // per-lane traversal-stack entries held in LDS
constexpr int kStackOvf = 48;               // further entries spilled to HBM (rarely touched)
constexpr int kWavesPerBlock = 4;
constexpr uint32_t kTriPosStride = 64;   // bytes per record of the intersection stream: 48 packed, 64 = never straddles a 128-B line
constexpr int kBlockThreads = 64 * kWavesPerBlock;
constexpr uint32_t kMaxTris = 1u << 25;     // stack-entry encoding: 25-bit triangle index
constexpr uint32_t kMaxPairs = 1u << 24;    // 24-bit pair index in the child-ref form

// Launchers (stream-ordered; no allocation, no synchronisation inside).  batch: NULL = one view (camera in pr.cam), else a
// batch of views (pr.total_work covers all of them).
hipError_t launch_trace(const DevScene &sc, const DevParams &pr, const DevBatch *batch, bool count, bool cull, int shading,
                        int grid_blocks, hipStream_t stream);
int trace_blocks_per_cu(bool batch, bool count, bool cull, int shading);     // occupancy query
// The batch launch with a count plane (pt_trace_adaptive_kernel; mipt_render_adaptive*): pixel p of view v runs
// min(counts[v * batch.view_pixels + p], pr.samples) samples; 0 = not traced.  pr and batch as for a batch launch.
hipError_t launch_trace_adaptive(const DevScene &sc, const DevParams &pr, const DevBatch &batch, const uint32_t *counts, bool count, bool cull,
                                 int shading, int grid_blocks, hipStream_t stream);
int trace_adaptive_blocks_per_cu(bool count, bool cull, int shading);        // occupancy query
// The trace launch over the caller's rays (pt_trace_rays_kernel; mipt_query_radiance*): rays = n_rays x 32 B (MiptRay, the last
// word the ray's seed), pr.total_work = n_rays, pr.hdr = n_rays x 3 f32.  Of pr the kernel reads samples, samples_f, max_depth,
// sum_only, accumulate, cull_scale, the schedule, hdr, ovf and stats; everything about a frame, its tiles and its camera is unused.
hipError_t launch_trace_rays(const DevScene &sc, const DevParams &pr, const float4 *rays, bool count, bool cull, int shading,
                             int grid_blocks, hipStream_t stream);
int trace_rays_blocks_per_cu(bool count, bool cull, int shading);            // occupancy query
hipError_t launch_unpack_tiles(const float *packed_all, uint32_t width, uint32_t height,
                               uint32_t tile_world, float *hdr, hipStream_t stream);
hipError_t launch_tonemap(const float *hdr, unsigned long long n_pixels, float divisor,
                          uint8_t *rgba8, hipStream_t stream);

// ---- ray queries (ray_query.hip; mipt_query_closest* / mipt_query_occluded*) ----
struct DevQuery {
    const float4 *rays;                     // n_rays x 32 B (MiptRay): {origin.xyz, t_max}, {direction.xyz, reserved}
    void *out;                              // closest hit: n_rays x 16 B (MiptHit); occlusion: n_rays bytes
    const uint32_t *tri_order;              // tree order -> the caller's order (the scene's d_tri_order); NULL = they are the same
    unsigned long long n_rays;
    float cull_scale;                       // 1 + cull_margin
    uint32_t *ovf;                          // traversal-stack overflow area [wave][entry][lane]
    DevStats *stats;                        // zeroed before the launch; `queue` hands out the ray indices
};
hipError_t launch_ray_query(const DevScene &sc, const DevQuery &q, bool count, bool cull, bool anyhit, int grid_blocks, hipStream_t stream);
int query_blocks_per_cu(bool count, bool cull, bool anyhit);                 // occupancy query

// ---- baking (bake.hip; mipt_bake_texels* / mipt_bake_gather*) ----
struct BakeCtl {                            // counters of one call, zeroed on the stream before its first kernel (32 B)
    unsigned long long covered;             // texels that found an owner
    unsigned long long bad_point;           // the first point whose triangle the scene does not have (all ones = none)
    uint32_t degenerate;                    // triangles whose UV determinant is 0 or not finite
    uint32_t n_huge;                        // triangles handed to the grid-wide coverage kernel (may count past the list's capacity)
    uint32_t pad[2];
};
// The texel pass: the memsets of `owner` (width * height u64) and `ctl`, the coverage kernels over the tree order and the resolve
// kernel that writes width * height 16-B records to `points` (stream-ordered; no allocation, no synchronisation inside).  `huge`:
// huge_cap words of scratch.
hipError_t launch_bake_texels(const DevScene &sc, const uint32_t *tri_order, uint32_t width, uint32_t height, unsigned long long *owner,
                              uint32_t *huge, uint32_t huge_cap, BakeCtl *ctl, void *points, int n_cu, hipStream_t stream);
// inv[the caller's index of the triangle in record q of tri_pos] = q for q < n_tris (tri_order NULL: the tree's order is the caller's)
hipError_t launch_bake_invert_order(const DevScene &sc, const uint32_t *tri_order, uint32_t *inv, int n_cu, hipStream_t stream);
// ctl->bad_point = the lowest i < n whose point names a triangle >= n_tris (ctl zeroed first, bad_point all ones)
hipError_t launch_bake_check_points(const void *points, unsigned long long n, uint32_t n_tris, BakeCtl *ctl, int n_cu, hipStream_t stream);
// One chunk of an entry that traces n * samples paths in chunks (mipt::chunked_trace, mipt_scene.h; the gather: items are surface
// points, bake.hip; the probe bake: items are probes, probe.hip): paths [first_path, first_path + n_paths), path q being sample
// q % samples of item q / samples.  The spans of the items in a chunk: chunk_paths.h.
constexpr uint32_t kCarrySlotWords = 32;    // one carry slot: the gather uses its first 3 words, the probe bake its first 27
struct PathChunk {
    unsigned long long first_path, n_paths;
    uint32_t samples, first_sample, sample_stride;
    uint32_t sum_only, accumulate;
    float samples_f;                        // samples as f32 (cpu.rs:60)
    const float *carry_in;                  // the running sums of the item whose samples began in a chunk before
    float *carry_out;                       // the running sums of the item whose samples go on in the next chunk
};
// rays[j] (n_paths x 32 B, MiptRay with the stream's state after the draws as its seed) for path first_path + j; points: all n
// records (MiptSurfacePoint); inv_order: the caller's triangle index -> its record in tri_pos
hipError_t launch_bake_rays(const DevScene &sc, const void *points, const uint32_t *inv_order, const PathChunk &c, float4 *rays, int n_cu,
                            hipStream_t stream);
// path: n_paths x 3 f32, the chunk's traced radiance; radiance: the caller's n x 3 f32
hipError_t launch_bake_reduce(const void *points, const PathChunk &c, const float *path, float *radiance, int n_cu, hipStream_t stream);
// position[i], normal[i] (3 f32 each; either may be NULL) of point i < n: P and N of the gather, N normalized if `unit`; +0 for no point
hipError_t launch_bake_surface(const DevScene &sc, const void *points, const uint32_t *inv_order, unsigned long long n, bool unit,
                               float *position, float *normal, int n_cu, hipStream_t stream);

// ---- lightmap finishing (lightmap.hip; mipt_lightmap_filter* / mipt_lightmap_dilate*) ----
struct DevLightmapFilter {
    // planar inputs; position / normal NULL = absent (their terms are left out).  out may be radiance.
    const float *radiance, *position, *normal;
    const uint4 *points;                    // the texel records; only `prim` (w) is read
    float *out;
    // the workspace: four float4 planes of width * height each -- two colour planes {r, g, b, covered ? 1 : 0}, position, normal
    float4 *colour[2], *pos4, *nrm4;
    uint32_t width, height, iterations;
    uint32_t tiles_x, tiles_y;              // 64x4-texel tiles per row / per column
    float kc[8], kd[8], kn, kl;             // 1 / sigma^2; colour and distance per iteration (include/mipt.h)
};
// the pack pass and `iterations` filter passes, one launch each (stream-ordered; no allocation, no synchronisation inside)
hipError_t launch_lightmap_filter(const DevLightmapFilter &d, hipStream_t stream);
struct DevLightmapDilate {
    const float *radiance;
    const uint4 *points;
    float *out;
    uint32_t *level;                        // NULL = not wanted
    float4 *state[2];                       // the workspace: two planes of {r, g, b, level as its bits}
    uint32_t width, height, radius;
    uint32_t tiles_x, tiles_y;
};
// the pack pass, `radius` passes and the unpack pass, one launch each (stream-ordered; no allocation, no synchronisation inside)
hipError_t launch_lightmap_dilate(const DevLightmapDilate &d, hipStream_t stream);

// ---- irradiance probes (probe.hip; mipt_probe_bake* / mipt_probe_irradiance*) ----
// rays[j] (n_paths x 32 B, MiptRay: origin P, direction d, the stream's state after the draws as its seed) for path first_path + j;
// probes: all n records (MiptProbe): {x, y, z, seed}
hipError_t launch_probe_rays(const void *probes, const PathChunk &c, float4 *rays, int n_cu, hipStream_t stream);
// path: n_paths x 3 f32, the chunk's traced radiance; rays: what launch_probe_rays wrote; sh: the caller's n x 27 f32
hipError_t launch_probe_project(const PathChunk &c, const float4 *rays, const float *path, float *sh, int n_cu, hipStream_t stream);
struct DevProbeLookup {
    const float *sh;                        // n_probes x 27
    const uint8_t *valid;                   // n_probes, or NULL
    const float *position, *normal;         // n x 3 each
    float *irradiance;                      // n x 3
    unsigned long long n;
    float origin[3], spacing[3];
    uint32_t dims[3];
    uint32_t clamp;
};
hipError_t launch_probe_irradiance(const DevProbeLookup &d, int n_cu, hipStream_t stream);

// ---- first-hit feature buffers (first_hit.hip; mipt_render_features*) ----
struct PartRec;                             // pt_mesh_rule.h
struct DevFeatures {
    const float4 *cams;                     // n_views x 64 B, the records of DevBatch::cams
    // planar outputs, view-major, NULL = not wanted: 1, 1, 1, 3, 2, 3, 3, 3 words per pixel
    float *depth; uint32_t *prim; uint32_t *material; float *position; float *uv; float *normal; float *albedo; float *emission;
    const uint32_t *tri_order;              // tree order -> the caller's order (the scene's d_tri_order); NULL = they are the same
    uint32_t width, height, samples, seed_mode;
    uint32_t sample_begin;                  // first sample number (already normalised 0 -> 1)
    uint32_t tiles_x, n_tiles;              // 8x8 tiles per row / per view
    uint32_t tiles_recip;                   // floor((2^32 - 1) / n_tiles), as DevBatch::tiles_recip
    uint32_t view_pixels;                   // width * height
    unsigned long long total_work;          // n_views * n_tiles * 64
    float aspect;                           // width as f32 / height as f32 (cpu.rs:34)
    float samples_f;                        // samples as f32 (cpu.rs:60)
    float cull_scale;                       // 1 + cull_margin
    uint32_t *ovf;                          // traversal-stack overflow area [wave][entry][lane]
    DevStats *stats;                        // zeroed before the launch; `queue` hands out the work indices
    // ---- the motion pass only (launch_motion; the feature kernels read nothing below) ----
    float *prev_position;                   // 3 words per pixel, view-major
    const float *prev_tris;                 // explicit source: the previous frame's fat triangles (28 words each); NULL = tracked source:
    const PartRec *prev_rec;                //   the previous generation's part table,
    const float *prev_pos;                  //   its position array
    const uint32_t *prev_idx;               //   and the mesh's position index stream
    uint32_t prev_n_parts, prev_n_pos;
};
hipError_t launch_first_hit(const DevScene &sc, const DevFeatures &f, bool count, bool cull, int grid_blocks, hipStream_t stream);
int first_hit_blocks_per_cu(bool count, bool cull);                          // occupancy query
// the motion pass (mipt_render_motion*): first_hit.hip's kernel with the previous-position step; explicit source = f.prev_tris set
hipError_t launch_motion(const DevScene &sc, const DevFeatures &f, bool cull, int grid_blocks, hipStream_t stream);
int motion_blocks_per_cu(bool explicit_source, bool cull);                   // occupancy query

// ---- a-trous denoiser (denoise.hip; mipt_denoise*) ----
struct DevDenoise {
    // planar inputs, view-major; normal / depth / albedo NULL = absent (the term is left out).  out may be hdr.
    const float *hdr, *normal, *depth, *albedo;
    float *out;
    // the workspace: three float4 planes of n_pixels each -- the packed guides {n.x, n.y, n.z, z}, then the two colour planes
    float4 *guides, *colour[2];
    uint32_t width, height, n_views, iterations;
    uint32_t tiles_x, tiles_y;              // 64x4-pixel tiles per row / per column of a view
    float kc[8], kn, kz;                    // 1 / sigma^2, the colour one per iteration (include/mipt.h)
};
// the pack pass and `iterations` filter passes, one launch each (stream-ordered; no allocation, no synchronisation inside)
hipError_t launch_denoise(const DevDenoise &d, hipStream_t stream);

// ---- temporal accumulation (temporal.hip; mipt_temporal*) ----
constexpr uint32_t kTemporalGroupViews = 8;     // views one launch covers: their camera records travel as kernel arguments
struct DevTemporal {
    // planar inputs, view-major; albedo NULL = absent.  out may be hdr.  length / variance NULL = not written.
    const float *hdr, *position, *normal, *depth, *albedo;
    const uint32_t *material;
    float *out, *length, *variance;
    // the histories (include/mipt.h): n_views records of 16 f32, then three float4 planes of n_pixels each.  in NULL = the first frame.
    const float *history_in;
    float *history_out;
    unsigned long long n_pixels;            // n_views * width * height
    uint32_t width, height, n_views;
    uint32_t tiles_x, tiles_y;              // 64x4-pixel tiles per row / per column of a view
    uint32_t view_begin, view_count;        // this launch: views view_begin ... view_begin + view_count - 1 (at most kTemporalGroupViews)
    float alpha_min, max_history, normal_tol, depth_tol;
    float camera[kTemporalGroupViews][16];  // this frame's records of the launch's views, for history_out's header
};
// mipt_temporal_counts*: the plain kernels' arguments, and behind them the plane mipt_render_adaptive was given and its cap.  The
// plain kernels keep DevTemporal as their argument, so nothing of theirs moves.
struct DevTemporalCounts {
    DevTemporal t;
    const uint32_t *counts;                 // one u32 per pixel, view-major
    uint32_t samples_cap;
};
// one launch per group of kTemporalGroupViews views; `records` holds n_views * 16 f32 (stream-ordered; no allocation, no
// synchronisation inside, and `records` is not read after the call returns).  counts NULL = mipt_temporal*: every pixel counts as one
// sample and samples_cap is not used.
hipError_t launch_temporal(DevTemporal d, const float *records, hipStream_t stream, const uint32_t *counts = nullptr, uint32_t samples_cap = 0u);

// ---- variance-guided a-trous filter (denoise_variance.hip; mipt_denoise_variance*) ----
struct DevVariance {
    // planar inputs, view-major; normal / depth / albedo NULL = absent (the term is left out); variance and length NULL together = a
    // single frame without history.  out may be hdr.  variance_out NULL = not written.
    const float *hdr, *normal, *depth, *albedo, *variance, *length;
    float *out, *variance_out;
    // the workspace: three float4 planes of n_pixels each -- the packed guides {n.x, n.y, n.z, z}, then two planes of {r, g, b, var}
    float4 *guides, *colour[2];
    uint32_t width, height, n_views, iterations;
    uint32_t tiles_x, tiles_y;              // 64x4-pixel tiles per row / per column of a view
    float sigma_l, kn, kz;                  // sigma_luminance as given; 1 / sigma^2 of the guides (include/mipt.h)
    float short_history;                    // 0 = the spatial-estimate pass is not launched
};
// the pack pass, the spatial-estimate pass and `iterations` filter passes, one launch each (stream-ordered; no allocation, no
// synchronisation inside)
hipError_t launch_denoise_variance(const DevVariance &d, hipStream_t stream);

// ---- guided upsampling (upsample.hip; mipt_upsample*) ----
struct DevUpsample {
    // planar inputs, view-major: the low frame (lo_width x lo_height) and its guides, then the same guides at full resolution.  A
    // guide is given at both resolutions or at neither (NULL = the term is left out).  weight NULL = not written.
    const float *lo_hdr, *lo_normal, *lo_depth, *lo_albedo;
    const uint32_t *lo_material;
    const float *normal, *depth, *albedo;
    const uint32_t *material;
    float *out, *weight;
    // the workspace: two float4 planes of one entry per LOW pixel -- {c.r, c.g, c.b, bits(lo_material)}, then {n.x, n.y, n.z, z}
    float4 *colour, *guides;
    uint32_t width, height, n_views, scale; // the full frame; lo_width * scale == width, lo_height * scale == height
    uint32_t lo_width, lo_height;
    uint32_t tiles_x, tiles_y;              // 64x4-pixel tiles per row / per column of a full-resolution view
    uint32_t lo_tiles_x, lo_tiles_y;        // and of a low-resolution view
    float kn, kz;                           // 1 / sigma^2 of the guides (include/mipt.h)
};
// the pack pass over the low frame and the upsampling pass over the full frame, one launch each (stream-ordered; no allocation, no
// synchronisation inside)
hipError_t launch_upsample(const DevUpsample &d, hipStream_t stream);

// ---- the sample map (sample_map.hip; mipt_sample_map*) ----
struct SampleMapWork {                      // the workspace, zeroed on the stream before the reduction (32 B)
    unsigned long long sum;                 // S: the sum of every pixel's weight qi
    double ratio;                           // r = E / S, formed once by the last block of the reduction (0 when S == 0)
    uint32_t done, pad[3];                  // blocks of the reduction that have added their part
};
struct DevSampleMap {
    // planar inputs, view-major; hdr NULL = the weight is the standard deviation itself; albedo NULL = hdr is not demodulated
    const float *variance, *hdr, *albedo;
    uint32_t *counts;
    SampleMapWork *work;
    unsigned long long n_pixels;            // N = n_views * width * height
    unsigned long long extra;               // E = T - min_samples * N: the samples to hand out above the floor (include/mipt.h)
    uint32_t min_samples, span;             // span = max_samples - min_samples
    uint32_t uniform_extra;                 // min(E / N, span): every pixel's share when S == 0
};
// the workspace's memset, the reduction and the assignment, one launch each (stream-ordered; no allocation, no synchronisation inside)
hipError_t launch_sample_map(const DevSampleMap &d, hipStream_t stream);
// mipt_sample_map_fill*: one slot per round, all zeroed by one memset.  Slot 0 begins like SampleMapWork, so round 1's sum is
// sample_map.hip's own reduction; slot k - 1 holds what round k's pass reads, left there by round k - 1's pass.
struct SampleMapFillWork {                  // 32 B
    unsigned long long sum;                 // S_k: the sum of qi over the pixels round k may still raise (round 1: over all)
    double ratio;                           // r_k = E_k / S_k, formed once by the last block to add its part
    uint32_t done;                          // blocks that have added their part
    uint32_t active;                        // rounds 2 ...: 1 when S_k != 0 and E_k != 0, else the round changes nothing
    unsigned long long assigned;            // A: the sum of e_{k-1} over all pixels
};
constexpr uint32_t kSampleMapMaxRounds = 8;
// the memset and rounds + 1 launches; d.work is not used, `slots` holds `rounds` slots
hipError_t launch_sample_map_fill(const DevSampleMap &d, SampleMapFillWork *slots, uint32_t rounds, hipStream_t stream);

// order[] = the n tiles by decreasing cost[] (1 024 buckets of rays per path x 16, tile index within a bucket): one block,
// stream-ordered (pt_kernel.hip "tile order").  A tile has 64 x samples paths.
hipError_t launch_tile_order(const uint32_t *cost, uint32_t n_tiles, uint32_t samples, uint32_t *order, hipStream_t stream);
// Hot pixels (pt_kernel.hip "hot pixels"), two launchers around launch_tile_order, stream-ordered.  pixel_cost[] holds rays per slot,
// n_slots of them (a pixel has `samples` paths); `work` is hot_work_words(n_slots) words of scratch shared by the two.
//   launch_pixel_reduce  tile_cost[t] = the sum of pixel_cost[64 t .. 64 t + 64) (NULL = not wanted), and the bucket counts in `work`
//   launch_hot_select    hot[0 .. n_hot) = the n_hot slots of highest cost, by decreasing bucket (1 024 buckets of rays per path x 16),
//                        slot index ascending within a bucket; hot_bits = one bit per slot, (n_slots + 63) / 64 * 2 words, all written.
//                        n_hot <= n_slots; n_hot == n_slots is the complete sort (slots of cost 0, which are no pixels, come last).
size_t hot_work_words(uint32_t n_slots);
hipError_t launch_pixel_reduce(const uint32_t *pixel_cost, uint32_t n_slots, uint32_t samples, uint32_t *tile_cost, uint32_t *work, hipStream_t stream);
hipError_t launch_hot_select(const uint32_t *pixel_cost, uint32_t n_slots, uint32_t samples, uint32_t n_hot, uint32_t *work, uint32_t *hot,
                             uint32_t *hot_bits, hipStream_t stream);
// number of set bits in words [0, n_words) of `bitmap`, added to *out (a device counter)
hipError_t launch_popcount(const uint32_t *bitmap, unsigned long long n_words, unsigned long long *out, hipStream_t stream);
hipError_t launch_divide(float *hdr, unsigned long long n_floats, float divisor, hipStream_t stream);
hipError_t launch_postprocess(const float *hdr, unsigned long long n_pixels, float divisor, uint16_t *rgba16,
                              hipStream_t stream);

} // namespace mipt
