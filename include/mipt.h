/*
 * mipt.h -- C ABI of the MI355X path-tracing backend (libmipt.so).
 *
 * This is the drop-in boundary for the reference's renderer seam: the
 * `match self.options.backend` in Renderer::render (reference src/renderer.rs:57-63)
 * whose arms all have the shape (Renderer, &Scene) -> Vec<u8>
 * (src/renderer/backend/cpu.rs:13, src/renderer/backend/gpu.rs:14).  A third arm
 * `RendererBackend::MI355X` calls mipt_scene_create / mipt_render / mipt_scene_destroy
 * (binding shown in INTEGRATION.md).  The payload is exactly what the reference's wgpu
 * backend already ships to a device (src/renderer/backend/gpu.rs:329-339,356-367,455-459):
 * bytemuck::Pod arrays of Triangle (112 B), Node (32 B), Material (80 B), RGBA8 textures
 * and the 80-byte UniformCamera.
 *
 * Conventions: plain pointers and sizes, no C++ or torch types; every entry point returns
 * 0 on success or a negative MiptStatus and never unwinds or aborts across the ABI; the
 * message for the last failure on the calling thread is mipt_last_error().  Inputs are
 * borrowed for the duration of the call only (mipt_scene_create copies to HBM); output
 * buffers are caller-allocated.  The library fails loudly (MIPT_ERR_HIP) when no gfx950
 * device or code object is available: there is no CPU fallback inside libmipt.so.
 */
#ifndef MIPT_H
#define MIPT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIPT_ABI_VERSION 4

/* libmipt.so is built with -fvisibility=hidden: exactly the functions declared here are exported
 * (tests/test_abi.py compares `nm -D --defined-only` with this header). */
#if defined(__GNUC__)
#define MIPT_API __attribute__((visibility("default")))
#else
#define MIPT_API
#endif

/* ---- PODs, byte-identical to the reference's #[repr(C, align(16))] structs ---------- */
typedef struct { float x, y, z; } MiptVec3;                 /* src/math/vec3.rs:55-59  (12 B) */

typedef struct {                                            /* src/scene.rs:87-94      (32 B) */
    MiptVec3 position; float tex_coord_x;
    MiptVec3 normal;   float tex_coord_y;
} MiptVertex;

typedef struct {                                            /* src/scene.rs:97-103    (112 B) */
    MiptVertex vertices[3];
    uint32_t   material_id;
    uint8_t    _pad[12];
} MiptTriangle;

typedef struct {                                            /* src/bvh.rs:164-171      (32 B) */
    MiptVec3 bounds_min; uint32_t first_tri_or_child;
    MiptVec3 bounds_max; uint32_t num_tris;                 /* leaf iff num_tris > 0 */
} MiptNode;

typedef struct {                                            /* src/scene.rs:129-146    (80 B) */
    MiptVec3 base_color;    float transmission;
    MiptVec3 specular_tint; float ior;
    MiptVec3 emission;      float roughness;
    float    metallic, transparency;
    uint32_t base_color_tex_id, transparency_tex_id, roughness_tex_id,
             metallic_tex_id, emission_tex_id, normal_tex_id;   /* UINT32_MAX = none */
} MiptMaterial;

typedef struct {                                            /* src/renderer/backend/gpu.rs:480-486 (80 B) */
    float    look_at[4][4];                                 /* Mat4f data[col][row], src/math/mat4.rs:6-10 */
    MiptVec3 position; float _pad;
} MiptCamera;

typedef struct {                                            /* src/texture.rs:4-10; payload as gpu.rs:360-367 */
    uint32_t width, height;
    const uint8_t *rgba8;                                   /* width*height*4 bytes, rows as stored by Texture::load (v-flipped) */
} MiptTexture;

typedef struct {                                            /* what StorageBuffers::new uploads, gpu.rs:329-391 */
    const MiptTriangle *tris;      uint32_t n_tris;
    const MiptNode     *nodes;     uint32_t n_nodes;        /* BVH::build output, src/bvh.rs:13-54 */
    const MiptMaterial *materials; uint32_t n_materials;    /* indexed by Triangle.material_id */
    const MiptTexture  *textures;  uint32_t n_textures;
} MiptSceneDesc;

typedef struct MiptScene MiptScene;                         /* opaque, device-resident */

/* ---- options: RendererOptions (src/renderer.rs:96-104) + what the MI355X path adds ---- */
enum MiptSeedMode {
    MIPT_SEED_PIXEL_STREAM = 0,  /* cpu.rs:28-29: one xorshift stream per pixel, all samples in sequence */
    MIPT_SEED_PER_SAMPLE   = 1   /* rt_compute.wgsl:102: reseed per (sample, x, y); splittable by sample */
};
enum MiptTraversal {
    MIPT_TRAVERSAL_REFERENCE = 0, /* cpu/ray.rs:69-81: slab test without t-max cull (the CPU backend) */
    MIPT_TRAVERSAL_CULLED    = 1  /* rt_compute.wgsl:341-349: + `t_near < best*(1+cull_margin)` cull (margin 0 = the wgpu backend's rule) */
};
/* Best-hit culling is not result-identical to the CPU backend at margin 0: Moller-Trumbore is not
 * watertight, so a ray on a shared edge can hit both neighbours with distances one ulp apart, and
 * culling the second leaf (slab t_near >= best) keeps the first-found instead of the closest
 * (measured: ~1e-5 of rays on the 10 M-triangle scene).  A relative margin keeps every near-tie
 * candidate in play; with 2^-7 the culled frame is bit-identical to the reference traversal on
 * every scene tested (tests/, bench.py re-checks it on each run) at +1 % node visits. */
#define MIPT_CULL_MARGIN_SAFE 0.0078125f
enum MiptShading {
    MIPT_SHADING_CPU  = 0,        /* cpu/ray.rs:141-202: the rayon backend's trace (the parity target) */
    MIPT_SHADING_WGPU = 1         /* rt_compute.wgsl:126-294: the wgpu shader's material model (GGX-VNDF specular, Schlick Fresnel,
                                   * refraction + Beer absorption, alpha cut-out, Russian roulette from depth 4, normal maps,
                                   * bilinear/repeat textures with 2.2 gamma); per-sample seeds always (rt_compute.wgsl:102) */
};
enum MiptFlags {
    MIPT_FLAG_COUNT  = 1u << 0,   /* counting build: fill rays / inner_steps / tri_tests / ... in MiptStats */
    MIPT_FLAG_PACKED = 1u << 1,   /* tile-sharded output is rank-packed (tile-major) instead of full-frame */
    MIPT_FLAG_SUM    = 1u << 2,   /* hdr = sum over samples (no division): sample-sharded accumulation */
    MIPT_FLAG_ACCUM  = 1u << 3,   /* with SUM, device buffers only: hdr += this call's samples (progressive rendering,
                                   * the resumable form of the per-sample loop at gpu.rs:17-77) */
    MIPT_FLAG_TOUCHED = 1u << 4   /* with COUNT: also mark every 128-byte line of the BVH / triangle streams the launch reads in a
                                   * device bitmap and report the number of distinct lines (MiptStats.touched_lines): the
                                   * compulsory memory traffic of the frame.  Diagnostic: slows the counting launch down */
};

typedef struct {
    uint32_t width, height;       /* output_image_dimensions, renderer.rs:100 */
    uint32_t samples;             /* renderer.rs:98  (> 0) */
    uint32_t max_ray_depth;       /* renderer.rs:99  (> 0) */
    uint32_t seed_mode;           /* MiptSeedMode */
    uint32_t traversal;           /* MiptTraversal */
    uint32_t flags;               /* MiptFlags */
    uint32_t tile_rank;           /* image-tile shard: this rank ...                        */
    uint32_t tile_world;          /* ... of this many (0 or 1 = whole image); 8x8 tiles, round-robin */
    uint32_t sample_begin;        /* PER_SAMPLE: first sample number (0 -> 1, as gpu.rs:252 starts at 1) */
    float    cull_margin;         /* MIPT_TRAVERSAL_CULLED: relative margin (>= 0); see MIPT_CULL_MARGIN_SAFE */
    uint32_t shading;             /* MiptShading */
    uint32_t reserved[4];         /* must be 0 */
} MiptOptions;

typedef struct {
    double   kernel_ms;           /* HIP-event time of the trace kernel on its launch stream */
    uint64_t rays;                /* traverse_bvh invocations (ray.rs:150) [COUNT] */
    uint64_t inner_steps;         /* inner-node visits, two child records each [COUNT] */
    uint64_t tri_tests;           /* intersect_tri calls [COUNT] */
    uint64_t hits;                /* rays that hit [COUNT] */
    uint64_t texel_fetches;       /* Texture::color_at calls [COUNT] */
    uint64_t stack_overflows;     /* pushes dropped: traversal stack full (reference panics, ray.rs:85) */
    uint64_t tex_clamped;         /* texel index clamped (reference panics, texture.rs:37) */
    uint64_t max_stack;           /* deepest stack occupancy [COUNT] */
    uint64_t pixels;              /* pixels this call produced */
    /* wave-occupancy diagnostics [COUNT]: traversal iterations (per wave); sum of lanes on an inner step; sum of lanes on
     * a leaf step; iterations that executed the inner branch; the leaf branch; service passes; lanes serviced;
     * wave-cycles inside service passes; wave-cycles alive; wave-cycles waiting for the traversal loads (only in a
     * -DMIPT_DIAG_STAMPS=1 build); wave-cycles between a wave first finding the queue empty and its exit (tail) */
    uint64_t diag[11];
    /* [COUNT | TOUCHED] distinct 128-byte lines read: [0] of the BVH pair records + triangle intersection stream (one
     * allocation), [1] of the triangle attribute stream.  x 128 = the bytes a launch must move at least once. */
    uint64_t touched_lines[2];
} MiptStats;

enum MiptStatus {
    MIPT_OK = 0,
    MIPT_ERR_INVALID_ARG   = -1,  /* renderer.rs:15-26 invariants, null pointers, bad ranges */
    MIPT_ERR_HIP           = -2,  /* HIP runtime error / no gfx950 device */
    MIPT_ERR_SCENE_LIMIT   = -3,  /* scene exceeds device-format limits */
    MIPT_ERR_BVH           = -4,  /* malformed BVH handed to mipt_scene_create */
    MIPT_ERR_IO            = -5,  /* file not found / parse error (OBJ loader) */
    MIPT_ERR_STACK         = -6,  /* traversal stack overflowed during render (result incomplete) */
    MIPT_ERR_RCCL          = -7   /* RCCL communicator / collective error (mipt_render_multi) */
};

/* ---- the seam ----------------------------------------------------------------------- */

/* Copies the scene to HBM of HIP device `device_id`, re-basing the BVH into 64-byte child-pair
 * records and splitting triangles into an intersection stream (40 B of payload -- v0, e1, e2 and the triangle's
 * reference index -- at a 64-byte stride, so a record never straddles a 128-byte line) and a 64-byte shading stream.  The tree is
 * validated on the host first (MIPT_ERR_BVH / _SCENE_LIMIT / _INVALID_ARG before any device call); triangles and nodes then cross PCIe
 * once and the layout is produced by GPU kernels (10 M triangles: 0.07 s).  Replaces State::new / StorageBuffers::new (gpu.rs:96-118, 329-401). */
MIPT_API int mipt_scene_create(const MiptSceneDesc *desc, int device_id, MiptScene **out);
MIPT_API void mipt_scene_destroy(MiptScene *scene);

/* The same scene from its TRIANGLES alone -- desc->nodes / n_nodes are ignored (may be NULL / 0): BVH::build (bvh.rs:13-161) runs on
 * the GPU and everything after the one host -> device copy of the triangle array stays in HBM: the node array in the reference's
 * order, the re-based pair records, both triangle streams.  The tree, the triangle order and every byte of the device layout are
 * identical to mipt_bvh_build + mipt_scene_create (sign of zero in a bound aside); only the time differs (10 M triangles: ~0.08 s
 * against ~10 s of host build or 1.3 s of mipt_bvh_build_device + mipt_scene_create).  The triangle array is read in the caller's
 * order and not modified; mipt_scene_get_bvh returns what BVH::build would have left in the host's Scene. */
MIPT_API int mipt_scene_create_from_triangles(const MiptSceneDesc *desc, int device_id, MiptScene **out);

/* The tree of a scene made by mipt_scene_create_from_triangles: nodes_out receives the node array (BVH::build's output, nodes_cap >=
 * 2 * n_tris - 1 is always enough), tri_order_out (n_tris entries, may be NULL) the permutation bvh.rs:99-108 applied to the
 * triangles: reordered[t] = original[tri_order_out[t]].  MIPT_ERR_INVALID_ARG for a scene made from host-built nodes. */
MIPT_API int mipt_scene_get_bvh(MiptScene *scene, MiptNode *nodes_out, uint32_t nodes_cap, uint32_t *n_nodes_out, uint32_t *tri_order_out);

/* What a scene holds and what it took to get it there (host clock, ms; build_ms: HIP events). */
typedef struct {
    uint32_t n_tris, n_nodes;
    uint32_t n_pair_records;      /* 64-byte pair records incl. line padding */
    uint32_t max_leaf;            /* largest leaf (triangles) */
    uint64_t geometry_bytes;      /* pair records + both triangle streams in HBM */
    uint32_t built_on_device;     /* 1: mipt_scene_create_from_triangles */
    uint32_t replica_of_device;   /* for a replica made by device-to-device copy: the source device ordinal + 1; else 0 */
    double   upload_ms;           /* host -> device copies (geometry + materials + textures) */
    double   build_ms;            /* device BVH build, kernels only; 0 for host-built nodes */
    double   layout_ms;           /* device layout: host re-layout (mipt_scene_create) or layout kernels */
    double   total_ms;            /* the whole create call */
} MiptSceneInfo;
MIPT_API int mipt_scene_info(const MiptScene *scene, MiptSceneInfo *out);

/* Renders into HOST buffers and blocks until done.  Replaces cpu::render_scene
 * (cpu.rs:13-68) / gpu::render_scene_to_buffer (gpu.rs:14-94).
 *   hdr_rgb : width*height*3 f32, linear mean radiance per pixel (the value cpu.rs:60 holds
 *             before sRGB), row 0 = top; may be NULL.
 *   rgba8   : width*height*4 bytes, exactly the Vec<u8> cpu.rs:63-67 returns; may be NULL. */
MIPT_API int mipt_render(MiptScene *scene, const MiptCamera *camera, const MiptOptions *opt,
                float *hdr_rgb, uint8_t *rgba8, MiptStats *stats);

/* Same, into DEVICE buffers (e.g. torch tensors), launched on `hip_stream` (hipStream_t, may
 * be NULL = the null stream).  Blocks until the kernel has finished (stats are read back).
 * With tile sharding and MIPT_FLAG_PACKED, d_hdr_rgb holds mipt_packed_pixels() * 3 floats. */
MIPT_API int mipt_render_device(MiptScene *scene, const MiptCamera *camera, const MiptOptions *opt,
                       float *d_hdr_rgb, uint8_t *d_rgba8, void *hip_stream, MiptStats *stats);

/* ---- many views of one scene in one launch ------------------------------------------------------------------------------
 * Renders n_views cameras of the same scene with the same options in ONE trace launch whose work queue runs over (view, tile,
 * pixel), so a batch of small views fills the GPU the way one large frame does.  Pixel seeds depend on the pixel position and the
 * sample number only (cpu.rs:28-29, rt_compute.wgsl:102), never on the launch: every view comes out bit-identical to a single render.
 *   cameras : n_views cameras in HOST memory, read during the call only.
 *   opt     : applies to every view; the per-frame rules of mipt_render apply per view.  tile_world must be 0 or 1 and
 *             MIPT_FLAG_PACKED is refused (a batch is not tile-sharded); MIPT_FLAG_SUM, MIPT_FLAG_ACCUM (device entry only),
 *             sample_begin, MIPT_FLAG_COUNT and MIPT_FLAG_TOUCHED work as in the single-view calls.
 *   output  : view-major.  View v occupies hdr[v*W*H*3 .. (v+1)*W*H*3) and rgba8[v*W*H*4 .. (v+1)*W*H*4) (W, H = opt->width,
 *             opt->height); each slice holds exactly the bytes mipt_render / mipt_render_device writes for cameras[v] with the same
 *             opt, in both seed modes, both traversal modes and both shading modes.  mipt_tonemap_device / mipt_postprocess_device
 *             over n_views*W*H pixels give the per-view results of the whole batch.
 *   limit   : n_views*W*H < MIPT_BATCH_MAX_PIXELS (2^32), else MIPT_ERR_INVALID_ARG.
 *   stats   : the one launch: kernel_ms is its HIP-event time, the counters are summed over the views (max_stack: the maximum),
 *             pixels = n_views*W*H.
 * Every argument is checked before any device work; errors set mipt_last_error(), and the scene renders as before afterwards.
 * MIPT_ERR_STACK is reported after the frame is written, as by mipt_render. */
#define MIPT_BATCH_MAX_PIXELS 4294967296ull
MIPT_API int mipt_render_batch(MiptScene *scene, const MiptCamera *cameras, uint32_t n_views, const MiptOptions *opt,
                               float *hdr_rgb, uint8_t *rgba8, MiptStats *stats);
/* Same, into DEVICE buffers (d_hdr_rgb: n_views*W*H*3 f32, required; d_rgba8: n_views*W*H*4 bytes, may be NULL) on `hip_stream`
 * (may be NULL); the camera table is copied on that stream.  Blocks until the kernel has finished (stats are read back). */
MIPT_API int mipt_render_batch_device(MiptScene *scene, const MiptCamera *cameras, uint32_t n_views, const MiptOptions *opt,
                                      float *d_hdr_rgb, uint8_t *d_rgba8, void *hip_stream, MiptStats *stats);

/* ---- ray queries: closest hit and occlusion for the caller's rays -----------------------------------------------------------
 * The traversal of the trace kernel, Ray::traverse_bvh (cpu/ray.rs:84-139), run over rays the caller supplies instead of camera
 * and scatter rays (csrc/ray_query.hip).  Nothing is generated or shaded: rays in, hits out.
 *
 * Closest hit.  hits[i] is exactly what traverse_bvh leaves in hit_info for ray i when hit_info.distance starts at rays[i].t_max
 * (t_max = 1e30f: the reference call itself): the reference's visit order (nearer child first, the other pushed; the root is not
 * slab-tested); a triangle replaces the hit iff has_hit && t < distance -- strict, so among equal t the first in visit order stays
 * (SURVEY T6); has_hit in the negated-OR form of ray.rs:56-59 (a NaN u or v passes, a NaN t fails); one rounded f32 operation per
 * operator, nothing fused.  t, u, v are the bits intersect_tri computed for the winning triangle (a NaN that this arithmetic
 * produces -- u or v of a degenerate winner -- is a NaN everywhere; its sign and payload are the implementation's, as in IEEE 754:
 * gfx950 and an x86 host differ there).  The direction is used as given
 * (not normalised: t is in units of its length).  Zero, denormal, huge, infinite or NaN components neither trap nor hang: such a
 * ray takes IEEE divisions in the slab test instead of the exact reciprocal path and returns what the reference arithmetic returns.
 *
 * prim.  The index of the triangle in the array the scene was last built from -- "the caller's order" of the update section below:
 * the tree order passed to mipt_scene_create; for scenes built on the device (mipt_scene_create_from_triangles / _from_mesh, or
 * after a REBUILD) the caller's own order, i.e. tri_order_out[tree index] of mipt_scene_get_bvh.
 *
 * Occlusion.  occluded[i] = 1 iff some triangle the traversal tests has has_hit && t < t_max, else 0; a ray stops at its first
 * such triangle.  MIPT_TRAVERSAL_REFERENCE tests every triangle whose leaf the un-culled slab tests reach, whatever the order.
 * With MIPT_TRAVERSAL_CULLED a child is skipped iff !(t_near < t_max * (1 + cull_margin)): the bound stays at t_max, so the answer
 * does not depend on the order either.
 *
 * Options (NULL = all zero): traversal / cull_margin as in MiptOptions (closest hit culls against the shrinking
 * best * (1 + cull_margin), as the trace kernel does); flags: MIPT_FLAG_COUNT only.  stats (may be NULL): kernel_ms and
 * stack_overflows always; with MIPT_FLAG_COUNT also rays, inner_steps, tri_tests, hits (rays that hit / are occluded) and
 * max_stack; every other field 0.
 *
 * Errors.  Checked before any device work, MIPT_ERR_INVALID_ARG with a message in mipt_last_error(): a null scene, rays or output;
 * n_rays >= MIPT_QUERY_MAX_RAYS; an unknown traversal or flag; a negative or non-finite cull_margin; non-zero reserved option
 * fields; for the _device entries rays / hits not 16-byte aligned, or a pointer that is not device memory of the scene's device.
 * n_rays == 0 is MIPT_OK without a launch.  A traversal-stack overflow (more than 64 entries) is MIPT_ERR_STACK after the results
 * are written, as in mipt_render.  After any error the scene renders and queries as before.
 *
 * The _device entries take buffers in HBM of the scene's device (e.g. torch tensors), are ordered after the earlier work of
 * `hip_stream` (hipStream_t, NULL = the null stream) and block until done, like mipt_render_device.  Queries see the geometry of
 * the last successful update (REFIT, REBUILD, mipt_scene_set_transforms, mipt_scene_update_mesh_device) and work on a replica
 * handle from mipt_multi_scene. */
typedef struct { float origin[3]; float t_max; float direction[3]; uint32_t reserved; } MiptRay;   /* 32 B; reserved is ignored here (mipt_query_radiance: the seed) */
typedef struct { float t, u, v; uint32_t prim; } MiptHit;                                          /* 16 B */
#define MIPT_HIT_NONE        0xffffffffu   /* prim of a miss; then t = 1e30f (HitInfo::default, ray.rs:214-226), u = v = 0 */
#define MIPT_HIT_FRONT_FACE  0x80000000u   /* bit 31 of prim: det > 0 (ray.rs:39); triangle = prim & 0x01ffffff */
typedef struct { uint32_t traversal; float cull_margin; uint32_t flags; uint32_t reserved[5]; } MiptQueryOptions;  /* NULL = all zero */
#define MIPT_QUERY_MAX_RAYS 2147483648ull

MIPT_API int mipt_query_closest(MiptScene *scene, const MiptRay *rays, uint64_t n_rays, const MiptQueryOptions *opt,
                                MiptHit *hits, MiptStats *stats);
MIPT_API int mipt_query_closest_device(MiptScene *scene, const MiptRay *d_rays, uint64_t n_rays, const MiptQueryOptions *opt,
                                       MiptHit *d_hits, void *hip_stream, MiptStats *stats);
MIPT_API int mipt_query_occluded(MiptScene *scene, const MiptRay *rays, uint64_t n_rays, const MiptQueryOptions *opt,
                                 uint8_t *occluded, MiptStats *stats);
MIPT_API int mipt_query_occluded_device(MiptScene *scene, const MiptRay *d_rays, uint64_t n_rays, const MiptQueryOptions *opt,
                                        uint8_t *d_occluded, void *hip_stream, MiptStats *stats);

/* ---- radiance queries: path-traced radiance along the caller's rays ------------------------------------------------------------
 * "How much light arrives along my ray": the trace loop of the renders (csrc/pt_kernel.hip) with the caller's rays in place of a
 * camera -- what a lightmap or vertex baker, an irradiance-probe grid or a radiance cache asks of a resident scene.  Rays in, one
 * RGB radiance per ray out.
 *
 * The ray.  origin and direction are used as given: the direction is not normalised, as in the queries above (the reference's
 * camera rays are unit vectors; a scatter ray is normalised by Ray::trace itself, so only the first segment sees the caller's
 * length).  t_max is ignored: every segment of a path starts from HitInfo::default (ray.rs:214-226), as Ray::trace does.  The
 * fourth word of the record's second half -- `reserved` of MiptRay, still ignored by the two queries above -- is this ray's SEED,
 * a u32.
 *
 * The value, shading = MIPT_SHADING_CPU.  rng = seed; then `samples` times Ray::trace(ray, max_ray_depth, rng) (ray.rs:141-202) on
 * that one xorshift stream, which continues from sample to sample; the results are summed in f32, in order, from +0, and the sum is
 * divided by (float)samples unless MIPT_FLAG_SUM is set.  This is cpu.rs:52,60 with the camera ray of cpu.rs:37-50 replaced by the
 * caller's: no jitter draws, no camera matrix.
 *
 * The value, shading = MIPT_SHADING_WGPU.  The same with `trace` of rt_compute.wgsl:126-229.  The per-sample reseed of
 * rt_compute.wgsl:102 does NOT happen -- there is no pixel to seed from: the stream continues from sample to sample here too.
 *
 * The seed is used as given.  Seed 0 is a stuck xorshift stream (every draw 0), exactly as it would be in the reference: give every
 * ray a non-zero seed, and rays that should be independent different ones.  (The pixel formula of cpu.rs:28-29,
 * 987612486 * (i + 87636354) mod 2^32, is what the Python wrapper hands out by default, with 1 in place of a 0.)
 *
 * MIPT_FLAG_ACCUM (device entry only, with MIPT_FLAG_SUM): d_radiance[i] += this call's sum, one f32 addition per channel.  The
 * caller brings fresh seeds with every call and divides once at the end: progressive baking.
 *
 * Results and indices.  radiance[i * 3 .. i * 3 + 3) depends on rays[i] and the options only -- never on i, on n_rays or on how the
 * launch was scheduled.  Every ray writes its slot and nothing behind n_rays * 3 floats is touched.  n_rays == 0 is MIPT_OK without
 * a launch; n_rays >= MIPT_QUERY_MAX_RAYS is MIPT_ERR_INVALID_ARG.
 *
 * Options (required): samples and max_ray_depth > 0; traversal / cull_margin / shading as in MiptOptions; flags: MIPT_FLAG_COUNT,
 * MIPT_FLAG_SUM and MIPT_FLAG_ACCUM -- MIPT_FLAG_TOUCHED, MIPT_FLAG_PACKED and unknown bits are refused; reserved words 0.
 *
 * stats (may be NULL).  kernel_ms and stack_overflows always.  With MIPT_FLAG_COUNT also rays, inner_steps, tri_tests, hits,
 * texel_fetches and max_stack, pixels = n_rays, and diag[] as a batch launch fills it.
 *
 * Errors.  Checked before any device work, MIPT_ERR_INVALID_ARG with a message in mipt_last_error(): a null scene, rays, options or
 * radiance; n_rays >= MIPT_QUERY_MAX_RAYS; zero samples or max_ray_depth; an unknown traversal, shading or flag; a negative or
 * non-finite cull_margin; non-zero reserved fields; MIPT_FLAG_ACCUM on the host entry or without MIPT_FLAG_SUM; for the device
 * entry d_rays not 16-byte aligned, d_radiance not 4-byte aligned, the two ranges overlapping, or a pointer that is not device
 * memory of the scene's device.  A traversal-stack overflow is MIPT_ERR_STACK after the results are written, as in mipt_render.
 * After any error the scene renders and queries as before.
 *
 * The device entry takes buffers in HBM of the scene's device, is ordered after the earlier work of `hip_stream` (NULL = the null
 * stream) and blocks until done, like the queries above.  Both entries see the geometry of the last successful update (REFIT,
 * REBUILD, mipt_scene_set_transforms, mipt_scene_update_mesh_device) and work on a replica handle from mipt_multi_scene. */
typedef struct {
    uint32_t samples;        /* > 0: paths per ray */
    uint32_t max_ray_depth;  /* > 0 */
    uint32_t traversal;      /* MiptTraversal */
    float    cull_margin;    /* MIPT_TRAVERSAL_CULLED: relative margin (>= 0); see MIPT_CULL_MARGIN_SAFE */
    uint32_t shading;        /* MiptShading */
    uint32_t flags;          /* MIPT_FLAG_COUNT, MIPT_FLAG_SUM, MIPT_FLAG_ACCUM (device entry only, needs SUM) */
    uint32_t reserved[10];   /* must be 0 */
} MiptRadianceOptions;      /* 64 B */

MIPT_API int mipt_query_radiance(MiptScene *scene, const MiptRay *rays, uint64_t n_rays, const MiptRadianceOptions *opt,
                                 float *radiance /* n_rays*3 */, MiptStats *stats);
MIPT_API int mipt_query_radiance_device(MiptScene *scene, const MiptRay *d_rays, uint64_t n_rays, const MiptRadianceOptions *opt,
                                        float *d_radiance /* n_rays*3 */, void *hip_stream, MiptStats *stats);

/* ---- baking: surface points and the light they gather ----------------------------------------------------------------------------
 * The two steps a lightmap or vertex baker had to do on the host around mipt_query_radiance: find the surface point behind every
 * lightmap texel (mipt_bake_texels: the scene's own UV layout, rasterised from tri_attr in HBM) and send one hemisphere ray per
 * point and sample, sum what comes back (mipt_bake_gather).  Kernels: csrc/bake.hip; the paths run in the ray kernel of the
 * radiance queries.  Every operator below is one rounded f32 operation, nothing is fused.
 *
 * The record.  MiptSurfacePoint = {seed, u, v, prim}.  prim is encoded as MiptHit.prim: the low 25 bits are the triangle in the
 * caller's order (as for the queries), MIPT_HIT_NONE = no point.  Bit 31 (MIPT_HIT_FRONT_FACE) set selects the side the
 * interpolated normal points to, bit 31 clear the reversed normal (ray.rs:46-48).  u, v are barycentrics, used as given: no range
 * check.  An array of MiptHit whose `t` word has been overwritten with a seed is an array of points: what mipt_query_closest found
 * can be handed to mipt_bake_gather as it is, once every record has its seed.
 *
 * mipt_bake_texels: texel -> surface point.  Texel (x, y) of a width x height atlas, index i = y * width + x, has its centre at
 *     s = ((float)x + 0.5f) / (float)width        t = ((float)y + 0.5f) / (float)height
 * Atlas row y is UV coordinate t: no flip, no wrap; UVs outside [0, 1] cover nothing there.  For a triangle with corner UVs a, b, c
 * (tex_coord_x, tex_coord_y of vertices 0, 1, 2):
 *     bx = b.x - a.x   by = b.y - a.y   cx = c.x - a.x   cy = c.y - a.y   px = s - a.x   py = t - a.y
 *     d = (bx * cy) - (cx * by)
 *     u = ((px * cy) - (cx * py)) / d             v = ((bx * py) - (px * by)) / d
 *     covered  iff  d is finite and != 0  &&  u >= 0 && v >= 0 && (u + v) <= 1                                  (any NaN fails)
 *                   &&  min(a.x, b.x, c.x) <= s <= max(a.x, b.x, c.x)  &&  min(a.y, b.y, c.y) <= t <= max(a.y, b.y, c.y)
 * The last line compares f32 values exactly.  In exact arithmetic it follows from the line above it; in f32 it keeps a sliver whose
 * d is mostly rounding noise from claiming texels along its extension, outside its own UV bounding box -- and makes the answer
 * independent of which texels a launch visits for a triangle, as long as it visits every texel of that box.
 * The owner of a texel is the covering triangle with the LOWEST INDEX IN THE CALLER'S ORDER, whatever the launch does.
 *     points[i] = {seed = i, u, v, prim = owner | MIPT_HIT_FRONT_FACE}     u, v of the owner by the formulas above
 *     points[i] = {i, 0, 0, MIPT_HIT_NONE}                                  no triangle covers the texel
 * Every texel is written; nothing behind width * height records is touched.  Consequences: a texel centre exactly on an edge two
 * triangles share goes to the lower index; rounding can leave such a texel to NEITHER triangle (each computes its own u, v);
 * dilating the atlas over such holes and over the chart borders is the baker's job and out of scope here.
 * Options: NULL = all zero; flags and reserved words must be 0.  info (may be NULL): covered_texels, degenerate_tris (triangles
 * whose d is 0 or not finite) and kernel_ms (HIP events around the memsets and kernels).  Limit: width * height < 2^31; an
 * atlas without texels (width or height 0) is MIPT_OK without a launch.  The workspace, 8 B per texel, belongs to the scene and
 * grows on demand.  The device entry wants d_points 16-byte aligned.  Both entries see the UVs of the last successful update, like
 * the queries, and work on a mesh scene and on a replica handle.
 *
 * mipt_bake_gather: the light a surface point gathers.  Point i lies on triangle k = prim & 0x01ffffff of the caller's array:
 *     P = (v0 + e1 * u) + e2 * v          e1 = v1 - v0, e2 = v2 - v0, each rounded once (ray.rs:24-25)
 *     N = (n0 * ((1 - u) - v) + n1 * u) + n2 * v       (ray.rs:45), reversed iff bit 31 is clear; not normalised, as in the reference
 * Sample g = first_sample + s, s < samples, runs on a stream of its own:
 *     rng = 987612486 * (seed + g * sample_stride + 87636354) mod 2^32, 1 in place of 0      (cpu.rs:28-29 with the point as the
 *           pixel and the sample as the frame; all of it wraps)
 *     new_dir = normalized(N + rand_in_unit_sphere(rng))                                       (ray.rs:179-181)
 *     L = trace(ray = (P + new_dir * 0.0001, new_dir), max_ray_depth, rng)                     the stream continues into the trace
 * trace is Ray::trace (MIPT_SHADING_CPU) or rt_compute.wgsl's trace (MIPT_SHADING_WGPU), as in the radiance queries.  The first
 * scatter is the CPU rule in both: the point is a Lambertian receiver, `shading` selects only how the path goes on.
 * The samples are summed in f32, in order, from +0, and the sum is divided by (float)samples unless MIPT_FLAG_SUM is set.
 * MIPT_FLAG_ACCUM (device entry only, with MIPT_FLAG_SUM) adds the call's samples to d_radiance[i]: the ordered sum starts from
 * the value found there instead of +0 and goes back there.  (The radiance query forms its sum apart and adds it with one addition;
 * here the samples are added one by one ON the running value, so that a sum can be split between calls.)  Hence two SUM|ACCUM
 * calls of 4 samples each, first_sample 0 and 4, into zeros, equal one SUM call of 8 samples bit for bit -- and so does any other
 * split of the samples into consecutive calls.
 * No pi is applied: the value is the mean radiance over the hemisphere (cosine-weighted for a unit N).  A lightmap that stores irradiance
 * multiplies by pi; one that stores outgoing radiance of a diffuse surface multiplies by its albedo and nothing else.
 * A MIPT_HIT_NONE point yields 0, 0, 0 and is left untouched under ACCUM.  Every other point's value depends on the point and the
 * options only -- never on i, on n or on how the work was scheduled.  sample_stride = the number of points (the Python wrapper's
 * default) gives every (point, sample) of an atlas whose seeds are 0 ... n-1 a seed of its own.
 * Options (required): samples, max_ray_depth, sample_stride > 0; traversal / cull_margin / shading / flags as MiptRadianceOptions.
 * stats (may be NULL): the work runs in chunks of at most 2^22 paths; counters are summed over the chunks, max_stack is their
 * maximum, pixels counts paths, and kernel_ms runs from the first kernel of the call to its last.  The paths of MIPT_HIT_NONE
 * points are counted as rays that miss.  Staging (32 + 12 B per path of a chunk, about 180 MB at most) and the map from the
 * caller's triangle index to the device record (4 B per triangle, made on first use, dropped whenever the tree changes) belong to
 * the scene.
 * Errors: the radiance queries' list, with `points` for `rays` (d_points 16-byte aligned); sample_stride == 0; a prim whose
 * triangle is >= the scene's count: MIPT_ERR_INVALID_ARG naming the first such index, found on the host by the host entry and by a
 * kernel over all points by the device entry, before anything is traced and with the output untouched.  n == 0 is MIPT_OK
 * without a launch.  MIPT_ERR_STACK is returned after all chunks have run and the results are written.  After any error the scene
 * renders, queries and bakes as before. */
typedef struct { uint32_t seed; float u, v; uint32_t prim; } MiptSurfacePoint;   /* 16 B */
typedef struct { uint32_t flags; uint32_t reserved[7]; } MiptBakeTexelOptions;   /* 32 B; all 0 */
typedef struct {
    uint64_t covered_texels;  /* texels that have an owner */
    uint32_t degenerate_tris; /* triangles whose UV determinant d is 0 or not finite: they cover nothing */
    float    kernel_ms;
    uint32_t reserved[4];
} MiptBakeTexelInfo;         /* 32 B */
typedef struct {
    uint32_t samples;        /* > 0: paths per point */
    uint32_t max_ray_depth;  /* > 0: segments behind the point */
    uint32_t traversal;      /* MiptTraversal */
    float    cull_margin;    /* as MiptRadianceOptions */
    uint32_t shading;        /* MiptShading: how a path goes on behind its first segment */
    uint32_t flags;          /* MIPT_FLAG_COUNT, MIPT_FLAG_SUM, MIPT_FLAG_ACCUM (device entry only, needs SUM) */
    uint32_t first_sample;   /* g of this call's first sample */
    uint32_t sample_stride;  /* > 0 */
    uint32_t reserved[8];    /* must be 0 */
} MiptBakeOptions;          /* 64 B */

MIPT_API int mipt_bake_texels(MiptScene *scene, uint32_t width, uint32_t height, const MiptBakeTexelOptions *opt,
                              MiptSurfacePoint *points /* width*height */, MiptBakeTexelInfo *info);
MIPT_API int mipt_bake_texels_device(MiptScene *scene, uint32_t width, uint32_t height, const MiptBakeTexelOptions *opt,
                                     MiptSurfacePoint *d_points /* width*height */, void *hip_stream, MiptBakeTexelInfo *info);
MIPT_API int mipt_bake_gather(MiptScene *scene, const MiptSurfacePoint *points, uint64_t n, const MiptBakeOptions *opt,
                              float *radiance /* n*3 */, MiptStats *stats);
MIPT_API int mipt_bake_gather_device(MiptScene *scene, const MiptSurfacePoint *d_points, uint64_t n, const MiptBakeOptions *opt,
                                     float *d_radiance /* n*3 */, void *hip_stream, MiptStats *stats);

/* mipt_bake_surface: where a surface point lies and which way its surface faces -- the guides of mipt_lightmap_filter.  For point i
 * the values are the P and N of mipt_bake_gather above, formed by the same rounded operations:
 *     position[i] = P = (v0 + e1 * u) + e2 * v
 *     normal[i]   = N = (n0 * ((1 - u) - v) + n1 * u) + n2 * v, reversed iff bit 31 of prim is clear
 * With MIPT_BAKE_SURFACE_UNIT_NORMALS, normal[i] = normalized(N) instead: N / sqrt((N.x*N.x + N.y*N.y) + N.z*N.z), one division per
 * component (vec3.rs:93-109).  A zero N then gives NaNs, and they are left as they are.  A MIPT_HIT_NONE point writes +0 to all six
 * words.  Either output may be NULL = not wanted (never written), not both.  Every point's values depend on the point alone.
 * Options: NULL = all zero; flags: MIPT_BAKE_SURFACE_UNIT_NORMALS only; reserved words 0.
 * Errors, in gather's order: a null scene or points, or both outputs NULL; n >= 2^31; flags; reserved words; for the device entry
 * d_points not 16-byte aligned, an output not 4-byte aligned; (n == 0 is MIPT_OK here, without a launch); for the device entry an
 * output that overlaps the points or the other output, a pointer that is not memory of the scene's device; a prim whose triangle is
 * >= the scene's count: MIPT_ERR_INVALID_ARG naming the first such index, as mipt_bake_gather finds it, with both outputs untouched.
 * The map from the caller's triangle index to the device record is the gather's, made by whichever call needs it first and dropped
 * whenever the tree changes.  Both entries block until done, see the geometry of the last successful update and work on a mesh scene
 * and on a replica handle. */
#define MIPT_BAKE_SURFACE_UNIT_NORMALS 1u
typedef struct { uint32_t flags; uint32_t reserved[7]; } MiptBakeSurfaceOptions;   /* 32 B */
MIPT_API int mipt_bake_surface(MiptScene *scene, const MiptSurfacePoint *points, uint64_t n, const MiptBakeSurfaceOptions *opt,
                               float *position /* n*3 or NULL */, float *normal /* n*3 or NULL */);
MIPT_API int mipt_bake_surface_device(MiptScene *scene, const MiptSurfacePoint *d_points, uint64_t n, const MiptBakeSurfaceOptions *opt,
                                      float *d_position /* n*3 or NULL */, float *d_normal /* n*3 or NULL */, void *hip_stream);

/* ---- lightmap finishing: an edge-avoiding filter over the covered texels of an atlas, and dilation into its gutters -------------------
 * What turns the atlas mipt_bake_texels + mipt_bake_gather leave -- a noisy mean per covered texel, zeros elsewhere -- into one a
 * renderer can sample (csrc/lightmap.hip).  Scene-free, like the denoiser: planes in, a plane out.  The reference has no baker:
 * both operators are defined HERE, and the kernels and tests/tools/lightmap_model.py obey them bit for bit.  Every operator is one
 * rounded f32 operation, nothing is fused, and the operations run in the order written.  Texel (x, y) of a width x height atlas is
 * index y * width + x of every plane.  A texel is COVERED iff prim of its record in `points` (the records mipt_bake_texels wrote)
 * is not MIPT_HIT_NONE; nothing else of the record is read.  Limit, as for mipt_bake_texels: width * height < 2^31, and here both
 * sides greater than 0.
 *
 * mipt_lightmap_filter: the a-trous filter of the denoiser section in atlas space.  Planes:
 *   radiance  3 f32 / texel, required
 *   points    16 B / texel, required (16-byte aligned for the device entry)
 *   position  3 f32 / texel, optional: the P of mipt_bake_surface
 *   normal    3 f32 / texel, optional; used as given, not normalised
 *   out       3 f32 / texel, required; may be radiance
 * A NULL guide means its terms are left out: not computed, not fetched.  There is no demodulation: the gather's value carries no
 * albedo.  c0 = radiance.
 * Iteration i = 0 ... iterations - 1 (1 <= iterations <= 8) has step s = 1 << i, reads the previous iteration's colours c and writes
 * new ones.  An UNCOVERED texel keeps its words: its `out` is its `radiance` word for word.  For a covered texel p = (x, y):
 *   - taps q = (x + s*dx, y + s*dy), dy = -2 ... 2 the outer loop and dx = -2 ... 2 the inner one.  A tap outside [0,W) x [0,H) and
 *     an UNCOVERED tap are skipped -- neither weighted nor added: what an uncovered texel holds reaches no covered one.
 *   - h = [1/16, 1/4, 3/8, 1/4, 1/16]; the tap's kernel weight h[dy+2] * h[dx+2] is an exact constant.
 *   - dc = ((dr*dr) + (dg*dg)) + (db*db) with dr = c_p.r - c_q.r and so on; dn likewise from the normals N_p - N_q.
 *   - D = P_q - P_p (three subtractions); dd = ((D.x*D.x) + (D.y*D.y)) + (D.z*D.z);
 *     l = ((N_p.x*D.x) + (N_p.y*D.y)) + (N_p.z*D.z); dl = l * l: the tap's squared distance from the centre's tangent plane (for a
 *     unit N_p), which lets the filter run along a flat chart and stops it at a chart that lies on another plane.
 *   - e = (((dc * kc_i) + (dn * kn)) + (dl * kl)) + (dd * kd_i); dn needs `normal`, dd needs `position`, dl needs both; an absent
 *     term is left out of the sum, the others keep their order.  The constants are formed on the host in f32:
 *     kn = 1.0f / (sigma_normal * sigma_normal), kl likewise from sigma_plane, kc_i = 1.0f / (sc * sc) with sc = sigma_color * 2^-i,
 *     kd_i = 1.0f / (sd * sd) with sd = sigma_distance * 2^i: the world distance a tap may lie away grows with the step, as the taps do.
 *   - e = e < 128.0f ? e : 128.0f (a NaN gives 128).
 *   - w = (h[dy+2] * h[dx+2]) * expf(-e), expf as in the denoiser section.  The centre tap has weight 9/64 without evaluation.
 *   - sum_ch = sum_ch + (w * c_q.ch) and wsum = wsum + w, both starting at +0.
 *   - the new colour is, per channel, wsum > 0 ? sum_ch / wsum : c_p.ch.
 * The NaN rule of the query section applies.  What the operators cannot do: two charts that are neighbours on the surface but not in
 * the atlas do not see each other (that takes a world-space neighbour search), and two charts that ARE neighbours in the atlas are
 * kept apart only by the guides: without position and normal, light leaks across a gutter narrower than the taps reach.
 * Errors, before any device work and in this order: a null opt, buffers, radiance, points or out; a zero side; width * height >= 2^31;
 * iterations outside 1 ... 8; non-zero flags or reserved fields; sigma_color, then sigma_normal (with normal), sigma_plane (with
 * both guides), sigma_distance (with position): each finite and greater than 0 with a finite k > 0, kc_i and kd_i for every i (a
 * sigma of an absent term is ignored); planes that overlap (out == radiance alone is allowed); for the device entry the
 * denoiser's list: workspace NULL, too small, misaligned, overlapped; a misaligned plane; memory not of radiance's device. */
typedef struct {
    uint32_t width, height;
    uint32_t iterations;          /* 1 ... 8 */
    float    sigma_color, sigma_normal, sigma_plane, sigma_distance;
    uint32_t flags;               /* must be 0 */
    uint32_t reserved[8];         /* must be 0 */
} MiptLightmapFilterOptions;      /* 64 B */
typedef struct {
    const float *radiance;
    const MiptSurfacePoint *points;
    const float *position, *normal;               /* NULL = absent */
    float       *out;                             /* may be radiance */
    void        *reserved[3];                     /* must be NULL */
} MiptLightmapFilterBuffers;      /* 64 B */
/* Bytes of workspace mipt_lightmap_filter_device needs: four float4 planes, 64 B per texel.  0 = an invalid size. */
MIPT_API uint64_t mipt_lightmap_filter_workspace_bytes(uint32_t width, uint32_t height);
/* HOST buffers, staged through memory of HIP device `device_id`; blocks until done. */
MIPT_API int mipt_lightmap_filter(const MiptLightmapFilterOptions *opt, const MiptLightmapFilterBuffers *host, int device_id);
/* DEVICE buffers of one device on `hip_stream`; stream-ordered, allocates nothing, writes `out` and the first
 * mipt_lightmap_filter_workspace_bytes() bytes of the caller's 16-byte aligned workspace and nothing else (as mipt_denoise_device). */
MIPT_API int mipt_lightmap_filter_device(const MiptLightmapFilterOptions *opt, const MiptLightmapFilterBuffers *device, void *d_workspace,
                                         uint64_t workspace_bytes, void *hip_stream);

/* mipt_lightmap_dilate: fill the gutter from the charts' borders outwards.  Planes:
 *   radiance  3 f32 / texel, required
 *   points    16 B / texel, required (16-byte aligned for the device entry)
 *   out       3 f32 / texel, required; may be radiance
 *   level     1 u32 / texel, optional
 * Level.  Every texel has a value (its radiance words at first) and a level: 1 if covered, 0 otherwise.
 * Pass k = 1 ... radius (0 <= radius <= 64) reads only the state after pass k - 1:
 *   - a texel of level 0 is FILLED if at least one of its eight neighbours has a non-zero level.  The neighbours are visited
 *     dy = -1 ... 1 the outer loop and dx = -1 ... 1 the inner one, the centre and texels outside the atlas skipped;
 *   - the filled value is, per channel, the sum of the values of the neighbours of non-zero level in that order, from +0, divided by
 *     (float)count, count being their number; the filled texel's level becomes k + 1;
 *   - every other texel keeps its value and level.
 * After the last pass `out` holds the values and `level` (if given) the levels: 1 + the Chebyshev distance to the nearest covered
 * texel where that is <= radius, else 0.  A texel still at level 0 keeps its radiance words, covered texels come back word for
 * word, and radius == 0 is a copy.  Because a pass reads only the previous pass's state the result does not depend on scheduling.
 * Errors, in this order: a null opt, buffers, radiance, points or out; a zero side; width * height >= 2^31; radius above 64; non-zero
 * flags or reserved fields; planes that overlap (out == radiance alone is allowed); the device entry's list as above. */
#define MIPT_LIGHTMAP_MAX_RADIUS 64u
typedef struct { uint32_t width, height, radius, flags; uint32_t reserved[4]; } MiptLightmapDilateOptions;   /* 32 B */
typedef struct {
    const float *radiance;
    const MiptSurfacePoint *points;
    float       *out;                             /* may be radiance */
    uint32_t    *level;                           /* NULL = not wanted */
    void        *reserved[4];                     /* must be NULL */
} MiptLightmapDilateBuffers;      /* 64 B */
/* Bytes of workspace mipt_lightmap_dilate_device needs: two float4 planes, 32 B per texel.  0 = an invalid size. */
MIPT_API uint64_t mipt_lightmap_dilate_workspace_bytes(uint32_t width, uint32_t height);
MIPT_API int mipt_lightmap_dilate(const MiptLightmapDilateOptions *opt, const MiptLightmapDilateBuffers *host, int device_id);
MIPT_API int mipt_lightmap_dilate_device(const MiptLightmapDilateOptions *opt, const MiptLightmapDilateBuffers *device, void *d_workspace,
                                         uint64_t workspace_bytes, void *hip_stream);

/* ---- irradiance probes: SH coefficients of the light that arrives at a point, and their lookup ------------------------------------------
 * What a lightmapped scene uses for everything that moves: a grid of probes, each holding the incoming radiance around its position
 * projected onto real spherical harmonics up to band 2 (9 coefficients x RGB), and a lookup that blends the grid at a shaded point
 * and convolves with the clamped cosine (Ramamoorthi-Hanrahan).  Kernels: csrc/probe.hip; the paths of the bake run in the ray
 * kernel of the radiance queries, staged as mipt_bake_gather stages its own.  Every operator below is one rounded f32 operation,
 * nothing is fused, and the operations run in the order written; tests/tools/probe_model.py restates them.
 *
 * The basis, for a direction (x, y, z), in the order (l, m) = (0,0) (1,-1) (1,0) (1,1) (2,-2) (2,-1) (2,0) (2,1) (2,2):
 *     Y0 = 0.2820948f
 *     Y1 = 0.48860252f * y            Y2 = 0.48860252f * z            Y3 = 0.48860252f * x
 *     Y4 = 1.0925485f * (x * y)       Y5 = 1.0925485f * (y * z)       Y6 = 0.31539157f * ((3.0f * (z * z)) - 1.0f)
 *     Y7 = 1.0925485f * (x * z)       Y8 = 0.54627424f * ((x * x) - (y * y))
 * Each literal is the float nearest to its closed form: sqrt(1/4pi), sqrt(3/4pi), sqrt(15/4pi), sqrt(5/16pi), sqrt(15/16pi).
 *
 * mipt_probe_bake: probes -> coefficients.  MiptProbe = {x, y, z, seed}.  sh[i * 27 + k * 3 + c] is coefficient k of channel c of
 * probe i.  Sample g = first_sample + s, s < samples, of probe i at P = (x, y, z) runs on a stream of its own:
 *     rng = 987612486 * (seed + g * sample_stride + 87636354) mod 2^32, 1 in place of 0       (the gather's formula; all of it wraps)
 *     d = rand_in_unit_sphere(rng)                           (vec3.rs:66-68: already a unit vector, used as given; uniform on the sphere)
 *     L = trace(ray = (P, d), max_ray_depth, rng)            the origin is exactly P -- a probe lies on no surface, there is no offset --
 *                                                            and the stream continues into the trace
 * trace is Ray::trace (MIPT_SHADING_CPU) or rt_compute.wgsl's trace (MIPT_SHADING_WGPU), as in the radiance queries.
 *     acc[k][c] = acc[k][c] + (L[c] * Y_k(d))                over the samples IN ORDER, from +0
 *     sh[i][k][c] = (acc[k][c] / (float)samples) * 12.566371f        unless MIPT_FLAG_SUM is set: then acc[k][c] as it is
 * 12.566371f is 4 pi: the estimate of the coefficient under the uniform pdf 1 / 4 pi.  MIPT_FLAG_ACCUM (device entry only, with
 * MIPT_FLAG_SUM) follows the GATHER's rule, not the radiance query's: the ordered sums go on from the 27 words found in d_sh[i]
 * and go back there, so any split of the samples into consecutive calls (first_sample 0 and 4 for 4 + 4, say) into zeros equals the
 * single call bit for bit.  Each probe's 27 words depend on that probe and the options only -- never on i, on n or on how the work
 * was scheduled.  NaN and inf -- a non-finite P, a NaN d from a degenerate draw -- are left as they are.
 * Limit of precision: an ordered f32 sum stops gaining precision as the running sum approaches 2^24 times the typical term.  Keep
 * one buffer to about 2^16 samples and average buffers beyond that; the entry accepts any `samples`, as the gather does.
 * Options (required): MiptBakeOptions field for field.  stats (may be NULL), chunks (at most 2^22 paths; path q is sample q % samples
 * of probe q / samples; a probe may span chunks, and one of more than 2^22 samples spans whole chunks) and staging (the gather's
 * buffers of the scene plus two carry slots of 27 words): as mipt_bake_gather.
 * Errors: the gather's list with `probes` for `points` and `sh` for `radiance` (d_probes 16-byte aligned, d_sh 4-byte aligned; n * 27
 * floats); there is no prim, so no index check.  n == 0 is MIPT_OK without a launch.  MIPT_ERR_STACK is returned after all chunks
 * have run and the results are written.  Both entries block until done, see the geometry of the last successful update and work on
 * a mesh scene and on a replica handle.  After any error the scene renders, queries and bakes as before. */
typedef struct { float x, y, z; uint32_t seed; } MiptProbe;   /* 16 B */
typedef struct {
    uint32_t samples;        /* > 0: paths per probe */
    uint32_t max_ray_depth;  /* > 0 */
    uint32_t traversal;      /* MiptTraversal */
    float    cull_margin;    /* as MiptRadianceOptions */
    uint32_t shading;        /* MiptShading */
    uint32_t flags;          /* MIPT_FLAG_COUNT, MIPT_FLAG_SUM, MIPT_FLAG_ACCUM (device entry only, needs SUM) */
    uint32_t first_sample;   /* g of this call's first sample */
    uint32_t sample_stride;  /* > 0 */
    uint32_t reserved[8];    /* must be 0 */
} MiptProbeBakeOptions;     /* 64 B */
MIPT_API int mipt_probe_bake(MiptScene *scene, const MiptProbe *probes, uint64_t n, const MiptProbeBakeOptions *opt,
                             float *sh /* n*27 */, MiptStats *stats);
MIPT_API int mipt_probe_bake_device(MiptScene *scene, const MiptProbe *d_probes, uint64_t n, const MiptProbeBakeOptions *opt,
                                    float *d_sh /* n*27 */, void *hip_stream, MiptStats *stats);

/* mipt_probe_irradiance: a grid of probes + points with normals -> irradiance.  Scene-free, like the denoiser and the lightmap
 * operators: buffers in, a buffer out.  The grid has dims[0] x dims[1] x dims[2] probes; probe (ix, iy, iz) lies at
 * origin + spacing * (ix, iy, iz) and has index (iz * dims[1] + iy) * dims[0] + ix.  Buffers:
 *   sh          n_probes * 27 f32, required: what mipt_probe_bake wrote (the mean, not the sum)
 *   valid       n_probes bytes, optional: 0 = the probe is left out of every blend (one the caller found inside a wall, say)
 *   position    n * 3 f32, required
 *   normal      n * 3 f32, required; used as given, not normalised
 *   irradiance  n * 3 f32, required
 * For query point p, per axis a:
 *     g = (p_a - origin_a) / spacing_a;   g = 0 unless g >= 0 (a NaN gives 0);   g = min(g, (float)(dims_a - 1))
 *     i0 = min((uint32_t)g, dims_a - 2) and f = g - (float)i0;   dims_a == 1: i0 = 0 and f = 0
 *     w_a[0] = 1.0f - f     w_a[1] = f
 * The eight corners (i0x + dx, i0y + dy, i0z + dz) are taken in the order dz * 4 + dy * 2 + dx = 0 ... 7, with weight
 * w = (w_x[dx] * w_y[dy]) * w_z[dz].  A corner whose weight is exactly 0 or whose `valid` byte is 0 is SKIPPED: neither read nor
 * added (a NaN probe behind a zero weight cannot leak; the corner beyond a one-probe axis is never addressed).  Over the kept
 * corners, in that order and from +0:
 *     b[k][c] = b[k][c] + (w * sh[probe][k][c])          wsum = wsum + w
 * Then, with Y_k the basis above evaluated at the normal and A0 = 3.1415927f, A1 = 2.0943952f, A2 = 0.7853982f (pi, 2 pi / 3, pi / 4):
 *     E[c] = ((A0 * (Y0 * b0)) + (A1 * (((Y1 * b1) + (Y2 * b2)) + (Y3 * b3))))
 *            + (A2 * (((((Y4 * b4) + (Y5 * b5)) + (Y6 * b6)) + (Y7 * b7)) + (Y8 * b8)))             b_k = b[k][c]
 * With a `valid` plane E[c] = E[c] / wsum, one division per channel, and +0 where wsum == 0 (every corner left out); without one
 * there is no division (the weights of a cell sum to 1 up to rounding).  With MIPT_PROBE_CLAMP (a flag of the grid) E[c] =
 * E[c] > 0 ? E[c] : +0 last of all (band-2 ringing can go negative; a NaN becomes 0).  Every point writes its three words and nothing
 * else is touched; irradiance[i] depends on point i and the grid only.
 * Errors, before any device work and in this order: a null grid or buffers; n >= 2^31; a null sh, position, normal or irradiance; a
 * zero dimension; a product of dims >= 2^31; a spacing that is zero, negative or not finite; unknown flags; non-zero reserved words
 * or pointers; irradiance overlapping an input; for the device entry a misaligned buffer (4 bytes; valid: any address) or one that
 * is not memory of sh's device.  n == 0 is then MIPT_OK without a launch.  No workspace is needed: a lane per point. */
#define MIPT_PROBE_CLAMP 1u
typedef struct {
    float    origin[3];
    float    spacing[3];     /* finite and > 0 */
    uint32_t dims[3];        /* > 0; their product < 2^31 */
    uint32_t flags;          /* MIPT_PROBE_CLAMP */
    uint32_t reserved[6];    /* must be 0 */
} MiptProbeGrid;            /* 64 B */
typedef struct {
    const float   *sh;
    const uint8_t *valid;                         /* NULL = every probe is valid */
    const float   *position, *normal;
    float         *irradiance;
    void          *reserved[3];                   /* must be NULL */
} MiptProbeIrradianceBuffers;   /* 64 B */
/* HOST buffers, staged through memory of HIP device `device_id`; blocks until done. */
MIPT_API int mipt_probe_irradiance(const MiptProbeGrid *grid, uint64_t n, const MiptProbeIrradianceBuffers *host, int device_id);
/* DEVICE buffers of one device on `hip_stream`; stream-ordered, allocates nothing, writes `irradiance` and nothing else. */
MIPT_API int mipt_probe_irradiance_device(const MiptProbeGrid *grid, uint64_t n, const MiptProbeIrradianceBuffers *device, void *hip_stream);

/* ---- first-hit feature buffers: depth, ids, position, uv, normal, albedo, emission per pixel --------------------------------------
 * What the camera ray of every pixel hits and what the surface looks like there: the guide images of a denoiser, the id and depth
 * planes of a compositor, G-buffers for training data (csrc/first_hit.hip).  No path is traced: a sample ends at its first hit.
 *
 * Camera ray.  The camera ray of sample s of a pixel is exactly the ray mipt_render traces first for that sample with the same opt:
 * cpu.rs:28-50 with MIPT_SEED_PIXEL_STREAM (seed 987612486 * (index + 87636354), cpu.rs:28-29; y flip of cpu.rs:32); with
 * MIPT_SEED_PER_SAMPLE the stream is reseeded per sample as rt_compute.wgsl:102 does (sample_begin normalised 0 -> 1 as in
 * mipt_render).  The arithmetic is the trace kernel's: two rand_f32 draws, * 2 - 1, * 0.0005 (cpu.rs:38-42), the upper 3x3 of
 * look_at in the operation order of mat4.rs:143-152, normalized (cpu.rs:43-45), origin = camera position.
 *
 * Samples.  With MIPT_SEED_PER_SAMPLE opt->samples camera rays are traced per pixel, the samples sample_begin ... sample_begin +
 * samples - 1, which are independent of each other.  With MIPT_SEED_PIXEL_STREAM a pixel's second camera ray depends on how many
 * numbers the first sample's whole path drew (cpu.rs:37-58): only the first is defined without path tracing, so samples must be 1
 * (anything else: MIPT_ERR_INVALID_ARG with a message that says why).
 *
 * Hit.  Ray::traverse_bvh (ray.rs:84-139) with hit_info.distance = 1e30 in the arm opt->traversal / opt->cull_margin select:
 * exactly what mipt_query_closest returns for that ray.
 *
 * Per-sample values of a hit -- the fields intersect_tri (ray.rs:19-67) and trace (ray.rs:141-202) compute for the winner:
 *   t         the hit distance
 *   prim      MiptHit.prim: the triangle in the caller's order, bit 31 (MIPT_HIT_FRONT_FACE) = front face (ray.rs:39)
 *   material  the triangle's material_id (ray.rs:153)
 *   position  origin + direction * t (ray.rs:60)
 *   uv        ray.rs:50-53
 *   normal    ray.rs:45-48: interpolated, NOT normalised, reversed on a back face
 *   albedo    the factor ray_color is multiplied by at ray.rs:162-169: base_color, or color_at(uv) / 255 from the base-colour texture
 *   emission  the term added at ray.rs:170-176: emission, or color_at(uv) / 255 from the emission texture
 * of a miss: t = 1e30, prim = MIPT_HIT_NONE, material = UINT32_MAX, position = uv = normal = 0 (HitInfo::default, ray.rs:214-226),
 * albedo = (1,1,1) (sky_color, ray.rs:185) and emission = (1,1,1) (sky_strength, ray.rs:186).
 *
 * What is written.  depth (= t), prim, material, position and uv come from the FIRST sample of the call.  normal, albedo and
 * emission are the MEAN over the samples, formed as final_color is (cpu.rs:30,52,60): the sum starts at +0.0f, the samples are added
 * in order and the sum is divided by `samples as f32` once at the end -- also for one sample, so a -0 comes out as +0.  One
 * rounded f32 operation per operator, nothing fused.  The NaN rule of the query section applies: a NaN this arithmetic produces is
 * a NaN everywhere, and its sign and payload are the implementation's.
 *
 * Layout.  View-major, row 0 = top, exactly like mipt_render_batch: view v occupies [v*W*H*k, (v+1)*W*H*k) of a buffer with k
 * values per pixel.  n_views == 1 is the ordinary single frame; `cameras` are in HOST memory, read during the call only.  Any
 * buffer pointer may be NULL = not wanted (nothing is computed or fetched for it, and it is never written); at least one must be set.
 *
 * Options.  Honoured: width, height, samples, seed_mode, sample_begin, traversal, cull_margin.  max_ray_depth must be > 0 and is
 * otherwise ignored.  flags: MIPT_FLAG_COUNT only.  tile_world must be 0 or 1 (tile_rank 0).  shading must be MIPT_SHADING_CPU:
 * the first hit of the wgpu material model (normal maps, bilinear sampler, cut-outs) is out of scope and refused.  reserved must be
 * zero.  n_views >= 1 and n_views*W*H < MIPT_BATCH_MAX_PIXELS.
 *
 * Stats (may be NULL).  Always: kernel_ms, stack_overflows, tex_clamped, pixels = n_views*W*H.  With MIPT_FLAG_COUNT also rays,
 * inner_steps, tri_tests, hits, texel_fetches, max_stack.  A texture is fetched only for a buffer that is wanted, so texel_fetches
 * counts the fetches actually made.  Every other field 0.
 *
 * Errors.  Every argument is checked before any device work: MIPT_ERR_INVALID_ARG with a message in mipt_last_error() that names
 * the offending field -- a null scene, cameras, opt or buffers; no buffer wanted; a non-NULL reserved pointer; any option rule
 * above; for the _device entry a wanted pointer that is not 4-byte aligned or not device memory of the scene's device.  A
 * traversal-stack overflow is MIPT_ERR_STACK after the buffers are written, as in mipt_render.  After any error the scene renders
 * and queries as before.  Both entries work on a replica handle from mipt_multi_scene and see the geometry of the last successful
 * update. */
typedef struct {
    float    *depth;      /* 1 f32  / pixel */
    uint32_t *prim;       /* 1 u32  / pixel, MiptHit.prim convention */
    uint32_t *material;   /* 1 u32  / pixel */
    float    *position;   /* 3 f32 */
    float    *uv;         /* 2 f32 */
    float    *normal;     /* 3 f32 */
    float    *albedo;     /* 3 f32 */
    float    *emission;   /* 3 f32 */
    void     *reserved[4];/* must be NULL */
} MiptFeatureBuffers;     /* 96 B; any pointer may be NULL = not wanted; at least one must be set */

/* Into HOST buffers; blocks until done. */
MIPT_API int mipt_render_features(MiptScene *scene, const MiptCamera *cameras, uint32_t n_views, const MiptOptions *opt,
                                  const MiptFeatureBuffers *host_out, MiptStats *stats);
/* Into DEVICE buffers (e.g. torch tensors) on `hip_stream` (hipStream_t, NULL = the null stream); the camera table is copied on that
 * stream.  Blocks until the kernel has finished (stats are read back), like mipt_render_batch_device. */
MIPT_API int mipt_render_features_device(MiptScene *scene, const MiptCamera *cameras, uint32_t n_views, const MiptOptions *opt,
                                         const MiptFeatureBuffers *device_out, void *hip_stream, MiptStats *stats);

/* ---- a-trous denoiser: a few-sample frame plus its first-hit guides -> a usable image -----------------------------------------------
 * An edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) with optional albedo demodulation (csrc/denoise.hip), for the
 * buffers mipt_render{,_batch}_device and mipt_render_features_device leave in HBM.  The reference has no denoiser: the filter is
 * defined HERE, and the kernels and tests/tools/denoise_model.py obey it bit for bit.  Every operator is one rounded f32 operation,
 * nothing is fused, and the operations run in the order written.
 *
 * Buffers.  View-major planar, row 0 = top -- the layouts mipt_render_batch and mipt_render_features write:
 *   hdr     3 f32 / pixel, required
 *   normal  3 f32 / pixel, optional; used as given, not normalised
 *   depth   1 f32 / pixel, optional; a miss is 1e30
 *   albedo  3 f32 / pixel, optional
 *   out     3 f32 / pixel, required
 * A NULL guide means its term is left out: not computed, not fetched.
 *
 * Demodulation.  With albedo, per channel: a = albedo > 1/256 ? albedo : 1/256 (a comparison-select: a NaN albedo gives the floor),
 * c0 = hdr / a, and after the last iteration out = c * a.  Without albedo c0 = hdr and out = c.
 *
 * Iteration i = 0 ... iterations - 1 (1 <= iterations <= 8) has step s = 1 << i, reads the previous iteration's colours c and writes
 * new ones.  For pixel p = (x, y) of view v:
 *   - taps q = (x + s*dx, y + s*dy), dy = -2 ... 2 the outer loop and dx = -2 ... 2 the inner one.  A tap outside [0,W) x [0,H) is
 *     skipped -- neither weighted nor added -- and views never see each other.
 *   - h = [1/16, 1/4, 3/8, 1/4, 1/16]; the tap's kernel weight h[dy+2] * h[dx+2] is an exact constant.
 *   - dc = ((dr*dr) + (dg*dg)) + (db*db) with dr = c_p.r - c_q.r and so on; dn likewise from the normals; dz = (z_p - z_q) * (z_p - z_q).
 *   - e = ((dc * kc_i) + (dn * kn)) + (dz * kz), an absent guide's term left out of the sum.  The constants are formed on the host in
 *     f32: kn = 1.0f / (sigma_normal * sigma_normal), kz likewise from sigma_depth, kc_i = 1.0f / (sc * sc) with
 *     sc = sigma_color * 2^-i.
 *   - e = e < 128.0f ? e : 128.0f (a NaN gives 128).
 *   - w = (h[dy+2] * h[dx+2]) * expf(-e), expf being glibc 2.35's (the one the render's libm restatement pins) on [-128, -0], where
 *     expf(-128) = 0.  The centre tap has weight 9/64 without evaluation.
 *   - sum_ch = sum_ch + (w * c_q.ch) and wsum = wsum + w, both starting at +0.
 *   - the new colour is, per channel, wsum > 0 ? sum_ch / wsum : c_p.ch.
 * A NaN this arithmetic produces is a NaN everywhere; its sign and payload are the implementation's (the rule of the query section).
 *
 * Errors.  Everything is checked before any device work: MIPT_ERR_INVALID_ARG with a message in mipt_last_error() that names the
 * field -- a null opt, buffers, hdr or out; zero width, height or n_views; n_views*W*H >= MIPT_BATCH_MAX_PIXELS; iterations outside
 * 1 ... 8; a sigma that is not finite and greater than 0 or whose k (kc_i for every i) does not come out finite and greater than 0
 * (a sigma given for an absent guide is ignored); non-zero flags or reserved fields; buffers that overlap (out == hdr alone is
 * allowed); for the device entry a workspace that is NULL, too small, not 16-byte aligned or overlapped by a buffer, a pointer that
 * is not 4-byte aligned, and a pointer that is not device memory of one common device (hdr's). */
typedef struct {
    uint32_t width, height, n_views;
    uint32_t iterations;          /* 1 ... 8 */
    float    sigma_color, sigma_normal, sigma_depth;
    uint32_t flags;               /* must be 0 */
    uint32_t reserved[8];         /* must be 0 */
} MiptDenoiseOptions;             /* 64 B */
typedef struct {
    const float *hdr, *normal, *depth, *albedo;   /* normal, depth, albedo: NULL = absent */
    float       *out;                             /* may be hdr */
    void        *reserved[3];                     /* must be NULL */
} MiptDenoiseBuffers;             /* 64 B */

/* Bytes of workspace mipt_denoise_device needs for this size: three float4 planes, 48 B per pixel.  0 = an invalid size. */
MIPT_API uint64_t mipt_denoise_workspace_bytes(uint32_t width, uint32_t height, uint32_t n_views);
/* HOST buffers, staged through memory of HIP device `device_id`; blocks until done. */
MIPT_API int mipt_denoise(const MiptDenoiseOptions *opt, const MiptDenoiseBuffers *host, int device_id);
/* DEVICE buffers of one device (e.g. torch tensors) on `hip_stream` (hipStream_t, NULL = the null stream).  Stream-ordered: it does
 * not block and allocates nothing, like mipt_tonemap_device.  d_workspace is the caller's: 16-byte aligned device memory of at least
 * mipt_denoise_workspace_bytes().  The call writes `out` and the first mipt_denoise_workspace_bytes() bytes of the workspace and
 * nothing else. */
MIPT_API int mipt_denoise_device(const MiptDenoiseOptions *opt, const MiptDenoiseBuffers *device, void *d_workspace,
                                 uint64_t workspace_bytes, void *hip_stream);

/* ---- temporal accumulation: last frame's history, reprojected into this frame and blended with it ----------------------------------
 * The step from a denoised still to a moving sequence (the first half of an SVGF-style pipeline; the a-trous filter above is the
 * second): every pixel looks up where its surface point was in the previous frame, gathers that frame's accumulated colour with four
 * bilinear taps that must agree with it in material, normal and depth, and blends this frame's sample into it (csrc/temporal.hip).
 * The reference has nothing of this kind: the operation is defined HERE, and the kernel and tests/tools/temporal_model.py obey it bit
 * for bit.  Every operator is one rounded f32 operation, nothing is fused, and the operations run in the order written.
 *
 * Buffers.  View-major planar, row 0 = top -- what mipt_render_batch and mipt_render_features write:
 *   hdr       3 f32 / pixel, required: this frame's radiance
 *   position  3 f32 / pixel, required: the first hit's world position
 *   normal    3 f32 / pixel, required; used as given, not normalised
 *   depth     1 f32 / pixel, required; a miss is 1e30
 *   material  1 u32 / pixel, required
 *   albedo    3 f32 / pixel, optional: the colour is demodulated before the blend and re-modulated after
 *   out       3 f32 / pixel, required; may be hdr
 *   length    1 f32 / pixel, optional: the history length of the pixel after this frame
 *   variance  1 f32 / pixel, optional: the variance of the luminance over the history
 * `cameras` holds n_views MiptCamera records in HOST memory, for both entries: the cameras that produced this frame.  The previous
 * frame's cameras are not passed in: a history carries the camera that made it.
 *
 * History.  mipt_temporal_history_bytes() = 64*V + 48*N bytes, N = V*W*H, 16-byte aligned, everything view-major:
 *   byte 0           V camera records of 16 f32: B[3][3] row-major, C[3], four zeros
 *   byte 64*V        plane 0: N float4 {c.r, c.g, c.b, len}   the accumulated (demodulated) colour and the history length
 *   byte 64*V + 16*N plane 1: N float4 {n.x, n.y, n.z, z}     the normal and depth of the frame that wrote it
 *   byte 64*V + 32*N plane 2: N float4 {m1, m2, bits(material), 0}   the first two moments of the luminance, the material id's bits
 * history_in = NULL is the first frame: every pixel starts anew.  history_out is always written in full and must not overlap
 * history_in; a sequence keeps two and swaps them.
 *
 * Camera record of view v, formed on the host in binary64 with nothing contracted: a[r][c] = look_at[c][r] (the matrix
 * mat4.rs:143-152 applies to the screen vector);
 *   k00 = (a11*a22) - (a12*a21)   k01 = (a12*a20) - (a10*a22)   k02 = (a10*a21) - (a11*a20)
 *   k10 = (a02*a21) - (a01*a22)   k11 = (a00*a22) - (a02*a20)   k12 = (a01*a20) - (a00*a21)
 *   k20 = (a01*a12) - (a02*a11)   k21 = (a02*a10) - (a00*a12)   k22 = (a00*a11) - (a01*a10)
 *   det = ((a00*k00) + (a01*k01)) + (a02*k02);   B[i][j] = k[j][i] / det rounded to f32 (the inverse of a);   C = camera.position.
 * A det that is 0 or not finite, or a B entry that is not finite, is MIPT_ERR_INVALID_ARG naming cameras[v].look_at.
 *
 * Pixel p = (x, y) of view v, in f32.  Every comparison is written so that a NaN takes the "reject / reset" side.
 *   - a = albedo > 1/256 ? albedo : 1/256 per channel and cc = hdr / a; without albedo cc = hdr.
 *   - l = ((0.2126f*cc.r) + (0.7152f*cc.g)) + (0.0722f*cc.b).
 *   - RESET means c = cc, len = 1, m1 = l, m2 = l*l.
 *   - reset if history_in is NULL; reset if !(depth < 1e30f).
 *   - with B, C of history_in's record for view v: d = position - C, v_i = ((B[i][0]*d.x) + (B[i][1]*d.y)) + (B[i][2]*d.z);
 *     reset if !(v_z > 0).
 *   - sx = -(v_x / v_z), sy = v_y / v_z, aspect = (float)W / (float)H;
 *     fx = (((sx / aspect) + 1) * 0.5f) * W and fy = H - (((sy + 1) * 0.5f) * H), W and H as f32: the exact inverse of
 *     cpu.rs:31-35,44 -- pixel column and row are integer coordinates, row 0 the top.
 *   - reset unless fx >= -1 && fx < W && fy >= -1 && fy < H.  Only then x0 = floorf(fx) as an integer, wx = fx - floorf(fx), and
 *     likewise y0, wy.
 *   - d2 = ((d.x*d.x) + (d.y*d.y)) + (d.z*d.z).
 *   - taps q in the order (x0,y0), (x0+1,y0), (x0,y0+1), (x0+1,y0+1) of view v of history_in, with the weights
 *     (1-wx)*(1-wy), wx*(1-wy), (1-wx)*wy, wx*wy.
 *   - a tap is accepted when it lies inside [0,W) x [0,H), its material bits equal the pixel's,
 *     ((dx*dx) + (dy*dy)) + (dz*dz) <= normal_tol for (dx,dy,dz) = n_p - n_q, and fabsf(d2 - (z_q*z_q)) <= depth_tol * d2.
 *   - an accepted tap adds: sw = sw + w, s_ch = s_ch + (w*c_q.ch), sl = sl + (w*len_q), s1 = s1 + (w*m1_q), s2 = s2 + (w*m2_q), all
 *     sums starting at +0.  A rejected tap is not added at all.
 *   - reset unless sw > 1/64.
 *   - otherwise cp = s/sw per channel, lp = sl/sw; ln = lp + 1, ln = ln < max_history ? ln : max_history; al = 1/ln,
 *     al = al > alpha_min ? al : alpha_min; c = cp + ((cc - cp) * al), m1 = (s1/sw) + ((l - (s1/sw)) * al),
 *     m2 = (s2/sw) + (((l*l) - (s2/sw)) * al), len = ln.
 *   - written: history_out {c, len}, {normal, depth}, {m1, m2, material, 0} and this frame's camera record in its header;
 *     out = c * a (c without albedo); length = len; variance = m2 - (m1*m1), then variance > 0 ? variance : 0.
 * The NaN rule of the query section applies: a NaN this arithmetic produces is a NaN everywhere, sign and payload the implementation's.
 *
 * Scope.  `position` is where the pixel's surface point was WHEN THE HISTORY WAS WRITTEN.  For geometry that has not moved since,
 * that is the first hit's position (mipt_render_features).  After mipt_scene_update_*, mipt_scene_set_transforms or
 * mipt_scene_update_mesh_device it is the prev_position plane of mipt_render_motion ("previous positions" below): the lookup and
 * the depth check are then right for a moving surface.  Handing this entry the current position after an update instead leaves the
 * material, normal and depth checks to reject what they catch, and the rest ghosts.  The normal check compares this frame's normal
 * with the history's either way: a part that turns by more than normal_tol allows starts anew.
 *
 * Errors.  Everything is checked before any device work: MIPT_ERR_INVALID_ARG with a message in mipt_last_error() that names the
 * field -- a null opt, cameras, buffers or required plane; zero width, height or n_views; n_views*W*H >= MIPT_BATCH_MAX_PIXELS;
 * alpha_min outside 0 ... 1, max_history not finite and >= 1, a tolerance not finite and >= 0; non-zero flags or reserved fields; a
 * singular camera; buffers that overlap (out == hdr alone is allowed); for the device entry a pointer that is not 4-byte aligned (a
 * history: 16-byte) and a pointer that is not device memory of one common device (hdr's). */
typedef struct {
    uint32_t width, height, n_views;
    uint32_t flags;               /* must be 0 */
    float    alpha_min;           /* 0 ... 1: floor of the blend factor; 0 = plain running mean up to max_history */
    float    max_history;         /* >= 1, finite: cap of the history length */
    float    normal_tol;          /* >= 0, finite: largest |n_p - n_q|^2 of an accepted tap */
    float    depth_tol;           /* >= 0, finite: largest |d2 - z_q^2| / d2 of an accepted tap */
    uint32_t reserved[8];         /* must be 0 */
} MiptTemporalOptions;            /* 64 B */
typedef struct {
    const float    *hdr, *position, *normal, *depth;   /* 3,3,3,1 f32 / pixel, required */
    const uint32_t *material;                          /* 1 u32 / pixel, required */
    const float    *albedo;                            /* 3 f32, optional: demodulate before, re-modulate after */
    const void     *history_in;                        /* NULL = first frame: every pixel starts anew */
    void           *history_out;                       /* required; must not overlap history_in */
    float          *out;                               /* 3 f32, required; may be hdr */
    float          *length, *variance;                 /* 1 f32 each, optional */
    void           *reserved[5];                       /* must be NULL */
} MiptTemporalBuffers;            /* 128 B */

/* Bytes of one history for this size: 64*V + 48*V*W*H.  0 = an invalid size. */
MIPT_API uint64_t mipt_temporal_history_bytes(uint32_t width, uint32_t height, uint32_t n_views);
/* HOST buffers and HOST histories, staged through memory of HIP device `device_id`; blocks until done. */
MIPT_API int mipt_temporal(const MiptTemporalOptions *opt, const MiptCamera *cameras, const MiptTemporalBuffers *host, int device_id);
/* DEVICE buffers and histories of one device (e.g. torch tensors) on `hip_stream` (hipStream_t, NULL = the null stream).
 * Stream-ordered: it does not block and allocates nothing, like mipt_denoise_device; the camera table is host memory and may be
 * freed on return.  The call writes history_out, out and the optional outputs that are given, and nothing else. */
MIPT_API int mipt_temporal_device(const MiptTemporalOptions *opt, const MiptCamera *cameras, const MiptTemporalBuffers *device,
                                  void *hip_stream);

/* mipt_temporal_counts: the same accumulation with the history length counted in SAMPLES, for frames traced by mipt_render_adaptive.
 * The structs, the buffers, the checks, the history layout and mipt_temporal_history_bytes() are mipt_temporal's; flags and reserved
 * fields are refused as there.  Two more arguments:
 *   counts      : one u32 per pixel, view-major -- the plane mipt_render_adaptive was given for this frame;
 *   samples_cap : that call's opt->samples, 1 ... 65535.
 * Pixel i was traced with n = min(counts[i], samples_cap) samples; nf = (float)n.  The contract is the one above, every operator one
 * rounded f32 operation, nothing fused, every comparison with a NaN on the reject / reset side, with these changes and no others:
 *   - a tap is additionally rejected unless len_q > 0 (a pixel no sample has reached yet carries no colour).  A history written by
 *     mipt_temporal never has such a tap.
 *   - RESET with n > 0: c = cc, len = nf < max_history ? nf : max_history, m1 = l, m2 = l*l.
 *   - an accepted history (sw > 1/64) with n > 0: ln = lp + nf, ln = ln < max_history ? ln : max_history; al = nf / ln,
 *     al = al > alpha_min ? al : alpha_min, al = al < 1 ? al : 1; c, m1 and m2 are blended with al as above; len = ln.
 *     max_history is therefore a number of samples.
 *   - n == 0 (the pixel was not traced: hdr holds nothing of this frame): hdr[i] is NOT READ -- a NaN there changes nothing.
 *     With an accepted history: c = cp, len = lp < max_history ? lp : max_history, m1 = s1/sw, m2 = s2/sw -- pure reprojection
 *     (lp is a mean of lengths that are at most max_history, but sl/sw can round one ulp past it: no stored length ever exceeds
 *     max_history).  Otherwise c = +0, len = 0, m1 = m2 = +0.
 *   - written as above: the three history planes, the camera record, out = c * a, length, variance.
 * Consequences.  (a) With counts all 1 (any samples_cap) every output byte and every history byte equals mipt_temporal's.
 * (b) Histories interchange: either entry accepts the other's history_out as history_in.
 * `variance` is the variance of the FRAME MEANS over the history, each weighted by its samples; it is not a per-sample variance (the
 * mean of n samples enters as one value with the weight n).  With min_samples = 0 in the map, a pixel that is never traced and never
 * reprojected keeps len 0 and variance 0, so the map never gives it a sample: it stays starved, which is the caller's choice.
 * Errors, before any device work and naming the field: everything of mipt_temporal, and a null counts; samples_cap outside
 * 1 ... 65535; for the device entry a counts that is not 4-byte aligned, not device memory of hdr's device, or that overlaps any
 * buffer or history. */
MIPT_API int mipt_temporal_counts(const MiptTemporalOptions *opt, const MiptCamera *cameras, const MiptTemporalBuffers *host,
                                  const uint32_t *counts, uint32_t samples_cap, int device_id);
MIPT_API int mipt_temporal_counts_device(const MiptTemporalOptions *opt, const MiptCamera *cameras, const MiptTemporalBuffers *device,
                                         const uint32_t *d_counts, uint32_t samples_cap, void *hip_stream);

/* ---- variance-guided a-trous filter: the accumulated frame plus its variance and history length -> the frame to show ----------------
 * The second half of the SVGF-style pipeline (Schied et al. 2017) whose first half is the temporal accumulation above: the a-trous
 * filter of the denoiser section with a colour bandwidth that follows each pixel's own noise instead of a fixed sigma_color * 2^-i
 * (csrc/denoise_variance.hip).  A pixel whose history has converged is left alone, one disoccluded a frame ago is filtered hard.  The
 * reference has nothing of this kind: the operation is defined HERE, and the kernels and tests/tools/variance_model.py obey it bit
 * for bit.  Every operator is one rounded f32 operation, nothing is fused, and the operations run in the order written.
 *
 * Buffers.  View-major planar, row 0 = top:
 *   hdr           3 f32 / pixel, required: the accumulated frame (mipt_temporal's out), or one noisy frame
 *   normal        3 f32 / pixel, optional; used as given, not normalised
 *   depth         1 f32 / pixel, optional; a miss is 1e30
 *   albedo        3 f32 / pixel, optional
 *   variance      1 f32 / pixel  } what mipt_temporal writes.  Both or neither; neither means a single frame without history.
 *   length        1 f32 / pixel  }
 *   out           3 f32 / pixel, required; may be hdr
 *   variance_out  1 f32 / pixel, optional: the filtered variance after the last iteration
 * A NULL guide means its term is left out: not computed, not fetched.  A tap outside [0,W) x [0,H) is skipped -- neither weighted nor
 * added -- in every sum below, and views never see each other.
 *
 * Pack.  a and c0 = hdr / a as in the denoiser section; without albedo c0 = hdr.  var0 = variance > 0 ? variance : 0 (a NaN gives 0)
 * and len = length; with neither plane given var0 = 0 and len = 1 for every pixel.  Luminance everywhere below is
 * l(c) = ((0.2126f*c.r) + (0.7152f*c.g)) + (0.0722f*c.b).  kn and kz are the denoiser section's, formed on the host.
 *
 * Spatial estimate, for a pixel with short_history > 0 && !(len >= short_history), so a NaN length takes this side unless
 * short_history is 0 -- a history too short for its own variance to mean much borrows one from its neighbourhood:
 *   - taps q = (x + dx, y + dy), dy = -2 ... 2 the outer loop and dx = -2 ... 2 the inner one, reading the packed c0.
 *   - the centre has weight w = 1 without evaluation.  Any other tap has eg = (dn*kn) + (dz*kz), dn and dz as in the denoiser
 *     section and an absent guide's term left out, eg = eg < 128.0f ? eg : 128.0f and w = expf(-eg); with no guide at all w = 1
 *     without evaluation.
 *   - s1 = s1 + (w*l_q), s2 = s2 + (w*(l_q*l_q)), ws = ws + w with l_q = l(c0_q), all starting at +0.
 *   - mu = s1/ws, v = (s2/ws) - (mu*mu), v = v > 0 ? v : 0; lc = len > 1 ? len : 1; var = v * (short_history / lc).
 * Every other pixel keeps var = var0.
 *
 * Iteration i = 0 ... iterations - 1 (1 <= iterations <= 8) has step s = 1 << i, reads the previous iteration's {c, var} and writes
 * new ones.  For pixel p = (x, y) of view v:
 *   - prefilter: gv = gs / gw with gs = gs + ((g[dy+1]*g[dx+1]) * var_q) and gw = gw + (g[dy+1]*g[dx+1]) over the neighbours
 *     q = (x + dx, y + dy) at distance 1 (not s), dy = -1 ... 1 outer and dx = -1 ... 1 inner, the centre included, both sums
 *     starting at +0; g = [1/4, 1/2, 1/4].
 *   - kl = 1.0f / ((sigma_luminance * sqrtf(gv)) + 1e-8f), sqrtf correctly rounded.
 *   - the 25 taps of the denoiser section at step s: e = ((fabsf(l(c_p) - l(c_q)) * kl) + (dn*kn)) + (dz*kz), an absent guide's
 *     term left out; e = e < 128.0f ? e : 128.0f (a NaN gives 128); w = (h[dy+2]*h[dx+2]) * expf(-e); the centre has weight 9/64
 *     without evaluation.
 *   - sum_ch = sum_ch + (w*c_q.ch), sv = sv + ((w*w)*var_q), wsum = wsum + w, all starting at +0.
 *   - the new colour is, per channel, wsum > 0 ? sum_ch / wsum : c_p.ch; the new variance wsum > 0 ? sv / (wsum*wsum) : var_p.
 * After the last iteration out = c * a (c without albedo) and variance_out = var.  With var = 0 and neighbouring luminances that
 * differ by more than 128e-8 every off-centre weight is 0: a converged frame comes back as it went in.  The NaN rule of the query
 * section applies: a NaN this arithmetic produces is a NaN everywhere, sign and payload the implementation's.
 *
 * Errors.  Everything is checked before any device work: MIPT_ERR_INVALID_ARG with a message in mipt_last_error() that names the
 * field -- the checks of mipt_denoise (sigma_normal and sigma_depth included), and: only one of variance / length given; a
 * short_history that is not finite and at least 0; a sigma_luminance that is not finite and greater than 0; variance_out, variance or
 * length overlapping anything (out == hdr alone is allowed). */
typedef struct {
    uint32_t width, height, n_views;
    uint32_t iterations;          /* 1 ... 8 */
    float    sigma_luminance, sigma_normal, sigma_depth;
    float    short_history;       /* >= 0, finite: a pixel with a shorter history takes the spatial estimate; 0 = never */
    uint32_t flags;               /* must be 0 */
    uint32_t reserved[7];         /* must be 0 */
} MiptVarianceOptions;            /* 64 B */
typedef struct {
    const float *hdr, *normal, *depth, *albedo;   /* normal, depth, albedo: NULL = absent */
    const float *variance, *length;               /* both or neither */
    float       *out;                             /* may be hdr */
    float       *variance_out;                    /* NULL = not written */
    void        *reserved[8];                     /* must be NULL */
} MiptVarianceBuffers;            /* 128 B */

/* Bytes of workspace mipt_denoise_variance_device needs for this size: three float4 planes, 48 B per pixel.  0 = an invalid size. */
MIPT_API uint64_t mipt_denoise_variance_workspace_bytes(uint32_t width, uint32_t height, uint32_t n_views);
/* HOST buffers, staged through memory of HIP device `device_id`; blocks until done. */
MIPT_API int mipt_denoise_variance(const MiptVarianceOptions *opt, const MiptVarianceBuffers *host, int device_id);
/* DEVICE buffers of one device (e.g. torch tensors) on `hip_stream` (hipStream_t, NULL = the null stream).  Stream-ordered: it does
 * not block and allocates nothing, like mipt_denoise_device.  d_workspace is the caller's: 16-byte aligned device memory of at least
 * mipt_denoise_variance_workspace_bytes().  The call writes `out`, `variance_out` if given and the first
 * mipt_denoise_variance_workspace_bytes() bytes of the workspace, and nothing else. */
MIPT_API int mipt_denoise_variance_device(const MiptVarianceOptions *opt, const MiptVarianceBuffers *device, void *d_workspace,
                                          uint64_t workspace_bytes, void *hip_stream);

/* ---- guided upsampling: a frame traced and filtered at W/k x H/k plus guides at both resolutions -> the frame at W x H ----------------
 * The step that closes the pipeline of the four sections above: a joint-bilateral upsampling filter (Kopf et al. 2007) with albedo
 * demodulation (csrc/upsample.hip).  The trace's cost is linear in the pixels it traces; the first-hit planes cost the same whatever
 * was traced.  So the frame is traced, accumulated and filtered at 1/k of the resolution, and the geometric edges and the textures
 * of the full-resolution frame come from the full-resolution normal, depth, material and albedo planes.  The reference has nothing
 * of this kind: the operation is defined HERE, and the kernels and tests/tools/upsample_model.py obey it bit for bit.  Every
 * operator is one rounded f32 operation, nothing is fused, and the operations run in the order written.
 *
 * Geometry.  width = k*w and height = k*h, k = scale.  cpu.rs:31-35 maps pixel column x to x / width and row r to
 * (height - r) / height: pixel corners, not centres.  Under the same MiptCamera low-resolution pixel (x, y) therefore traces the ray
 * of full-resolution pixel (k*x, k*y) up to the jitter, and full-resolution pixel (X, Y) sits at the low-resolution coordinate
 * (X/k, Y/k) with no half-pixel offset.
 *
 * Buffers.  View-major planar, row 0 = top, the low frame w x h and the full frame width x height:
 *   lo_hdr       3 f32 / low pixel, required: the low-resolution frame, filtered or not
 *   lo_normal    3 f32 / low pixel  }
 *   lo_depth     1 f32 / low pixel  } the guides of the low frame, each optional
 *   lo_albedo    3 f32 / low pixel  }
 *   lo_material  1 u32 / low pixel  }
 *   normal, depth, albedo, material   the same planes per full pixel
 *   out          3 f32 / full pixel, required
 *   weight       1 f32 / full pixel, optional: wsum below; 0 marks a pixel that found no accepted tap
 * A guide is given at both resolutions or at neither; one alone is an error that names the missing one.  An absent guide's term is
 * not computed and not fetched.  The workspace is 32 B per low pixel: two float4 planes.
 *
 * Pack, over the low frame.  a_q = lo_albedo > 1/256 ? lo_albedo : 1/256 per channel (the floor of the denoiser section: a NaN gives
 * the floor) and c_q = lo_hdr / a_q; without albedo c_q = lo_hdr.
 *
 * Full-resolution pixel P = (X, Y) of view v:
 *   - x0 = X / k and rx = X - x0*k in integers; wx = (float)rx / (float)k, ux = 1.0f - wx.  Likewise y0, ry, wy, uy.
 *   - taps q in the order (x0,y0), (x0+1,y0), (x0,y0+1), (x0+1,y0+1) of view v of the low frame, with the bilinear weights
 *     b = ux*uy, wx*uy, ux*wy, wx*wy.
 *   - a tap is skipped when it lies outside [0,w) x [0,h), or when its b is 0 because rx == 0 or ry == 0.  A skipped tap is neither
 *     fetched, nor weighted, nor added to any sum, and views never see each other.
 *   - every tap that takes part adds to the plain bilinear sums: sb_ch = sb_ch + (b * c_q.ch) and bsum = bsum + b, all starting at +0.
 *   - with material: a tap whose lo_material bits differ from the pixel's material bits takes no further part.
 *   - otherwise e = (dn * kn) + (dz * kz), an absent guide's term left out, with dn = ((dx*dx) + (dy*dy)) + (dz*dz) from n_P - n_q,
 *     dz = (z_P - z_q) * (z_P - z_q), and kn, kz formed on the host as in the denoiser section; e = e < 128.0f ? e : 128.0f (a NaN
 *     gives 128); w = b * expf(-e), expf as in the denoiser section.  With neither normal nor depth w = b without evaluation.
 *   - the tap adds to the guided sums: sum_ch = sum_ch + (w * c_q.ch) and wsum = wsum + w, all starting at +0.
 *   - the colour is, per channel, c = wsum > 0 ? sum_ch / wsum : sb_ch / bsum.  bsum > 0 always holds: tap (x0, y0) is never skipped
 *     and its b is above 0.  The second arm is the fallback of a pixel none of whose taps was accepted: plain bilinear.
 *   - a_P = the floor rule applied to the full-resolution albedo; out = c * a_P (c without albedo); weight = wsum.
 * A pixel whose X and Y are multiples of k has one tap, (x0, y0) with b = 1.  The NaN rule of the query section applies: a NaN this
 * arithmetic produces is a NaN everywhere, sign and payload the implementation's.
 *
 * Errors.  Everything is checked before any device work: MIPT_ERR_INVALID_ARG with a message in mipt_last_error() that names the
 * field -- a null opt, buffers, lo_hdr or out; zero width, height or n_views; scale outside 2 ... 8; width or height not a multiple
 * of scale; n_views*W*H >= MIPT_BATCH_MAX_PIXELS; a sigma that fails the denoiser's rule (a sigma given for an absent guide is
 * ignored); a guide given at one resolution only; non-zero flags or reserved fields; any two buffers that overlap -- nothing may
 * alias here; for the device entry a workspace that is NULL, too small, not 16-byte aligned or overlapped by a buffer, a pointer
 * that is not 4-byte aligned, and a pointer that is not device memory of one common device (lo_hdr's). */
typedef struct {
    uint32_t width, height, n_views;   /* the FULL frame */
    uint32_t scale;                    /* k, 2 ... 8; width and height must be multiples of it */
    float    sigma_normal, sigma_depth;
    uint32_t flags;                    /* must be 0 */
    uint32_t reserved[9];              /* must be 0 */
} MiptUpsampleOptions;                 /* 64 B */
typedef struct {
    const float    *lo_hdr;                          /* 3 f32 / low pixel, required */
    const float    *lo_normal, *lo_depth, *lo_albedo;/* 3, 1, 3 f32 / low pixel */
    const uint32_t *lo_material;                     /* 1 u32 / low pixel */
    const float    *normal, *depth, *albedo;         /* the same planes at full resolution */
    const uint32_t *material;
    float          *out;                             /* 3 f32 / full pixel, required */
    float          *weight;                          /* 1 f32 / full pixel, optional: wsum */
    void           *reserved[5];                     /* must be NULL */
} MiptUpsampleBuffers;                 /* 128 B */

/* Bytes of workspace mipt_upsample_device needs for this size: two float4 planes over the low frame, 32 B per low pixel.  0 = an
 * invalid size: a zero, n_views*width*height not below MIPT_BATCH_MAX_PIXELS, a scale outside 2 ... 8 or one that does not divide
 * width and height. */
MIPT_API uint64_t mipt_upsample_workspace_bytes(uint32_t width, uint32_t height, uint32_t n_views, uint32_t scale);
/* HOST buffers, staged through memory of HIP device `device_id`; blocks until done. */
MIPT_API int mipt_upsample(const MiptUpsampleOptions *opt, const MiptUpsampleBuffers *host, int device_id);
/* DEVICE buffers of one device (e.g. torch tensors) on `hip_stream` (hipStream_t, NULL = the null stream).  Stream-ordered: it does
 * not block and allocates nothing, like mipt_denoise_device.  d_workspace is the caller's: 16-byte aligned device memory of at least
 * mipt_upsample_workspace_bytes().  The call writes `out`, `weight` if given and the first mipt_upsample_workspace_bytes() bytes of
 * the workspace, and nothing else. */
MIPT_API int mipt_upsample_device(const MiptUpsampleOptions *opt, const MiptUpsampleBuffers *device, void *d_workspace,
                                  uint64_t workspace_bytes, void *hip_stream);

/* ---- adaptive sampling: per-pixel sample counts, and the map that makes them from the variance plane ----------------------------------
 * The pipeline above measures per pixel how noisy the frame still is; these two operations spend the samples of the next frame where
 * that measurement says they pay.  mipt_render_adaptive* is mipt_render_batch* with one u32 per pixel saying how many samples the pixel
 * gets (csrc/pt_kernel.hip, pt_trace_adaptive_kernel); mipt_sample_map* makes such a plane from a variance plane under a budget on the
 * frame's mean (csrc/sample_map.hip).
 *
 * mipt_render_adaptive.  Everything is as in mipt_render_batch / mipt_render_batch_device -- view-major planes, the same limits, the
 * same flag rules, tile_world 0 or 1 -- with one more argument:
 *   counts : one u32 per pixel, view-major like hdr (pixel p of view v at counts[v*W*H + p]), row 0 = top.
 * Pixel p of view v is traced with n = min(counts[v*W*H + p], opt->samples) samples: opt->samples is the cap the caller promises, so no
 * plane makes a launch longer than mipt_render_batch with the same options.
 *   n > 0  : the pixel's three hdr values are exactly the bytes mipt_render writes for cameras[v] with opt and samples = n -- the mean
 *            over n samples, divided by (float)n as cpu.rs:60 divides by samples as f32 -- in both seed modes, both traversal modes
 *            and both shading modes, and with sample_begin.  With MIPT_FLAG_SUM the pixel holds the undivided sum; with SUM | ACCUM
 *            (device entry) the sum is added to what is there.  rgba8, when given, is the tone-map epilogue over the mean; rgba8
 *            together with MIPT_FLAG_SUM is MIPT_ERR_INVALID_ARG.
 *   n == 0 : no ray is traced.  hdr is +0, +0, +0, or left untouched under MIPT_FLAG_ACCUM.
 *   stats  : pixels counts the pixels with n > 0; under MIPT_FLAG_COUNT the counters are the sums over the traced paths, as in the
 *            batch call.
 * The pixels are handed out in the batch call's order, (view, tile, pixel).  MIPT_FLAG_PACKED and MIPT_FLAG_TOUCHED are refused.
 * Errors: every argument is checked before any device work, with the messages of the batch entry, and: a null counts; for the device
 * entry a counts or d_hdr_rgb that is not 4-byte aligned, a counts that is not device memory of d_hdr_rgb's device, and a counts that
 * overlaps d_hdr_rgb or d_rgba8.  The tile-order and hot-pixel state of the scene handle is neither used nor touched. */
MIPT_API int mipt_render_adaptive(MiptScene *scene, const MiptCamera *cameras, uint32_t n_views, const MiptOptions *opt,
                                  const uint32_t *counts, float *hdr_rgb, uint8_t *rgba8, MiptStats *stats);
/* Same, with DEVICE buffers (d_counts: n_views*W*H u32; d_hdr_rgb: n_views*W*H*3 f32, required; d_rgba8: n_views*W*H*4 bytes, may be
 * NULL) on `hip_stream` (may be NULL).  Blocks until the kernel has finished (stats are read back). */
MIPT_API int mipt_render_adaptive_device(MiptScene *scene, const MiptCamera *cameras, uint32_t n_views, const MiptOptions *opt,
                                         const uint32_t *d_counts, float *d_hdr_rgb, uint8_t *d_rgba8, void *hip_stream, MiptStats *stats);

/* mipt_sample_map: noise in, counts out.  The reference has nothing of this kind: the operation is defined HERE, and the kernels and
 * tests/tools/sample_map_model.py obey it bit for bit.  Every operator is rounded once, nothing is fused, and every comparison is
 * written so that a NaN takes the "zero" side.
 *
 * Buffers.  View-major planar, row 0 = top, N = n_views*width*height pixels:
 *   variance  1 f32 / pixel, required: e.g. variance_out of mipt_denoise_variance, or variance of mipt_temporal
 *   hdr       3 f32 / pixel, optional: the frame the variance belongs to; makes the weight relative
 *   albedo    3 f32 / pixel, optional, only with hdr: hdr is demodulated first
 *   counts    1 u32 / pixel, required: the result
 *
 * Per pixel, in f32:
 *   v = variance > 0 ? variance : 0;  s = sqrtf(v), correctly rounded.
 *   without hdr: w = s.
 *   with hdr: c = hdr, or per channel hdr / a with a = albedo > 1/256 ? albedo : 1/256 (the temporal section's rule);
 *             l = ((0.2126f*c.r) + (0.7152f*c.g)) + (0.0722f*c.b);  l = l > 0 ? l : 0;  w = s / (l + 0.00390625f)
 *             -- the relative standard deviation, so that bright and dark regions compete fairly.
 *   q = w * 4096.0f;  qi = q > 0 ? (q < 16777215.0f ? (uint32_t)q : 16777215u) : 0u.
 * The frame: S = the sum of qi over all N pixels in uint64 -- an integer sum, exact in any order.  The host forms
 * T = (uint64_t)floor((double)budget * (double)N) and E = T - (uint64_t)min_samples * N.
 *   S == 0 : e = min((uint32_t)(E / N), max_samples - min_samples) for every pixel.
 *   else   : in binary64, one rounded operation each: r = (double)E / (double)S, formed once on the device; x = (double)qi * r;
 *            e = x < (double)(max_samples - min_samples) ? (uint32_t)x : max_samples - min_samples.
 *   counts = min_samples + e.
 * So min_samples <= counts <= max_samples and the sum of counts is at most T.  What the clamp at max_samples cuts off is NOT
 * redistributed: budget is an upper bound on the frame's mean sample count, not a target that is met.
 *
 * Errors.  Everything is checked before any device work: MIPT_ERR_INVALID_ARG with a message in mipt_last_error() that names the
 * field -- a null opt, buffers, variance or counts; albedo without hdr; zero width, height or n_views; n_views*W*H >=
 * MIPT_BATCH_MAX_PIXELS; max_samples outside 1 ... 65535; min_samples > max_samples; a budget that is not finite or outside
 * [min_samples, max_samples]; non-zero flags or reserved fields; any two buffers that overlap; for the device entry a workspace that is
 * NULL, not 16-byte aligned or overlapped by a buffer, a pointer that is not 4-byte aligned, and a pointer that is not device memory
 * of one common device (variance's). */
typedef struct {
    uint32_t width, height, n_views;
    uint32_t flags;                   /* must be 0 */
    uint32_t min_samples;             /* 0 <= min_samples <= max_samples */
    uint32_t max_samples;             /* 1 ... 65535 */
    float    budget;                  /* finite, min_samples <= budget <= max_samples: the upper bound on the mean of counts */
    uint32_t reserved[9];             /* must be 0 */
} MiptSampleMapOptions;               /* 64 B */
typedef struct {
    const float *variance;            /* 1 f32 / pixel, required */
    const float *hdr;                 /* 3 f32 / pixel, optional */
    const float *albedo;              /* 3 f32 / pixel, optional, only with hdr */
    uint32_t    *counts;              /* 1 u32 / pixel, required */
    void        *reserved[4];         /* must be NULL */
} MiptSampleMapBuffers;               /* 64 B */

/* Bytes of workspace mipt_sample_map_device needs for this size: S, r and the reduction's ticket, 32 B whatever the size.  0 = an
 * invalid size. */
MIPT_API uint64_t mipt_sample_map_workspace_bytes(uint32_t width, uint32_t height, uint32_t n_views);
/* HOST buffers, staged through memory of HIP device `device_id`; blocks until done. */
MIPT_API int mipt_sample_map(const MiptSampleMapOptions *opt, const MiptSampleMapBuffers *host, int device_id);
/* DEVICE buffers of one device (e.g. torch tensors) on `hip_stream` (hipStream_t, NULL = the null stream).  Stream-ordered: it does
 * not block and allocates nothing, like mipt_denoise_device.  d_workspace is the caller's: 16-byte aligned device memory of at least
 * mipt_sample_map_workspace_bytes().  The call writes `counts` and the first mipt_sample_map_workspace_bytes() bytes of the
 * workspace, and nothing else. */
MIPT_API int mipt_sample_map_device(const MiptSampleMapOptions *opt, const MiptSampleMapBuffers *device, void *d_workspace, void *hip_stream);

/* mipt_sample_map_fill: the same map, but what the clamp at max_samples cuts off is handed on, `rounds` times.  The buffers, qi, S, T,
 * E and span = max_samples - min_samples are mipt_sample_map's, and round 1 is mipt_sample_map itself: it gives e_1(p), the uniform
 * value at S == 0 included.  For each round k = 2 ... rounds:
 *   A   = the sum of e_{k-1}(p) over all pixels, S_k = the sum of qi(p) over the pixels with e_{k-1}(p) < span: uint64 sums, exact in
 *         any order.  E_k = A < E ? E - A : 0.
 *   If S_k == 0 or E_k == 0 the round changes nothing -- and then no later round does, as its sums are the same.
 *   Otherwise r_k = (double)E_k / (double)S_k, formed once on the device, and for each pixel with e_{k-1} < span, in binary64, one
 *   rounded operation each: x = (double)qi * r_k; room = span - e_{k-1}; add = x < (double)room ? (uint32_t)x : room;
 *   e_k = e_{k-1} + add.  Every other pixel keeps e_k = e_{k-1}.
 *   counts = min_samples + e_rounds.
 * So rounds = 1 is mipt_sample_map bit for bit; every count stays in [min_samples, max_samples]; no count falls from one round count
 * to the next, so the sum of counts does not decrease in `rounds`; and the sum never exceeds T, in the rounded arithmetic too.  Round 1
 * leaves A <= E (the argument above).  In round k the exact shares qi * E_k / S_k of the pixels below the span add up to E_k, S_k
 * being the sum of exactly their qi.  (double)S_k, r_k and qi * r_k carry three relative errors of 2^-53, so a pixel's `add` can pass
 * the floor of its exact share only if that share lay within share * 3 * 2^-53 below an integer (the clamp at `room`, an integer, is
 * such a crossing too); `add` is at most span < 2^16, so over N < 2^32 pixels those excesses add up to less than 2^-3, and a sum of
 * integers that exceeds E_k by less than 1 does not exceed it.  The sum of e_k is thus at most A + E_k = E, which is the next round's
 * A <= E; and the sum of counts is at most min_samples * N + E = T after every round.
 * `rounds` passes cost rounds + 1 kernel launches (each pass also forms the next round's two sums). */
typedef struct {
    uint32_t width, height, n_views;
    uint32_t flags;                   /* must be 0 */
    uint32_t min_samples;             /* 0 <= min_samples <= max_samples */
    uint32_t max_samples;             /* 1 ... 65535 */
    float    budget;                  /* finite, min_samples <= budget <= max_samples: the upper bound on the mean of counts */
    uint32_t rounds;                  /* 1 ... 8; 1 = mipt_sample_map */
    uint32_t reserved[8];             /* must be 0 */
} MiptSampleMapFillOptions;           /* 64 B: MiptSampleMapOptions with `rounds` taken from its reserved words */

/* Bytes of workspace mipt_sample_map_fill_device needs: 32 B per round ({S_k, r_k, the ticket, A}).  0 = an invalid size or a
 * `rounds` outside 1 ... 8. */
MIPT_API uint64_t mipt_sample_map_fill_workspace_bytes(uint32_t width, uint32_t height, uint32_t n_views, uint32_t rounds);
/* As mipt_sample_map / mipt_sample_map_device, with their errors and: rounds outside 1 ... 8.  The device entry writes `counts` and
 * the first mipt_sample_map_fill_workspace_bytes() bytes of the workspace, and nothing else. */
MIPT_API int mipt_sample_map_fill(const MiptSampleMapFillOptions *opt, const MiptSampleMapBuffers *host, int device_id);
MIPT_API int mipt_sample_map_fill_device(const MiptSampleMapFillOptions *opt, const MiptSampleMapBuffers *device, void *d_workspace,
                                         void *hip_stream);

/* ---- previous positions: where every pixel's surface point was in the previous geometry ------------------------------------------------
 * The link between the geometry updates and the temporal accumulation above: per pixel the world position that the first hit's
 * surface point had before the last update, to be passed to mipt_temporal as `position` (csrc/first_hit.hip, the MOTION form of the
 * feature kernel).  The reference has nothing of this kind: the value is defined HERE, and the kernel and tests/tools/motion_model.py
 * obey it bit for bit.  Every operator is one rounded f32 operation, nothing is fused, and the operations run in the order written.
 *
 * Ray and hit.  The camera ray of pixel (x, y) of view v is the ray mipt_render_features traces for the FIRST sample of a call with
 * the same opt: the same seed rule, the same sample_begin normalisation (0 -> 1), the same arithmetic.  The hit is
 * Ray::traverse_bvh's winner in the arm opt->traversal / opt->cull_margin select; its u, v and triangle are bit for bit those of
 * mipt_query_closest.  T = the triangle in the caller's order (the `prim` convention without bit 31).
 *
 * Previous corners.  P0, P1, P2 = the positions of corners 0, 1, 2 of triangle T in the previous geometry, from one of two sources:
 *   explicit  prev_tris != NULL: the previous frame's triangle array in the order of mipt_scene_update_triangles, host memory for
 *             mipt_render_motion and device memory for mipt_render_motion_device; n_prev_tris must equal the scene's triangle
 *             count.  Pc = prev_tris[T].vertex[c].position.  Works on any scene and on the replicas of mipt_multi_scene; it suits
 *             callers of mipt_scene_update_triangles_device, who hold two arrays anyway.
 *   tracked   prev_tris == NULL: the previous generation a mesh scene keeps while mipt_scene_track_motion(scene, 1) is on.  Right
 *             after enabling, the previous generation equals the current one.  Every successful mipt_scene_set_transforms or
 *             mipt_scene_update_mesh_device makes what was resident -- the positions array and the part table, with or without
 *             transforms -- the previous generation; a failed update leaves both generations as they were.  Pc = the expansion rule
 *             ("resident indexed meshes") applied to previous position indices[3T + c] with the previous matrix of T's part, so it
 *             equals mipt_mesh_expand(previous mesh)[T].vertex[c].position bit for bit.  Two updates between two frames leave only
 *             the second step tracked: the motion pass then sees the geometry between them as the previous one.
 *             mipt_scene_track_motion(scene, 0) frees what tracking holds (a copy of the positions and a third part table);
 *             MiptMeshInfo.array_bytes and hbm_bytes include it while tracking is on.  A scene without a mesh is refused.
 *
 * Value.  w = (1.0f - u) - v; per component prev = ((P0*w) + (P1*u)) + (P2*v) -- the order the feature pass uses for the normal.  A
 * miss writes (0, 0, 0), as `position` does.  The NaN rule of the query section applies.
 *
 * Options and stats.  opt is read exactly as mipt_render_features reads it; samples is validated as there and otherwise unused (only
 * the first sample is traced); MIPT_FLAG_COUNT is refused.  Stats (may be NULL): kernel_ms, stack_overflows, tex_clamped = 0,
 * pixels = n_views*W*H; every other field 0.
 *
 * Normal check.  With prev_position as mipt_temporal's `position` the normal check still compares this frame's normal with the
 * history's: a part that turns by more than normal_tol allows starts anew instead of ghosting.  A previous-frame normal is out of scope.
 *
 * Errors.  Every argument is checked before any device work: MIPT_ERR_INVALID_ARG with a message in mipt_last_error() that names the
 * field -- everything mipt_render_features checks; a null prev_position; a non-zero reserved0 or non-NULL reserved pointer;
 * n_prev_tris that is not the scene's triangle count; prev_tris == NULL on a scene that is not a mesh tracking motion; for the
 * _device entry a pointer that is not 4-byte aligned or not device memory of the scene's device.  A traversal-stack overflow is
 * MIPT_ERR_STACK after the buffer is written.  After any error the scene renders and queries as before. */
typedef struct {
    const MiptTriangle *prev_tris;   /* NULL = the generation the scene tracks (mesh scenes) */
    uint32_t n_prev_tris, reserved0; /* reserved0 must be 0 */
    float   *prev_position;          /* 3 f32 / pixel, view-major, row 0 = top; required */
    void    *reserved[5];            /* must be NULL */
} MiptMotionBuffers;                 /* 64 B */

/* Into a HOST buffer, prev_tris (if given) in HOST memory; blocks until done. */
MIPT_API int mipt_render_motion(MiptScene *scene, const MiptCamera *cameras, uint32_t n_views, const MiptOptions *opt,
                                const MiptMotionBuffers *host, MiptStats *stats);
/* Into a DEVICE buffer, prev_tris (if given) in DEVICE memory, on `hip_stream` (hipStream_t, NULL = the null stream); blocks until the
 * kernel has finished (stats are read back), like mipt_render_features_device. */
MIPT_API int mipt_render_motion_device(MiptScene *scene, const MiptCamera *cameras, uint32_t n_views, const MiptOptions *opt,
                                       const MiptMotionBuffers *device, void *hip_stream, MiptStats *stats);
/* enable != 0: keep the previous generation of a mesh scene from now on (it starts equal to the current one); 0: free it. */
MIPT_API int mipt_scene_track_motion(MiptScene *scene, uint32_t enable);

/* Tile-shard helpers (image tiles shard across GPUs; one RCCL all-gather of packed slices). */
MIPT_API uint64_t mipt_packed_pixels(uint32_t width, uint32_t height, uint32_t tile_world);
/* d_packed_all: tile_world slices of mipt_packed_pixels()*3 floats, rank-major (the layout an
 * all-gather produces); writes the full width*height*3 frame. */
MIPT_API int mipt_unpack_tiles(const float *d_packed_all, uint32_t width, uint32_t height,
                      uint32_t tile_world, float *d_hdr_rgb, void *hip_stream);
/* linear HDR -> sRGB -> RGBA8 epilogue on device (vec3.rs:80-90, 262-270; cpu.rs:61-64).
 * The radiance is first divided by `divisor` (the sample count for a summed buffer, cpu.rs:60;
 * 1 for a buffer that already holds the mean). */
MIPT_API int mipt_tonemap_device(const float *d_hdr_rgb, uint64_t n_pixels, float divisor,
                        uint8_t *d_rgba8, void *hip_stream);

/* The wgpu backend's post-process pass (pp_compute.wgsl:7-34): radiance / divisor, clamped to [0,1] (its accumulator is
 * rgba16unorm), linear_to_srgb, THEN aces_filmic, written as RGBA16 unorm (4 x u16 per pixel, alpha 65535) -- the pixel
 * format Renderer::render saves (renderer.rs:67-73, ColorType::Rgba16).  The CPU backend's epilogue is mipt_tonemap_device. */
MIPT_API int mipt_postprocess_device(const float *d_hdr_rgb, uint64_t n_pixels, float divisor, uint16_t *d_rgba16, void *hip_stream);

/* ---- all GPUs of one node behind one call --------------------------------------------- */

/* The reference's host is a single process with one Rc<RefCell<Scene>> (src/main.rs:46) and a blocking
 * `match backend` arm (src/renderer.rs:57-63), so its multi-GPU arm must be one call from one thread.
 * A MiptMulti holds a scene replica, a HIP stream and an RCCL communicator (ncclCommInitAll) per device. */
typedef struct MiptMulti MiptMulti;

enum MiptMultiMode {
    MIPT_MULTI_TILES   = 0,  /* 8x8 image tiles round-robin over the devices (pixel seeds, cpu.rs:28-29, make the frame
                              * bit-identical to the single-GPU frame); ONE ncclGather of rank-packed f32 slices to
                              * device 0 over xGMI + a de-interleave kernel.  BASELINE config 4. */
    MIPT_MULTI_SAMPLES = 1   /* every device renders all pixels for a disjoint sample range with the per-sample seeds of
                              * rt_compute.wgsl:102 (seed_mode is forced to MIPT_SEED_PER_SAMPLE: the pixel stream cannot be
                              * entered mid-way) into un-normalised sums; ONE ncclReduce(sum, f32) to device 0, then / samples.
                              * The f32 sum order differs from a sequential accumulation.  BASELINE config 5. */
};

typedef struct {
    MiptStats total;              /* counters summed over devices; kernel_ms = the slowest device's trace kernel */
    double    collective_ms;      /* gather/reduce + assemble (+ tonemap) on device 0's stream, HIP events */
    double    wall_ms;            /* the whole call on the host clock; mipt_render_multi: incl. the D2H copy of the outputs */
    double    device_kernel_ms[8];/* trace-kernel time of devices 0..7 */
    uint32_t  n_devices, reserved;
} MiptMultiStats;

/* device_ids: n_devices HIP device ordinals (NULL = 0..n_devices-1; n_devices 0 = every visible device).  The scene crosses PCIe
 * ONCE, to device_ids[0]; the other replicas are device-to-device copies over xGMI, all queued before the first is waited for
 * (pulls from one GPU use one link per destination).  Creates the communicators. */
MIPT_API int  mipt_multi_create(const MiptSceneDesc *desc, const int *device_ids, int n_devices, MiptMulti **out);
/* Same from the triangles alone (mipt_scene_create_from_triangles on device_ids[0], then the xGMI replicas). */
MIPT_API int  mipt_multi_create_from_triangles(const MiptSceneDesc *desc, const int *device_ids, int n_devices, MiptMulti **out);
/* The replica on device `index` (0 .. mipt_multi_device_count()-1), owned by `multi`: for mipt_scene_info / mipt_scene_get_bvh. */
MIPT_API MiptScene *mipt_multi_scene(MiptMulti *multi, int index);
MIPT_API void mipt_multi_destroy(MiptMulti *multi);
MIPT_API int  mipt_multi_device_count(const MiptMulti *multi);

/* Renders one frame on all devices of `multi` into HOST buffers (either may be NULL) and blocks until done; same outputs
 * as mipt_render.  `opt` describes the whole frame: tile_rank / tile_world / sample_begin and the PACKED / SUM / ACCUM
 * flags must be 0 (the call owns the sharding); MIPT_FLAG_COUNT is honoured. */
MIPT_API int  mipt_render_multi(MiptMulti *multi, const MiptCamera *camera, const MiptOptions *opt, uint32_t mode,
                       float *hdr_rgb, uint8_t *rgba8, MiptMultiStats *stats);

/* Same, but the frame stays in HBM: d_hdr_rgb (width*height*3 f32, required) and d_rgba8 (width*height*4 bytes, may be
 * NULL) are buffers in the memory of the ROOT device (mipt_multi_root_device(): device_ids[0]); the assemble kernels write
 * them directly and nothing crosses PCIe.  The multi-GPU counterpart of mipt_render_device. */
MIPT_API int  mipt_render_multi_device(MiptMulti *multi, const MiptCamera *camera, const MiptOptions *opt, uint32_t mode,
                              float *d_hdr_rgb, uint8_t *d_rgba8, MiptMultiStats *stats);
/* HIP ordinal of the device that gathers / reduces and holds the assembled frame, or a negative MiptStatus. */
MIPT_API int  mipt_multi_root_device(const MiptMulti *multi);
/* Trace-kernel stats of device `index` (0 .. mipt_multi_device_count()-1) in the last mipt_render_multi* call:
 * MiptMultiStats.total sums the counters, this is one device's share (what its one launch did). */
MIPT_API int  mipt_multi_device_stats(const MiptMulti *multi, int index, MiptStats *out);

/* ---- updating the geometry of a resident scene ------------------------------------------------------------------------
 * The reference's realtime loop mutates its Rc<RefCell<Scene>> (src/main.rs:46) and restarts progressive accumulation
 * (window.rs:349-389); these calls swap new triangles into an existing scene (or MiptMulti) without re-uploading its materials,
 * texel pool or workspace.  They add nothing to the frame itself: after a successful call the scene renders exactly as a scene
 * created from the new geometry would (see each mode).
 *
 * Triangle order: `tris` holds the triangles in the order of the array the scene was last built from -- for mipt_scene_create the
 * tree order the caller passed; for mipt_scene_create_from_triangles the caller's own order (the one mipt_scene_get_bvh's
 * tri_order_out maps); after a REBUILD the order of that call's input.  So a caller keeps writing into its own mesh array and
 * passes it again.  The array is read during the call only; it is neither kept nor modified.
 *
 * Errors are status codes with a message in mipt_last_error(), and in every case the scene renders exactly as before the call
 * (everything is validated before anything resident is overwritten): a null argument, n_tris == 0 or a bad mode:
 * MIPT_ERR_INVALID_ARG; a REFIT whose n_tris differs from the scene's: MIPT_ERR_INVALID_ARG; material_id >= n_materials:
 * MIPT_ERR_INVALID_ARG; a bound that comes out non-finite or beyond 2^40: MIPT_ERR_SCENE_LIMIT (mipt_scene_create's rule); more
 * than 2^25 triangles on REBUILD: MIPT_ERR_SCENE_LIMIT. */
enum MiptUpdateMode {
    MIPT_UPDATE_REFIT   = 0,  /* same tree topology, bounds recomputed from the new triangles.  n_tris must equal the scene's.  The
                               * pair-record order and the triangle slots stay; every bound becomes what Node::grow_by_tri
                               * (bvh.rs:185-193) folds over that node's triangles; both triangle streams are rewritten (material_ids
                               * may change).  The layout equals mipt_scene_create's from the new triangles in tree order and the old
                               * node array with refit bounds, byte for byte (sign of a zero in a bound aside), except that the pair
                               * records keep the order of the original tree (a fresh layout orders its lower levels by child surface
                               * area, which the new bounds may change).  A scene that keeps its
                               * tree (mipt_scene_get_bvh) returns the refit node array afterwards.  The first REFIT of a tree groups
                               * its pair records by depth and keeps that plan in HBM (8 bytes per record) until the tree changes. */
    MIPT_UPDATE_REBUILD = 1   /* BVH::build on the GPU from the new triangles (the count may change): the scene becomes what
                               * mipt_scene_create_from_triangles would have made from them -- the same layout bytes, mipt_scene_get_bvh
                               * and MiptSceneInfo size fields, built_on_device = 1 -- and keeps its materials, textures and
                               * workspace.  Works for scenes made either way. */
};
typedef struct {
    double   upload_ms;       /* host -> device copy of the triangles (0 for the _device entry) */
    double   build_ms;        /* device kernels of the refit / the build, HIP events */
    double   layout_ms;       /* rewriting pair records + both triangle streams */
    double   total_ms;        /* whole call, host clock */
    uint32_t n_tris, n_nodes, n_pair_records, reserved;
} MiptUpdateInfo;

/* `tris` in host memory: staged into HBM of the scene's device, then the same device path as below.  info may be NULL. */
MIPT_API int mipt_scene_update_triangles(MiptScene *scene, const MiptTriangle *tris, uint32_t n_tris,
                                         uint32_t mode, MiptUpdateInfo *info);
/* `d_tris` in HBM of the scene's device (e.g. a torch tensor); the triangles never cross PCIe and REBUILD builds straight from
 * them.  Ordered after the earlier work of `hip_stream` (hipStream_t, NULL = the null stream); blocks until done, like
 * mipt_render_device.  info may be NULL. */
MIPT_API int mipt_scene_update_triangles_device(MiptScene *scene, const MiptTriangle *d_tris, uint32_t n_tris,
                                                uint32_t mode, void *hip_stream, MiptUpdateInfo *info);
/* Updates the root replica (device_ids[0]) from host `tris`, then refreshes every other replica by device-to-device copies (the
 * mechanism of mipt_multi_create).  Handles returned by mipt_multi_scene stay valid.  On success mipt_render_multi* in both modes
 * equals a single-GPU render of the updated scene.  An error in a replica refresh (MIPT_ERR_HIP) leaves the root updated: destroy
 * the MiptMulti then. */
MIPT_API int mipt_multi_update_triangles(MiptMulti *multi, const MiptTriangle *tris, uint32_t n_tris,
                                         uint32_t mode, MiptUpdateInfo *info);

/* ---- resident indexed meshes ------------------------------------------------------------------------------------------
 * What a caller holds before scene.rs:48-76 expands it -- vertex arrays plus index triples, cut into objects ("parts") -- kept in
 * HBM and expanded to fat triangles ON THE GPU (csrc/scene_mesh.hip).  A scene made from a mesh is animated by one 4x4 matrix per
 * part (64 B each over PCIe) or by new vertex arrays already in HBM; the expanded array then goes through MIPT_UPDATE_REFIT /
 * _REBUILD above.  The trace kernels see an ordinary scene.
 *
 * Expansion rule (mipt_mesh_expand, the expansion kernel and tests/tools/mesh_model.py obey it bit for bit; every operator is one
 * rounded f32 operation, nothing is fused):
 *   - triangle t of part p, corner c: Vertex{position, tex_coord_x, normal, tex_coord_y} from the three indexed arrays (entry
 *     3*t + c of each index stream), material_id = parts[p].material_id, _pad = 0.  Output order: part order, then triangle order
 *     -- "the caller's order" of mipt_scene_create_from_triangles / mipt_scene_get_bvh.
 *   - a normal / tex-coord index >= its array's count (UINT32_MAX, or any index when the array is NULL) gives zeros
 *     (unwrap_or(&[0.0; _]), scene.rs:56-65).  A POSITION index out of range is MIPT_ERR_INVALID_ARG (the message names the first
 *     offending index entry); on the device the expansion kernel detects it before anything resident is replaced.
 *   - transforms == NULL: no arithmetic, attribute bits are copied (-0.0, NaN payloads and infinities survive).
 *   - with a transform M of the part (Mat4f data[col][row], mat4.rs:6-10; columns a0,a1,a2 = data[0..2][0..2], translation
 *     t = data[3][0..2], row 3 ignored): p' = M*p + t in the operation order of mat4.rs:146-149, x' = ((a0.x*p.x + a1.x*p.y) +
 *     a2.x*p.z) + t.x.  Normal: c = c0*n.x + c1*n.y + c2*n.z in the same order with the cofactor columns c0 = cross(a1,a2),
 *     c1 = cross(a2,a0), c2 = cross(a0,a1) (vec3.rs:137-143), which keeps the normal on the side of the moved triangle's winding
 *     even under a mirror; its length is kept (the CPU shading path uses the un-normalised normal, ray.rs:179-180):
 *     L0 = length(n), L1 = length(c) (vec3.rs:94-96); L1 > 0 and finite: n' = c * (L0 / L1), else n' = c.  Tex coords are copied.
 *     (A NaN that this arithmetic produces is a NaN everywhere; its sign and payload are the implementation's, as in IEEE 754.)
 *
 * Errors: everything is validated before anything resident is overwritten, and after any error the scene renders exactly as
 * before.  The host-visible checks (null pointers, n_indices % 3, parts not tiling the index range, reserved != 0, material_id >=
 * n_materials, n_parts mismatch, bad mode, no triangles: MIPT_ERR_INVALID_ARG; more than 2^25 triangles: MIPT_ERR_SCENE_LIMIT) run
 * before any device call.  A bound that comes out non-finite or beyond 2^40 after a transform: MIPT_ERR_SCENE_LIMIT from the update
 * path.  mipt_scene_update_triangles{,_device} on a scene that owns a mesh and every mesh call on a scene without one:
 * MIPT_ERR_INVALID_ARG.  Replicas (MiptMulti) are made from the geometry only: a replica of a mesh scene is a plain scene. */
typedef struct {            /* one object: a run of triangles with one material and one transform (16 B) */
    uint32_t first_tri;     /* first triangle of the part; corner c of triangle t is index entry 3*t + c */
    uint32_t n_tris;        /* may be 0 */
    uint32_t material_id;   /* Triangle.material_id of every triangle of the part */
    uint32_t reserved;      /* must be 0 */
} MiptMeshPart;

typedef struct {
    const float    *positions;   uint32_t n_positions;    /* 3 f32 each */
    const float    *normals;     uint32_t n_normals;      /* 3 f32 each; NULL / 0 allowed */
    const float    *tex_coords;  uint32_t n_tex_coords;   /* 2 f32 each; NULL / 0 allowed */
    const uint32_t *indices;     uint32_t n_indices;      /* 3 per triangle: position index of each corner */
    const uint32_t *normal_indices;                       /* n_indices entries, NULL = use `indices` */
    const uint32_t *tex_coord_indices;                    /* n_indices entries, NULL = use `indices` */
    const MiptMeshPart *parts;   uint32_t n_parts;        /* must tile [0, n_indices/3) in order, no gaps, no overlap */
    const float    *transforms;                           /* n_parts x 16 f32, Mat4f data[col][row] (mat4.rs:6-10); NULL = none */
} MiptMeshDesc;

typedef struct {
    uint32_t n_positions, n_normals, n_tex_coords, n_indices;
    uint32_t n_tris, n_parts;
    uint32_t has_transforms;      /* 1: the last successful create / update applied per-part matrices */
    uint32_t index_streams;       /* index arrays held: 1 (shared) ... 3 */
    uint64_t array_bytes;         /* HBM held for vertex arrays, index streams, part records and the transform staging buffer */
    uint64_t expanded_bytes;      /* HBM held for the expanded triangle array (112 B per triangle), kept between updates */
    uint64_t hbm_bytes;           /* the sum: what the mesh costs on top of MiptSceneInfo.geometry_bytes */
} MiptMeshInfo;

/* The expansion rule on the host: writes n_indices / 3 triangles to `out` (cap >= that, else MIPT_ERR_INVALID_ARG) and their count to
 * n_out (may be NULL).  No device is touched; parts[].material_id is copied unchecked (there is no material table here). */
MIPT_API int mipt_mesh_expand(const MiptMeshDesc *mesh, MiptTriangle *out, uint32_t cap, uint32_t *n_out);

/* `desc` supplies materials and textures (tris / nodes are ignored).  The mesh arrays cross PCIe once, stay resident and are expanded
 * by the GPU; BVH::build and the layout then run as in mipt_scene_create_from_triangles.  The result is THAT scene: the layout bytes,
 * mipt_scene_get_bvh and the size fields of MiptSceneInfo equal those of mipt_scene_create_from_triangles(mipt_mesh_expand(mesh));
 * upload_ms includes the mesh arrays, build_ms the expansion kernel. */
MIPT_API int mipt_scene_create_from_mesh(const MiptSceneDesc *desc, const MiptMeshDesc *mesh, int device_id, MiptScene **out);

/* New per-part matrices from HOST memory (n_parts x 16 f32; n_parts must equal the mesh's; NULL = back to no transforms): 64 B per
 * part are copied, the resident mesh is expanded again and the scene updated with `mode` (MiptUpdateMode).  info (may be NULL):
 * upload_ms = the matrix copy; build_ms = the update's build_ms + the HIP-event time of the expansion kernels; layout_ms as above. */
MIPT_API int mipt_scene_set_transforms(MiptScene *scene, const float *transforms, uint32_t n_parts, uint32_t mode, MiptUpdateInfo *info);

/* A deforming mesh from HBM of the scene's device (e.g. torch tensors): each pointer may be NULL = keep what is resident; the
 * counts are the resident mesh's (the topology is fixed; d_transforms: n_parts x 16 f32).  The arrays are read, not modified; after
 * a successful update they replace the resident copies (device-to-device).  Ordered after the earlier work of `hip_stream`
 * (hipStream_t, NULL = the null stream); blocks until done.  build_ms includes the expansion as above; upload_ms = 0. */
MIPT_API int mipt_scene_update_mesh_device(MiptScene *scene, const float *d_positions, const float *d_normals, const float *d_transforms,
                                           uint32_t mode, void *hip_stream, MiptUpdateInfo *info);

/* What the scene's mesh holds.  MIPT_ERR_INVALID_ARG for a scene without a mesh. */
MIPT_API int mipt_scene_mesh_info(const MiptScene *scene, MiptMeshInfo *out);

/* ---- host-side restatements of the scene model that feeds the path ------------------- */

/* BVH::build (src/bvh.rs:13-161): binned SAH, 8 bins; reorders `tris` in place exactly as
 * bvh.rs:99-108 does and emits the identical node array.  nodes_cap >= 2*n_tris-1.
 * threads: 0 = hardware concurrency. */
MIPT_API int mipt_bvh_build(MiptTriangle *tris, uint32_t n_tris, MiptNode *nodes_out,
                   uint32_t nodes_cap, uint32_t *n_nodes_out, uint32_t threads);

/* Scene::load for Wavefront OBJ + MTL (src/scene.rs:22-85, src/loader/obj.rs:16-436): parses the
 * file, expands indexed faces into fat triangles and runs BVH::build.  The returned object owns
 * host arrays; mipt_obj_get fills a MiptSceneDesc that borrows them (valid until mipt_obj_free)
 * and, optionally, the material names in material-id order. */
typedef struct MiptObj MiptObj;
MIPT_API int  mipt_obj_load(const char *path, MiptObj **out);
/* The same without BVH::build (scene.rs:80): triangles in file order, no nodes (mipt_obj_get: nodes = NULL, n_nodes = 0) -- the input
 * of mipt_scene_create_from_triangles, which builds the tree on the GPU.  (A 10 M-triangle file: parsing takes seconds on 16 cores,
 * the host BVH build ten times that.) */
MIPT_API int  mipt_obj_load_triangles(const char *path, MiptObj **out);
MIPT_API int  mipt_obj_get(MiptObj *obj, MiptSceneDesc *desc_out, const char ***material_names_out);
MIPT_API void mipt_obj_free(MiptObj *obj);

/* Texture::load (src/texture.rs:13-31): decodes an image file (PNG, JPEG, TGA, BMP or binary PPM, chosen by extension like
 * image::open), flips it vertically and expands to RGBA8; hash_out (may be NULL) receives the djb2 hash the loader
 * de-duplicates textures by (texture.rs:40-48).  desc_out borrows the image's pixels until mipt_texture_free. */
typedef struct MiptImage MiptImage;
MIPT_API int  mipt_texture_load(const char *path, MiptImage **out, MiptTexture *desc_out, uint32_t *hash_out);
MIPT_API void mipt_texture_free(MiptImage *img);

/* The image output of Renderer::render (src/renderer.rs:66-83, image::save_buffer): writes width x height RGBA pixels,
 * top row first, as a PNG with 8 or 16 bits per sample (16-bit samples in host byte order; the reference saves
 * ColorType::Rgba16, and the bytes of its CPU arm are RGBA8 -- SURVEY T12).  Uncompressed deflate blocks. */
MIPT_API int mipt_image_save_png(const char *path, uint32_t width, uint32_t height, uint32_t bits_per_sample, const void *rgba);

/* The same build on the GPU (level-synchronous binned SAH with the partition's closed-form permutation); identical output
 * (sign of zero in a bound aside).  Uploads `tris`, downloads the reordered triangles and the nodes; build_ms_out (may be
 * NULL) receives the device time of the build itself without the transfers. */
MIPT_API int mipt_bvh_build_device(MiptTriangle *tris, uint32_t n_tris, MiptNode *nodes_out, uint32_t nodes_cap,
                          uint32_t *n_nodes_out, int device_id, double *build_ms_out);

/* Camera::update_view + Mat4f::look_at (src/scene.rs:181-194, src/math/mat4.rs:25-44). */
MIPT_API int mipt_camera_from_pose(const float position[3], float pitch_deg, float yaw_deg, MiptCamera *out);

/* Material::default() (src/scene.rs:148-167). */
MIPT_API void mipt_material_default(MiptMaterial *out);

MIPT_API const char *mipt_last_error(void);
MIPT_API int mipt_abi_version(void);
/* number of HIP devices visible, or a negative MiptStatus */
MIPT_API int mipt_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* MIPT_H */
