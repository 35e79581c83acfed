/*
 * pt_oracle.h -- CPU ORACLE (test infrastructure, NOT product code).
 *
 * A plain-C restatement of the reference's rayon CPU path tracer
 * (MiksuNy/rust_ray_tracing, src/renderer/backend/cpu.rs + cpu/ray.rs and the
 * math / scene / bvh pieces they call).  Only tests/, __graft_entry__.smoke()
 * and bench.py's cpu_baseline leg may load this library; the product
 * (rust_ray_tracing_amd/csrc, libmipt.so) never links, includes or calls it.
 *
 * PARITY STATUS: "parity unpinned" by the reference -- the reference ships no
 * tests, golden vectors or fixtures and cannot be compiled here
 * (Rust toolchain absent).  The oracle is pinned instead by the
 * hand-derived known answers of SURVEY.md Appendix B (tests/test_oracle_kat.py),
 * by goldens it emitted itself (tests/golden/), and by a second restatement written
 * from the Rust sources independently (pt_oracle_py.py) that must agree with it bit
 * for bit (tests/test_oracle_second_reading.py).
 *
 * Every function cites the reference file:line it follows.
 */
#ifndef PT_ORACLE_H
#define PT_ORACLE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- PODs: byte-identical to the reference's #[repr(C, align(16))] structs ---- */
typedef struct { float x, y, z; } OrcVec3;                    /* math/vec3.rs:55-59 */

typedef struct {                                              /* scene.rs:87-94   */
    OrcVec3 position; float tex_coord_x;
    OrcVec3 normal;   float tex_coord_y;
} OrcVertex;                                                  /* 32 B */

typedef struct {                                              /* scene.rs:97-103  */
    OrcVertex vertices[3];
    uint32_t  material_id;
    uint8_t   _pad[12];
} OrcTriangle;                                                /* 112 B */

typedef struct {                                              /* bvh.rs:164-171   */
    OrcVec3  bounds_min; uint32_t first_tri_or_child;
    OrcVec3  bounds_max; uint32_t num_tris;
} OrcNode;                                                    /* 32 B */

typedef struct {                                              /* scene.rs:129-146 */
    OrcVec3 base_color;    float transmission;
    OrcVec3 specular_tint; float ior;
    OrcVec3 emission;      float roughness;
    float metallic, transparency;
    uint32_t base_color_tex_id, transparency_tex_id, roughness_tex_id,
             metallic_tex_id, emission_tex_id, normal_tex_id;
} OrcMaterial;                                                /* 80 B */

typedef struct {                                              /* gpu.rs:480-486   */
    float   look_at[4][4];       /* data[col][row], mat4.rs:6-10 */
    OrcVec3 position; float _pad;
} OrcCamera;                                                  /* 80 B */

typedef struct {                                              /* texture.rs:4-10  */
    uint32_t width, height;
    const uint8_t *rgba8;        /* width*height*4, already v-flipped */
} OrcTexture;

enum { ORC_SEED_PIXEL_STREAM = 0,   /* cpu.rs:28-29           */
       ORC_SEED_PER_SAMPLE   = 1 }; /* rt_compute.wgsl:102    */
enum { ORC_LIBM_GLIBC235 = 0,       /* restated glibc 2.35 cosf/log10f/powf (same spec as the kernel) */
       ORC_LIBM_HOST = 1 };         /* this process's libm = what the Rust binary would call     */

typedef struct {
    uint32_t width, height;          /* renderer.rs:100 output_image_dimensions */
    uint32_t samples;                /* renderer.rs:98  */
    uint32_t max_ray_depth;          /* renderer.rs:99  */
    uint32_t seed_mode;              /* ORC_SEED_*      */
    uint32_t cull;                   /* 0 = cpu/ray.rs:69-81 (no t-max cull); 1 = rt_compute.wgsl:341-349 */
    uint32_t libm;                   /* ORC_LIBM_*      */
    uint32_t threads;                /* 0 = hardware concurrency */
    uint64_t pix_begin, pix_end;     /* pixel-index range (end 0 = width*height) */
    uint32_t pix_stride;             /* 0/1 = every pixel */
    uint32_t sample_begin;           /* PER_SAMPLE mode: first sample number (>=1), 0 -> 1 */
    uint32_t stack_cap;              /* traversal stack entries; 0 -> 64 (reference: 32, ray.rs:85) */
    uint32_t sum_only;               /* 1: hdr = sum over samples (no /samples), for sample-sharding */
    float    cull_margin;            /* cull=1: skip a child iff !(t_near < best*(1+margin)); 0 = the WGSL rule */
    uint32_t shading;                /* 0 = cpu/ray.rs trace; 1 = rt_compute.wgsl trace (GGX/Fresnel/refraction/RR; per-sample seeds) */
    uint32_t spread_pages;           /* timing aid (bench.py cpu_baseline): 0 = read the caller's arrays where they lie -- the reference's
                                      * `Vec`s are allocated and filled by the main thread (scene.rs:44-85), so on a multi-socket host all
                                      * pages sit on one NUMA node; 1 = first copy tris and nodes into fresh mappings, each worker thread
                                      * copying (first-touching) one 1/T share, so the pages spread over the nodes the workers run on */
} OrcOptions;

typedef struct {
    uint64_t rays;            /* traverse_bvh invocations (ray.rs:150)                 */
    uint64_t inner_steps;     /* inner-node visits (two child slab tests each)         */
    uint64_t tri_tests;       /* intersect_tri calls                                   */
    uint64_t hits;            /* rays that hit something                               */
    uint64_t texel_fetches;   /* Texture::color_at calls                               */
    uint64_t stack_overflows; /* pushes dropped because the stack was full             */
    uint64_t max_stack;       /* deepest stack occupancy seen                          */
    uint64_t tex_clamped;     /* texel index clamped (reference would panic, T10)      */
    double   seconds;         /* wall time of the pixel loop                           */
    uint32_t threads_used;
    uint32_t n_blocks;        /* uniform pixel blocks handed out (cpu.rs:22-26)        */
    double   block_sec_max;   /* slowest block                                         */
    double   block_sec_mean;  /* mean block time: max/mean = the imbalance rayon's by_uniform_blocks leaves */
} OrcStats;

/* bvh.rs:13-161.  Reorders tris in place, writes <= 2*n-1 nodes. */
int orc_bvh_build(OrcTriangle *tris, uint32_t n_tris, OrcNode *nodes_out,
                  uint32_t nodes_cap, uint32_t *n_nodes_out);

/* scene.rs:181-194 + mat4.rs:25-44 */
void orc_camera_from_pose(const float position[3], float pitch_deg, float yaw_deg,
                          OrcCamera *out);

/* cpu.rs:13-68.  hdr: width*height*3 f32 linear mean (or sum), may be NULL.
 * rgba8: width*height*4, may be NULL.  Returns 0 or a negative error. */
int orc_render(const OrcTriangle *tris, uint32_t n_tris,
               const OrcNode *nodes, uint32_t n_nodes,
               const OrcMaterial *materials, uint32_t n_materials,
               const OrcTexture *textures, uint32_t n_textures,
               const OrcCamera *camera, const OrcOptions *opt,
               float *hdr, uint8_t *rgba8, OrcStats *stats);

/* record-visit trace for layout analysis (tests/tools/layout_model.py); see pt_oracle.c */
uint64_t orc_visit_log(const OrcTriangle *tris, uint32_t n_tris, const OrcNode *nodes, uint32_t n_nodes,
                       const OrcMaterial *materials, uint32_t n_materials, const OrcTexture *textures, uint32_t n_textures,
                       const OrcCamera *camera, const OrcOptions *opt, uint64_t pix_begin, uint64_t pix_stride, uint64_t n_pixels,
                       uint32_t *log, uint64_t cap);
uint32_t orc_debug_pixel(const OrcTriangle *tris, uint32_t n_tris, const OrcNode *nodes, uint32_t n_nodes,
                         const OrcMaterial *materials, uint32_t n_materials,
                         const OrcTexture *textures, uint32_t n_textures,
                         const OrcCamera *camera, const OrcOptions *opt, uint64_t pixel_index,
                         float *records, uint32_t rec_cap, float out_rgb[3]);

/* pp_compute.wgsl:7-34 (sRGB then ACES filmic, unorm16 RGBA) */
void orc_postprocess(const float *hdr, uint64_t n_pixels, float divisor, int libm, uint16_t *out);

/* ---- small entry points for the known-answer tests ---- */
uint32_t orc_pixel_seed(uint32_t index);                        /* cpu.rs:28-29 */
uint32_t orc_sample_seed(uint32_t s, uint32_t x, uint32_t y);   /* rt_compute.wgsl:102 */
uint32_t orc_xor_shift(uint32_t *state);                        /* math.rs:6-13 */
float    orc_rand_f32(uint32_t *state);                         /* math.rs:22-24 */
float    orc_rand_f32_nd(uint32_t *state, int libm);            /* math.rs:15-19 */
void     orc_rand_in_unit_sphere(uint32_t *state, int libm, float out[3]); /* vec3.rs:66-68 */
float    orc_intersect_node(const float o[3], const float d[3], const OrcNode *n); /* ray.rs:69-81 */
/* ray.rs:19-67: out = {has_hit, t, u, v, front_face, nx,ny,nz, uvx,uvy, px,py,pz} */
void     orc_intersect_tri(const float o[3], const float d[3], const OrcTriangle *t, float out[13]);
void     orc_linear_to_srgb(const float in[3], int libm, float out[3]);  /* vec3.rs:80-90 */
void     orc_quantize(const float in[3], uint8_t out[3]);       /* vec3.rs:262-270 */
void     orc_texture_color_at(const OrcTexture *t, float u, float v, uint8_t out[4]); /* texture.rs:33-38 */
/* the same lookup on n pairs, with the flag trace adds to tex_clamped per lookup (clamped_out may be NULL); returns the flags' sum */
uint64_t orc_texture_lookup_many(const OrcTexture *t, const float *u, const float *v, uint64_t n, uint8_t *rgba_out, uint8_t *clamped_out);
void     orc_pixel_screen(uint32_t index, uint32_t w, uint32_t h, float out[2]); /* cpu.rs:31-35 */
float    orc_glibc_cosf(float x);
float    orc_glibc_sinf(float x);
float    orc_glibc_logf(float x);
float    orc_glibc_log10f(float x);
float    orc_glibc_expf(float x);
float    orc_glibc_powf(float x, float y);
void     orc_eval_array(int op, int libm, const float *a, const float *b, uint64_t n, float *out);
/* trace one explicit ray (ray.rs:141-202); returns radiance in out[3] */
void     orc_trace_ray(const OrcTriangle *tris, uint32_t n_tris, const OrcNode *nodes, uint32_t n_nodes,
                       const OrcMaterial *materials, uint32_t n_materials,
                       const OrcTexture *textures, uint32_t n_textures,
                       const float o[3], const float d[3], uint32_t max_depth,
                       uint32_t *rng, int cull, int libm, float out[3]);
/* the same, culled (if cull) at best * (1 + cull_margin) as orc_render culls; counters_out (may be NULL) as orc_trace_ray_wgsl's.
 * orc_trace_ray is this at margin 0 without counters. */
void     orc_trace_ray_m(const OrcTriangle *tris, uint32_t n_tris, const OrcNode *nodes, uint32_t n_nodes,
                         const OrcMaterial *materials, uint32_t n_materials,
                         const OrcTexture *textures, uint32_t n_textures,
                         const float o[3], const float d[3], uint32_t max_depth,
                         uint32_t *rng, int cull, float cull_margin, int libm, float out[3], uint64_t counters_out[5]);

/* ---- the wgpu material model (rt_compute.wgsl, shading mode 1) piece by piece, element-wise over n inputs ---- */
/* linear / repeat sampler (:500-502): out_rgba 4 floats per element; out_idx (may be NULL) the 4 texel indices read: (i0,j0) (i1,j0) (i0,j1) (i1,j1) */
void     orc_wgsl_sample_texture(const OrcTexture *t, const float *u, const float *v, uint64_t n, float *out_rgba, int64_t *out_idx);
void     orc_wgsl_onb(const float *normal, uint64_t n, float *tangent, float *bitangent);                  /* :565-569 */
void     orc_wgsl_frame(int op, const float *normal, const float *l, uint64_t n, float *out);              /* 0 to_world, 1 to_local on the basis of `normal` */
void     orc_wgsl_vndf(const float *ve, const float *ax, const float *ay, uint32_t *rng, uint64_t n, int libm, float *out);   /* :504-525; rng[i] advances */
void     orc_wgsl_cosine_hemisphere(uint32_t *rng, uint64_t n, int libm, float *out);                       /* :546-551; rng[i] advances */
void     orc_wgsl_cosine_from(const float *ux, const float *uy, uint64_t n, int libm, float *out);          /* the same after its two draws */
/* :158-163: out = 13 floats per element: f0.xyz, fresnel.xyz, normalize(reflect).xyz, normalize(refract).xyz (NaN when k < 0), k */
void     orc_wgsl_fresnel_step(const float *dir, const float *normal, const float *ior, const float *metallic, const float *base, uint64_t n, float *out);
/* trace (:126-229) on one explicit ray; counters_out (may be NULL) = rays, inner_steps, tri_tests, hits, texel_fetches */
void     orc_trace_ray_wgsl(const OrcTriangle *tris, uint32_t n_tris, const OrcNode *nodes, uint32_t n_nodes,
                            const OrcMaterial *materials, uint32_t n_materials,
                            const OrcTexture *textures, uint32_t n_textures,
                            const float o[3], const float d[3], uint32_t max_depth,
                            uint32_t *rng, int cull, int libm, float out[3], uint64_t counters_out[5]);
/* the same with a cull margin; orc_trace_ray_wgsl is this at margin 0 */
void     orc_trace_ray_wgsl_m(const OrcTriangle *tris, uint32_t n_tris, const OrcNode *nodes, uint32_t n_nodes,
                              const OrcMaterial *materials, uint32_t n_materials,
                              const OrcTexture *textures, uint32_t n_textures,
                              const float o[3], const float d[3], uint32_t max_depth,
                              uint32_t *rng, int cull, float cull_margin, int libm, float out[3], uint64_t counters_out[5]);

#ifdef __cplusplus
}
#endif
#endif
