/*
 * mipt_diag.h -- diagnostic probe library (libmipt_diag.so).  Test infrastructure for the GPU box; NOT part of the
 * drop-in boundary (include/mipt.h) and not exported by libmipt.so.
 *
 * Evaluates one device arithmetic primitive of the path-tracing kernel element-wise on the GPU, so tests can pin the
 * kernel's f32/f64 building blocks against the CPU oracle bit for bit.  The functions evaluated are the very ones the
 * kernel inlines (rust_ray_tracing_amd/csrc/pt_device_math.h): the restatement of glibc 2.35's cosf / log10f / powf
 * that stands in for Rust std f32::cos / f32::log10 / f32::powf (reference src/math.rs:15-19, src/math/vec3.rs:80-90);
 * pt_device_wgsl.h: the material model of shading mode 1; pt_texel.h: the nearest-texel lookup of the default shading path.
 * Beside the probes: the product's epilogue and tile-order launchers on the caller's buffers, the library-internal layout orders,
 * and read-back hooks for what a scene handle of libmipt.so holds in device memory (geometry, attributes, texel pool, material tables).
 */
#ifndef MIPT_DIAG_H
#define MIPT_DIAG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define MIPT_DIAG_API __attribute__((visibility("default")))
#else
#define MIPT_DIAG_API
#endif

/* host buffers in/out.  op: 0 cosf, 1 log10f, 2 powf(a,b), 3 a/b, 4 sqrt(a), 5 a*b, 6 a+b, 7 min, 8 max,
 *     9 rand_f32(seed=bits(a)), 10 rand_f32_nd(seed), 11 rand_in_unit_sphere(seed)[b], 12 srgb+quantise(a)
 *     (result as integer bits), 13 fract(a), 14 the per-ray-reciprocal division a/b (valid on its checked range),
 *     15 u8 -> f32/255 for the integer whose bits are a, 16 sinf, 17 expf, 18 logf,
 *     19 the kernel's log10f specialised to rand_f32's range {0} u [2^-32, 1], 20 its cosf specialised to [0, 6.2831855].
 * Returns 0, or -1 (bad argument) / -2 (HIP error); device buffers are released on every path. */
MIPT_DIAG_API int mipt_debug_eval(int op, const float *a, const float *b, uint64_t n, float *out);

/* ops 0, 1, 2 (with second argument y), 16, 17, 18, 19, 20 on the n consecutive binary32 bit patterns first_bits, first_bits+1, ...
 * (first_bits + n <= 2^32): the exhaustive sweeps of tests/test_gpu_libm.py. */
MIPT_DIAG_API int mipt_debug_eval_range(int op, uint32_t first_bits, uint64_t n, float y, float *out);

/* The building blocks of shading mode 1 (the wgpu shader's material model; rust_ray_tracing_amd/csrc/pt_device_wgsl.h, the very
 * functions shade_wgsl inlines), element-wise: row i of `in` -> row i of `out`, host buffers, integers as float bit patterns.
 *   op 0  sample_texture_bilinear   in: u, v                                   out: r, g, b, a
 *         over the one texture texels[0 .. tex_w*tex_h) (packed RGBA8 words, rows of tex_w); every index it forms stays inside it
 *   op 1  build_onb                 in: n.xyz                                  out: tangent.xyz, bitangent.xyz
 *   op 2  to_world / op 3 to_local  in: n.xyz, l.xyz  (basis of n, and n)      out: xyz
 *   op 4  sample_ggx_vndf           in: ve.xyz, ax, ay, bits(xorshift state)   out: Ne.xyz, bits(state after the two draws)
 *   op 5  cosine_hemisphere_from    in: ux, uy  (the two draws)                out: xyz
 *   op 6  Fresnel / reflect / refract step   in: d.xyz, n.xyz, eta, metallic, base.rgb
 *                                   out: f0.rgb, fresnel.rgb, normalize(reflect).xyz, normalize(refract).xyz (NaN when k < 0), k
 * tex_* are read by op 0 only (texels may be NULL otherwise).  n <= 2^26.  Returns as mipt_debug_eval. */
MIPT_DIAG_API int mipt_debug_wgsl(int op, const float *in, uint64_t n, const uint32_t *texels, uint32_t tex_w, uint32_t tex_h, float *out);

/* The nearest-texel lookup of the default shading path (rust_ray_tracing_amd/csrc/pt_texel.h texel_rgb: Texture::color_at, texture.rs:33-38,
 * then / 255), the one function the trace kernels and the first-hit pass inline, element-wise: rgb_out[3i .. 3i+3) = the colour of texture
 * {offset, w, h} -- w * h packed RGBA8 words from word `offset` of `pool`, rows of w -- at (uv[2i], uv[2i+1]).  The pool is uploaded as the
 * texel pool of a device scene and the lookup runs against a zeroed counter block, whose tex_clamped (lookups whose index left the
 * texture and was clamped) comes back in *clamped_out.  Host buffers; n <= 2^26, pool_words <= 2^28; offset + w*h > pool_words is refused.
 * Returns as mipt_debug_eval. */
MIPT_DIAG_API int mipt_debug_texel(const float *uv, uint64_t n, const uint32_t *pool, uint64_t pool_words, uint32_t offset, uint32_t w, uint32_t h,
                                   float *rgb_out, uint64_t *clamped_out);

/* The two kernels of the frame epilogue that include/mipt.h reaches only through mipt_render_multi and MIPT_FLAG_TOUCHED, launched by the
 * product's own launchers (pt_kernel.hip launch_divide / launch_popcount, linked into this library unchanged) on the CALLER'S DEVICE
 * buffers, stream-ordered on `stream` (a hipStream_t, NULL = the null stream) without synchronising:
 *   divide    d_buf[i] = d_buf[i] / divisor in place, i < n_floats  (cpu.rs:60 on a reduced sum buffer)
 *   popcount  *d_out += number of set bits in d_bitmap[0 .. n_words)   (it adds: the caller presets *d_out)
 * Returns 0, -1 (null pointer or a count of zero; nothing is launched) or -2 (HIP error). */
MIPT_DIAG_API int mipt_debug_divide(float *d_buf, uint64_t n_floats, float divisor, void *stream);
MIPT_DIAG_API int mipt_debug_popcount(const uint32_t *d_bitmap, uint64_t n_words, uint64_t *d_out, void *stream);

/* The tile order of the trace kernel (pt_kernel.hip "tile order"), for tests/test_gpu_tile_order.py.
 *   mipt_debug_tile_order       the product's sort kernel on host arrays: order_out[] = the n_tiles tiles by decreasing cost[] --
 *                               bucket min(1023, floor(cost * 16 / (64 * samples))) descending, tile index ascending within a bucket
 *   mipt_diag_scene_tile_order  what a scene handle of libmipt.so keeps after its last plain single-view launch: info_out[0] = local
 *                               tiles (0 = no valid state), [1] = the state is valid, [2] = that launch itself ran in the order made
 *                               before it; with non-NULL buffers of `cap` words, that launch's rays per local tile and the order
 *                               sorted from them -- by the launch where a later one can read it, else (a list of every slot leaves
 *                               the tiles no walk, so the launch queued no sort) here, by the same kernel.
 * Return as mipt_debug_eval. */
MIPT_DIAG_API int mipt_debug_tile_order(const uint32_t *cost, uint32_t n_tiles, uint32_t samples, uint32_t *order_out);
MIPT_DIAG_API int mipt_diag_scene_tile_order(const void *scene, uint32_t *cost_out, uint32_t *order_out, uint32_t cap, uint32_t info_out[3]);

/* The hot pixels of the trace kernel (pt_kernel.hip "hot pixels"), for tests/test_gpu_hot_pixels.py.
 *   mipt_debug_hot_select       the product's selection kernels on host arrays: hot_out[0 .. n_hot) = the n_hot of the n_slots slots of
 *                               highest cost[] -- bucket min(1023, floor(cost * 16 / samples)) descending, slot index ascending within
 *                               a bucket -- and bits_out = one bit per slot, set for those, (n_slots + 63) / 64 * 2 words.
 *                               1 <= n_hot <= n_slots.
 *   mipt_diag_scene_hot_pixels  what a scene handle of libmipt.so keeps beside its tile order: info_out[0] = slots, 64 per local tile
 *                               (0 = no valid state), [1] = H, the entries of the list made behind that launch, [2] = the entries
 *                               that launch itself took from the list made before it (0 = it ran without one); with non-NULL
 *                               buffers of cap_slots / cap_hot words, that launch's rays per slot and the list.
 *   mipt_diag_scene_list        the whole list, of which the H hot pixels are the head: info_out[0] = its entries (0 = no valid state;
 *                               the local slots where the list is complete, slots of cost 0 last), [1] = the entries that launch
 *                               itself took from the list made before it; with a non-NULL buffer of `cap` words, the list.
 *   mipt_diag_scene_hot_bits    the bitmap of the listed slots that goes with that list, 2 words per local tile, into `cap_words` words
 *                               (-1 without a valid state or a list).
 *   mipt_diag_scene_cost_atomics  on != 0: the handle's launches measure their pixels' costs with one atomic per path, as a launch
 *                               does whose sample count or ray depth is too large for the packed counter; 0: the product's choice again.
 * Return as mipt_debug_eval. */
MIPT_DIAG_API int mipt_debug_hot_select(const uint32_t *cost, uint32_t n_slots, uint32_t samples, uint32_t n_hot, uint32_t *hot_out, uint32_t *bits_out);
MIPT_DIAG_API int mipt_diag_scene_hot_pixels(const void *scene, uint32_t *pixel_cost_out, uint32_t cap_slots, uint32_t *hot_out, uint32_t cap_hot, uint32_t info_out[3]);
MIPT_DIAG_API int mipt_diag_scene_list(const void *scene, uint32_t *list_out, uint32_t cap, uint32_t info_out[2]);
MIPT_DIAG_API int mipt_diag_scene_hot_bits(const void *scene, uint32_t *bits_out, uint32_t cap_words);
MIPT_DIAG_API int mipt_diag_scene_cost_atomics(void *scene, int on);

MIPT_DIAG_API const char *mipt_diag_last_error(void);

/* The library-internal device-layout orders of libmipt.so (rust_ray_tracing_amd/csrc/bvh_build.cpp, hidden there), re-exported for
 * tests/test_host_layout.py: order of the 64-byte pair records in HBM (order_out[j] = reference pair index of record j, 0xffffffff = a
 * pad record), the number of breadth-first levels at its top, and the slot of every triangle's record in the intersection stream.
 * nodes: the reference's 32-byte Node array (MiptNode). */
MIPT_DIAG_API int mipt_internal_pair_order(const void *nodes, uint32_t n_nodes, uint32_t *order_out, uint32_t cap, uint32_t *n_records_out);
MIPT_DIAG_API uint32_t mipt_internal_pair_order_top(void);
MIPT_DIAG_API int mipt_internal_tri_slots(const void *nodes, uint32_t n_nodes, uint32_t n_tris, uint32_t *slot_out, uint32_t *n_slots_out);

/* The device layout behind a MiptScene handle of libmipt.so (tests/cpp/scene_hooks.hip), for comparing the layout the GPU kernels
 * build (mipt_scene_create_from_triangles) with the host-built one (mipt_scene_create): sizes in bytes of [pair records | intersection
 * stream] and of the attribute stream; a copy of either (which = 0 / 1) to the host; an order-dependent 64-bit fingerprint of each.
 * mipt_diag_scene_tables (mipt_diag.hip, beside mipt_diag_scene_tile_order, the other reader of a handle's state): the payload bytes of the texel pool (texels * 4), of the 64-B material table and of the 128-B material table
 * (materials * 64 / * 128) -- not the padded allocations; mipt_diag_scene_read copies them with which = 2 / 3 / 4. */
MIPT_DIAG_API int mipt_diag_scene_sizes(const void *scene, uint64_t out[2]);
MIPT_DIAG_API int mipt_diag_scene_tables(const void *scene, uint64_t out[3]);
MIPT_DIAG_API int mipt_diag_scene_read(const void *scene, int which, void *dst, uint64_t bytes);
MIPT_DIAG_API int mipt_diag_scene_hash(const void *scene, uint64_t out[2]);

/* The HOST layout of a scene's geometry (tests/cpp/host_layout.cpp): byte for byte the buffers rounds 1-3 built on host threads from the
 * reference's arrays -- geom = pair records | intersection stream, attr = attribute stream -- which the product now produces with GPU
 * kernels for both mipt_scene_create and mipt_scene_create_from_triangles; the tests compare mipt_diag_scene_read's bytes with these.
 * `desc` is a MiptSceneDesc with a well-formed tree and triangles in its order.  sizes_out[2] = bytes of geom and attr (call with
 * null buffers first); info_out[4] (may be NULL) = pair records incl. padding, largest leaf, the root's slot and triangle count. */
MIPT_DIAG_API int mipt_diag_host_layout(const void *desc, uint8_t *geom_out, uint64_t geom_cap, uint8_t *attr_out, uint64_t attr_cap,
                                        uint64_t *sizes_out, uint32_t *info_out);

/* mipt_diag_scene_hash's fingerprint of a word stream in HOST memory (for the buffers of mipt_diag_host_layout at sizes where a
 * byte compare is unwieldy). */
MIPT_DIAG_API int mipt_diag_hash_words(const void *words, uint64_t n_words, uint64_t *out);

/* Writes `n_tris` reference Triangles (112 B each) as an OBJ body (tests/cpp/obj_writer.cpp): per triangle 3 v, 3 vt, 3 vn lines and one
 * face line, shortest round-trip decimals; `mtllib` (may be NULL) names the material library, material_names[material_id] go into
 * usemtl lines.  0, -1 (bad argument) or -2 (I/O).  For rust_ray_tracing_amd/synth.py write_obj. */
MIPT_DIAG_API int mipt_diag_write_obj(const char *path, const void *tris, uint64_t n_tris, const char *mtllib, const char *const *material_names,
                                      uint32_t n_materials);

#ifdef __cplusplus
}
#endif
#endif /* MIPT_DIAG_H */
