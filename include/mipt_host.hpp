// mipt_host.hpp -- C++ host-side mirror of the reference's Renderer / Scene interface for the path-tracing hot path,
// header-only over the C ABI of mipt.h.  The reference is Rust (no toolchain in this image), so the host side above the
// ABI is C++: same type and member names, same argument meaning, same error behaviour --
//   Renderer::create  = Renderer::new            (src/renderer.rs:14-48)  -> std::nullopt + the reference's log line
//   Renderer::render                             (src/renderer.rs:50-85)  -> the Vec<u8> of the backend arm
//   Scene::load / Scene::set_camera              (src/scene.rs:22-41)
//   Camera::update_view                          (src/scene.rs:181-194)
//   RendererBackend::{GPU, CPU} + MI355X         (src/renderer/backend.rs:6-10)
#pragma once
#include "mipt.h"

#include <cmath>
#include <cstdio>
#include <memory>
#include <optional>
#include <string>
#include <utility>
#include <vector>

namespace mipt {

inline void log_error(const std::string &m) { fprintf(stderr, "[ERROR] %s\n", m.c_str()); }   // src/log.rs:22-29

enum class RendererBackend { GPU, CPU, MI355X };

struct RendererOptions {                                   // src/renderer.rs:96-116 (same defaults)
    size_t samples = 1;
    size_t max_ray_depth = 6;
    std::pair<size_t, size_t> output_image_dimensions{1920, 1080};
    std::optional<std::string> output_image_path;
    RendererBackend backend = RendererBackend::GPU;
    bool is_realtime = true;
    // MI355X arm only: the recommended traversal (best-hit cull with MIPT_CULL_MARGIN_SAFE: the CPU backend's frame bit for bit,
    // 1.7x faster).  MIPT_TRAVERSAL_REFERENCE = the CPU backend's own un-culled traversal (ray.rs:69-81).
    uint32_t traversal = MIPT_TRAVERSAL_CULLED;
    int device_id = 0;
};

struct Camera {                                            // src/scene.rs:169-195
    float pitch = 0.0f, yaw = 0.0f;
    float position[3] = {0.0f, 0.0f, 0.0f};
    MiptCamera uniform{};                                  // look_at + position as uploaded (gpu.rs:480-486)
    void update_view() { mipt_camera_from_pose(position, pitch, yaw, &uniform); }
};

struct Texture {                                           // src/texture.rs:4-10
    uint32_t width = 0, height = 0, hash = 0;
    std::vector<uint8_t> pixel_data;                       // RGBA8, rows as Texture::load stores them (flipv applied)
    static std::optional<Texture> load(const std::string &path) {   // src/texture.rs:13-31
        MiptImage *img = nullptr;
        MiptTexture d{};
        Texture t;
        if (mipt_texture_load(path.c_str(), &img, &d, &t.hash) != MIPT_OK) {
            log_error(mipt_last_error());
            return std::nullopt;
        }
        t.width = d.width; t.height = d.height;
        t.pixel_data.assign(d.rgba8, d.rgba8 + (size_t)d.width * d.height * 4);
        mipt_texture_free(img);
        return t;
    }
};

// mipt_query_closest / mipt_query_occluded on any resident scene handle, vectors in and out (MIPT_ERR_STACK leaves the results written)
inline int query_closest_on(MiptScene *scene, const std::vector<MiptRay> &rays, std::vector<MiptHit> &hits, const MiptQueryOptions *opt = nullptr,
                            MiptStats *stats = nullptr) {
    hits.resize(rays.size());
    static const MiptRay no_ray{};
    static MiptHit no_hit{};
    const int rc = mipt_query_closest(scene, rays.empty() ? &no_ray : rays.data(), rays.size(), opt, hits.empty() ? &no_hit : hits.data(), stats);
    if (rc != MIPT_OK) log_error(mipt_last_error());
    return rc;
}
inline int query_occluded_on(MiptScene *scene, const std::vector<MiptRay> &rays, std::vector<uint8_t> &occluded, const MiptQueryOptions *opt = nullptr,
                             MiptStats *stats = nullptr) {
    occluded.resize(rays.size());
    static const MiptRay no_ray{};
    static uint8_t no_byte = 0;
    const int rc = mipt_query_occluded(scene, rays.empty() ? &no_ray : rays.data(), rays.size(), opt, occluded.empty() ? &no_byte : occluded.data(), stats);
    if (rc != MIPT_OK) log_error(mipt_last_error());
    return rc;
}
// mipt_query_radiance on any resident scene handle: radiance[3 i .. 3 i + 3) for rays[i], whose `reserved` word is its seed (non-zero;
// include/mipt.h "radiance queries").  MIPT_ERR_STACK leaves the results written.
inline int query_radiance_on(MiptScene *scene, const std::vector<MiptRay> &rays, std::vector<float> &radiance, const MiptRadianceOptions &opt,
                             MiptStats *stats = nullptr) {
    radiance.assign(rays.size() * 3, 0.0f);
    static const MiptRay no_ray{};
    static float no_value = 0.0f;
    const int rc = mipt_query_radiance(scene, rays.empty() ? &no_ray : rays.data(), rays.size(), &opt, radiance.empty() ? &no_value : radiance.data(), stats);
    if (rc != MIPT_OK) log_error(mipt_last_error());
    return rc;
}
// mipt_bake_texels on any resident scene handle: points[y * width + x] is the surface point behind texel (x, y) of the atlas the
// scene's UVs lay out, prim == MIPT_HIT_NONE where no triangle covers the texel's centre (include/mipt.h "baking").
inline int bake_texels_on(MiptScene *scene, uint32_t width, uint32_t height, std::vector<MiptSurfacePoint> &points, MiptBakeTexelInfo *info = nullptr) {
    points.assign((size_t)width * height, MiptSurfacePoint{});
    static MiptSurfacePoint no_point{};
    const int rc = mipt_bake_texels(scene, width, height, nullptr, points.empty() ? &no_point : points.data(), info);
    if (rc != MIPT_OK) log_error(mipt_last_error());
    return rc;
}
// mipt_bake_gather on any resident scene handle: radiance[3 i .. 3 i + 3) is the light points[i] gathers over its hemisphere.
// MIPT_ERR_STACK leaves the results written.
inline int bake_gather_on(MiptScene *scene, const std::vector<MiptSurfacePoint> &points, std::vector<float> &radiance, const MiptBakeOptions &opt,
                          MiptStats *stats = nullptr) {
    radiance.assign(points.size() * 3, 0.0f);
    static const MiptSurfacePoint no_point{};
    static float no_value = 0.0f;
    const int rc = mipt_bake_gather(scene, points.empty() ? &no_point : points.data(), points.size(), &opt, radiance.empty() ? &no_value : radiance.data(), stats);
    if (rc != MIPT_OK) log_error(mipt_last_error());
    return rc;
}
// mipt_bake_surface on any resident scene handle: position[3 i .. 3 i + 3) and normal[3 i .. 3 i + 3) of points[i] -- the P and N of
// the gather, N normalized with `unit_normals` -- the guides of lightmap_filter.  Both are computed.
inline int bake_surface_on(MiptScene *scene, const std::vector<MiptSurfacePoint> &points, std::vector<float> &position, std::vector<float> &normal,
                           bool unit_normals = false) {
    position.assign(points.size() * 3, 0.0f);
    normal.assign(points.size() * 3, 0.0f);
    static const MiptSurfacePoint no_point{};
    static float no_value[2] = {0.0f, 0.0f};
    MiptBakeSurfaceOptions opt{};
    opt.flags = unit_normals ? MIPT_BAKE_SURFACE_UNIT_NORMALS : 0u;
    const int rc = mipt_bake_surface(scene, points.empty() ? &no_point : points.data(), points.size(), &opt, position.empty() ? &no_value[0] : position.data(),
                                     normal.empty() ? &no_value[1] : normal.data());
    if (rc != MIPT_OK) log_error(mipt_last_error());
    return rc;
}

// lightmap_filter: the filter's settings (MiptLightmapFilterOptions; the defaults of the Python mirror)
struct LightmapFilterSettings {
    uint32_t iterations = 5;
    float sigma_color = 4.0f, sigma_normal = 0.5f, sigma_plane = 0.05f, sigma_distance = 0.5f;
};
// mipt_lightmap_filter over host planes of a width x height atlas (include/mipt.h "lightmap finishing"): `radiance` 3 f32 per texel,
// `points` the records of bake_texels, `position` and `normal` 3 f32 per texel or empty = absent.  `out` is resized; it may be
// `radiance` itself.  A plane of the wrong size is refused here with MIPT_ERR_INVALID_ARG.
inline int lightmap_filter(uint32_t width, uint32_t height, const std::vector<float> &radiance, const std::vector<MiptSurfacePoint> &points,
                           const std::vector<float> &position, const std::vector<float> &normal, std::vector<float> &out,
                           const LightmapFilterSettings &settings = {}, int device_id = 0) {
    const size_t n = (size_t)width * height;
    if (radiance.size() != n * 3 || points.size() != n || (!position.empty() && position.size() != n * 3) || (!normal.empty() && normal.size() != n * 3)) {
        log_error("lightmap_filter: radiance, position and normal hold 3 values and points one record per texel of the atlas");
        return MIPT_ERR_INVALID_ARG;
    }
    if (&out != &radiance) out.assign(n * 3, 0.0f);
    MiptLightmapFilterOptions o{};
    o.width = width; o.height = height; o.iterations = settings.iterations;
    o.sigma_color = settings.sigma_color; o.sigma_normal = settings.sigma_normal; o.sigma_plane = settings.sigma_plane; o.sigma_distance = settings.sigma_distance;
    MiptLightmapFilterBuffers b{};
    b.radiance = radiance.data(); b.points = points.data(); b.out = out.data();
    b.position = position.empty() ? nullptr : position.data();
    b.normal = normal.empty() ? nullptr : normal.data();
    const int rc = mipt_lightmap_filter(&o, &b, device_id);
    if (rc != MIPT_OK) log_error(mipt_last_error());
    return rc;
}
// mipt_lightmap_dilate over host planes: `radius` passes into the gutter.  `out` is resized and may be `radiance` itself; `level`, if
// given, receives 1 for a covered texel, k + 1 for one filled in pass k and 0 for one still empty.
inline int lightmap_dilate(uint32_t width, uint32_t height, const std::vector<float> &radiance, const std::vector<MiptSurfacePoint> &points, uint32_t radius,
                           std::vector<float> &out, std::vector<uint32_t> *level = nullptr, int device_id = 0) {
    const size_t n = (size_t)width * height;
    if (radiance.size() != n * 3 || points.size() != n) {
        log_error("lightmap_dilate: radiance holds 3 values and points one record per texel of the atlas");
        return MIPT_ERR_INVALID_ARG;
    }
    if (&out != &radiance) out.assign(n * 3, 0.0f);
    if (level) level->assign(n, 0u);
    MiptLightmapDilateOptions o{};
    o.width = width; o.height = height; o.radius = radius;
    MiptLightmapDilateBuffers b{};
    b.radiance = radiance.data(); b.points = points.data(); b.out = out.data();
    b.level = level ? level->data() : nullptr;
    const int rc = mipt_lightmap_dilate(&o, &b, device_id);
    if (rc != MIPT_OK) log_error(mipt_last_error());
    return rc;
}

// mipt_probe_bake on any resident scene handle (include/mipt.h "irradiance probes"): sh[27 i + 3 k + c] is coefficient k of channel c
// of the light that arrives at probes[i].  MIPT_ERR_STACK leaves the results written.
inline int bake_probes_on(MiptScene *scene, const std::vector<MiptProbe> &probes, std::vector<float> &sh, const MiptProbeBakeOptions &opt,
                          MiptStats *stats = nullptr) {
    sh.assign(probes.size() * 27, 0.0f);
    static const MiptProbe no_probe{};
    static float no_value = 0.0f;
    const int rc = mipt_probe_bake(scene, probes.empty() ? &no_probe : probes.data(), probes.size(), &opt, sh.empty() ? &no_value : sh.data(), stats);
    if (rc != MIPT_OK) log_error(mipt_last_error());
    return rc;
}
// The positions of a grid's probes in index order, (iz * dims[1] + iy) * dims[0] + ix: origin + spacing * index, one f32 product and
// sum per coordinate; each probe's seed is its index, to go with sample_stride = the count.
inline std::vector<MiptProbe> probe_grid(const MiptProbeGrid &grid) {
    std::vector<MiptProbe> probes;
    probes.reserve((size_t)grid.dims[0] * grid.dims[1] * grid.dims[2]);
    for (uint32_t iz = 0; iz < grid.dims[2]; iz++)
        for (uint32_t iy = 0; iy < grid.dims[1]; iy++)
            for (uint32_t ix = 0; ix < grid.dims[0]; ix++)
                probes.push_back({grid.origin[0] + grid.spacing[0] * (float)ix, grid.origin[1] + grid.spacing[1] * (float)iy,
                                  grid.origin[2] + grid.spacing[2] * (float)iz, (uint32_t)probes.size()});
    return probes;
}
// mipt_probe_irradiance over host buffers: `sh` 27 f32 per probe of `grid` (what bake_probes wrote for probe_grid(grid)), `position`
// and `normal` 3 f32 per point, `valid` one byte per probe or empty = every probe counts.  `irradiance` is resized to 3 f32 per point.
// A buffer of the wrong size is refused here with MIPT_ERR_INVALID_ARG.
inline int probe_irradiance(const MiptProbeGrid &grid, const std::vector<float> &sh, const std::vector<float> &position, const std::vector<float> &normal,
                            std::vector<float> &irradiance, const std::vector<uint8_t> &valid = {}, int device_id = 0) {
    const uint64_t n_probes = (uint64_t)grid.dims[0] * grid.dims[1] * grid.dims[2];       // a product that wraps is the library's to refuse
    if (position.size() % 3 != 0 || normal.size() != position.size() || sh.size() != n_probes * 27 || (!valid.empty() && valid.size() != n_probes)) {
        log_error("probe_irradiance: sh holds 27 values and valid one byte per probe of the grid, position and normal 3 values per point");
        return MIPT_ERR_INVALID_ARG;
    }
    irradiance.assign(position.size(), 0.0f);
    static float no_value[3] = {0.0f, 0.0f, 0.0f};
    MiptProbeIrradianceBuffers b{};
    b.sh = sh.empty() ? &no_value[0] : sh.data();
    b.valid = valid.empty() ? nullptr : valid.data();
    b.position = position.empty() ? &no_value[0] : position.data();
    b.normal = normal.empty() ? &no_value[1] : normal.data();
    b.irradiance = irradiance.empty() ? &no_value[2] : irradiance.data();
    const int rc = mipt_probe_irradiance(&grid, position.size() / 3, &b, device_id);
    if (rc != MIPT_OK) log_error(mipt_last_error());
    return rc;
}

// mipt_render_features on any resident scene handle: first-hit feature buffers (include/mipt.h "first-hit feature buffers") for
// `cameras` with `opt`.  `wanted`: FeatureBit flags; only those images are computed and filled, each view-major [view][row][column][k]
// with row 0 the top row; the others are left empty.  MIPT_ERR_STACK leaves the images written.
enum FeatureBit : uint32_t {
    FEATURE_DEPTH = 1u << 0, FEATURE_PRIM = 1u << 1, FEATURE_MATERIAL = 1u << 2, FEATURE_POSITION = 1u << 3,
    FEATURE_UV = 1u << 4, FEATURE_NORMAL = 1u << 5, FEATURE_ALBEDO = 1u << 6, FEATURE_EMISSION = 1u << 7, FEATURE_ALL = 0xffu
};
struct FeatureImages {
    uint32_t n_views = 0, width = 0, height = 0;
    std::vector<float> depth;                              // 1 f32 / pixel; 1e30f = miss
    std::vector<uint32_t> prim, material;                  // MiptHit.prim convention (MIPT_HIT_NONE = miss); material_id (UINT32_MAX = miss)
    std::vector<float> position, uv, normal, albedo, emission;   // 3, 2, 3, 3, 3 f32 / pixel
};
inline int render_features_on(MiptScene *scene, const std::vector<MiptCamera> &cameras, const MiptOptions &opt, uint32_t wanted,
                              FeatureImages &out, MiptStats *stats = nullptr) {
    const uint64_t n_pix = (uint64_t)cameras.size() * opt.width * opt.height;
    const size_t n = n_pix < MIPT_BATCH_MAX_PIXELS ? (size_t)n_pix : 0;      // an impossible size is left to the library to refuse
    out.n_views = (uint32_t)cameras.size(); out.width = opt.width; out.height = opt.height;
    MiptFeatureBuffers b{};
    auto take = [&](auto &v, uint32_t bit, size_t k) { v.assign((wanted & bit) ? (n ? n * k : 1) : 0, 0); return (wanted & bit) ? v.data() : nullptr; };
    b.depth = take(out.depth, FEATURE_DEPTH, 1); b.prim = take(out.prim, FEATURE_PRIM, 1); b.material = take(out.material, FEATURE_MATERIAL, 1);
    b.position = take(out.position, FEATURE_POSITION, 3); b.uv = take(out.uv, FEATURE_UV, 2); b.normal = take(out.normal, FEATURE_NORMAL, 3);
    b.albedo = take(out.albedo, FEATURE_ALBEDO, 3); b.emission = take(out.emission, FEATURE_EMISSION, 3);
    static const MiptCamera no_camera{};
    const int rc = mipt_render_features(scene, cameras.empty() ? &no_camera : cameras.data(), (uint32_t)cameras.size(), &opt, &b, stats);
    if (rc != MIPT_OK) log_error(mipt_last_error());
    return rc;
}

// mipt_render_motion on any resident scene handle (include/mipt.h "previous positions"): per pixel of `cameras` with `opt` the world
// position the first hit's surface point had in the previous geometry, 3 f32 / pixel, view-major [view][row][column][3].  `prev_tris`:
// the previous frame's triangles in the caller's order; empty = the generation a mesh scene tracks (mipt_scene_track_motion).
// MIPT_ERR_STACK leaves the image written.
inline int render_motion_on(MiptScene *scene, const std::vector<MiptCamera> &cameras, const MiptOptions &opt, const std::vector<MiptTriangle> &prev_tris,
                            std::vector<float> &prev_position, MiptStats *stats = nullptr) {
    const uint64_t n_pix = (uint64_t)cameras.size() * opt.width * opt.height;
    const size_t n = n_pix < MIPT_BATCH_MAX_PIXELS ? (size_t)n_pix : 0;      // an impossible size is left to the library to refuse
    prev_position.assign(n ? n * 3 : 1, 0.0f);
    MiptMotionBuffers b{};
    b.prev_tris = prev_tris.empty() ? nullptr : prev_tris.data();
    b.n_prev_tris = (uint32_t)prev_tris.size();
    b.prev_position = prev_position.data();
    static const MiptCamera no_camera{};
    const int rc = mipt_render_motion(scene, cameras.empty() ? &no_camera : cameras.data(), (uint32_t)cameras.size(), &opt, &b, stats);
    if (rc != MIPT_OK) log_error(mipt_last_error());
    return rc;
}

// Renderer::denoise: the filter's settings (MiptDenoiseOptions; the defaults of the Python mirror)
struct DenoiseSettings {
    uint32_t iterations = 5;                               // 1 ... 8; iteration i has step 1 << i
    float sigma_color = 4.0f, sigma_normal = 0.5f, sigma_depth = 0.5f;
};

// Renderer::temporal: the blend's settings (MiptTemporalOptions; the defaults of the Python mirror) and what a call keeps
struct TemporalSettings {
    float alpha_min = 0.0f, max_history = 32.0f;           // floor of the blend factor; cap of the history length
    float normal_tol = 0.1f, depth_tol = 0.1f;             // largest |n_p - n_q|^2 and |d2 - z_q^2| / d2 of an accepted tap
    bool want_length = false, want_variance = false;
};
struct TemporalState {
    std::vector<uint32_t> history;                         // mipt_temporal_history_bytes() / 4 words in the header's layout; empty = no frame yet
    std::vector<float> length, variance;                   // 1 f32 / pixel where asked for
};

// Renderer::denoise_variance: the filter's settings (MiptVarianceOptions; the defaults of the Python mirror)
struct VarianceSettings {
    uint32_t iterations = 5;                               // 1 ... 8; iteration i has step 1 << i
    float sigma_luminance = 16.0f, sigma_normal = 0.5f, sigma_depth = 0.5f;
    float short_history = 4.0f;                            // a pixel with a shorter history takes the spatial estimate; 0 = never
};

// Renderer::upsample: the filter's settings (MiptUpsampleOptions; the defaults of the Python mirror)
struct UpsampleSettings {
    uint32_t scale = 2;                                    // k, 2 ... 8: the low frame is width/k x height/k
    float sigma_normal = 0.5f, sigma_depth = 0.5f;
};

// Renderer::sample_map: the map's settings (MiptSampleMapOptions; the defaults of the Python mirror: max_samples 0 = options.samples,
// a negative budget = min_samples).  rounds 0 = mipt_sample_map; 1 ... 8 = mipt_sample_map_fill, which hands on what the clamp at
// max_samples cuts off (MiptSampleMapFillOptions).
struct SampleMapSettings {
    uint32_t min_samples = 1, max_samples = 0;
    float budget = -1.0f;
    uint32_t rounds = 0;
};

// An indexed mesh kept resident on one device (include/mipt.h "resident indexed meshes"): what OBJ holds before scene.rs:48-76 expands
// it.  The vectors are the caller's to edit between create() calls; the device copy follows set_transforms / update_device only.
class Mesh {
  public:
    std::vector<float> positions, normals, tex_coords;     // 3 / 3 / 2 f32 each
    std::vector<uint32_t> indices, normal_indices, tex_coord_indices;   // the last two empty = shared with `indices`
    std::vector<MiptMeshPart> parts;
    std::vector<float> transforms;                         // empty or parts.size() x 16 (Mat4f data[col][row])

    MiptMeshDesc desc() const {
        MiptMeshDesc d{};
        d.positions = positions.data(); d.n_positions = (uint32_t)(positions.size() / 3);
        d.normals = normals.empty() ? nullptr : normals.data(); d.n_normals = (uint32_t)(normals.size() / 3);
        d.tex_coords = tex_coords.empty() ? nullptr : tex_coords.data(); d.n_tex_coords = (uint32_t)(tex_coords.size() / 2);
        d.indices = indices.data(); d.n_indices = (uint32_t)indices.size();
        d.normal_indices = normal_indices.empty() ? nullptr : normal_indices.data();
        d.tex_coord_indices = tex_coord_indices.empty() ? nullptr : tex_coord_indices.data();
        d.parts = parts.data(); d.n_parts = (uint32_t)parts.size();
        d.transforms = transforms.empty() ? nullptr : transforms.data();
        return d;
    }
    // mipt_mesh_expand: the fat triangles on the host (empty + a log line on error)
    std::vector<MiptTriangle> expand() const {
        std::vector<MiptTriangle> out(indices.size() / 3);
        const MiptMeshDesc d = desc();
        uint32_t n = 0;
        if (mipt_mesh_expand(&d, out.data(), (uint32_t)out.size(), &n) != MIPT_OK) { log_error(mipt_last_error()); out.clear(); }
        return out;
    }
    // mipt_scene_create_from_mesh with `materials` / `textures` of a MiptSceneDesc; the handle is owned here
    int create(const MiptSceneDesc &materials_and_textures, int device_id = 0) {
        const MiptMeshDesc d = desc();
        MiptScene *s = nullptr;
        const int rc = mipt_scene_create_from_mesh(&materials_and_textures, &d, device_id, &s);
        if (rc != MIPT_OK) { log_error(mipt_last_error()); return rc; }
        scene_ = std::shared_ptr<MiptScene>(s, [](MiptScene *p) { mipt_scene_destroy(p); });
        return MIPT_OK;
    }
    MiptScene *handle() const { return scene_.get(); }
    // `transforms` (empty = none) to the device, then REFIT / REBUILD
    int set_transforms(uint32_t mode = MIPT_UPDATE_REFIT, MiptUpdateInfo *info = nullptr) {
        const int rc = mipt_scene_set_transforms(scene_.get(), transforms.empty() ? nullptr : transforms.data(), (uint32_t)parts.size(), mode, info);
        if (rc != MIPT_OK) log_error(mipt_last_error());
        return rc;
    }
    // arrays already in HBM of the scene's device (null = keep the resident one)
    int update_device(const float *d_positions, const float *d_normals, const float *d_transforms, uint32_t mode = MIPT_UPDATE_REFIT,
                      void *hip_stream = nullptr, MiptUpdateInfo *info = nullptr) {
        const int rc = mipt_scene_update_mesh_device(scene_.get(), d_positions, d_normals, d_transforms, mode, hip_stream, info);
        if (rc != MIPT_OK) log_error(mipt_last_error());
        return rc;
    }
    int info(MiptMeshInfo *out) const { return mipt_scene_mesh_info(scene_.get(), out); }
    // ray queries on the resident mesh scene (mipt_query_closest / mipt_query_occluded): hits[i] / occluded[i] for rays[i]
    int query_closest(const std::vector<MiptRay> &rays, std::vector<MiptHit> &hits, const MiptQueryOptions *opt = nullptr, MiptStats *stats = nullptr) {
        return query_closest_on(scene_.get(), rays, hits, opt, stats);
    }
    int query_occluded(const std::vector<MiptRay> &rays, std::vector<uint8_t> &occluded, const MiptQueryOptions *opt = nullptr, MiptStats *stats = nullptr) {
        return query_occluded_on(scene_.get(), rays, occluded, opt, stats);
    }

  private:
    std::shared_ptr<MiptScene> scene_;
};

class Scene {                                              // src/scene.rs:12-19
  public:
    Scene() = default;
    // The device residency (replicas + communicators) is NOT shared between copies: a copy starts without one and creates its own on
    // its first render_node -- two copies rendering from two threads must not meet in one MiptMulti's buffers and streams.
    Scene(const Scene &o) : tris(o.tris), materials(o.materials), textures(o.textures), bvh_nodes(o.bvh_nodes), camera(o.camera) {}
    Scene &operator=(const Scene &o) {
        if (this != &o) { tris = o.tris; materials = o.materials; textures = o.textures; bvh_nodes = o.bvh_nodes; camera = o.camera; release_device(); }
        return *this;
    }
    Scene(Scene &&) = default;
    Scene &operator=(Scene &&) = default;

    std::vector<MiptTriangle> tris;
    std::vector<std::pair<std::string, MiptMaterial>> materials;   // name -> Material, in material-id order
    std::vector<Texture> textures;
    std::vector<MiptNode> bvh_nodes;                       // scene.bvh.nodes
    Camera camera;

    // build_bvh = false: Scene::load without the BVH::build call at scene.rs:80 -- triangles in file order, bvh_nodes empty; the
    // MI355X arm then builds the tree on the GPU (Renderer::render -> mipt_scene_create_from_triangles).
    static std::optional<Scene> load(const std::string &path, bool build_bvh = true) {    // src/scene.rs:22-36
        MiptObj *obj = nullptr;
        if ((build_bvh ? mipt_obj_load(path.c_str(), &obj) : mipt_obj_load_triangles(path.c_str(), &obj)) != MIPT_OK) { log_error(mipt_last_error()); return std::nullopt; }
        MiptSceneDesc d{};
        const char **names = nullptr;
        mipt_obj_get(obj, &d, &names);
        Scene s;
        s.release_device();
        s.tris.assign(d.tris, d.tris + d.n_tris);
        if (d.n_nodes) s.bvh_nodes.assign(d.nodes, d.nodes + d.n_nodes);
        for (uint32_t i = 0; i < d.n_materials; i++) s.materials.emplace_back(names[i], d.materials[i]);
        for (uint32_t i = 0; i < d.n_textures; i++) {
            Texture t;
            t.width = d.textures[i].width; t.height = d.textures[i].height;
            t.pixel_data.assign(d.textures[i].rgba8, d.textures[i].rgba8 + (size_t)t.width * t.height * 4);
            s.textures.push_back(std::move(t));
        }
        mipt_obj_free(obj);
        return s;
    }
    void set_camera(const Camera &c) { camera = c; camera.update_view(); }   // src/scene.rs:38-41

    // Device residency for Renderer::render_node: the per-device replicas, streams and RCCL communicators (MiptMulti) are
    // created on first use and kept -- like the wgpu backend's State, built once in State::new (gpu.rs:96-118) -- so a
    // second frame costs no upload and no ncclCommInitAll.  build_bvh() invalidates it.  After editing the public tris (positions,
    // normals, uvs, material ids -- or the count, with MIPT_UPDATE_REBUILD) call update_device(): the replicas take the new
    // geometry in place and keep materials, textures and communicators.  After editing bvh_nodes / materials / textures directly call
    // release_device() (the camera is passed per frame and needs no re-upload).
    void release_device() const { multi_.reset(); multi_devices_ = -1; }
    // mipt_multi_update_triangles from `tris` (in the order the replicas were built from: the tree order with bvh_nodes, else the
    // caller's).  REFIT keeps the tree and refits bvh_nodes here too; REBUILD builds a new tree on the GPU, after which bvh_nodes is
    // cleared (the scene is then one made from its triangles).  Without replicas there is nothing to update: the next render_node
    // uploads the current arrays.  Returns a MiptStatus.
    int update_device(uint32_t mode = MIPT_UPDATE_REFIT, MiptUpdateInfo *info = nullptr) {
        if (multi_) {
            const int rc = mipt_multi_update_triangles(multi_.get(), tris.data(), (uint32_t)tris.size(), mode, info);
            if (rc != MIPT_OK) { log_error(mipt_last_error()); return rc; }
        }
        if (mode == MIPT_UPDATE_REBUILD) bvh_nodes.clear();
        else refit_nodes();
        return MIPT_OK;
    }
    // Node::grow_by_tri (bvh.rs:185-193) over every node's triangles, children before parents (BVH::build pushes them after it)
    void refit_nodes() {
        for (size_t i = bvh_nodes.size(); i-- > 0;) {
            MiptNode &n = bvh_nodes[i];
            float lo[3] = {3.40282347e38f, 3.40282347e38f, 3.40282347e38f}, hi[3] = {-3.40282347e38f, -3.40282347e38f, -3.40282347e38f};
            auto grow = [&](const float *a, const float *b) { for (int k = 0; k < 3; k++) { lo[k] = std::fmin(lo[k], a[k]); hi[k] = std::fmax(hi[k], b[k]); } };
            if (n.num_tris > 0) {
                for (uint32_t t = n.first_tri_or_child; t < n.first_tri_or_child + n.num_tris; t++)
                    for (const MiptVertex &v : tris[t].vertices) grow(&v.position.x, &v.position.x);
            } else {
                for (uint32_t c = n.first_tri_or_child; c < n.first_tri_or_child + 2; c++) grow(&bvh_nodes[c].bounds_min.x, &bvh_nodes[c].bounds_max.x);
            }
            n.bounds_min = {lo[0], lo[1], lo[2]};
            n.bounds_max = {hi[0], hi[1], hi[2]};
        }
    }
    MiptMulti *node_handle(int n_devices) const {
        if (multi_ && multi_devices_ == n_devices) return multi_.get();
        release_device();
        std::vector<MiptMaterial> mats;
        for (const auto &kv : materials) mats.push_back(kv.second);
        std::vector<MiptTexture> texs;
        for (const Texture &t : textures) texs.push_back({t.width, t.height, t.pixel_data.data()});
        MiptSceneDesc d{tris.data(), (uint32_t)tris.size(), bvh_nodes.data(), (uint32_t)bvh_nodes.size(),
                        mats.data(), (uint32_t)mats.size(), texs.data(), (uint32_t)texs.size()};
        MiptMulti *m = nullptr;
        if ((bvh_nodes.empty() ? mipt_multi_create_from_triangles(&d, nullptr, n_devices, &m) : mipt_multi_create(&d, nullptr, n_devices, &m)) != MIPT_OK) { log_error(mipt_last_error()); return nullptr; }
        multi_ = std::shared_ptr<MiptMulti>(m, [](MiptMulti *p) { mipt_multi_destroy(p); });
        multi_devices_ = n_devices;
        return m;
    }

    // ray queries on the root replica of the scene's device residency (created on first use, like render_node's)
    int query_closest(const std::vector<MiptRay> &rays, std::vector<MiptHit> &hits, const MiptQueryOptions *opt = nullptr, MiptStats *stats = nullptr) const {
        MiptMulti *m = node_handle(multi_devices_ > 0 ? multi_devices_ : 1);
        return m ? query_closest_on(mipt_multi_scene(m, 0), rays, hits, opt, stats) : MIPT_ERR_HIP;
    }
    int query_occluded(const std::vector<MiptRay> &rays, std::vector<uint8_t> &occluded, const MiptQueryOptions *opt = nullptr, MiptStats *stats = nullptr) const {
        MiptMulti *m = node_handle(multi_devices_ > 0 ? multi_devices_ : 1);
        return m ? query_occluded_on(mipt_multi_scene(m, 0), rays, occluded, opt, stats) : MIPT_ERR_HIP;
    }
    // path-traced radiance along the caller's rays (mipt_query_radiance), on the same replica
    int query_radiance(const std::vector<MiptRay> &rays, std::vector<float> &radiance, const MiptRadianceOptions &opt, MiptStats *stats = nullptr) const {
        MiptMulti *m = node_handle(multi_devices_ > 0 ? multi_devices_ : 1);
        return m ? query_radiance_on(mipt_multi_scene(m, 0), rays, radiance, opt, stats) : MIPT_ERR_HIP;
    }
    // baking (mipt_bake_texels, mipt_bake_gather), on the same replica: the surface points behind the texels of a lightmap atlas, and
    // the light surface points gather
    int bake_texels(uint32_t width, uint32_t height, std::vector<MiptSurfacePoint> &points, MiptBakeTexelInfo *info = nullptr) const {
        MiptMulti *m = node_handle(multi_devices_ > 0 ? multi_devices_ : 1);
        return m ? bake_texels_on(mipt_multi_scene(m, 0), width, height, points, info) : MIPT_ERR_HIP;
    }
    int bake_gather(const std::vector<MiptSurfacePoint> &points, std::vector<float> &radiance, const MiptBakeOptions &opt, MiptStats *stats = nullptr) const {
        MiptMulti *m = node_handle(multi_devices_ > 0 ? multi_devices_ : 1);
        return m ? bake_gather_on(mipt_multi_scene(m, 0), points, radiance, opt, stats) : MIPT_ERR_HIP;
    }
    // the guides of lightmap_filter (mipt_bake_surface), on the same replica
    int bake_surface(const std::vector<MiptSurfacePoint> &points, std::vector<float> &position, std::vector<float> &normal, bool unit_normals = false) const {
        MiptMulti *m = node_handle(multi_devices_ > 0 ? multi_devices_ : 1);
        return m ? bake_surface_on(mipt_multi_scene(m, 0), points, position, normal, unit_normals) : MIPT_ERR_HIP;
    }
    // irradiance probes (mipt_probe_bake), on the same replica: 9 SH coefficients x RGB of the light that arrives at every probe
    int bake_probes(const std::vector<MiptProbe> &probes, std::vector<float> &sh, const MiptProbeBakeOptions &opt, MiptStats *stats = nullptr) const {
        MiptMulti *m = node_handle(multi_devices_ > 0 ? multi_devices_ : 1);
        return m ? bake_probes_on(mipt_multi_scene(m, 0), probes, sh, opt, stats) : MIPT_ERR_HIP;
    }

  private:
    mutable std::shared_ptr<MiptMulti> multi_;
    mutable int multi_devices_ = -1;

  public:
    void build_bvh(uint32_t threads = 0) {                 // BVH::build (src/bvh.rs:13-54)
        bvh_nodes.resize(tris.empty() ? 1 : 2 * tris.size());
        uint32_t n = 0;
        if (mipt_bvh_build(tris.data(), (uint32_t)tris.size(), bvh_nodes.data(), (uint32_t)bvh_nodes.size(), &n, threads) != MIPT_OK) n = 0;
        bvh_nodes.resize(n);
        release_device();                                  // the replicas hold the old tree and triangle order
    }
};

class Renderer {                                           // src/renderer.rs:8-85
  public:
    RendererOptions options;

    static std::optional<Renderer> create(const RendererOptions &o) {      // Renderer::new, renderer.rs:14-48
        if (o.output_image_dimensions.first == 0 || o.output_image_dimensions.second == 0) { log_error("Width and height must be greater than 0"); return std::nullopt; }
        if (o.max_ray_depth == 0) { log_error("Max ray depth must be greater than 0"); return std::nullopt; }
        if (o.samples == 0) { log_error("Sample count must be greater than 0"); return std::nullopt; }
        if (!o.output_image_path && !o.is_realtime) { log_error("Output image path must be Some if realtime mode is disabled"); return std::nullopt; }
        if (o.backend != RendererBackend::GPU && o.is_realtime) { log_error("Only the GPU backend is supported for realtime mode"); return std::nullopt; }
        Renderer r;
        r.options = o;
        return r;
    }

    // The offline arm of Renderer::render (renderer.rs:55-64): returns the backend's Vec<u8> (w*h*4 RGBA8 for the
    // MI355X arm, exactly what cpu::render_scene returns).  Empty on error (message logged).
    std::vector<uint8_t> render(const Scene &scene) const {
        if (options.backend != RendererBackend::MI355X) { log_error("this build only provides RendererBackend::MI355X"); return {}; }
        std::vector<MiptMaterial> mats;
        for (const auto &kv : scene.materials) mats.push_back(kv.second);
        std::vector<MiptTexture> texs;
        for (const Texture &t : scene.textures) texs.push_back({t.width, t.height, t.pixel_data.data()});
        MiptSceneDesc d{scene.tris.data(), (uint32_t)scene.tris.size(), scene.bvh_nodes.data(), (uint32_t)scene.bvh_nodes.size(),
                        mats.data(), (uint32_t)mats.size(), texs.data(), (uint32_t)texs.size()};
        MiptScene *h = nullptr;
        // no host-built tree (Scene::load(path, false)): BVH::build + layout on the GPU, identical tree and bytes
        const int rc_create = scene.bvh_nodes.empty() ? mipt_scene_create_from_triangles(&d, options.device_id, &h) : mipt_scene_create(&d, options.device_id, &h);
        if (rc_create != MIPT_OK) { log_error(mipt_last_error()); return {}; }
        MiptOptions o{};
        o.width = (uint32_t)options.output_image_dimensions.first; o.height = (uint32_t)options.output_image_dimensions.second;
        o.samples = (uint32_t)options.samples; o.max_ray_depth = (uint32_t)options.max_ray_depth;
        o.traversal = options.traversal; o.cull_margin = MIPT_CULL_MARGIN_SAFE;
        std::vector<uint8_t> out((size_t)o.width * o.height * 4);
        const int rc = mipt_render(h, &scene.camera.uniform, &o, nullptr, out.data(), nullptr);
        mipt_scene_destroy(h);
        if (rc != MIPT_OK) { log_error(mipt_last_error()); return {}; }
        if (options.output_image_path) {                                   // renderer.rs:66-83 (as Rgba8: SURVEY T12)
            if (mipt_image_save_png(options.output_image_path->c_str(), o.width, o.height, 8, out.data()) == MIPT_OK)
                std::fprintf(stderr, "[INFO] Succesfully wrote image data to '%s'\n", options.output_image_path->c_str());
            else
                log_error(mipt_last_error());
        }
        return out;
    }

    // First-hit feature buffers of the frame(s) this renderer would render (mipt_render_features): `cameras` empty = the scene's camera;
    // `wanted`: FeatureBit flags.  Width, height, samples, max_ray_depth and traversal are this renderer's options; seed_mode is a
    // MiptSeedMode (more than one sample needs MIPT_SEED_PER_SAMPLE).  Runs on the root replica of the scene's device residency
    // (created on first use, like render_node's).  Returns a MiptStatus.
    int render_features(const Scene &scene, const std::vector<MiptCamera> &cameras, uint32_t wanted, FeatureImages &out,
                        uint32_t seed_mode = MIPT_SEED_PIXEL_STREAM, uint32_t flags = 0, MiptStats *stats = nullptr) const {
        if (options.backend != RendererBackend::MI355X) { log_error("this build only provides RendererBackend::MI355X"); return MIPT_ERR_INVALID_ARG; }
        MiptOptions o{};
        o.width = (uint32_t)options.output_image_dimensions.first; o.height = (uint32_t)options.output_image_dimensions.second;
        o.samples = (uint32_t)options.samples; o.max_ray_depth = (uint32_t)options.max_ray_depth;
        o.seed_mode = seed_mode; o.flags = flags;
        o.traversal = options.traversal; o.cull_margin = MIPT_CULL_MARGIN_SAFE;
        const std::vector<MiptCamera> own{scene.camera.uniform};
        const std::vector<MiptCamera> &cams = cameras.empty() ? own : cameras;
        MiptMulti *m = scene.node_handle(1);
        return m ? render_features_on(mipt_multi_scene(m, 0), cams, o, wanted, out, stats) : MIPT_ERR_HIP;
    }

    // Radiance along the caller's rays (mipt_query_radiance) with this renderer's samples, max_ray_depth and traversal, the safe cull
    // margin and CPU-backend shading; `flags`: MIPT_FLAG_COUNT / MIPT_FLAG_SUM.  Residency as render_features.  Returns a MiptStatus.
    int query_radiance(const Scene &scene, const std::vector<MiptRay> &rays, std::vector<float> &radiance, uint32_t flags = 0,
                       MiptStats *stats = nullptr) const {
        if (options.backend != RendererBackend::MI355X) { log_error("this build only provides RendererBackend::MI355X"); return MIPT_ERR_INVALID_ARG; }
        MiptRadianceOptions o{};
        o.samples = (uint32_t)options.samples; o.max_ray_depth = (uint32_t)options.max_ray_depth;
        o.traversal = options.traversal; o.cull_margin = MIPT_CULL_MARGIN_SAFE; o.flags = flags;
        MiptMulti *m = scene.node_handle(1);
        return m ? query_radiance_on(mipt_multi_scene(m, 0), rays, radiance, o, stats) : MIPT_ERR_HIP;
    }

    // Previous positions of the frame(s) this renderer would render (mipt_render_motion): what Renderer::temporal takes as the
    // position image when triangles have moved since the last frame.  `cameras` empty = the scene's camera; `prev_tris`: the previous
    // frame's scene.tris (the order the replicas were built from).  Options and residency as render_features.  Returns a MiptStatus.
    int render_motion(const Scene &scene, const std::vector<MiptCamera> &cameras, const std::vector<MiptTriangle> &prev_tris,
                      std::vector<float> &prev_position, uint32_t seed_mode = MIPT_SEED_PIXEL_STREAM, MiptStats *stats = nullptr) const {
        if (options.backend != RendererBackend::MI355X) { log_error("this build only provides RendererBackend::MI355X"); return MIPT_ERR_INVALID_ARG; }
        MiptOptions o{};
        o.width = (uint32_t)options.output_image_dimensions.first; o.height = (uint32_t)options.output_image_dimensions.second;
        o.samples = (uint32_t)options.samples; o.max_ray_depth = (uint32_t)options.max_ray_depth;
        o.seed_mode = seed_mode;
        o.traversal = options.traversal; o.cull_margin = MIPT_CULL_MARGIN_SAFE;
        const std::vector<MiptCamera> own{scene.camera.uniform};
        const std::vector<MiptCamera> &cams = cameras.empty() ? own : cameras;
        MiptMulti *m = scene.node_handle(1);
        return m ? render_motion_on(mipt_multi_scene(m, 0), cams, o, prev_tris, prev_position, stats) : MIPT_ERR_HIP;
    }

    // The a-trous denoiser (mipt_denoise, include/mipt.h "a-trous denoiser") over host images of this renderer's width and height:
    // `hdr` holds n_views frames of 3 f32 per pixel, view-major, row 0 the top row -- what mipt_render_batch writes.  The guides are
    // the normal, depth and albedo images of `guides` (render_features); an empty one is absent and its term is left out.  `out` is
    // resized and filled; it may be `hdr` itself.  Returns a MiptStatus; a size that does not fit is MIPT_ERR_INVALID_ARG before the
    // library is called.
    int denoise(const std::vector<float> &hdr, uint32_t n_views, const FeatureImages &guides, std::vector<float> &out,
                const DenoiseSettings &settings = DenoiseSettings()) const {
        MiptDenoiseOptions o{};
        o.width = (uint32_t)options.output_image_dimensions.first; o.height = (uint32_t)options.output_image_dimensions.second;
        o.n_views = n_views; o.iterations = settings.iterations;
        o.sigma_color = settings.sigma_color; o.sigma_normal = settings.sigma_normal; o.sigma_depth = settings.sigma_depth;
        const uint64_t n = (uint64_t)o.width * o.height * n_views;
        auto fits = [&](const std::vector<float> &v, uint64_t k, const char *name, bool required) {
            if ((v.empty() && !required) || v.size() == n * k) return true;
            log_error(std::string("Renderer::denoise: ") + name + " holds " + std::to_string(v.size()) + " values, expected " + std::to_string(n * k));
            return false;
        };
        if (n != 0 && n < MIPT_BATCH_MAX_PIXELS &&                         // an impossible size is left to the library to refuse
            !(fits(hdr, 3, "hdr", true) && fits(guides.normal, 3, "normal", false) && fits(guides.depth, 1, "depth", false) && fits(guides.albedo, 3, "albedo", false)))
            return MIPT_ERR_INVALID_ARG;
        static const float no_pixel[3] = {0.0f, 0.0f, 0.0f};
        if (&out != &hdr) out.assign(n != 0 && n < MIPT_BATCH_MAX_PIXELS ? (size_t)n * 3 : 3, 0.0f);
        MiptDenoiseBuffers b{};
        b.hdr = hdr.empty() ? no_pixel : hdr.data();
        b.normal = guides.normal.empty() ? nullptr : guides.normal.data();
        b.depth = guides.depth.empty() ? nullptr : guides.depth.data();
        b.albedo = guides.albedo.empty() ? nullptr : guides.albedo.data();
        b.out = out.data();
        const int rc = mipt_denoise(&o, &b, options.device_id);
        if (rc != MIPT_OK) log_error(mipt_last_error());
        return rc;
    }

    // The variance-guided a-trous filter (mipt_denoise_variance, include/mipt.h "variance-guided a-trous filter") over host images of
    // this renderer's width and height: `hdr` as for denoise, typically what temporal() wrote; `variance` and `length` hold 1 f32 per
    // pixel -- TemporalState's -- and are both empty for a single frame without history; the guides as for denoise.  `out` is resized
    // and filled and may be `hdr` itself; `variance_out`, if given, receives the filtered variance.  Returns a MiptStatus; a size that
    // does not fit is MIPT_ERR_INVALID_ARG before the library is called.
    int denoise_variance(const std::vector<float> &hdr, uint32_t n_views, const std::vector<float> &variance, const std::vector<float> &length,
                         const FeatureImages &guides, std::vector<float> &out, const VarianceSettings &settings = VarianceSettings(),
                         std::vector<float> *variance_out = nullptr) const {
        MiptVarianceOptions o{};
        o.width = (uint32_t)options.output_image_dimensions.first; o.height = (uint32_t)options.output_image_dimensions.second;
        o.n_views = n_views; o.iterations = settings.iterations;
        o.sigma_luminance = settings.sigma_luminance; o.sigma_normal = settings.sigma_normal; o.sigma_depth = settings.sigma_depth;
        o.short_history = settings.short_history;
        const uint64_t n = (uint64_t)o.width * o.height * n_views;
        const bool sized = n != 0 && n < MIPT_BATCH_MAX_PIXELS;            // an impossible size is left to the library to refuse
        auto fits = [&](const std::vector<float> &v, uint64_t k, const char *name, bool required) {
            if ((v.empty() && !required) || v.size() == n * k) return true;
            log_error(std::string("Renderer::denoise_variance: ") + name + " holds " + std::to_string(v.size()) + " values, expected " + std::to_string(n * k));
            return false;
        };
        if (sized && !(fits(hdr, 3, "hdr", true) && fits(guides.normal, 3, "normal", false) && fits(guides.depth, 1, "depth", false) &&
                       fits(guides.albedo, 3, "albedo", false) && fits(variance, 1, "variance", false) && fits(length, 1, "length", false)))
            return MIPT_ERR_INVALID_ARG;
        static const float no_pixel[3] = {0.0f, 0.0f, 0.0f};
        if (&out != &hdr) out.assign(sized ? (size_t)n * 3 : 3, 0.0f);
        if (variance_out) variance_out->assign(sized ? (size_t)n : 1, 0.0f);
        MiptVarianceBuffers b{};
        b.hdr = hdr.empty() ? no_pixel : hdr.data();
        b.normal = guides.normal.empty() ? nullptr : guides.normal.data();
        b.depth = guides.depth.empty() ? nullptr : guides.depth.data();
        b.albedo = guides.albedo.empty() ? nullptr : guides.albedo.data();
        b.variance = variance.empty() ? nullptr : variance.data();
        b.length = length.empty() ? nullptr : length.data();
        b.out = out.data();
        b.variance_out = variance_out ? variance_out->data() : nullptr;
        const int rc = mipt_denoise_variance(&o, &b, options.device_id);
        if (rc != MIPT_OK) log_error(mipt_last_error());
        return rc;
    }

    // The guided upsampling (mipt_upsample, include/mipt.h "guided upsampling") over host images: this renderer's width and height are
    // the FULL frame, `lo_hdr` holds n_views frames of (width/scale) x (height/scale) pixels, 3 f32 each, view-major; `lo_guides` and
    // `guides` the normal, depth, albedo and material images of render_features at the low and at the full resolution, each at both
    // or at neither (empty = absent).  `out` is resized to the full frame and filled; `weight`, if given, receives the sum of the
    // accepted taps' weights, 0 where a pixel fell back to plain bilinear.  Returns a MiptStatus; a size that does not fit is
    // MIPT_ERR_INVALID_ARG before the library is called.
    int upsample(const std::vector<float> &lo_hdr, uint32_t n_views, const FeatureImages &lo_guides, const FeatureImages &guides,
                 std::vector<float> &out, const UpsampleSettings &settings = UpsampleSettings(), std::vector<float> *weight = nullptr) const {
        MiptUpsampleOptions o{};
        o.width = (uint32_t)options.output_image_dimensions.first; o.height = (uint32_t)options.output_image_dimensions.second;
        o.n_views = n_views; o.scale = settings.scale;
        o.sigma_normal = settings.sigma_normal; o.sigma_depth = settings.sigma_depth;
        const uint64_t n = (uint64_t)o.width * o.height * n_views;
        // an impossible size or scale is left to the library to refuse
        const bool sized = n != 0 && n < MIPT_BATCH_MAX_PIXELS && o.scale >= 2 && o.scale <= 8 && o.width % o.scale == 0 && o.height % o.scale == 0;
        const uint64_t n_lo = sized ? n / ((uint64_t)o.scale * o.scale) : 0;
        auto fits = [&](size_t have, uint64_t want, const char *name, bool required) {
            if ((have == 0 && !required) || have == want) return true;
            log_error(std::string("Renderer::upsample: ") + name + " holds " + std::to_string(have) + " values, expected " + std::to_string(want));
            return false;
        };
        if (sized && !(fits(lo_hdr.size(), n_lo * 3, "lo_hdr", true) && fits(lo_guides.normal.size(), n_lo * 3, "lo_normal", false) &&
                       fits(lo_guides.depth.size(), n_lo, "lo_depth", false) && fits(lo_guides.albedo.size(), n_lo * 3, "lo_albedo", false) &&
                       fits(lo_guides.material.size(), n_lo, "lo_material", false) && fits(guides.normal.size(), n * 3, "normal", false) &&
                       fits(guides.depth.size(), n, "depth", false) && fits(guides.albedo.size(), n * 3, "albedo", false) &&
                       fits(guides.material.size(), n, "material", false)))
            return MIPT_ERR_INVALID_ARG;
        static const float no_pixel[3] = {0.0f, 0.0f, 0.0f};
        out.assign(sized ? (size_t)n * 3 : 3, 0.0f);
        if (weight) weight->assign(sized ? (size_t)n : 1, 0.0f);
        auto plane = [](const auto &v) { return v.empty() ? nullptr : v.data(); };
        MiptUpsampleBuffers b{};
        b.lo_hdr = lo_hdr.empty() ? no_pixel : lo_hdr.data();
        b.lo_normal = plane(lo_guides.normal); b.lo_depth = plane(lo_guides.depth); b.lo_albedo = plane(lo_guides.albedo);
        b.lo_material = plane(lo_guides.material);
        b.normal = plane(guides.normal); b.depth = plane(guides.depth); b.albedo = plane(guides.albedo); b.material = plane(guides.material);
        b.out = out.data();
        b.weight = weight ? weight->data() : nullptr;
        const int rc = mipt_upsample(&o, &b, options.device_id);
        if (rc != MIPT_OK) log_error(mipt_last_error());
        return rc;
    }

    // A batch render with a count plane (mipt_render_adaptive, include/mipt.h "adaptive sampling"): `counts` holds one u32 per pixel of
    // every view, view-major; pixel p of view v is traced with min(counts, options.samples) samples and holds what a render with that
    // many samples gives, a pixel with 0 is not traced and holds 0.  `cameras` empty = the scene's camera.  `hdr` is resized and
    // filled (3 f32 per pixel); `rgba8`, if given, receives the tone-mapped frame.  seed_mode and flags as render_features
    // (MIPT_FLAG_COUNT, MIPT_FLAG_SUM).  Runs on the root replica of the scene's device residency.  Returns a MiptStatus; a count
    // plane of the wrong size is MIPT_ERR_INVALID_ARG before the library is called.
    int render_adaptive(const Scene &scene, const std::vector<MiptCamera> &cameras, const std::vector<uint32_t> &counts, std::vector<float> &hdr,
                        std::vector<uint8_t> *rgba8 = nullptr, uint32_t seed_mode = MIPT_SEED_PIXEL_STREAM, uint32_t flags = 0,
                        uint32_t sample_begin = 0, MiptStats *stats = nullptr) const {
        if (options.backend != RendererBackend::MI355X) { log_error("this build only provides RendererBackend::MI355X"); return MIPT_ERR_INVALID_ARG; }
        MiptOptions o{};
        o.width = (uint32_t)options.output_image_dimensions.first; o.height = (uint32_t)options.output_image_dimensions.second;
        o.samples = (uint32_t)options.samples; o.max_ray_depth = (uint32_t)options.max_ray_depth;
        o.seed_mode = seed_mode; o.flags = flags; o.sample_begin = sample_begin;
        o.traversal = options.traversal; o.cull_margin = MIPT_CULL_MARGIN_SAFE;
        const std::vector<MiptCamera> own{scene.camera.uniform};
        const std::vector<MiptCamera> &cams = cameras.empty() ? own : cameras;
        const uint64_t n = (uint64_t)o.width * o.height * cams.size();
        const bool sized = n != 0 && n < MIPT_BATCH_MAX_PIXELS;            // an impossible size is left to the library to refuse
        if (sized && counts.size() != n) {
            log_error("Renderer::render_adaptive: counts holds " + std::to_string(counts.size()) + " values, expected " + std::to_string(n));
            return MIPT_ERR_INVALID_ARG;
        }
        MiptMulti *m = scene.node_handle(1);
        if (!m) return MIPT_ERR_HIP;
        hdr.assign(sized ? (size_t)n * 3 : 3, 0.0f);
        if (rgba8) rgba8->assign(sized ? (size_t)n * 4 : 4, 0);
        const int rc = mipt_render_adaptive(mipt_multi_scene(m, 0), cams.data(), (uint32_t)cams.size(), &o, counts.empty() ? nullptr : counts.data(),
                                            hdr.data(), rgba8 ? rgba8->data() : nullptr, stats);
        if (rc != MIPT_OK) log_error(mipt_last_error());
        return rc;
    }

    // The sample map (mipt_sample_map, include/mipt.h "adaptive sampling") over host images of this renderer's width and height:
    // `variance` holds n_views planes of 1 f32 per pixel -- denoise_variance's variance_out, or TemporalState's -- and becomes
    // `counts`, one u32 per pixel in [min_samples, max_samples] with a mean of at most `budget`, for render_adaptive.  `hdr` (3 f32
    // per pixel, empty = absent) makes the weight relative to the frame's luminance; `albedo` (only with hdr) demodulates it first.
    // `counts` is resized and filled.  Returns a MiptStatus; a size that does not fit is MIPT_ERR_INVALID_ARG before the library is
    // called.
    int sample_map(const std::vector<float> &variance, uint32_t n_views, const std::vector<float> &hdr, const std::vector<float> &albedo,
                   std::vector<uint32_t> &counts, const SampleMapSettings &settings = SampleMapSettings()) const {
        MiptSampleMapOptions o{};
        o.width = (uint32_t)options.output_image_dimensions.first; o.height = (uint32_t)options.output_image_dimensions.second;
        o.n_views = n_views;
        o.min_samples = settings.min_samples;
        o.max_samples = settings.max_samples ? settings.max_samples : (uint32_t)options.samples;
        o.budget = settings.budget < 0.0f ? (float)settings.min_samples : settings.budget;
        const uint64_t n = (uint64_t)o.width * o.height * n_views;
        const bool sized = n != 0 && n < MIPT_BATCH_MAX_PIXELS;            // an impossible size is left to the library to refuse
        auto fits = [&](const std::vector<float> &v, uint64_t k, const char *name, bool required) {
            if ((v.empty() && !required) || v.size() == n * k) return true;
            log_error(std::string("Renderer::sample_map: ") + name + " holds " + std::to_string(v.size()) + " values, expected " + std::to_string(n * k));
            return false;
        };
        if (sized && !(fits(variance, 1, "variance", true) && fits(hdr, 3, "hdr", false) && fits(albedo, 3, "albedo", false))) return MIPT_ERR_INVALID_ARG;
        static const float no_pixel[3] = {0.0f, 0.0f, 0.0f};
        counts.assign(sized ? (size_t)n : 1, 0u);
        MiptSampleMapBuffers b{};
        b.variance = variance.empty() ? no_pixel : variance.data();
        b.hdr = hdr.empty() ? nullptr : hdr.data();
        b.albedo = albedo.empty() ? nullptr : albedo.data();
        b.counts = counts.data();
        int rc;
        if (settings.rounds) {
            MiptSampleMapFillOptions f{};
            f.width = o.width; f.height = o.height; f.n_views = o.n_views;
            f.min_samples = o.min_samples; f.max_samples = o.max_samples; f.budget = o.budget; f.rounds = settings.rounds;
            rc = mipt_sample_map_fill(&f, &b, options.device_id);
        } else {
            rc = mipt_sample_map(&o, &b, options.device_id);
        }
        if (rc != MIPT_OK) log_error(mipt_last_error());
        return rc;
    }

    // The temporal accumulation (mipt_temporal, include/mipt.h "temporal accumulation") over host images of this renderer's width and
    // height: `hdr` holds cameras.size() frames of 3 f32 per pixel, view-major; `guides` the position, normal, depth and material
    // images of render_features for the same cameras, and the albedo image if the frame is to be demodulated (empty = absent).
    // `state.history` is the previous call's (empty = the first frame) and is replaced by this frame's; `out` is resized and filled
    // and may be `hdr` itself.  Returns a MiptStatus; a size that does not fit is MIPT_ERR_INVALID_ARG before the library is called.
    int temporal(const std::vector<float> &hdr, const std::vector<MiptCamera> &cameras, const FeatureImages &guides, TemporalState &state,
                 std::vector<float> &out, const TemporalSettings &settings = TemporalSettings()) const {
        return temporal_call(hdr, cameras, guides, state, out, nullptr, 0, settings);
    }
    // The same with the history length counted in samples (mipt_temporal_counts): `counts` is the plane render_adaptive was given for
    // this frame, one u32 per pixel, and `samples_cap` that call's cap (0 = options.samples).  settings.max_history is then a
    // number of samples.
    int temporal(const std::vector<float> &hdr, const std::vector<MiptCamera> &cameras, const FeatureImages &guides, TemporalState &state,
                 std::vector<float> &out, const std::vector<uint32_t> &counts, uint32_t samples_cap = 0,
                 const TemporalSettings &settings = TemporalSettings()) const {
        return temporal_call(hdr, cameras, guides, state, out, &counts, samples_cap ? samples_cap : (uint32_t)options.samples, settings);
    }

  private:
    int temporal_call(const std::vector<float> &hdr, const std::vector<MiptCamera> &cameras, const FeatureImages &guides, TemporalState &state,
                      std::vector<float> &out, const std::vector<uint32_t> *counts, uint32_t samples_cap, const TemporalSettings &settings) const {
        MiptTemporalOptions o{};
        o.width = (uint32_t)options.output_image_dimensions.first; o.height = (uint32_t)options.output_image_dimensions.second;
        o.n_views = (uint32_t)cameras.size();
        o.alpha_min = settings.alpha_min; o.max_history = settings.max_history; o.normal_tol = settings.normal_tol; o.depth_tol = settings.depth_tol;
        const uint64_t n = (uint64_t)o.width * o.height * o.n_views;
        const bool sized = n != 0 && n < MIPT_BATCH_MAX_PIXELS;              // an impossible size is left to the library to refuse
        const uint64_t words = mipt_temporal_history_bytes(o.width, o.height, o.n_views) / 4;
        auto fits = [&](size_t have, uint64_t want, const char *name, bool required) {
            if ((have == 0 && !required) || have == want) return true;
            log_error(std::string("Renderer::temporal: ") + name + " holds " + std::to_string(have) + " values, expected " + std::to_string(want));
            return false;
        };
        if (sized && !(fits(hdr.size(), n * 3, "hdr", true) && fits(guides.position.size(), n * 3, "position", true) &&
                       fits(guides.normal.size(), n * 3, "normal", true) && fits(guides.depth.size(), n, "depth", true) &&
                       fits(guides.material.size(), n, "material", true) && fits(guides.albedo.size(), n * 3, "albedo", false) &&
                       fits(state.history.size(), words, "history", false) && (!counts || fits(counts->size(), n, "counts", true))))
            return MIPT_ERR_INVALID_ARG;
        static const float no_pixel[3] = {0.0f, 0.0f, 0.0f};
        static const uint32_t no_material = 0;
        static const MiptCamera no_camera{};
        if (&out != &hdr) out.assign(sized ? (size_t)n * 3 : 3, 0.0f);
        std::vector<uint32_t> next(sized ? (size_t)words : 4, 0u);
        state.length.assign(settings.want_length ? (sized ? (size_t)n : 1) : 0, 0.0f);
        state.variance.assign(settings.want_variance ? (sized ? (size_t)n : 1) : 0, 0.0f);
        MiptTemporalBuffers b{};
        b.hdr = hdr.empty() ? no_pixel : hdr.data();
        b.position = guides.position.empty() ? no_pixel : guides.position.data();
        b.normal = guides.normal.empty() ? no_pixel : guides.normal.data();
        b.depth = guides.depth.empty() ? no_pixel : guides.depth.data();
        b.material = guides.material.empty() ? &no_material : guides.material.data();
        b.albedo = guides.albedo.empty() ? nullptr : guides.albedo.data();
        b.history_in = state.history.empty() ? nullptr : state.history.data();
        b.history_out = next.data();
        b.out = out.data();
        b.length = settings.want_length ? state.length.data() : nullptr;
        b.variance = settings.want_variance ? state.variance.data() : nullptr;
        const MiptCamera *cams = cameras.empty() ? &no_camera : cameras.data();
        const int rc = counts ? mipt_temporal_counts(&o, cams, &b, counts->empty() ? nullptr : counts->data(), samples_cap, options.device_id)
                              : mipt_temporal(&o, cams, &b, options.device_id);
        if (rc != MIPT_OK) log_error(mipt_last_error());
        else state.history.swap(next);
        return rc;
    }

  public:

    // The same arm over EVERY GPU of the node from this single-threaded host (mipt_render_multi: scene replicas, RCCL
    // communicators and the one gather / sum-reduce per frame live inside the library).  mode = MIPT_MULTI_TILES reproduces
    // render()'s bytes exactly; MIPT_MULTI_SAMPLES uses the wgpu shader's per-sample seeds (rt_compute.wgsl:102).
    std::vector<uint8_t> render_node(const Scene &scene, uint32_t mode = MIPT_MULTI_TILES, int n_devices = 0) const {
        if (options.backend != RendererBackend::MI355X) { log_error("this build only provides RendererBackend::MI355X"); return {}; }
        MiptMulti *m = scene.node_handle(n_devices);                       // cached in the Scene: created on the first frame only
        if (!m) return {};
        MiptOptions o{};
        o.width = (uint32_t)options.output_image_dimensions.first; o.height = (uint32_t)options.output_image_dimensions.second;
        o.samples = (uint32_t)options.samples; o.max_ray_depth = (uint32_t)options.max_ray_depth;
        o.traversal = options.traversal; o.cull_margin = MIPT_CULL_MARGIN_SAFE;
        std::vector<uint8_t> out((size_t)o.width * o.height * 4);
        const int rc = mipt_render_multi(m, &scene.camera.uniform, &o, mode, nullptr, out.data(), nullptr);
        if (rc != MIPT_OK) { log_error(mipt_last_error()); return {}; }
        return out;
    }
};

} // namespace mipt
