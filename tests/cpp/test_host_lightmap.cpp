// Exercises the lightmap methods of include/mipt_host.hpp (bake_surface_on, Scene::bake_surface, mipt::lightmap_filter,
// mipt::lightmap_dilate) against the C entries they wrap.
//   test_host_lightmap cpu                   argument handling without a device
//   test_host_lightmap gpu scene.obj out.bin Scene::bake_texels at 24 x 24, bake_gather (2 samples, depth 4), bake_surface (unit
//                                            normals), lightmap_filter (2 iterations, both guides), lightmap_dilate (radius 2, levels);
//                                            each is compared here with a direct call of its C entry, and out.bin receives the points
//                                            (576 x 16 B), then radiance, position, normal, filtered, dilated (576 x 3 f32 each) and
//                                            the levels (576 u32) for the models
#include "mipt_host.hpp"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "CHECK failed at line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static bool says(const char *what) { return std::string(mipt_last_error()).find(what) != std::string::npos; }

static int run_cpu() {
    MiptScene *opaque = reinterpret_cast<MiptScene *>(0x1000);           // never dereferenced by the checks below
    std::vector<MiptSurfacePoint> none, points(6);
    std::vector<float> position(5, 1.0f), normal(5, 1.0f);
    CHECK(mipt::bake_surface_on(opaque, none, position, normal) == MIPT_OK && position.empty() && normal.empty());
    CHECK(mipt::bake_surface_on(nullptr, points, position, normal, true) == MIPT_ERR_INVALID_ARG && position.size() == 18 && normal.size() == 18);
    CHECK(says("mipt_bake_surface: null scene or points"));
    const int no_device = 1 << 20;
    std::vector<float> radiance(6 * 3, 0.5f), out, guide(6 * 3, 0.0f), empty, wrong(7);
    mipt::LightmapFilterSettings s;
    CHECK(mipt::lightmap_filter(3, 2, wrong, points, empty, empty, out) == MIPT_ERR_INVALID_ARG);       // refused by the wrapper
    CHECK(mipt::lightmap_filter(3, 2, radiance, points, wrong, empty, out) == MIPT_ERR_INVALID_ARG);
    CHECK(mipt::lightmap_filter(3, 2, radiance, none, empty, empty, out) == MIPT_ERR_INVALID_ARG);
    s.iterations = 9;
    CHECK(mipt::lightmap_filter(3, 2, radiance, points, empty, empty, out, s, no_device) == MIPT_ERR_INVALID_ARG && says("iterations 9") && out.size() == 18);
    s = {};
    s.sigma_plane = 0.0f;                                                // ignored without both guides, refused with them
    CHECK(mipt::lightmap_filter(3, 2, radiance, points, guide, empty, out, s, no_device) == MIPT_ERR_HIP && says("hipSetDevice"));
    CHECK(mipt::lightmap_filter(3, 2, radiance, points, guide, guide, out, s, no_device) == MIPT_ERR_INVALID_ARG && says("sigma_plane"));
    CHECK(mipt::lightmap_filter(3, 2, radiance, points, empty, empty, radiance, {}, no_device) == MIPT_ERR_HIP && radiance.size() == 18);   // out == radiance
    std::vector<uint32_t> level(2, 7u);
    CHECK(mipt::lightmap_dilate(3, 2, wrong, points, 1, out) == MIPT_ERR_INVALID_ARG);
    CHECK(mipt::lightmap_dilate(3, 2, radiance, points, 65, out, &level, no_device) == MIPT_ERR_INVALID_ARG && says("radius 65") && level.size() == 6);
    CHECK(mipt::lightmap_dilate(3, 2, radiance, points, 64, out, &level, no_device) == MIPT_ERR_HIP && says("hipSetDevice"));
    CHECK(mipt::lightmap_dilate(0, 2, empty, none, 1, out) == MIPT_ERR_INVALID_ARG);                   // an atlas without texels is refused
    std::puts("cpu ok");
    return 0;
}

template <class T> static bool same(const std::vector<T> &a, const std::vector<T> &b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0;
}

static int run_gpu(const char *obj, const char *out_path) {
    auto scene = mipt::Scene::load(obj);
    CHECK(scene.has_value());
    const uint32_t w = 24, h = 24;
    const size_t n = (size_t)w * h;
    std::vector<MiptSurfacePoint> points;
    CHECK(scene->bake_texels(w, h, points) == MIPT_OK && points.size() == n);
    MiptBakeOptions opt{};
    opt.samples = 2; opt.max_ray_depth = 4; opt.sample_stride = w * h;
    std::vector<float> radiance, position, normal, filtered, dilated;
    std::vector<uint32_t> level;
    CHECK(scene->bake_gather(points, radiance, opt) == MIPT_OK && radiance.size() == n * 3);
    CHECK(scene->bake_surface(points, position, normal, true) == MIPT_OK && position.size() == n * 3 && normal.size() == n * 3);
    mipt::LightmapFilterSettings s;
    s.iterations = 2; s.sigma_color = 2.0f; s.sigma_plane = 0.1f;
    CHECK(mipt::lightmap_filter(w, h, radiance, points, position, normal, filtered, s) == MIPT_OK && filtered.size() == n * 3);
    CHECK(mipt::lightmap_dilate(w, h, filtered, points, 2, dilated, &level) == MIPT_OK && dilated.size() == n * 3 && level.size() == n);
    std::vector<float> in_place = filtered;                              // out == radiance
    CHECK(mipt::lightmap_dilate(w, h, in_place, points, 2, in_place) == MIPT_OK && same(in_place, dilated));
    // the C entries, on a scene made of the same arrays
    std::vector<MiptMaterial> mats;
    for (const auto &kv : scene->materials) mats.push_back(kv.second);
    std::vector<MiptTexture> texs;
    for (const mipt::Texture &t : scene->textures) texs.push_back({t.width, t.height, t.pixel_data.data()});
    MiptSceneDesc d{scene->tris.data(), (uint32_t)scene->tris.size(), scene->bvh_nodes.data(), (uint32_t)scene->bvh_nodes.size(),
                    mats.data(), (uint32_t)mats.size(), texs.data(), (uint32_t)texs.size()};
    MiptScene *raw = nullptr;
    CHECK(mipt_scene_create(&d, 0, &raw) == MIPT_OK);
    std::vector<float> position2(n * 3), normal2(n * 3), filtered2(n * 3), dilated2(n * 3);
    std::vector<uint32_t> level2(n);
    MiptBakeSurfaceOptions so{};
    so.flags = MIPT_BAKE_SURFACE_UNIT_NORMALS;
    CHECK(mipt_bake_surface(raw, points.data(), n, &so, position2.data(), normal2.data()) == MIPT_OK);
    CHECK(same(position, position2) && same(normal, normal2));
    mipt_scene_destroy(raw);
    MiptLightmapFilterOptions fo{};
    fo.width = w; fo.height = h; fo.iterations = 2; fo.sigma_color = 2.0f; fo.sigma_normal = 0.5f; fo.sigma_plane = 0.1f; fo.sigma_distance = 0.5f;
    MiptLightmapFilterBuffers fb{};
    fb.radiance = radiance.data(); fb.points = points.data(); fb.position = position.data(); fb.normal = normal.data(); fb.out = filtered2.data();
    CHECK(mipt_lightmap_filter(&fo, &fb, 0) == MIPT_OK && same(filtered, filtered2));
    MiptLightmapDilateOptions dopt{};
    dopt.width = w; dopt.height = h; dopt.radius = 2;
    MiptLightmapDilateBuffers db{};
    db.radiance = filtered.data(); db.points = points.data(); db.out = dilated2.data(); db.level = level2.data();
    CHECK(mipt_lightmap_dilate(&dopt, &db, 0) == MIPT_OK && same(dilated, dilated2) && same(level, level2));
    std::FILE *out = std::fopen(out_path, "wb");
    CHECK(out);
    std::fwrite(points.data(), sizeof(MiptSurfacePoint), n, out);
    for (const std::vector<float> *v : {&radiance, &position, &normal, &filtered, &dilated}) std::fwrite(v->data(), sizeof(float), n * 3, out);
    std::fwrite(level.data(), sizeof(uint32_t), n, out);
    std::fclose(out);
    std::puts("gpu ok");
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && std::string(argv[1]) == "cpu") return run_cpu();
    if (argc >= 4 && std::string(argv[1]) == "gpu") return run_gpu(argv[2], argv[3]);
    std::fprintf(stderr, "usage: test_host_lightmap cpu | gpu scene.obj out.bin\n");
    return 2;
}
