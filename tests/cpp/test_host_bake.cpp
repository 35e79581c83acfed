// Exercises the baking methods of include/mipt_host.hpp (bake_texels_on, bake_gather_on, Scene::bake_texels, Scene::bake_gather)
// against the C entries they wrap.
//   test_host_bake cpu                   argument handling without a device
//   test_host_bake gpu scene.obj out.bin Scene::bake_texels at 24 x 24, then Scene::bake_gather (3 samples, depth 4) on those points;
//                                        both are compared here with direct calls of the C entries on a scene of the same arrays, and
//                                        out.bin receives the points (576 x 16 B) and the radiance (576 x 3 f32) for the model
#include "mipt_host.hpp"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "CHECK failed at line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static int run_cpu() {
    MiptScene *opaque = reinterpret_cast<MiptScene *>(0x1000);           // never dereferenced by the checks below
    std::vector<MiptSurfacePoint> none, points(5);
    std::vector<float> radiance(7, 1.0f);
    MiptBakeOptions opt{};
    opt.samples = 2; opt.max_ray_depth = 4; opt.sample_stride = 1;
    MiptStats st;
    std::memset(&st, 0xff, sizeof st);
    CHECK(mipt::bake_gather_on(opaque, none, radiance, opt, &st) == MIPT_OK && radiance.empty() && st.rays == 0);
    std::vector<MiptSurfacePoint> two(2);
    MiptBakeOptions bad = opt;
    bad.sample_stride = 0;
    CHECK(mipt::bake_gather_on(opaque, two, radiance, bad) == MIPT_ERR_INVALID_ARG && radiance.size() == 6);
    CHECK(std::string(mipt_last_error()).find("sample_stride") != std::string::npos);
    bad = opt; bad.shading = 9;
    CHECK(mipt::bake_gather_on(opaque, two, radiance, bad) == MIPT_ERR_INVALID_ARG);
    bad = opt; bad.flags = MIPT_FLAG_SUM | MIPT_FLAG_ACCUM;                 // a running sum lives in device memory
    CHECK(mipt::bake_gather_on(opaque, two, radiance, bad) == MIPT_ERR_INVALID_ARG);
    CHECK(std::string(mipt_last_error()).find("mipt_bake_gather_device") != std::string::npos);
    CHECK(mipt::bake_gather_on(nullptr, two, radiance, opt) == MIPT_ERR_INVALID_ARG && radiance.size() == 6);
    MiptBakeTexelInfo info;
    std::memset(&info, 0xff, sizeof info);
    CHECK(mipt::bake_texels_on(opaque, 0, 9, points, &info) == MIPT_OK && points.empty() && info.covered_texels == 0);
    CHECK(mipt::bake_texels_on(nullptr, 2, 2, points) == MIPT_ERR_INVALID_ARG && points.size() == 4);
    std::puts("cpu ok");
    return 0;
}

static int run_gpu(const char *obj, const char *out_path) {
    auto scene = mipt::Scene::load(obj);
    CHECK(scene.has_value());
    const uint32_t w = 24, h = 24;
    std::vector<MiptSurfacePoint> points;
    MiptBakeTexelInfo info{};
    CHECK(scene->bake_texels(w, h, points, &info) == MIPT_OK && points.size() == (size_t)w * h);
    size_t covered = 0;
    for (const MiptSurfacePoint &p : points) covered += p.prim != MIPT_HIT_NONE;
    CHECK(covered == info.covered_texels && covered > 0);
    MiptBakeOptions opt{};
    opt.samples = 3; opt.max_ray_depth = 4; opt.sample_stride = w * h; opt.flags = MIPT_FLAG_COUNT;
    std::vector<float> radiance;
    MiptStats st{};
    CHECK(scene->bake_gather(points, radiance, opt, &st) == MIPT_OK && radiance.size() == points.size() * 3);
    CHECK(st.pixels == points.size() * 3 && st.rays >= points.size() * 3);
    // the C entries, on a scene made of the same arrays
    std::vector<MiptMaterial> mats;
    for (const auto &kv : scene->materials) mats.push_back(kv.second);
    std::vector<MiptTexture> texs;
    for (const mipt::Texture &t : scene->textures) texs.push_back({t.width, t.height, t.pixel_data.data()});
    MiptSceneDesc d{scene->tris.data(), (uint32_t)scene->tris.size(), scene->bvh_nodes.data(), (uint32_t)scene->bvh_nodes.size(),
                    mats.data(), (uint32_t)mats.size(), texs.data(), (uint32_t)texs.size()};
    MiptScene *raw = nullptr;
    CHECK(mipt_scene_create(&d, 0, &raw) == MIPT_OK);
    std::vector<MiptSurfacePoint> points2(points.size());
    std::vector<float> radiance2(radiance.size());
    CHECK(mipt_bake_texels(raw, w, h, nullptr, points2.data(), nullptr) == MIPT_OK);
    CHECK(std::memcmp(points.data(), points2.data(), points.size() * sizeof(MiptSurfacePoint)) == 0);
    CHECK(mipt_bake_gather(raw, points2.data(), points2.size(), &opt, radiance2.data(), nullptr) == MIPT_OK);
    CHECK(std::memcmp(radiance.data(), radiance2.data(), radiance.size() * sizeof(float)) == 0);
    mipt_scene_destroy(raw);
    std::FILE *out = std::fopen(out_path, "wb");
    CHECK(out);
    std::fwrite(points.data(), sizeof(MiptSurfacePoint), points.size(), out);
    std::fwrite(radiance.data(), sizeof(float), radiance.size(), out);
    std::fclose(out);
    std::puts("gpu ok");
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && std::string(argv[1]) == "cpu") return run_cpu();
    if (argc >= 4 && std::string(argv[1]) == "gpu") return run_gpu(argv[2], argv[3]);
    std::fprintf(stderr, "usage: test_host_bake cpu | gpu scene.obj out.bin\n");
    return 2;
}
