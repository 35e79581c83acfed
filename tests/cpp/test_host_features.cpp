// Exercises the first-hit feature methods of include/mipt_host.hpp (render_features_on, Renderer::render_features).
//   test_host_features cpu                      argument handling without a device
//   test_host_features gpu scene.obj out.bin x y z pitch yaw    out.bin: the eight images of that camera at 24 x 16, two samples,
//                                                               in MiptFeatureBuffers order
#include "mipt_host.hpp"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "CHECK failed at line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static bool says(const char *what) { return std::string(mipt_last_error()).find(what) != std::string::npos; }

static int run_cpu() {
    static_assert(sizeof(MiptFeatureBuffers) == 96, "ABI struct size");
    MiptScene *opaque = reinterpret_cast<MiptScene *>(0x1000);           // never dereferenced by the checks below
    std::vector<MiptCamera> cams(2);
    MiptOptions o{};
    o.width = 8; o.height = 4; o.samples = 1; o.max_ray_depth = 1;
    mipt::FeatureImages img;
    CHECK(mipt::render_features_on(nullptr, cams, o, mipt::FEATURE_ALL, img) == MIPT_ERR_INVALID_ARG && says("null scene"));
    CHECK(img.n_views == 2 && img.width == 8 && img.height == 4);
    CHECK(img.depth.size() == 64 && img.prim.size() == 64 && img.material.size() == 64 && img.position.size() == 192 && img.uv.size() == 128);
    CHECK(img.normal.size() == 192 && img.albedo.size() == 192 && img.emission.size() == 192);
    CHECK(mipt::render_features_on(opaque, cams, o, 0u, img) == MIPT_ERR_INVALID_ARG && says("no buffer wanted") && img.depth.empty());
    CHECK(mipt::render_features_on(opaque, {}, o, mipt::FEATURE_DEPTH, img) == MIPT_ERR_INVALID_ARG && says("n_views"));
    MiptOptions bad = o;
    bad.samples = 2;                                                     // the pixel stream defines one sample only
    CHECK(mipt::render_features_on(opaque, cams, bad, mipt::FEATURE_NORMAL, img) == MIPT_ERR_INVALID_ARG && says("MIPT_SEED_PIXEL_STREAM"));
    CHECK(img.normal.size() == 192 && img.depth.empty());
    bad = o; bad.shading = MIPT_SHADING_WGPU;
    CHECK(mipt::render_features_on(opaque, cams, bad, mipt::FEATURE_ALBEDO, img) == MIPT_ERR_INVALID_ARG && says("shading") && says("out of scope"));
    bad = o; bad.flags = MIPT_FLAG_SUM;
    CHECK(mipt::render_features_on(opaque, cams, bad, mipt::FEATURE_ALBEDO, img) == MIPT_ERR_INVALID_ARG && says("flags"));
    bad = o; bad.tile_world = 2;
    CHECK(mipt::render_features_on(opaque, cams, bad, mipt::FEATURE_ALBEDO, img) == MIPT_ERR_INVALID_ARG && says("tile_world"));
    bad = o; bad.width = 70000; bad.height = 70000;                      // an impossible frame is refused before anything is allocated
    CHECK(mipt::render_features_on(opaque, cams, bad, mipt::FEATURE_ALL, img) == MIPT_ERR_INVALID_ARG && img.emission.size() == 1);
    mipt::RendererOptions ro;
    ro.output_image_path = "unused.png"; ro.is_realtime = false; ro.backend = mipt::RendererBackend::CPU;
    auto r = mipt::Renderer::create(ro);
    CHECK(r.has_value());
    CHECK(r->render_features(mipt::Scene(), {}, mipt::FEATURE_DEPTH, img) == MIPT_ERR_INVALID_ARG);   // not the MI355X arm
    std::puts("cpu ok");
    return 0;
}

static int run_gpu(const char *obj, const char *out_path, char **pose) {
    auto scene = mipt::Scene::load(obj);
    CHECK(scene.has_value());
    mipt::Camera cam;
    for (int k = 0; k < 3; k++) cam.position[k] = std::stof(pose[k]);
    cam.pitch = std::stof(pose[3]); cam.yaw = std::stof(pose[4]);
    scene->set_camera(cam);
    mipt::RendererOptions ro;
    ro.samples = 2; ro.max_ray_depth = 3; ro.output_image_dimensions = {24, 16};
    ro.output_image_path = "unused.png"; ro.is_realtime = false; ro.backend = mipt::RendererBackend::MI355X;
    ro.traversal = MIPT_TRAVERSAL_REFERENCE;
    auto r = mipt::Renderer::create(ro);
    CHECK(r.has_value());
    mipt::FeatureImages img;
    MiptStats st{};
    CHECK(r->render_features(*scene, {}, mipt::FEATURE_ALL, img, MIPT_SEED_PER_SAMPLE, MIPT_FLAG_COUNT, &st) == MIPT_OK);
    CHECK(st.pixels == 24 * 16 && st.rays == 2 * 24 * 16 && img.n_views == 1);
    mipt::FeatureImages two;
    CHECK(r->render_features(*scene, {}, mipt::FEATURE_DEPTH | mipt::FEATURE_ALBEDO, two, MIPT_SEED_PER_SAMPLE) == MIPT_OK);
    CHECK(two.depth == img.depth && two.prim.empty() && two.normal.empty());
    CHECK(std::memcmp(two.albedo.data(), img.albedo.data(), img.albedo.size() * sizeof(float)) == 0);
    std::FILE *out = std::fopen(out_path, "wb");
    CHECK(out);
    std::fwrite(img.depth.data(), 4, img.depth.size(), out); std::fwrite(img.prim.data(), 4, img.prim.size(), out);
    std::fwrite(img.material.data(), 4, img.material.size(), out); std::fwrite(img.position.data(), 4, img.position.size(), out);
    std::fwrite(img.uv.data(), 4, img.uv.size(), out); std::fwrite(img.normal.data(), 4, img.normal.size(), out);
    std::fwrite(img.albedo.data(), 4, img.albedo.size(), out); std::fwrite(img.emission.data(), 4, img.emission.size(), out);
    std::fclose(out);
    std::puts("gpu ok");
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && std::string(argv[1]) == "cpu") return run_cpu();
    if (argc >= 9 && std::string(argv[1]) == "gpu") return run_gpu(argv[2], argv[3], argv + 4);
    std::fprintf(stderr, "usage: test_host_features cpu | gpu scene.obj out.bin x y z pitch yaw\n");
    return 2;
}
