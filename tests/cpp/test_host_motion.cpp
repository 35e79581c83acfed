// Exercises the previous-position methods of include/mipt_host.hpp (render_motion_on, Renderer::render_motion).
//   test_host_motion cpu                      argument handling without a device
//   test_host_motion gpu scene.obj out.bin x y z pitch yaw    out.bin: prev_position of that camera at 24 x 16 (per-sample seeds), the
//                                                             previous frame being the scene moved by (0.25, -0.5, 0.125)
#include "mipt_host.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "CHECK failed at line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static bool says(const char *what) { return std::string(mipt_last_error()).find(what) != std::string::npos; }

static int run_cpu() {
    static_assert(sizeof(MiptMotionBuffers) == 64, "ABI struct size");
    MiptScene *opaque = reinterpret_cast<MiptScene *>(0x1000);           // never dereferenced by the checks below
    std::vector<MiptCamera> cams(2);
    std::vector<MiptTriangle> none;
    MiptOptions o{};
    o.width = 8; o.height = 4; o.samples = 1; o.max_ray_depth = 1;
    std::vector<float> img;
    CHECK(mipt::render_motion_on(nullptr, cams, o, none, img) == MIPT_ERR_INVALID_ARG && says("null scene"));
    CHECK(img.size() == 2 * 8 * 4 * 3);
    CHECK(mipt::render_motion_on(opaque, {}, o, none, img) == MIPT_ERR_INVALID_ARG && says("n_views"));
    MiptOptions bad = o;
    bad.samples = 2;                                                     // validated as the feature pass validates it
    CHECK(mipt::render_motion_on(opaque, cams, bad, none, img) == MIPT_ERR_INVALID_ARG && says("MIPT_SEED_PIXEL_STREAM"));
    bad = o; bad.flags = MIPT_FLAG_COUNT;
    CHECK(mipt::render_motion_on(opaque, cams, bad, none, img) == MIPT_ERR_INVALID_ARG && says("flags"));
    bad = o; bad.shading = MIPT_SHADING_WGPU;
    CHECK(mipt::render_motion_on(opaque, cams, bad, none, img) == MIPT_ERR_INVALID_ARG && says("shading"));
    bad = o; bad.tile_world = 2;
    CHECK(mipt::render_motion_on(opaque, cams, bad, none, img) == MIPT_ERR_INVALID_ARG && says("tile_world"));
    bad = o; bad.width = 70000; bad.height = 70000;                      // an impossible frame is refused before anything is allocated
    CHECK(mipt::render_motion_on(opaque, cams, bad, none, img) == MIPT_ERR_INVALID_ARG && img.size() == 1);
    MiptMotionBuffers b{};
    float px[3] = {0.0f, 0.0f, 0.0f};
    b.prev_position = px; b.reserved0 = 1;
    CHECK(mipt_render_motion(opaque, cams.data(), 1, &o, &b, nullptr) == MIPT_ERR_INVALID_ARG && says("reserved0"));
    b.reserved0 = 0; b.reserved[4] = px;
    CHECK(mipt_render_motion(opaque, cams.data(), 1, &o, &b, nullptr) == MIPT_ERR_INVALID_ARG && says("reserved buffer pointers"));
    b.reserved[4] = nullptr; b.prev_position = nullptr;
    CHECK(mipt_render_motion(opaque, cams.data(), 1, &o, &b, nullptr) == MIPT_ERR_INVALID_ARG && says("prev_position"));
    CHECK(mipt_scene_track_motion(nullptr, 1) == MIPT_ERR_INVALID_ARG && says("null scene"));
    mipt::RendererOptions ro;
    ro.output_image_path = "unused.png"; ro.is_realtime = false; ro.backend = mipt::RendererBackend::CPU;
    auto r = mipt::Renderer::create(ro);
    CHECK(r.has_value());
    CHECK(r->render_motion(mipt::Scene(), {}, none, img) == MIPT_ERR_INVALID_ARG);   // not the MI355X arm
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
    ro.samples = 1; ro.max_ray_depth = 3; ro.output_image_dimensions = {24, 16};
    ro.output_image_path = "unused.png"; ro.is_realtime = false; ro.backend = mipt::RendererBackend::MI355X;
    ro.traversal = MIPT_TRAVERSAL_REFERENCE;
    auto r = mipt::Renderer::create(ro);
    CHECK(r.has_value());
    std::vector<MiptTriangle> prev = scene->tris;
    for (MiptTriangle &t : prev)
        for (MiptVertex &v : t.vertices) { v.position.x += 0.25f; v.position.y += -0.5f; v.position.z += 0.125f; }
    std::vector<float> img, same;
    MiptStats st{};
    CHECK(r->render_motion(*scene, {}, prev, img, MIPT_SEED_PER_SAMPLE, &st) == MIPT_OK);
    CHECK(st.pixels == 24 * 16 && st.rays == 0 && img.size() == 24 * 16 * 3);
    // the scene itself as its previous frame: the first hit's position up to rounding
    mipt::FeatureImages f;
    CHECK(r->render_features(*scene, {}, mipt::FEATURE_POSITION | mipt::FEATURE_DEPTH, f, MIPT_SEED_PER_SAMPLE) == MIPT_OK);
    CHECK(r->render_motion(*scene, {}, scene->tris, same, MIPT_SEED_PER_SAMPLE) == MIPT_OK);
    for (size_t i = 0; i < same.size(); i++) CHECK(std::fabs(same[i] - f.position[i]) <= 1e-5f);
    // a plain scene tracks nothing, and a wrong count is refused; the scene goes on
    std::vector<MiptTriangle> none, short_one(prev.begin(), prev.end() - 1);
    CHECK(r->render_motion(*scene, {}, none, same, MIPT_SEED_PER_SAMPLE) == MIPT_ERR_INVALID_ARG && says("tracks motion"));
    CHECK(r->render_motion(*scene, {}, short_one, same, MIPT_SEED_PER_SAMPLE) == MIPT_ERR_INVALID_ARG && says("n_prev_tris"));
    CHECK(r->render_motion(*scene, {}, prev, same, MIPT_SEED_PER_SAMPLE) == MIPT_OK);
    CHECK(std::memcmp(same.data(), img.data(), img.size() * sizeof(float)) == 0);
    std::FILE *out = std::fopen(out_path, "wb");
    CHECK(out);
    std::fwrite(img.data(), 4, img.size(), out);
    std::fclose(out);
    std::puts("gpu ok");
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && std::string(argv[1]) == "cpu") return run_cpu();
    if (argc >= 9 && std::string(argv[1]) == "gpu") return run_gpu(argv[2], argv[3], argv + 4);
    std::fprintf(stderr, "usage: test_host_motion cpu | gpu scene.obj out.bin x y z pitch yaw\n");
    return 2;
}
