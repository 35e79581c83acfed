// Exercises the radiance-query methods of include/mipt_host.hpp (query_radiance_on, Scene::query_radiance, Renderer::query_radiance).
//   test_host_radiance cpu                              argument handling without a device
//   test_host_radiance gpu scene.obj rays.bin out.bin   rays.bin: n x MiptRay (the last word the seed); out.bin: n x 3 f32 of
//                                                       Scene::query_radiance (3 samples, depth 6, mean), then of Renderer's form (sum)
#include "mipt_host.hpp"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "CHECK failed at line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static int run_cpu() {
    MiptScene *opaque = reinterpret_cast<MiptScene *>(0x1000);           // never dereferenced by the checks below
    std::vector<MiptRay> none;
    std::vector<float> radiance(7, 1.0f);
    MiptRadianceOptions opt{};
    opt.samples = 2; opt.max_ray_depth = 4;
    MiptStats st;
    std::memset(&st, 0xff, sizeof st);
    CHECK(mipt::query_radiance_on(opaque, none, radiance, opt, &st) == MIPT_OK && radiance.empty() && st.rays == 0);
    std::vector<MiptRay> two(2);
    MiptRadianceOptions bad = opt;
    bad.traversal = 7;
    CHECK(mipt::query_radiance_on(opaque, two, radiance, bad) == MIPT_ERR_INVALID_ARG && radiance.size() == 6);
    CHECK(std::string(mipt_last_error()).find("unknown traversal") != std::string::npos);
    bad = opt; bad.samples = 0;
    CHECK(mipt::query_radiance_on(opaque, two, radiance, bad) == MIPT_ERR_INVALID_ARG);
    bad = opt; bad.flags = MIPT_FLAG_SUM | MIPT_FLAG_ACCUM;                 // a running sum lives in device memory
    CHECK(mipt::query_radiance_on(opaque, two, radiance, bad) == MIPT_ERR_INVALID_ARG);
    CHECK(std::string(mipt_last_error()).find("mipt_query_radiance_device") != std::string::npos);
    CHECK(mipt::query_radiance_on(nullptr, two, radiance, opt) == MIPT_ERR_INVALID_ARG && radiance.size() == 6);
    std::puts("cpu ok");
    return 0;
}

static int run_gpu(const char *obj, const char *rays_path, const char *out_path) {
    auto scene = mipt::Scene::load(obj);
    CHECK(scene.has_value());
    std::vector<MiptRay> rays;
    {
        std::FILE *f = std::fopen(rays_path, "rb");
        CHECK(f);
        MiptRay r;
        while (std::fread(&r, sizeof r, 1, f) == 1) rays.push_back(r);
        std::fclose(f);
    }
    CHECK(!rays.empty());
    std::FILE *out = std::fopen(out_path, "wb");
    CHECK(out);
    MiptRadianceOptions opt{};
    opt.samples = 3; opt.max_ray_depth = 6; opt.flags = MIPT_FLAG_COUNT;
    std::vector<float> radiance;
    MiptStats st{};
    CHECK(scene->query_radiance(rays, radiance, opt, &st) == MIPT_OK && radiance.size() == rays.size() * 3);
    CHECK(st.pixels == rays.size() && st.rays >= rays.size() * 3);
    std::fwrite(radiance.data(), sizeof(float), radiance.size(), out);
    mipt::RendererOptions ro;
    ro.samples = 3; ro.max_ray_depth = 6;
    ro.backend = mipt::RendererBackend::MI355X; ro.is_realtime = false;
    ro.traversal = MIPT_TRAVERSAL_REFERENCE;                              // the traversal the one-ray oracle models at any margin
    ro.output_image_path = std::string("/dev/null");
    auto renderer = mipt::Renderer::create(ro);
    CHECK(renderer.has_value());
    radiance.clear();
    CHECK(renderer->query_radiance(*scene, rays, radiance, MIPT_FLAG_SUM) == MIPT_OK && radiance.size() == rays.size() * 3);
    std::fwrite(radiance.data(), sizeof(float), radiance.size(), out);
    std::fclose(out);
    std::puts("gpu ok");
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && std::string(argv[1]) == "cpu") return run_cpu();
    if (argc >= 5 && std::string(argv[1]) == "gpu") return run_gpu(argv[2], argv[3], argv[4]);
    std::fprintf(stderr, "usage: test_host_radiance cpu | gpu scene.obj rays.bin out.bin\n");
    return 2;
}
