// Exercises the probe methods of include/mipt_host.hpp (bake_probes_on, Scene::bake_probes, mipt::probe_grid, mipt::probe_irradiance)
// against the C entries they wrap.
//   test_host_probe cpu                   argument handling without a device
//   test_host_probe gpu scene.obj out.bin Scene::bake_probes on a 2 x 2 x 2 grid (4 samples, depth 4, stride 8), probe_irradiance at
//                                         10 points with and without a valid plane; each is compared here with a direct call of its C
//                                         entry, and out.bin receives the probes (8 x 16 B), the coefficients (8 x 27 f32), then
//                                         position, normal, irradiance, irradiance with the valid plane (10 x 3 f32 each) for the models
#include "mipt_host.hpp"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "CHECK failed at line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static bool says(const char *what) { return std::string(mipt_last_error()).find(what) != std::string::npos; }

static MiptProbeGrid make_grid() {
    MiptProbeGrid g{};
    g.origin[0] = g.origin[1] = g.origin[2] = -0.5f;
    g.spacing[0] = g.spacing[1] = g.spacing[2] = 1.0f;
    g.dims[0] = g.dims[1] = g.dims[2] = 2;
    return g;
}

static int run_cpu() {
    MiptScene *opaque = reinterpret_cast<MiptScene *>(0x1000);           // never dereferenced by the checks below
    std::vector<MiptProbe> none, probes(6);
    std::vector<float> sh(5, 1.0f);
    MiptProbeBakeOptions opt{};
    opt.samples = 2; opt.max_ray_depth = 4; opt.sample_stride = 6;
    CHECK(mipt::bake_probes_on(opaque, none, sh, opt) == MIPT_OK && sh.empty());
    CHECK(mipt::bake_probes_on(nullptr, probes, sh, opt) == MIPT_ERR_INVALID_ARG && sh.size() == 6 * 27 && says("mipt_probe_bake: null scene, probes, options or sh"));
    opt.sample_stride = 0;
    CHECK(mipt::bake_probes_on(opaque, probes, sh, opt) == MIPT_ERR_INVALID_ARG && says("sample_stride must be > 0"));
    opt.sample_stride = 6; opt.flags = MIPT_FLAG_SUM | MIPT_FLAG_ACCUM;
    CHECK(mipt::bake_probes_on(opaque, probes, sh, opt) == MIPT_ERR_INVALID_ARG && says("use mipt_probe_bake_device"));

    const MiptProbeGrid g = make_grid();
    const std::vector<MiptProbe> grid = mipt::probe_grid(g);
    CHECK(grid.size() == 8 && grid[0].x == -0.5f && grid[1].x == 0.5f && grid[1].y == -0.5f && grid[2].y == 0.5f && grid[4].z == 0.5f && grid[7].seed == 7u);
    const int no_device = 1 << 20;
    std::vector<float> coeff(8 * 27, 0.25f), position(6 * 3, 0.0f), normal(6 * 3, 1.0f), irradiance, wrong(7), empty;
    std::vector<uint8_t> valid(8, 1), short_valid(5, 1);
    CHECK(mipt::probe_irradiance(g, wrong, position, normal, irradiance) == MIPT_ERR_INVALID_ARG);          // refused by the wrapper
    CHECK(mipt::probe_irradiance(g, coeff, wrong, wrong, irradiance) == MIPT_ERR_INVALID_ARG);
    CHECK(mipt::probe_irradiance(g, coeff, position, wrong, irradiance) == MIPT_ERR_INVALID_ARG);
    CHECK(mipt::probe_irradiance(g, coeff, position, normal, irradiance, short_valid) == MIPT_ERR_INVALID_ARG);
    CHECK(mipt::probe_irradiance(g, coeff, empty, empty, irradiance, valid, no_device) == MIPT_OK && irradiance.empty());     // no points: no device either
    CHECK(mipt::probe_irradiance(g, coeff, position, normal, irradiance, valid, no_device) == MIPT_ERR_HIP && says("hipSetDevice") && irradiance.size() == 18);
    MiptProbeGrid bad = g;
    bad.spacing[1] = 0.0f;
    CHECK(mipt::probe_irradiance(bad, coeff, position, normal, irradiance, {}, no_device) == MIPT_ERR_INVALID_ARG && says("spacing[1] must be finite and greater than 0"));
    bad = g;
    bad.flags = 2u;
    CHECK(mipt::probe_irradiance(bad, coeff, position, normal, irradiance, {}, no_device) == MIPT_ERR_INVALID_ARG && says("only MIPT_PROBE_CLAMP is accepted"));
    std::puts("cpu ok");
    return 0;
}

template <class T> static bool same(const std::vector<T> &a, const std::vector<T> &b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0;
}

static int run_gpu(const char *obj, const char *out_path) {
    auto scene = mipt::Scene::load(obj);
    CHECK(scene.has_value());
    const MiptProbeGrid g = make_grid();
    const std::vector<MiptProbe> probes = mipt::probe_grid(g);
    const size_t n_probes = probes.size(), n = 10;
    MiptProbeBakeOptions opt{};
    opt.samples = 4; opt.max_ray_depth = 4; opt.sample_stride = (uint32_t)n_probes;
    std::vector<float> sh, position, normal, irradiance, masked;
    MiptStats stats{};
    CHECK(scene->bake_probes(probes, sh, opt, &stats) == MIPT_OK && sh.size() == n_probes * 27 && stats.pixels == n_probes * 4);
    for (size_t i = 0; i < n; i++) {
        const float t = (float)i;
        position.insert(position.end(), {-0.625f + 0.125f * t, 0.0625f * t - 0.25f, 0.375f - 0.0625f * t});
        normal.insert(normal.end(), {i % 3 == 0 ? 1.0f : 0.0f, i % 3 == 1 ? -1.0f : 0.0f, i % 3 == 2 ? 1.0f : 0.25f});
    }
    std::vector<uint8_t> valid(n_probes, 1);
    valid[0] = valid[3] = valid[6] = 0;
    MiptProbeGrid clamped = g;
    clamped.flags = MIPT_PROBE_CLAMP;
    CHECK(mipt::probe_irradiance(g, sh, position, normal, irradiance) == MIPT_OK && irradiance.size() == n * 3);
    CHECK(mipt::probe_irradiance(clamped, sh, position, normal, masked, valid) == MIPT_OK && masked.size() == n * 3);
    // the C entries, on a scene made of the same arrays
    std::vector<MiptMaterial> mats;
    for (const auto &kv : scene->materials) mats.push_back(kv.second);
    std::vector<MiptTexture> texs;
    for (const mipt::Texture &t : scene->textures) texs.push_back({t.width, t.height, t.pixel_data.data()});
    MiptSceneDesc d{scene->tris.data(), (uint32_t)scene->tris.size(), scene->bvh_nodes.data(), (uint32_t)scene->bvh_nodes.size(),
                    mats.data(), (uint32_t)mats.size(), texs.data(), (uint32_t)texs.size()};
    MiptScene *raw = nullptr;
    CHECK(mipt_scene_create(&d, 0, &raw) == MIPT_OK);
    std::vector<float> sh2(n_probes * 27), irradiance2(n * 3), masked2(n * 3);
    CHECK(mipt_probe_bake(raw, probes.data(), n_probes, &opt, sh2.data(), nullptr) == MIPT_OK && same(sh, sh2));
    mipt_scene_destroy(raw);
    MiptProbeIrradianceBuffers b{};
    b.sh = sh.data(); b.position = position.data(); b.normal = normal.data(); b.irradiance = irradiance2.data();
    CHECK(mipt_probe_irradiance(&g, n, &b, 0) == MIPT_OK && same(irradiance, irradiance2));
    b.valid = valid.data(); b.irradiance = masked2.data();
    CHECK(mipt_probe_irradiance(&clamped, n, &b, 0) == MIPT_OK && same(masked, masked2));
    std::FILE *out = std::fopen(out_path, "wb");
    CHECK(out);
    std::fwrite(probes.data(), sizeof(MiptProbe), n_probes, out);
    std::fwrite(sh.data(), sizeof(float), sh.size(), out);
    for (const std::vector<float> *v : {&position, &normal, &irradiance, &masked}) std::fwrite(v->data(), sizeof(float), n * 3, out);
    std::fclose(out);
    std::puts("gpu ok");
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && std::string(argv[1]) == "cpu") return run_cpu();
    if (argc >= 4 && std::string(argv[1]) == "gpu") return run_gpu(argv[2], argv[3]);
    std::fprintf(stderr, "usage: test_host_probe cpu | gpu scene.obj out.bin\n");
    return 2;
}
