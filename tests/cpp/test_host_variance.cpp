// Exercises Renderer::denoise_variance of include/mipt_host.hpp (mipt_denoise_variance over host images).
//   test_host_variance cpu                              argument handling without a device
//   test_host_variance gpu in.bin out.bin W H V         in.bin: hdr, normal, depth, albedo, variance, length planes of V views of W x H
//                                                       (f32); out.bin: the result with everything, its variance_out, the result
//                                                       without history, the result with depth alone and other settings, and in place
#include "mipt_host.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "CHECK failed at line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static bool says(const char *what) { return std::string(mipt_last_error()).find(what) != std::string::npos; }

static mipt::Renderer renderer(size_t w, size_t h) {
    mipt::RendererOptions o;
    o.output_image_dimensions = {w, h};
    o.output_image_path = "unused.png";
    o.backend = mipt::RendererBackend::MI355X;
    o.is_realtime = false;
    return *mipt::Renderer::create(o);
}

static int run_cpu() {
    static_assert(sizeof(MiptVarianceOptions) == 64 && sizeof(MiptVarianceBuffers) == 128, "ABI struct sizes");
    const uint32_t w = 6, h = 4, v = 2;
    const size_t n = (size_t)w * h * v;
    const mipt::Renderer r = renderer(w, h);
    std::vector<float> hdr(n * 3, 0.5f), var(n, 0.1f), len(n, 3.0f), out, vout;
    const std::vector<float> absent;
    mipt::FeatureImages none, g;
    // sizes that do not fit never reach the library
    std::vector<float> shorter(n * 3 - 1, 0.5f);
    CHECK(r.denoise_variance(shorter, v, var, len, none, out) == MIPT_ERR_INVALID_ARG);
    CHECK(r.denoise_variance(hdr, v, shorter, len, none, out) == MIPT_ERR_INVALID_ARG);
    CHECK(r.denoise_variance(hdr, v, var, hdr, none, out) == MIPT_ERR_INVALID_ARG);
    g.normal.assign(n * 3, 0.0f); g.depth.assign(n * 3, 1.0f);
    CHECK(r.denoise_variance(hdr, v, var, len, g, out) == MIPT_ERR_INVALID_ARG);
    g.depth.assign(n, 1.0f); g.albedo.assign(n * 3 + 3, 1.0f);
    CHECK(r.denoise_variance(hdr, v, var, len, g, out) == MIPT_ERR_INVALID_ARG);
    g.albedo.assign(n * 3, 1.0f);
    // what the library checks, with its message
    CHECK(r.denoise_variance(hdr, v, var, absent, g, out) == MIPT_ERR_INVALID_ARG && says("null length"));
    CHECK(r.denoise_variance(hdr, v, absent, len, g, out) == MIPT_ERR_INVALID_ARG && says("null variance"));
    mipt::VarianceSettings s;
    s.iterations = 0;
    CHECK(r.denoise_variance(hdr, v, var, len, g, out, s) == MIPT_ERR_INVALID_ARG && says("iterations"));
    s.iterations = 9;
    CHECK(r.denoise_variance(hdr, v, var, len, g, out, s) == MIPT_ERR_INVALID_ARG && says("iterations"));
    s = mipt::VarianceSettings();
    s.sigma_luminance = 0.0f;
    CHECK(r.denoise_variance(hdr, v, var, len, g, out, s) == MIPT_ERR_INVALID_ARG && says("sigma_luminance"));
    s = mipt::VarianceSettings();
    s.short_history = -1.0f;
    CHECK(r.denoise_variance(hdr, v, var, len, g, out, s) == MIPT_ERR_INVALID_ARG && says("short_history"));
    s = mipt::VarianceSettings();
    s.sigma_normal = -1.0f;
    CHECK(r.denoise_variance(hdr, v, var, len, g, out, s) == MIPT_ERR_INVALID_ARG && says("sigma_normal"));
    CHECK(r.denoise_variance(hdr, v, var, len, none, out, s) != MIPT_ERR_INVALID_ARG);      // a sigma given for an absent guide is ignored
    s = mipt::VarianceSettings();
    s.sigma_depth = 1e-25f;
    CHECK(r.denoise_variance(hdr, v, var, len, g, out, s) == MIPT_ERR_INVALID_ARG && says("sigma_depth"));
    CHECK(r.denoise_variance(hdr, 0, var, len, none, out) == MIPT_ERR_INVALID_ARG && says("n_views"));
    CHECK(renderer(1u << 16, 1u << 16).denoise_variance(hdr, 1, absent, absent, none, out) == MIPT_ERR_INVALID_ARG && says("below 2^32"));
    // well-formed calls: results of the right size on a GPU, MIPT_ERR_HIP without one -- never a CPU filter
    s = mipt::VarianceSettings();
    CHECK(s.iterations == 5 && s.sigma_luminance == 16.0f && s.short_history == 4.0f);
    const int rc = r.denoise_variance(hdr, v, var, len, g, out, s, &vout);
    CHECK(rc == MIPT_OK || rc == MIPT_ERR_HIP);
    CHECK(out.size() == n * 3 && vout.size() == n);
    CHECK(r.denoise_variance(hdr, v, absent, absent, none, out) == rc);
    CHECK(mipt_denoise_variance_workspace_bytes(w, h, v) == n * 48 && mipt_denoise_variance_workspace_bytes(0, h, v) == 0);
    std::puts(rc == MIPT_OK ? "cpu ok (device present)" : "cpu ok");
    return 0;
}

static int run_gpu(const char *in_path, const char *out_path, uint32_t w, uint32_t h, uint32_t v) {
    const size_t n = (size_t)w * h * v;
    std::vector<float> hdr(n * 3), var(n), len(n);
    const std::vector<float> absent;
    mipt::FeatureImages g;
    g.normal.resize(n * 3); g.depth.resize(n); g.albedo.resize(n * 3);
    {
        std::FILE *f = std::fopen(in_path, "rb");
        CHECK(f);
        CHECK(std::fread(hdr.data(), 4, hdr.size(), f) == hdr.size() && std::fread(g.normal.data(), 4, g.normal.size(), f) == g.normal.size());
        CHECK(std::fread(g.depth.data(), 4, g.depth.size(), f) == g.depth.size() && std::fread(g.albedo.data(), 4, g.albedo.size(), f) == g.albedo.size());
        CHECK(std::fread(var.data(), 4, var.size(), f) == var.size() && std::fread(len.data(), 4, len.size(), f) == len.size());
        std::fclose(f);
    }
    const mipt::Renderer r = renderer(w, h);
    std::FILE *out = std::fopen(out_path, "wb");
    CHECK(out);
    std::vector<float> res, vout;
    CHECK(r.denoise_variance(hdr, v, var, len, g, res, mipt::VarianceSettings(), &vout) == MIPT_OK && res.size() == n * 3 && vout.size() == n);
    std::fwrite(res.data(), 4, res.size(), out);
    std::fwrite(vout.data(), 4, vout.size(), out);
    CHECK(r.denoise_variance(hdr, v, absent, absent, g, res) == MIPT_OK);    // a single frame without history
    std::fwrite(res.data(), 4, res.size(), out);
    mipt::FeatureImages depth_only;
    depth_only.depth = g.depth;
    mipt::VarianceSettings s;
    s.iterations = 3; s.sigma_depth = 0.25f; s.sigma_luminance = 4.0f; s.short_history = 0.0f;
    CHECK(r.denoise_variance(hdr, v, var, len, depth_only, res, s) == MIPT_OK);
    std::fwrite(res.data(), 4, res.size(), out);
    CHECK(r.denoise_variance(hdr, v, var, len, g, hdr) == MIPT_OK && hdr.size() == n * 3);     // in place
    std::fwrite(hdr.data(), 4, hdr.size(), out);
    std::fclose(out);
    std::puts("gpu ok");
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && std::string(argv[1]) == "cpu") return run_cpu();
    if (argc >= 7 && std::string(argv[1]) == "gpu")
        return run_gpu(argv[2], argv[3], (uint32_t)std::atoi(argv[4]), (uint32_t)std::atoi(argv[5]), (uint32_t)std::atoi(argv[6]));
    std::fprintf(stderr, "usage: test_host_variance cpu | gpu in.bin out.bin W H V\n");
    return 2;
}
