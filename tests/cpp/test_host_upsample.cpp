// Exercises Renderer::upsample of include/mipt_host.hpp (mipt_upsample over host images).
//   test_host_upsample cpu                              argument handling without a device
//   test_host_upsample gpu in.bin out.bin W H V K       W x H is the FULL frame.  in.bin: lo_hdr, lo_normal, lo_depth, lo_albedo (f32),
//                                                       lo_material (u32) of V views of W/K x H/K, then normal, depth, albedo, material
//                                                       of V views of W x H; out.bin: the result with everything, its weight, the result
//                                                       without guides, and the result with depth and material alone and other sigmas
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
    static_assert(sizeof(MiptUpsampleOptions) == 64 && sizeof(MiptUpsampleBuffers) == 128, "ABI struct sizes");
    const uint32_t w = 6, h = 4, v = 2, k = 2;
    const size_t n = (size_t)w * h * v, n_lo = n / (k * k);
    const mipt::Renderer r = renderer(w, h);
    std::vector<float> lo_hdr(n_lo * 3, 0.5f), out, weight;
    mipt::FeatureImages none, lo, hi;
    // sizes that do not fit never reach the library
    std::vector<float> full_sized(n * 3, 0.5f);
    CHECK(r.upsample(full_sized, v, none, none, out) == MIPT_ERR_INVALID_ARG);
    lo.normal.assign(n * 3, 0.0f); hi.normal.assign(n * 3, 0.0f);
    CHECK(r.upsample(lo_hdr, v, lo, hi, out) == MIPT_ERR_INVALID_ARG);
    lo.normal.assign(n_lo * 3, 0.0f); hi.normal.assign(n_lo * 3, 0.0f);
    CHECK(r.upsample(lo_hdr, v, lo, hi, out) == MIPT_ERR_INVALID_ARG);
    hi.normal.assign(n * 3, 0.0f);
    lo.material.assign(n_lo, 1u); hi.material.assign(n + 1, 1u);
    CHECK(r.upsample(lo_hdr, v, lo, hi, out) == MIPT_ERR_INVALID_ARG);
    hi.material.assign(n, 1u);
    lo.depth.assign(n_lo, 1.0f); hi.depth.assign(n, 1.0f); lo.albedo.assign(n_lo * 3, 1.0f); hi.albedo.assign(n * 3, 1.0f);
    // what the library checks, with its message
    mipt::FeatureImages partial = hi;
    partial.depth.clear();
    CHECK(r.upsample(lo_hdr, v, lo, partial, out) == MIPT_ERR_INVALID_ARG && says("null depth"));
    partial = lo;
    partial.material.clear();
    CHECK(r.upsample(lo_hdr, v, partial, hi, out) == MIPT_ERR_INVALID_ARG && says("null lo_material"));
    mipt::UpsampleSettings s;
    s.scale = 1;
    CHECK(r.upsample(lo_hdr, v, lo, hi, out, s) == MIPT_ERR_INVALID_ARG && says("scale"));
    s.scale = 9;
    CHECK(r.upsample(lo_hdr, v, lo, hi, out, s) == MIPT_ERR_INVALID_ARG && says("scale"));
    s.scale = 4;
    CHECK(r.upsample(lo_hdr, v, lo, hi, out, s) == MIPT_ERR_INVALID_ARG && says("width 6 is not a multiple of scale 4"));
    s = mipt::UpsampleSettings();
    s.sigma_normal = -1.0f;
    CHECK(r.upsample(lo_hdr, v, lo, hi, out, s) == MIPT_ERR_INVALID_ARG && says("sigma_normal"));
    CHECK(r.upsample(lo_hdr, v, none, none, out, s) != MIPT_ERR_INVALID_ARG);        // a sigma given for an absent guide is ignored
    s = mipt::UpsampleSettings();
    s.sigma_depth = 1e-25f;
    CHECK(r.upsample(lo_hdr, v, lo, hi, out, s) == MIPT_ERR_INVALID_ARG && says("sigma_depth"));
    CHECK(r.upsample(lo_hdr, 0, none, none, out) == MIPT_ERR_INVALID_ARG && says("n_views"));
    CHECK(renderer(1u << 16, 1u << 16).upsample(lo_hdr, 1, none, none, out) == MIPT_ERR_INVALID_ARG && says("below 2^32"));
    // well-formed calls: results of the right size on a GPU, MIPT_ERR_HIP without one -- never a CPU filter
    s = mipt::UpsampleSettings();
    CHECK(s.scale == 2 && s.sigma_normal == 0.5f && s.sigma_depth == 0.5f);
    const int rc = r.upsample(lo_hdr, v, lo, hi, out, s, &weight);
    CHECK(rc == MIPT_OK || rc == MIPT_ERR_HIP);
    CHECK(out.size() == n * 3 && weight.size() == n);
    CHECK(r.upsample(lo_hdr, v, none, none, out) == rc);
    CHECK(mipt_upsample_workspace_bytes(w, h, v, k) == n_lo * 32 && mipt_upsample_workspace_bytes(w, h, v, 4) == 0 && mipt_upsample_workspace_bytes(0, h, v, k) == 0);
    std::puts(rc == MIPT_OK ? "cpu ok (device present)" : "cpu ok");
    return 0;
}

template <class T> static bool read_plane(std::FILE *f, std::vector<T> &v, size_t count) {
    v.resize(count);
    return std::fread(v.data(), 4, count, f) == count;
}

static int run_gpu(const char *in_path, const char *out_path, uint32_t w, uint32_t h, uint32_t v, uint32_t k) {
    const size_t n = (size_t)w * h * v, n_lo = n / ((size_t)k * k);
    std::vector<float> lo_hdr;
    mipt::FeatureImages none, lo, hi;
    {
        std::FILE *f = std::fopen(in_path, "rb");
        CHECK(f);
        CHECK(read_plane(f, lo_hdr, n_lo * 3) && read_plane(f, lo.normal, n_lo * 3) && read_plane(f, lo.depth, n_lo) && read_plane(f, lo.albedo, n_lo * 3) &&
              read_plane(f, lo.material, n_lo));
        CHECK(read_plane(f, hi.normal, n * 3) && read_plane(f, hi.depth, n) && read_plane(f, hi.albedo, n * 3) && read_plane(f, hi.material, n));
        std::fclose(f);
    }
    const mipt::Renderer r = renderer(w, h);
    std::FILE *out = std::fopen(out_path, "wb");
    CHECK(out);
    std::vector<float> res, weight;
    mipt::UpsampleSettings s;
    s.scale = k;
    CHECK(r.upsample(lo_hdr, v, lo, hi, res, s, &weight) == MIPT_OK && res.size() == n * 3 && weight.size() == n);
    std::fwrite(res.data(), 4, res.size(), out);
    std::fwrite(weight.data(), 4, weight.size(), out);
    CHECK(r.upsample(lo_hdr, v, none, none, res, s) == MIPT_OK);             // plain bilinear
    std::fwrite(res.data(), 4, res.size(), out);
    mipt::FeatureImages lo2, hi2;
    lo2.depth = lo.depth; lo2.material = lo.material; hi2.depth = hi.depth; hi2.material = hi.material;
    s.sigma_depth = 0.25f; s.sigma_normal = -1.0f;                           // ignored: no normal
    CHECK(r.upsample(lo_hdr, v, lo2, hi2, res, s) == MIPT_OK);
    std::fwrite(res.data(), 4, res.size(), out);
    std::fclose(out);
    std::puts("gpu ok");
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && std::string(argv[1]) == "cpu") return run_cpu();
    if (argc >= 8 && std::string(argv[1]) == "gpu")
        return run_gpu(argv[2], argv[3], (uint32_t)std::atoi(argv[4]), (uint32_t)std::atoi(argv[5]), (uint32_t)std::atoi(argv[6]), (uint32_t)std::atoi(argv[7]));
    std::fprintf(stderr, "usage: test_host_upsample cpu | gpu in.bin out.bin W H V K\n");
    return 2;
}
