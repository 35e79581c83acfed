// Exercises Renderer::render_adaptive and Renderer::sample_map of include/mipt_host.hpp (mipt_render_adaptive / mipt_sample_map over
// host images).
//   test_host_adaptive cpu                          argument handling without a device
//   test_host_adaptive gpu in.bin out.bin W H V     in.bin: variance (1 f32), hdr, albedo (3 f32 each) of V views of W x H;
//                                                   out.bin: the counts with everything, with hdr alone, and with variance alone
#include "mipt_host.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "CHECK failed at line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static bool says(const char *what) { return std::string(mipt_last_error()).find(what) != std::string::npos; }

static mipt::Renderer renderer(size_t w, size_t h, size_t samples = 8) {
    mipt::RendererOptions o;
    o.output_image_dimensions = {w, h};
    o.output_image_path = "unused.png";
    o.backend = mipt::RendererBackend::MI355X;
    o.is_realtime = false;
    o.samples = samples;
    return *mipt::Renderer::create(o);
}

static int run_cpu() {
    static_assert(sizeof(MiptSampleMapOptions) == 64 && sizeof(MiptSampleMapBuffers) == 64, "ABI struct sizes");
    const uint32_t w = 6, h = 4, v = 2;
    const size_t n = (size_t)w * h * v;
    const mipt::Renderer r = renderer(w, h);
    std::vector<float> variance(n, 0.25f), hdr(n * 3, 0.5f), albedo(n * 3, 0.5f), none;
    std::vector<uint32_t> counts;
    // sizes that do not fit never reach the library
    std::vector<float> short_plane(n - 1, 0.25f);
    CHECK(r.sample_map(short_plane, v, none, none, counts) == MIPT_ERR_INVALID_ARG);
    CHECK(r.sample_map(none, v, none, none, counts) == MIPT_ERR_INVALID_ARG);
    CHECK(r.sample_map(variance, v, variance, none, counts) == MIPT_ERR_INVALID_ARG);
    CHECK(r.sample_map(variance, v, hdr, variance, counts) == MIPT_ERR_INVALID_ARG);
    // what the library checks, with its message
    CHECK(r.sample_map(variance, v, none, albedo, counts) == MIPT_ERR_INVALID_ARG && says("albedo is given only with hdr"));
    mipt::SampleMapSettings s;
    CHECK(s.min_samples == 1 && s.max_samples == 0 && s.budget < 0.0f);
    s.max_samples = 70000;
    CHECK(r.sample_map(variance, v, hdr, albedo, counts, s) == MIPT_ERR_INVALID_ARG && says("max_samples 70000"));
    s = mipt::SampleMapSettings();
    s.min_samples = 9;                                                       // above options.samples = 8, the default max
    CHECK(r.sample_map(variance, v, hdr, albedo, counts, s) == MIPT_ERR_INVALID_ARG && says("min_samples 9"));
    s = mipt::SampleMapSettings();
    s.budget = 8.5f;
    CHECK(r.sample_map(variance, v, hdr, albedo, counts, s) == MIPT_ERR_INVALID_ARG && says("budget"));
    s.budget = 0.5f;
    CHECK(r.sample_map(variance, v, hdr, albedo, counts, s) == MIPT_ERR_INVALID_ARG && says("budget"));
    CHECK(r.sample_map(variance, 0, none, none, counts) == MIPT_ERR_INVALID_ARG && says("n_views"));
    CHECK(renderer(1u << 16, 1u << 16).sample_map(variance, 1, none, none, counts) == MIPT_ERR_INVALID_ARG && says("below 2^32"));
    // well-formed calls: counts of the right size on a GPU, MIPT_ERR_HIP without one -- never a CPU map
    s = mipt::SampleMapSettings();
    s.budget = 2.0f;
    const int rc = r.sample_map(variance, v, hdr, albedo, counts, s);
    CHECK(rc == MIPT_OK || rc == MIPT_ERR_HIP);
    CHECK(counts.size() == n);
    CHECK(r.sample_map(variance, v, none, none, counts) == rc);
    CHECK(mipt_sample_map_workspace_bytes(w, h, v) == 32 && mipt_sample_map_workspace_bytes(0, h, v) == 0 &&
          mipt_sample_map_workspace_bytes(1u << 16, 1u << 16, 1) == 0);
    // render_adaptive: a count plane of the wrong size never reaches the library, and nothing is uploaded for it
    mipt::Scene scene;
    std::vector<float> frame;
    std::vector<uint32_t> wrong(n + 1, 1u);
    std::vector<MiptCamera> cams(v);
    CHECK(r.render_adaptive(scene, cams, wrong, frame) == MIPT_ERR_INVALID_ARG);
    wrong.assign(1, 1u);
    CHECK(r.render_adaptive(scene, cams, wrong, frame) == MIPT_ERR_INVALID_ARG);
    std::puts(rc == MIPT_OK ? "cpu ok (device present)" : "cpu ok");
    return 0;
}

static bool read_plane(std::FILE *f, std::vector<float> &v, size_t count) {
    v.resize(count);
    return std::fread(v.data(), 4, count, f) == count;
}

static int run_gpu(const char *in_path, const char *out_path, uint32_t w, uint32_t h, uint32_t v) {
    const size_t n = (size_t)w * h * v;
    std::vector<float> variance, hdr, albedo, none;
    {
        std::FILE *f = std::fopen(in_path, "rb");
        CHECK(f);
        CHECK(read_plane(f, variance, n) && read_plane(f, hdr, n * 3) && read_plane(f, albedo, n * 3));
        std::fclose(f);
    }
    const mipt::Renderer r = renderer(w, h);
    std::FILE *out = std::fopen(out_path, "wb");
    CHECK(out);
    std::vector<uint32_t> counts;
    mipt::SampleMapSettings s;
    s.budget = 2.0f;                                                         // min 1, max = options.samples = 8
    CHECK(r.sample_map(variance, v, hdr, albedo, counts, s) == MIPT_OK && counts.size() == n);
    std::fwrite(counts.data(), 4, counts.size(), out);
    s.min_samples = 0; s.max_samples = 16; s.budget = 1.5f;
    CHECK(r.sample_map(variance, v, hdr, none, counts, s) == MIPT_OK && counts.size() == n);
    std::fwrite(counts.data(), 4, counts.size(), out);
    CHECK(r.sample_map(variance, v, none, none, counts, s) == MIPT_OK && counts.size() == n);
    std::fwrite(counts.data(), 4, counts.size(), out);
    std::fclose(out);
    std::puts("gpu ok");
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && std::string(argv[1]) == "cpu") return run_cpu();
    if (argc >= 7 && std::string(argv[1]) == "gpu")
        return run_gpu(argv[2], argv[3], (uint32_t)std::atoi(argv[4]), (uint32_t)std::atoi(argv[5]), (uint32_t)std::atoi(argv[6]));
    std::fprintf(stderr, "usage: test_host_adaptive cpu | gpu in.bin out.bin W H V\n");
    return 2;
}
