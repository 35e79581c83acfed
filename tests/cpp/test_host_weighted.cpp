// Exercises the count-aware Renderer::temporal overload and SampleMapSettings::rounds of include/mipt_host.hpp (mipt_temporal_counts /
// mipt_sample_map_fill over host images).
//   test_host_weighted cpu                              argument handling without a device
//   test_host_weighted gpu in.bin out.bin W H V         in.bin: V cameras (80 B each), then for each of two frames the hdr, position,
//                                                       normal, depth, material, albedo and counts planes of V views of W x H, then
//                                                       a variance plane;
//                                                       out.bin: per temporal call out, history, length, variance -- the first
//                                                       frame, the second from its history -- then the counts of the map over the
//                                                       variance plane with rounds = 0, 1 and 4
#include "mipt_host.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "CHECK failed at line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static bool says(const char *what) { return std::string(mipt_last_error()).find(what) != std::string::npos; }

static mipt::Renderer renderer(size_t w, size_t h, size_t samples = 5) {
    mipt::RendererOptions o;
    o.output_image_dimensions = {w, h};
    o.output_image_path = "unused.png";
    o.backend = mipt::RendererBackend::MI355X;
    o.is_realtime = false;
    o.samples = samples;
    return *mipt::Renderer::create(o);
}

static MiptCamera camera(float x) {
    MiptCamera c{};
    const float position[3] = {x, 1.0f, -2.0f};
    mipt_camera_from_pose(position, 3.0f, 20.0f + x, &c);
    return c;
}

static int run_cpu() {
    static_assert(sizeof(MiptSampleMapFillOptions) == 64, "ABI struct size");
    const uint32_t w = 6, h = 4, v = 2;
    const size_t n = (size_t)w * h * v;
    const mipt::Renderer r = renderer(w, h);
    std::vector<MiptCamera> cams = {camera(0.0f), camera(0.5f)};
    std::vector<float> hdr(n * 3, 0.5f), out;
    mipt::FeatureImages g;
    g.position.assign(n * 3, 1.0f); g.normal.assign(n * 3, 0.0f); g.depth.assign(n, 2.0f); g.material.assign(n, 1u);
    mipt::TemporalState st;
    std::vector<uint32_t> counts(n, 2u);
    // a count plane of the wrong size never reaches the library
    CHECK(r.temporal(hdr, cams, g, st, out, std::vector<uint32_t>(n - 1, 1u)) == MIPT_ERR_INVALID_ARG);
    CHECK(r.temporal(hdr, cams, g, st, out, std::vector<uint32_t>()) == MIPT_ERR_INVALID_ARG);
    // what the library checks, with its message
    CHECK(r.temporal(hdr, cams, g, st, out, counts, 70000) == MIPT_ERR_INVALID_ARG && says("samples_cap 70000"));
    mipt::TemporalSettings s;
    s.max_history = 0.5f;
    CHECK(r.temporal(hdr, cams, g, st, out, counts, 0, s) == MIPT_ERR_INVALID_ARG && says("max_history") && says("mipt_temporal_counts"));
    // a well-formed call: the result of the right size on a GPU, MIPT_ERR_HIP without one -- never a CPU blend
    s = mipt::TemporalSettings(); s.want_length = true;
    const int rc = r.temporal(hdr, cams, g, st, out, counts, 0, s);          // the cap: options.samples
    CHECK(rc == MIPT_OK || rc == MIPT_ERR_HIP);
    CHECK(out.size() == n * 3 && st.length.size() == n);
    CHECK(rc == MIPT_OK ? st.history.size() == 16 * v + 12 * n : st.history.empty());
    // the map's rounds
    std::vector<float> variance(n, 0.25f), none;
    mipt::SampleMapSettings m;
    CHECK(m.rounds == 0);
    m.budget = 2.0f; m.rounds = 9;
    CHECK(r.sample_map(variance, v, none, none, counts, m) == MIPT_ERR_INVALID_ARG && says("rounds 9") && says("mipt_sample_map_fill"));
    m.rounds = 2; m.budget = 9.0f;
    CHECK(r.sample_map(variance, v, none, none, counts, m) == MIPT_ERR_INVALID_ARG && says("budget"));
    m.budget = 2.0f;
    CHECK(r.sample_map(variance, v, none, none, counts, m) == rc && counts.size() == n);
    CHECK(mipt_sample_map_fill_workspace_bytes(w, h, v, 3) == 96 && mipt_sample_map_fill_workspace_bytes(w, h, v, 0) == 0 &&
          mipt_sample_map_fill_workspace_bytes(0, h, v, 3) == 0);
    std::puts(rc == MIPT_OK ? "cpu ok (device present)" : "cpu ok");
    return 0;
}

static bool read_frame(std::FILE *f, size_t n, std::vector<float> &hdr, mipt::FeatureImages &g, std::vector<uint32_t> &counts) {
    hdr.resize(n * 3); g.position.resize(n * 3); g.normal.resize(n * 3); g.depth.resize(n); g.material.resize(n); g.albedo.resize(n * 3);
    counts.resize(n);
    return std::fread(hdr.data(), 4, n * 3, f) == n * 3 && std::fread(g.position.data(), 4, n * 3, f) == n * 3 &&
           std::fread(g.normal.data(), 4, n * 3, f) == n * 3 && std::fread(g.depth.data(), 4, n, f) == n &&
           std::fread(g.material.data(), 4, n, f) == n && std::fread(g.albedo.data(), 4, n * 3, f) == n * 3 &&
           std::fread(counts.data(), 4, n, f) == n;
}

static void write_call(std::FILE *f, const std::vector<float> &out, const mipt::TemporalState &st) {
    std::fwrite(out.data(), 4, out.size(), f);
    std::fwrite(st.history.data(), 4, st.history.size(), f);
    std::fwrite(st.length.data(), 4, st.length.size(), f);
    std::fwrite(st.variance.data(), 4, st.variance.size(), f);
}

static int run_gpu(const char *in_path, const char *out_path, uint32_t w, uint32_t h, uint32_t v) {
    const size_t n = (size_t)w * h * v;
    std::vector<MiptCamera> cams(v);
    std::vector<float> hdr[2], variance(n), none;
    std::vector<uint32_t> counts[2];
    mipt::FeatureImages g[2];
    {
        std::FILE *f = std::fopen(in_path, "rb");
        CHECK(f);
        CHECK(std::fread(cams.data(), sizeof(MiptCamera), v, f) == v);
        CHECK(read_frame(f, n, hdr[0], g[0], counts[0]) && read_frame(f, n, hdr[1], g[1], counts[1]));
        CHECK(std::fread(variance.data(), 4, n, f) == n);
        std::fclose(f);
    }
    const mipt::Renderer r = renderer(w, h);                                 // options.samples = 5: the cap
    std::FILE *out = std::fopen(out_path, "wb");
    CHECK(out);
    mipt::TemporalSettings s;
    s.want_length = s.want_variance = true;
    mipt::TemporalState st;
    std::vector<float> res;
    CHECK(r.temporal(hdr[0], cams, g[0], st, res, counts[0], 0, s) == MIPT_OK && res.size() == n * 3 && st.history.size() == 16 * v + 12 * n);
    write_call(out, res, st);
    CHECK(r.temporal(hdr[1], cams, g[1], st, res, counts[1], 5, s) == MIPT_OK && st.length.size() == n && st.variance.size() == n);
    write_call(out, res, st);
    mipt::SampleMapSettings m;
    m.max_samples = 8; m.budget = 2.0f;
    std::vector<uint32_t> map;
    for (uint32_t rounds : {0u, 1u, 4u}) {
        m.rounds = rounds;
        CHECK(r.sample_map(variance, v, none, none, map, m) == MIPT_OK && map.size() == n);
        std::fwrite(map.data(), 4, map.size(), out);
    }
    std::fclose(out);
    std::puts("gpu ok");
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && std::string(argv[1]) == "cpu") return run_cpu();
    if (argc >= 7 && std::string(argv[1]) == "gpu")
        return run_gpu(argv[2], argv[3], (uint32_t)std::atoi(argv[4]), (uint32_t)std::atoi(argv[5]), (uint32_t)std::atoi(argv[6]));
    std::fprintf(stderr, "usage: test_host_weighted cpu | gpu in.bin out.bin W H V\n");
    return 2;
}
