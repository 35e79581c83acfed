// Exercises Renderer::temporal of include/mipt_host.hpp (mipt_temporal over host images).
//   test_host_temporal cpu                              argument handling without a device
//   test_host_temporal gpu in.bin out.bin W H V         in.bin: V cameras (80 B each), then for each of two frames the hdr, position,
//                                                       normal, depth, material and albedo planes of V views of W x H;
//                                                       out.bin: per call out, history, length, variance -- the first frame with
//                                                       albedo, the second from its history, the second again without albedo
//                                                       and in place
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

static MiptCamera camera(float x) {
    MiptCamera c{};
    const float position[3] = {x, 1.0f, -2.0f};
    mipt_camera_from_pose(position, 3.0f, 20.0f + x, &c);
    return c;
}

static int run_cpu() {
    static_assert(sizeof(MiptTemporalOptions) == 64 && sizeof(MiptTemporalBuffers) == 128, "ABI struct sizes");
    const uint32_t w = 6, h = 4, v = 2;
    const size_t n = (size_t)w * h * v;
    const mipt::Renderer r = renderer(w, h);
    std::vector<MiptCamera> cams = {camera(0.0f), camera(0.5f)};
    std::vector<float> hdr(n * 3, 0.5f), out;
    mipt::FeatureImages g;
    g.position.assign(n * 3, 1.0f); g.normal.assign(n * 3, 0.0f); g.depth.assign(n, 2.0f); g.material.assign(n, 1u);
    mipt::TemporalState st;
    // sizes that do not fit never reach the library
    std::vector<float> shorter(n * 3 - 1, 0.5f);
    CHECK(r.temporal(shorter, cams, g, st, out) == MIPT_ERR_INVALID_ARG);
    mipt::FeatureImages bad = g;
    bad.depth.assign(n * 3, 1.0f);
    CHECK(r.temporal(hdr, cams, bad, st, out) == MIPT_ERR_INVALID_ARG);
    bad = g; bad.material.clear();
    CHECK(r.temporal(hdr, cams, bad, st, out) == MIPT_ERR_INVALID_ARG);
    bad = g; bad.albedo.assign(n * 3 + 3, 1.0f);
    CHECK(r.temporal(hdr, cams, bad, st, out) == MIPT_ERR_INVALID_ARG);
    st.history.assign(5, 0u);
    CHECK(r.temporal(hdr, cams, g, st, out) == MIPT_ERR_INVALID_ARG && st.history.size() == 5);
    st.history.clear();
    // what the library checks, with its message
    mipt::TemporalSettings s;
    s.alpha_min = 1.5f;
    CHECK(r.temporal(hdr, cams, g, st, out, s) == MIPT_ERR_INVALID_ARG && says("alpha_min"));
    s = mipt::TemporalSettings(); s.max_history = 0.5f;
    CHECK(r.temporal(hdr, cams, g, st, out, s) == MIPT_ERR_INVALID_ARG && says("max_history"));
    s = mipt::TemporalSettings(); s.normal_tol = -1.0f;
    CHECK(r.temporal(hdr, cams, g, st, out, s) == MIPT_ERR_INVALID_ARG && says("normal_tol"));
    s = mipt::TemporalSettings(); s.depth_tol = -1.0f;
    CHECK(r.temporal(hdr, cams, g, st, out, s) == MIPT_ERR_INVALID_ARG && says("depth_tol"));
    CHECK(r.temporal(hdr, std::vector<MiptCamera>(), g, st, out) == MIPT_ERR_INVALID_ARG && says("n_views"));
    CHECK(renderer(1u << 16, 1u << 16).temporal(hdr, {cams[0]}, g, st, out) == MIPT_ERR_INVALID_ARG && says("below 2^32"));
    std::vector<MiptCamera> singular = cams;
    std::memset(singular[1].look_at, 0, sizeof singular[1].look_at);
    CHECK(r.temporal(hdr, singular, g, st, out) == MIPT_ERR_INVALID_ARG && says("cameras[1].look_at") && st.history.empty());
    // a well-formed call: the result of the right size on a GPU, MIPT_ERR_HIP without one -- never a CPU blend
    s = mipt::TemporalSettings(); s.want_length = true;
    const int rc = r.temporal(hdr, cams, g, st, out, s);
    CHECK(rc == MIPT_OK || rc == MIPT_ERR_HIP);
    CHECK(out.size() == n * 3 && st.length.size() == n && st.variance.empty());
    CHECK(rc == MIPT_OK ? st.history.size() == 16 * v + 12 * n : st.history.empty());
    CHECK(mipt_temporal_history_bytes(w, h, v) == 64 * v + 48 * n && mipt_temporal_history_bytes(0, h, v) == 0);
    std::puts(rc == MIPT_OK ? "cpu ok (device present)" : "cpu ok");
    return 0;
}

static bool read_frame(std::FILE *f, size_t n, std::vector<float> &hdr, mipt::FeatureImages &g) {
    hdr.resize(n * 3); g.position.resize(n * 3); g.normal.resize(n * 3); g.depth.resize(n); g.material.resize(n); g.albedo.resize(n * 3);
    return std::fread(hdr.data(), 4, n * 3, f) == n * 3 && std::fread(g.position.data(), 4, n * 3, f) == n * 3 &&
           std::fread(g.normal.data(), 4, n * 3, f) == n * 3 && std::fread(g.depth.data(), 4, n, f) == n &&
           std::fread(g.material.data(), 4, n, f) == n && std::fread(g.albedo.data(), 4, n * 3, f) == n * 3;
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
    std::vector<float> hdr[2];
    mipt::FeatureImages g[2];
    {
        std::FILE *f = std::fopen(in_path, "rb");
        CHECK(f);
        CHECK(std::fread(cams.data(), sizeof(MiptCamera), v, f) == v);
        CHECK(read_frame(f, n, hdr[0], g[0]) && read_frame(f, n, hdr[1], g[1]));
        std::fclose(f);
    }
    const mipt::Renderer r = renderer(w, h);
    std::FILE *out = std::fopen(out_path, "wb");
    CHECK(out);
    mipt::TemporalSettings s;
    s.want_length = s.want_variance = true;
    mipt::TemporalState first, st;
    std::vector<float> res;
    CHECK(r.temporal(hdr[0], cams, g[0], first, res, s) == MIPT_OK && res.size() == n * 3 && first.history.size() == 16 * v + 12 * n);
    write_call(out, res, first);
    st = first;
    CHECK(r.temporal(hdr[1], cams, g[1], st, res, s) == MIPT_OK && st.length.size() == n && st.variance.size() == n);
    write_call(out, res, st);
    mipt::FeatureImages plain = g[1];
    plain.albedo.clear();
    st = first;
    CHECK(r.temporal(hdr[1], cams, plain, st, res, s) == MIPT_OK);
    write_call(out, res, st);
    st = first;
    CHECK(r.temporal(hdr[1], cams, g[1], st, hdr[1], s) == MIPT_OK && hdr[1].size() == n * 3);     // in place
    write_call(out, hdr[1], st);
    std::fclose(out);
    std::puts("gpu ok");
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && std::string(argv[1]) == "cpu") return run_cpu();
    if (argc >= 7 && std::string(argv[1]) == "gpu")
        return run_gpu(argv[2], argv[3], (uint32_t)std::atoi(argv[4]), (uint32_t)std::atoi(argv[5]), (uint32_t)std::atoi(argv[6]));
    std::fprintf(stderr, "usage: test_host_temporal cpu | gpu in.bin out.bin W H V\n");
    return 2;
}
