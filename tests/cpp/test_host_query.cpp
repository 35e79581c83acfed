// Exercises the ray-query methods of include/mipt_host.hpp (Scene / Mesh query_closest, query_occluded and the *_on helpers).
//   test_host_query cpu                              argument handling without a device
//   test_host_query gpu scene.obj rays.bin out.bin   rays.bin: n x MiptRay; out.bin: for Scene then Mesh: n x MiptHit, n occlusion bytes
#include "mipt_host.hpp"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "CHECK failed at line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static int run_cpu() {
    MiptScene *opaque = reinterpret_cast<MiptScene *>(0x1000);           // never dereferenced by the checks below
    std::vector<MiptRay> none;
    std::vector<MiptHit> hits(3);
    std::vector<uint8_t> occ(3);
    MiptStats st;
    std::memset(&st, 0xff, sizeof st);
    CHECK(mipt::query_closest_on(opaque, none, hits, nullptr, &st) == MIPT_OK && hits.empty() && st.rays == 0);
    CHECK(mipt::query_occluded_on(opaque, none, occ) == MIPT_OK && occ.empty());
    std::vector<MiptRay> two(2);
    MiptQueryOptions bad{};
    bad.traversal = 7;
    CHECK(mipt::query_closest_on(opaque, two, hits, &bad) == MIPT_ERR_INVALID_ARG && hits.size() == 2);
    CHECK(std::string(mipt_last_error()).find("unknown traversal") != std::string::npos);
    bad.traversal = 0; bad.flags = MIPT_FLAG_SUM;
    CHECK(mipt::query_occluded_on(opaque, two, occ, &bad) == MIPT_ERR_INVALID_ARG && occ.size() == 2);
    mipt::Mesh mesh;                                                      // not created: a null scene
    CHECK(mesh.query_closest(two, hits) == MIPT_ERR_INVALID_ARG && mesh.query_occluded(two, occ) == MIPT_ERR_INVALID_ARG);
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
    MiptQueryOptions opt{};
    opt.flags = MIPT_FLAG_COUNT;
    std::vector<MiptHit> hits;
    std::vector<uint8_t> occ;
    MiptStats st{};
    CHECK(scene->query_closest(rays, hits, &opt, &st) == MIPT_OK && hits.size() == rays.size() && st.rays == rays.size());
    CHECK(scene->query_occluded(rays, occ) == MIPT_OK && occ.size() == rays.size());
    std::fwrite(hits.data(), sizeof(MiptHit), hits.size(), out);
    std::fwrite(occ.data(), 1, occ.size(), out);
    // the same triangles, in the scene's order, as a resident mesh: one part per run of equal material ids
    mipt::Mesh mesh;
    for (size_t t = 0; t < scene->tris.size(); t++) {
        const MiptTriangle &tri = scene->tris[t];
        for (const MiptVertex &v : tri.vertices) {
            mesh.positions.insert(mesh.positions.end(), {v.position.x, v.position.y, v.position.z});
            mesh.normals.insert(mesh.normals.end(), {v.normal.x, v.normal.y, v.normal.z});
            mesh.tex_coords.insert(mesh.tex_coords.end(), {v.tex_coord_x, v.tex_coord_y});
            mesh.indices.push_back((uint32_t)mesh.indices.size());
        }
        if (mesh.parts.empty() || mesh.parts.back().material_id != tri.material_id) mesh.parts.push_back({(uint32_t)t, 0u, tri.material_id, 0u});
        mesh.parts.back().n_tris++;
    }
    std::vector<MiptMaterial> mats;
    for (const auto &kv : scene->materials) mats.push_back(kv.second);
    MiptSceneDesc d{};
    d.materials = mats.data(); d.n_materials = (uint32_t)mats.size();
    CHECK(mesh.create(d) == MIPT_OK);
    hits.clear(); occ.clear();
    CHECK(mesh.query_closest(rays, hits) == MIPT_OK && mesh.query_occluded(rays, occ) == MIPT_OK);
    std::fwrite(hits.data(), sizeof(MiptHit), hits.size(), out);
    std::fwrite(occ.data(), 1, occ.size(), out);
    std::fclose(out);
    std::puts("gpu ok");
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && std::string(argv[1]) == "cpu") return run_cpu();
    if (argc >= 5 && std::string(argv[1]) == "gpu") return run_gpu(argv[2], argv[3], argv[4]);
    std::fprintf(stderr, "usage: test_host_query cpu | gpu scene.obj rays.bin out.bin\n");
    return 2;
}
