// pt_mesh_rule.h -- the position half of the mesh expansion rule (include/mipt.h, "resident indexed meshes"): the record of a part as
// the expansion reads it and the arithmetic that places a position.  ONE function for the host (mipt_mesh_expand), the expansion
// kernel (scene_mesh.hip) and the motion pass (first_hit.hip, the tracked source), compiled everywhere under -ffp-contract=off, so
// the three agree bit for bit.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace mipt {

// one part as the expansion reads it (24 dwords)
struct PartRec {
    float a[4][3];          // matrix columns a0, a1, a2 and the translation
    float c[3][3];          // cofactor columns cross(a1,a2), cross(a2,a0), cross(a0,a1)
    uint32_t first_tri, material_id, has_xf;
};

__host__ __device__ inline void xf_position(const PartRec &r, float *p) {               // mat4.rs:146-149, then + translation
    const float x = p[0], y = p[1], z = p[2];
    for (int k = 0; k < 3; k++) p[k] = (((r.a[0][k] * x) + (r.a[1][k] * y)) + (r.a[2][k] * z)) + r.a[3][k];
}

// the part that owns triangle t: the last record with first_tri <= t (empty parts own nothing); n_parts >= 1
__host__ __device__ inline uint32_t part_of(const PartRec *parts, uint32_t n_parts, uint32_t t) {
    uint32_t lo = 0u, hi = n_parts;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (parts[mid].first_tri <= t) lo = mid; else hi = mid;
    }
    return lo;
}

} // namespace mipt
