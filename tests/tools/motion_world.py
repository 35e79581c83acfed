"""Scenes with a part that moves, for the previous-position tests (tests/test_motion_model.py, tests/test_gpu_motion.py):

* cornell_block(): the synth Cornell box plus one block of 12 triangles with a material of its own -- an emission texture, so that
  its radiance follows the surface and is not divided out by the albedo -- cut into parts by mesh_model.mesh_from_triangles;
* block_pose(): one matrix per part, the identity but for the block, which is translated and turned about its own vertical axis;
* three_parts(): a ground of 2 triangles, a box of 12 and a fan of 60 thin ones as an indexed mesh of three parts."""
import numpy as np

import mesh_model

BLOCK_CENTER = np.array([-0.2, -0.62, 0.25])
BLOCK_HALF = np.array([0.3, 0.36, 0.3])
CAMERA = ((1.15, -0.25, 0.0), 0.0, 0.0)                       # inside the box, looking down -X at the block


def mat4(lin, trans=(0.0, 0.0, 0.0)):
    """Mat4f data[col][row] as 16 f32 from a 3x3 matrix (applied to column vectors) and a translation"""
    m = np.zeros((4, 4), dtype=np.float32)
    m[:3, :3] = np.asarray(lin, dtype=np.float64).T
    m[3, :3] = trans
    m[3, 3] = 1.0
    return m.reshape(16)


def _box(center, half, mat, synth):
    c, h = np.asarray(center, dtype=np.float64), np.asarray(half, dtype=np.float64)
    faces = []
    for axis in range(3):
        for sign in (-1.0, 1.0):
            a, b = (axis + 1) % 3, (axis + 2) % 3
            n = np.zeros(3)
            n[axis] = sign
            corners = []
            for sa, sb in ((-1, -1), (1, -1), (1, 1), (-1, 1)):
                p = c.copy()
                p[axis] += sign * h[axis]
                p[a] += sa * h[a]
                p[b] += sb * h[b]
                corners.append(tuple(p))
            if sign < 0:
                corners = corners[::-1]
            faces.append(synth.quad(*corners, tuple(n), mat, uv_scale=2.0))
    return np.concatenate(faces)


def cornell_block(min_parts=7):
    """-> (mesh keyword arguments of Scene.from_mesh / mesh_model.expand, materials, textures, camera pose, index of the block's part)"""
    from rust_ray_tracing_amd import synth
    tris, mats, texs, _ = synth.make_scene("cornell")
    mats = list(mats.values())
    rng = np.random.default_rng(23)
    texs = list(texs) + [synth.value_noise_texture(rng, 32, (0.9, 0.5, 0.2), contrast=0.6, cells=4, checker=True)]
    block_mat = len(mats)
    mats.append(synth.material(base=(0.6, 0.6, 0.6), emission_tex=len(texs) - 1))
    tris = np.concatenate([tris, _box(BLOCK_CENTER, BLOCK_HALF, block_mat, synth)])
    mesh, _ = mesh_model.mesh_from_triangles(tris, min_parts)
    parts = mesh["parts"]
    block = [i for i in range(len(parts)) if parts[i]["material_id"] == block_mat and parts[i]["n_tris"] > 0]
    return mesh, mats, texs, CAMERA, block


def block_pose(n_parts, block, shift, turn_deg):
    """[n_parts, 16]: the identity, but the parts in `block` are turned by turn_deg about the vertical axis through the block's
    centre and then moved by `shift`"""
    out = np.stack([mat4(np.eye(3)) for _ in range(n_parts)])
    a = np.deg2rad(turn_deg)
    rot = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
    trans = BLOCK_CENTER - rot @ BLOCK_CENTER + np.asarray(shift, dtype=np.float64)
    for p in block:
        out[p] = mat4(rot, trans)
    return out


def expand(mesh, transforms=None, positions=None):
    """mesh_model.expand of the mesh, with other positions where given"""
    m = dict(mesh)
    if positions is not None:
        m["positions"] = positions
    return mesh_model.expand(m["positions"], m["normals"], m["tex_coords"], m["indices"], m["parts"], m["normal_indices"], m["tex_coord_indices"],
                             transforms=transforms)


def three_parts():
    """-> (mesh keyword arguments, materials, camera pose): ground (2 triangles), box (12), fan (60 thin triangles round one apex)"""
    from rust_ray_tracing_amd import synth
    pos, idx = [], []
    pos += [(-2.0, -1.0, -2.0), (2.0, -1.0, -2.0), (2.0, -1.0, 2.0), (-2.0, -1.0, 2.0)]
    idx += [(0, 1, 3), (1, 2, 3)]
    c, h = np.array([0.1, -0.55, -0.6]), 0.4
    base = len(pos)
    pos += [tuple(c + h * np.array([sx, sy, sz])) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]
    for q in ((0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)):
        idx += [(base + q[0], base + q[1], base + q[3]), (base + q[1], base + q[2], base + q[3])]
    apex = len(pos)
    pos.append((-0.3, 0.45, 0.7))
    n_fan = 60
    for i in range(n_fan + 1):
        a = 2.0 * np.pi * i / n_fan
        pos.append((-0.3 + 0.05 * np.sin(3 * a), 0.45 + 0.85 * np.cos(a), 0.7 + 0.85 * np.sin(a)))
    idx += [(apex, apex + 1 + i, apex + 2 + i) for i in range(n_fan)]
    parts = np.zeros(3, dtype=mesh_model.PART)
    parts[0], parts[1], parts[2] = (0, 2, 0, 0), (2, 12, 1, 0), (14, n_fan, 2, 0)
    mesh = dict(positions=np.asarray(pos, dtype=np.float32), normals=None, tex_coords=None, indices=np.asarray(idx, dtype=np.uint32).reshape(-1),
                normal_indices=None, tex_coord_indices=None, parts=parts)
    mats = [synth.material(base=(0.7, 0.7, 0.7)), synth.material(base=(0.8, 0.3, 0.2)), synth.material(base=(0.2, 0.4, 0.9))]
    return mesh, mats, ((2.6, 0.1, 0.0), 0.0, 0.0)
