"""The model of the first-hit feature buffers (include/mipt.h "first-hit feature buffers"), in Python over the HOST arrays of a Scene.
Nothing comes from the library under test:

* the camera ray of (pixel, sample) is the first record orc_debug_pixel writes with samples = 1, max_ray_depth = 1 in the given seed
  mode (for MIPT_SEED_PER_SAMPLE sample s: sample_begin = s);
* the hit is query_model.traverse (Ray::traverse_bvh restated over orc_intersect_node / orc_intersect_tri, either arm);
* the attributes are orc_intersect_tri's out[5..12] on the winning triangle (normal, uv, point), the material arrays and
  orc_texture_color_at(...) / 255;
* the mean is numpy float32: +0, the samples added in order, one division.

tests/test_features_model.py holds this model to the oracle's renders."""
import ctypes as C

import numpy as np

import query_model as Q

NAMES = ("depth", "prim", "material", "position", "uv", "normal", "albedo", "emission")
WIDTH = dict(depth=1, prim=1, material=1, position=3, uv=2, normal=3, albedo=3, emission=3)
UINT = ("prim", "material")
COUNTERS = ("rays", "inner_steps", "tri_tests", "hits", "texel_fetches", "max_stack")
NO_MATERIAL = 0xFFFFFFFF
_F3 = C.c_float * 3


def camera_rays(orc, sc, camera, width, height, seed_mode, sample=0, pixels=None):
    """The camera ray of sample number `sample` (0 -> 1, as the renderers normalise it) of every pixel in `pixels` (None = the whole
    frame, row-major from the top row) -> (RAY records with t_max = 1e30, the oracle's recorded tree triangle [n] (NONE = miss), its
    recorded t [n])."""
    lib = orc.load()
    lib.orc_debug_pixel.restype = C.c_uint32
    mats = np.ascontiguousarray(sc.materials_array())
    texs = [np.ascontiguousarray(t) for t in sc.textures]
    texarr = orc._tex_array(texs)
    cam = np.ascontiguousarray(camera)
    opt = orc.OrcOptions(width, height, 1, 1, seed_mode, 0, orc.LIBM_GLIBC235, 1, 0, 0, 0, sample, 0, 0, 0.0, 0, 0)
    pixels = np.arange(width * height) if pixels is None else np.asarray(pixels)
    rec = np.zeros((4, 8), dtype=np.float32)
    rows = np.zeros((len(pixels), 8), dtype=np.float32)
    for i, pix in enumerate(pixels):
        n = lib.orc_debug_pixel(C.c_void_p(sc.tris.ctypes.data), C.c_uint32(len(sc.tris)), C.c_void_p(sc.bvh_nodes.ctypes.data),
                                C.c_uint32(len(sc.bvh_nodes)), C.c_void_p(mats.ctypes.data), C.c_uint32(len(mats)), texarr,
                                C.c_uint32(len(texs)), C.c_void_p(cam.ctypes.data), C.byref(opt), C.c_uint64(int(pix)),
                                C.c_void_p(rec.ctypes.data), C.c_uint32(len(rec)), None)
        assert n == 1                                                  # depth 1: the camera ray and nothing else
        rows[i] = rec[0]
    return Q.make_rays(rows[:, 0:3], rows[:, 3:6]), rows[:, 6].copy().view(np.uint32), rows[:, 7].copy()


def _texel(orc_lib, orc, tex, u, v):
    t = orc.OrcTexture(tex.shape[1], tex.shape[0], tex.ctypes.data)
    px = (C.c_uint8 * 4)()
    orc_lib.orc_texture_color_at(C.byref(t), C.c_float(float(u)), C.c_float(float(v)), C.byref(px))
    return np.array([px[0], px[1], px[2]], dtype=np.float32) / np.float32(255.0)        # vec3.rs:252-260


def sample_values(orc, sc, ray, cull=False, margin=0.0, tri_order=None, counters=None, mats=None, texs=None):
    """One camera ray -> dict of the eight per-sample values (prim / material as int, the rest float32 arrays)."""
    lib = orc.load()
    mats = sc.materials_array() if mats is None else mats
    texs = sc.textures if texs is None else texs
    c = counters if counters is not None else {}
    t_bits, _, _, tri, front = Q.traverse(lib, sc.tris, sc.bvh_nodes, ray, cull, margin, False, c)
    if tri == Q.NONE:                                                  # HitInfo::default (ray.rs:214-226), the sky (ray.rs:184-193)
        z3 = np.zeros(3, np.float32)
        return dict(depth=np.float32(Q.MISS), prim=Q.NONE, material=NO_MATERIAL, position=z3, uv=np.zeros(2, np.float32), normal=z3,
                    albedo=np.ones(3, np.float32), emission=np.ones(3, np.float32))
    out = np.zeros(13, dtype=np.float32)
    o, d = _F3(*[float(x) for x in ray["origin"]]), _F3(*[float(x) for x in ray["direction"]])
    tri8 = sc.tris.view(np.uint8).reshape(-1, 112)
    lib.orc_intersect_tri(C.byref(o), C.byref(d), C.c_void_p(tri8.ctypes.data + 112 * tri), out.ctypes.data_as(C.POINTER(C.c_float * 13)))
    assert int(out.view(np.uint32)[1]) == t_bits
    mid = int(sc.tris["material_id"][tri])
    m = mats[mid]
    uv = out[8:10].copy()
    if int(m["base_color_tex_id"]) != NO_MATERIAL:                     # ray.rs:162-169
        albedo = _texel(lib, orc, texs[int(m["base_color_tex_id"])], uv[0], uv[1])
        c["texel_fetches"] = c.get("texel_fetches", 0) + 1
    else:
        albedo = np.array(m["base_color"], dtype=np.float32)
    if int(m["emission_tex_id"]) != NO_MATERIAL:                       # ray.rs:170-176
        emission = _texel(lib, orc, texs[int(m["emission_tex_id"])], uv[0], uv[1])
        c["texel_fetches"] = c.get("texel_fetches", 0) + 1
    else:
        emission = np.array(m["emission"], dtype=np.float32)
    prim = int(tri if tri_order is None else tri_order[tri]) | (Q.FRONT if front else 0)
    return dict(depth=out[1].copy(), prim=prim, material=mid, position=out[10:13].copy(), uv=uv, normal=out[5:8].copy(), albedo=albedo,
                emission=emission)


def frame(orc, sc, camera, width, height, seed_mode, samples=1, sample_begin=0, cull=False, margin=0.0, tri_order=None, rays=None):
    """What mipt_render_features writes for one view with all eight buffers wanted -> ({name: array [H,W] or [H,W,k]}, counters dict
    with COUNTERS and "pixels", the recorded (tree triangle, t) of every pixel's first sample as the oracle's own traversal found
    them).  `camera`: a CAMERA record.  `rays`: a dict that keeps the camera rays of a sample number between calls (they do not depend
    on the arm)."""
    assert seed_mode == 1 or samples == 1
    n = width * height
    out = {k: np.zeros((n, WIDTH[k]), dtype=np.uint32 if k in UINT else np.float32) for k in NAMES}
    counters = {k: 0 for k in COUNTERS}
    mats = np.ascontiguousarray(sc.materials_array())
    texs = [np.ascontiguousarray(t) for t in sc.textures]
    s0 = sample_begin if sample_begin else 1
    rays = {} if rays is None else rays
    for s in range(s0, s0 + samples):
        if s not in rays:
            rays[s] = camera_rays(orc, sc, camera, width, height, seed_mode, s)
    per_sample = [rays[s0 + s] for s in range(samples)]
    with np.errstate(all="ignore"):
        for i in range(n):
            acc = {k: np.zeros(3, dtype=np.float32) for k in ("normal", "albedo", "emission")}      # cpu.rs:30
            for s in range(samples):
                v = sample_values(orc, sc, per_sample[s][0][i], cull, margin, tri_order, counters, mats, texs)
                if s == 0:
                    for k in ("depth", "prim", "material", "position", "uv"):
                        out[k][i] = v[k]
                for k in acc:
                    acc[k] = acc[k] + v[k]                                                        # cpu.rs:52
            for k in acc:
                out[k][i] = acc[k] / np.float32(samples)                                          # cpu.rs:60
    counters["pixels"] = n
    shaped = {k: (a.reshape(height, width) if WIDTH[k] == 1 else a.reshape(height, width, WIDTH[k])) for k, a in out.items()}
    return shaped, counters, (per_sample[0][1], per_sample[0][2])


# ---- batches larger than one launch holds in flight: a few distinct cameras, cycled -------------------------------------------------
# (dx, dy, dz, dpitch, dyaw) from the scene's own camera: poses around it that keep the helmet's silhouette in the frame, so that sky
# pixels (over after the root's step) and hits (sixteen steps or more) share tiles
BATCH_POSES = ((0.0, 0.0, 0.0, 0.0, 0.0), (0.3, -0.2, 0.1, 7.0, -11.0), (-0.4, 0.1, 0.0, -5.0, 9.0), (0.1, 0.3, -0.3, 12.0, -25.0))


def batch_cameras(rrt, own):
    """the distinct cameras of a large batch: `own` and the poses of BATCH_POSES around it"""
    cams = [own]
    for dx, dy, dz, dp, dyaw in BATCH_POSES[1:]:
        c = rrt.Camera(position=(own.position[0] + dx, own.position[1] + dy, own.position[2] + dz), pitch=own.pitch + dp, yaw=own.yaw + dyaw)
        c.update_view()
        cams.append(c)
    return cams


def batch_cycle(n_views, n_cameras=len(BATCH_POSES)):
    """camera of view v: stride 3 from camera 1 (coprime to the four cameras), so neighbouring views differ"""
    assert np.gcd(3, n_cameras) == 1
    return (3 * np.arange(n_views) + 1) % n_cameras


def pixel_steps(orc, sc, camera, width, height, seed_mode, sample=0, cull=False, margin=0.0, rays=None):
    """What the camera ray of every pixel costs first_hit_kernel: inner_steps + tri_tests of its traversal, one loop iteration each
    (a fresh counter dict per pixel) -> int64 [height, width].  `rays`: camera_rays(...)[0] of the same frame, if already at hand."""
    rays = camera_rays(orc, sc, camera, width, height, seed_mode, sample)[0] if rays is None else rays
    lib = orc.load()
    out = np.zeros(width * height, dtype=np.int64)
    with np.errstate(all="ignore"):
        for i in range(width * height):
            c = {}
            Q.traverse(lib, sc.tris, sc.bvh_nodes, rays[i], cull, margin, False, c)
            out[i] = c["inner_steps"] + c["tri_tests"]
    return out.reshape(height, width)


def work_order_steps(steps_by_view):
    """The step counts of a batch in first_hit_kernel's work-item order -- view, 8x8 tile of the view row-major, pixel of the tile
    row-major -- from [height, width] arrays, one per view; an item off the frame's ragged edge is 0 (the fetch skips it and the lane
    asks again) -> int64 [n_views * n_tiles * 64]"""
    out = []
    for s in steps_by_view:
        h, w = s.shape
        ty, tx = (h + 7) // 8, (w + 7) // 8
        padded = np.zeros((ty * 8, tx * 8), dtype=np.int64)
        padded[:h, :w] = s
        out.append(padded.reshape(ty, 8, tx, 8).transpose(0, 2, 1, 3).reshape(-1))
    return np.concatenate(out)


def radiance(albedo, emission):
    """What ray.rs:177,197-201 and cpu.rs:52,60 make of a depth-1 path from the two buffers, as f32: (0 + albedo * emission) + 0"""
    a, e = np.asarray(albedo, dtype=np.float32), np.asarray(emission, dtype=np.float32)
    with np.errstate(all="ignore"):
        return (np.float32(0.0) + a * e) + np.float32(0.0)


def same_bits(a, b):
    """bit for bit on uint32 views"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype.itemsize == 4 and b.dtype.itemsize == 4 and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))
