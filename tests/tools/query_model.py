"""The model of the ray queries (include/mipt.h "ray queries"): Ray::traverse_bvh (reference src/renderer/backend/cpu/ray.rs:84-139)
restated in Python over the HOST node and triangle arrays, with hit_info.distance starting at the ray's t_max, the culled arm of
rt_compute.wgsl:341-349 and the early exit of an occlusion query.  All arithmetic is the oracle's (orc_intersect_node,
orc_intersect_tri); nothing comes from the library under test.  Also: the rays the oracle itself traces (orc_debug_pixel), as
test input and as the check of this model (tests/test_query_model.py)."""
import ctypes as C

import numpy as np

MISS = float(np.float32(1e30))
NONE = 0xFFFFFFFF
FRONT = 0x80000000
STACK_CAP = 64                                     # the kernel's: 16 entries in LDS + 48 spilled
RAY = np.dtype([("origin", "<f4", 3), ("t_max", "<f4"), ("direction", "<f4", 3), ("reserved", "<u4")])
HIT = np.dtype([("t", "<f4"), ("u", "<f4"), ("v", "<f4"), ("prim", "<u4")])
COUNTERS = ("rays", "inner_steps", "tri_tests", "hits", "max_stack")
_F3 = C.c_float * 3


def make_rays(origins, directions, t_max=1e30):
    o = np.asarray(origins, dtype=np.float32).reshape(-1, 3)
    r = np.zeros(len(o), dtype=RAY)
    r["origin"], r["direction"], r["t_max"] = o, np.asarray(directions, dtype=np.float32).reshape(-1, 3), t_max
    return r


def _f32_mul(a, b):
    with np.errstate(all="ignore"):
        return float(np.float32(a) * np.float32(b))


def traverse(orc_lib, tris, nodes, ray, cull=False, margin=0.0, anyhit=False, counters=None):
    """One ray.  Closest hit: -> (t bits, u bits, v bits, tree triangle index or NONE, front_face).  Occlusion (anyhit): the same
    tuple for the FIRST triangle in visit order with has_hit && t < t_max (the bound never shrinks).  `counters` (dict) is updated."""
    tris8 = tris.view(np.uint8).reshape(-1, 112)
    nodes8 = nodes.view(np.uint8).reshape(-1, 32)
    tri_base, node_base = tris8.ctypes.data, nodes8.ctypes.data
    first = nodes["first_tri_or_child"]
    count = nodes["num_tris"]
    o, d = _F3(*[float(x) for x in ray["origin"]]), _F3(*[float(x) for x in ray["direction"]])
    t_max = float(ray["t_max"])
    scale = float(np.float32(1.0) + np.float32(margin))
    out = np.zeros(13, dtype=np.float32)
    out_p = out.ctypes.data_as(C.POINTER(C.c_float * 13))
    out_bits = out.view(np.uint32)
    best = t_max
    res = (int(np.float32(MISS).view(np.uint32)), 0, 0, NONE, False)       # HitInfo::default (ray.rs:214-226)
    stack, node = [], 0
    c = counters if counters is not None else {}
    c["rays"] = c.get("rays", 0) + 1
    inner = tests = 0
    max_stack = c.get("max_stack", 0)

    def slab(i, max_d):
        t = orc_lib.orc_intersect_node(C.byref(o), C.byref(d), C.c_void_p(node_base + 32 * i))     # ray.rs:69-81
        if cull and t != MISS and not (t < max_d):                                                   # rt_compute.wgsl:348
            return MISS
        return t

    done = False
    while not done:
        n = int(count[node])
        if n > 0:                                                                                    # ray.rs:90-99
            a = int(first[node])
            for i in range(a, a + n):
                orc_lib.orc_intersect_tri(C.byref(o), C.byref(d), C.c_void_p(tri_base + 112 * i), out_p)
                tests += 1
                if out[0] != 0.0 and float(out[1]) < best:                                           # strict <: ties keep the first
                    res = (int(out_bits[1]), int(out_bits[2]), int(out_bits[3]), i, out[4] != 0.0)
                    if anyhit:
                        done = True
                        break
                    best = float(out[1])
            if done or not stack:
                break
            node = stack.pop()
            continue
        c1 = int(first[node])
        c2 = c1 + 1
        inner += 1
        max_d = _f32_mul(best, scale)
        d1, d2 = slab(c1, max_d), slab(c2, max_d)
        if d1 > d2:                                                                                  # ray.rs:120-123
            d1, d2, c1, c2 = d2, d1, c2, c1
        if d1 == MISS:                                                                               # ray.rs:124-130
            if not stack:
                break
            node = stack.pop()
        else:
            node = c1
            if d2 < MISS:                                                                            # ray.rs:133-136
                if len(stack) < STACK_CAP:
                    stack.append(c2)
                    max_stack = max(max_stack, len(stack))
                else:
                    c["stack_overflows"] = c.get("stack_overflows", 0) + 1                           # the reference panics here
    c["inner_steps"] = c.get("inner_steps", 0) + inner
    c["tri_tests"] = c.get("tri_tests", 0) + tests
    c["hits"] = c.get("hits", 0) + (1 if res[3] != NONE else 0)
    c["max_stack"] = max_stack
    return res


def query(orc_lib, tris, nodes, rays, cull=False, margin=0.0, anyhit=False, tri_order=None):
    """Every ray of `rays` (RAY records).  -> (HIT records exactly as mipt_query_closest writes them -- prim in the caller's order
    through `tri_order` (None: the tree order is the caller's), bit 31 = front face; a miss is {1e30, 0, 0, NONE} -- , occluded
    uint8 [n] (for anyhit: the query's answer; else hit-or-not), counters dict)."""
    tris, nodes = np.ascontiguousarray(tris), np.ascontiguousarray(nodes)
    hits = np.zeros(len(rays), dtype=HIT)
    words = hits.view(np.uint32).reshape(-1, 4)
    occ = np.zeros(len(rays), dtype=np.uint8)
    counters = {k: 0 for k in COUNTERS}
    for i in range(len(rays)):
        t, u, v, tri, ff = traverse(orc_lib, tris, nodes, rays[i], cull, margin, anyhit, counters)
        if tri == NONE:
            words[i] = (t, 0, 0, NONE)
        else:
            prim = int(tri if tri_order is None else tri_order[tri])
            words[i] = (t, u, v, prim | (FRONT if ff else 0))
            occ[i] = 1
    return hits, occ, counters


def oracle_path_rays(orc, sc, width, height, pixels, spp=2, depth=8):
    """Every ray the oracle traces for `pixels` of a width x height frame of Scene `sc` (camera rays and the scatter rays that
    start on a surface), as orc_debug_pixel records them: -> (RAY records with t_max = 1e30, recorded tree triangle index (NONE =
    miss) [n], recorded t [n])."""
    lib = orc.load()
    lib.orc_debug_pixel.restype = C.c_uint32
    mats = np.ascontiguousarray(sc.materials_array())
    texs = [np.ascontiguousarray(t) for t in sc.textures]
    texarr = orc._tex_array(texs)
    opt = orc.OrcOptions(width, height, spp, depth, 0, 0, orc.LIBM_GLIBC235, 1, 0, 0, 0, 0, 0, 0, 0.0, 0, 0)
    rec = np.zeros((spp * (depth + 1) + 8, 8), dtype=np.float32)
    rows = []
    for pix in pixels:
        n = lib.orc_debug_pixel(C.c_void_p(sc.tris.ctypes.data), C.c_uint32(len(sc.tris)), C.c_void_p(sc.bvh_nodes.ctypes.data),
                                C.c_uint32(len(sc.bvh_nodes)), C.c_void_p(mats.ctypes.data), C.c_uint32(len(mats)), texarr,
                                C.c_uint32(len(texs)), C.c_void_p(sc.camera.uniform.ctypes.data), C.byref(opt), C.c_uint64(int(pix)),
                                C.c_void_p(rec.ctypes.data), C.c_uint32(len(rec)), None)
        rows.append(rec[:n].copy())
    r = np.concatenate(rows)
    return make_rays(r[:, 0:3], r[:, 3:6]), r[:, 6].copy().view(np.uint32), r[:, 7].copy()


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))
