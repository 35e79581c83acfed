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


def traverse(orc_lib, tris, nodes, ray, cull=False, margin=0.0, anyhit=False, counters=None, events=None):
    """One ray.  Closest hit: -> (t bits, u bits, v bits, tree triangle index or NONE, front_face).  Occlusion (anyhit): the same
    tuple for the FIRST triangle in visit order with has_hit && t < t_max (the bound never shrinks).  `counters` (dict) is updated.
    `events` (list) records what happens to LEAVES on the way, as the kernels' stack entries see them: ("push", node, triangle
    count, swapped, stack size after the push) when a leaf is stacked as the far child (swapped: it is the pair's first child, stacked
    after the d1 > d2 swap), ("pop", node, triangle count, stack size before the pop) when one comes off the stack, and ("enter",
    node, triangle count) when one is entered without the stack: the near child, or the root."""
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

    def pop():
        depth, top = len(stack), stack.pop()
        if events is not None and count[top] > 0:
            events.append(("pop", top, int(count[top]), depth))
        return top

    if events is not None and count[0] > 0:
        events.append(("enter", 0, int(count[0])))

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
            node = pop()
            continue
        c1 = int(first[node])
        c2 = c1 + 1
        inner += 1
        max_d = _f32_mul(best, scale)
        d1, d2 = slab(c1, max_d), slab(c2, max_d)
        swapped = d1 > d2
        if swapped:                                                                                  # ray.rs:120-123
            d1, d2, c1, c2 = d2, d1, c2, c1
        if d1 == MISS:                                                                               # ray.rs:124-130
            if not stack:
                break
            node = pop()
        else:
            node = c1
            if events is not None and count[c1] > 0:
                events.append(("enter", c1, int(count[c1])))
            if d2 < MISS:                                                                            # ray.rs:133-136
                if len(stack) < STACK_CAP:
                    stack.append(c2)
                    max_stack = max(max_stack, len(stack))
                    if events is not None and count[c2] > 0:
                        events.append(("push", c2, int(count[c2]), swapped, len(stack)))
                else:
                    c["stack_overflows"] = c.get("stack_overflows", 0) + 1                           # the reference panics here
    c["inner_steps"] = c.get("inner_steps", 0) + inner
    c["tri_tests"] = c.get("tri_tests", 0) + tests
    c["hits"] = c.get("hits", 0) + (1 if res[3] != NONE else 0)
    c["max_stack"] = max_stack
    return res


def _record(words, occ, i, res, tri_order):
    t, u, v, tri, ff = res
    if tri == NONE:
        words[i] = (t, 0, 0, NONE)
    else:
        prim = int(tri if tri_order is None else tri_order[tri])
        words[i] = (t, u, v, prim | (FRONT if ff else 0))
        occ[i] = 1


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
        _record(words, occ, i, traverse(orc_lib, tris, nodes, rays[i], cull, margin, anyhit, counters), tri_order)
    return hits, occ, counters


# ---- batches larger than one launch holds in flight: a small modelled pool, repeated in a chosen order ---------------------------
# A ray's answer and its step counts do not depend on which lane traces it or when, so the model of a million-ray batch is the
# model of its few hundred distinct rays, gathered.  What does depend on the order is the wave's scheduling, restated below.
PER_RAY = ("inner_steps", "tri_tests", "hits", "max_stack")
SHORT, LONG, UNUSED = 0, 1, 2
SHORT_MAX_STEPS, LONG_MIN_STEPS = 2, 16


def per_ray(orc_lib, tris, nodes, rays, cull=False, margin=0.0, anyhit=False, tri_order=None):
    """`query` with a fresh counter dict per ray: -> (HIT records, occluded uint8 [n], {name: int64 [n]} for PER_RAY and
    "stack_overflows").  A ray costs the kernel inner_steps + tri_tests loop iterations, one each (`steps`)."""
    tris, nodes = np.ascontiguousarray(tris), np.ascontiguousarray(nodes)
    hits = np.zeros(len(rays), dtype=HIT)
    words = hits.view(np.uint32).reshape(-1, 4)
    occ = np.zeros(len(rays), dtype=np.uint8)
    per = {k: np.zeros(len(rays), dtype=np.int64) for k in PER_RAY + ("stack_overflows",)}
    for i in range(len(rays)):
        c = {}
        _record(words, occ, i, traverse(orc_lib, tris, nodes, rays[i], cull, margin, anyhit, c), tri_order)
        for k in per:
            per[k][i] = c.get(k, 0)
    return hits, occ, per


def steps(per):
    return per["inner_steps"] + per["tri_tests"]


def classify(n_steps):
    """SHORT: done within two iterations of the wave's loop; LONG: still traversing long after; the rest is left out of a tiling"""
    n_steps = np.asarray(n_steps)
    return np.where(n_steps <= SHORT_MAX_STEPS, SHORT, np.where(n_steps >= LONG_MIN_STEPS, LONG, UNUSED)).astype(np.uint8)


def _coprime_stride(m, start):
    s = start
    while np.gcd(s, m) != 1:
        s += 1
    return s


def tiled(pool_len, classes, n, period=8):
    """Index array [n] into a pool of `pool_len` rays with `classes` [pool_len] of SHORT / LONG / UNUSED: position i holds a SHORT
    ray when i % period < period - period // 4 and a LONG one otherwise (6 and 2 of every 8), each class cycling through its
    members with a fixed stride coprime to their number, so that every member is used and neighbouring windows differ.  Any 8 * k
    consecutive positions AT ANY ALIGNMENT hold 6 * k short and 2 * k long rays: a refill hands a wave a contiguous index range at
    an arbitrary base, and 48 finished lanes of 64 is what makes the next refill a partial one."""
    classes = np.asarray(classes)
    assert len(classes) == pool_len and period % 4 == 0
    short, long_ = np.flatnonzero(classes == SHORT), np.flatnonzero(classes == LONG)
    assert len(short) and len(long_), "a tiling needs both classes"
    n_short = period - period // 4
    i = np.arange(n, dtype=np.int64)
    tile, pos = i // period, i % period
    k_short = (tile * n_short + pos) * _coprime_stride(len(short), 7)
    k_long = (tile * (period - n_short) + (pos - n_short)) * _coprime_stride(len(long_), 5)
    return np.where(pos < n_short, short[k_short % len(short)], long_[k_long % len(long_)])


def wave_refills(n_steps, bases=None, refill_num=1, refill_den=4, skips=False):
    """The scheduling rule of ONE wave of ray_query_kernel, and nothing else, driven by the step count of every ray of a batch
    (`n_steps` [n], each >= 1): the lane states QS_T (traversing) / QS_D (done, result to write) / QS_N (needs a ray) / QS_X
    (retired); a refill pass when `n_need * den >= (n_t + n_need) * num or n_t == 0`; otherwise one step per traversing lane.  A
    refill takes a contiguous block of indices, one per needing lane in lane order, starting at the next value of `bases` (what the
    global counter returned: other waves move it in between); None = the wave is alone and the counter is its own; an exhausted
    iterator = the queue has run out.  `skips` (first_hit_kernel, whose queue runs over whole 8x8 tiles): an index with 0 steps is
    off the frame's ragged edge and leaves its lane needing a ray.  -> the number of refills that delivered at least one ray while another lane was mid-
    traversal: the refills no batch that fits into one launch's first fetch can produce."""
    n_steps = np.asarray(n_steps, dtype=np.int64)
    n = len(n_steps)
    assert n == 0 or n_steps.min() >= (0 if skips else 1)  # the root costs one iteration, inner node or leaf
    T, D, N, X = 0, 1, 2, 3
    state = np.full(64, N)
    left = np.zeros(64, dtype=np.int64)
    it = iter(bases) if bases is not None else None
    counter = 0
    partial = 0
    while True:
        n_t = int((state == T).sum())
        need = (state == D) | (state == N)
        n_need = int(need.sum())
        if n_t == 0 and n_need == 0:
            return partial
        if n_need and (n_t == 0 or n_need * refill_den >= (n_t + n_need) * refill_num):
            state[state == D] = N                        # the result is written here, under the old ray index
            lanes = np.flatnonzero(state == N)           # lane order = rank order
            if it is None:
                base, counter = counter, counter + len(lanes)
            else:
                base = next(it, n)
            ray = base + np.arange(len(lanes))
            got = ray < n
            state[lanes[~got]] = X
            state[lanes[got]] = T
            left[lanes[got]] = n_steps[ray[got]]
            if skips and n:                              # nothing to trace at this index: the lane asks again
                got = got & (n_steps[np.minimum(ray, n - 1)] > 0)
                state[lanes[(ray < n) & ~got]] = N
            if n_t > 0 and got.any():
                partial += 1
            continue
        trav = state == T
        left[trav] -= 1
        state[trav & (left == 0)] = D


def away_rays(tris, n, seed):
    """n rays that start outside the scene's bounds and point away from it: the root's two children are missed and the ray is over
    after one step"""
    p = np.asarray(tris["vertices"]["position"], dtype=np.float64).reshape(-1, 3)
    lo, hi = p.min(axis=0), p.max(axis=0)
    centre, radius = 0.5 * (lo + hi), 0.5 * float(np.linalg.norm(hi - lo))
    rng = np.random.default_rng(seed)
    out = rng.normal(size=(n, 3))
    out /= np.linalg.norm(out, axis=1, keepdims=True)
    return make_rays((centre + 2.0 * radius * out).astype(np.float32), (out + rng.normal(0, 0.05, (n, 3))).astype(np.float32))


def chain_rays(n=70, seed=3):
    """For the chain scene (tests/test_gpu_batch.py _chain_bvh): n rays along +x, which descend the whole chain with one stack
    entry per level, and the rays along -x from the same origins, which leave at the root"""
    rng = np.random.default_rng(seed)
    o = np.zeros((n, 3), np.float32)
    o[:, 1:] = rng.uniform(-0.2, 0.2, (n, 2))
    return np.concatenate([make_rays(o, np.tile(np.float32([1, 0, 0]), (n, 1))), make_rays(o, np.tile(np.float32([-1, 0, 0]), (n, 1)))])


def refill_pool(orc, sc, n_pixels=120, n_away=64, seed=17):
    """The pool of a large batch on a scene with a camera: the rays the oracle traces for n_pixels pixels of a 64 x 48 frame
    (two samples, depth 8), then n_away rays aimed away from the scene"""
    rays, _, _ = oracle_path_rays(orc, sc, 64, 48, np.linspace(0, 64 * 48 - 1, n_pixels).astype(np.int64), spp=2, depth=8)
    return np.concatenate([rays, away_rays(sc.tris, n_away, seed)])


def refill_conditions(n_steps, classes, n=64 * 64 + 77, refill_den=4):
    """What makes a tiling of this pool reach the partial refill on the device: SHORT rays are over within two iterations, LONG
    rays are still traversing at sixteen, both exist, and the restated scheduling rule then refills a wave whose other lanes are
    mid-traversal -- with the wave alone on the queue, and with blocks at seeded random bases (any alignment)."""
    n_steps, classes = np.asarray(n_steps), np.asarray(classes)
    short, long_ = n_steps[classes == SHORT], n_steps[classes == LONG]
    assert len(short) and len(long_), (len(short), len(long_))
    assert short.max() <= 2 and long_.min() >= 16, (short.max(), long_.min())
    batch = n_steps[tiled(len(classes), classes, n)]
    alone = wave_refills(batch, None, refill_den=refill_den)
    assert alone > 0, "no refill into a partly busy wave with sequential bases"
    bases = np.random.default_rng(23).integers(0, n - 64, 48)
    scattered = wave_refills(batch, bases, refill_den=refill_den)
    assert scattered > 0, "no refill into a partly busy wave with random bases"
    return alone, scattered


def occlusion_t_max(rays, closest):
    """`rays` with t_max set around the closest hit's t (`closest`: the reference arm's HIT records), so that about half of the
    rays that hit anything are occluded: factors 0.5, 1, 2, 0.999, 1.001 in turn and one ulp either side"""
    t = closest["t"].copy()
    out = rays.copy()
    out["t_max"] = t * np.float32([0.5, 1.0, 2.0, 0.999, 1.001])[np.arange(len(t)) % 5]
    out["t_max"][3::7] = np.nextafter(t[3::7], np.float32(np.inf))
    out["t_max"][5::7] = np.nextafter(t[5::7], np.float32(0))
    return out


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
