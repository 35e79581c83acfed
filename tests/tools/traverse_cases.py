"""Scenes and rays for the forms of a traversal stack entry (csrc/pt_traverse.h encode_child), CPU only.

The traversal step exists three times (pt_kernel.hip, ray_query.hip, first_hit.hip), each with its own push and pop.  A pop decodes an
inner pair, an INLINE leaf (bit31 | n << 25 | first_tri, 1 <= n <= 63) or the CHILD-REF form (bit31 | pair * 2 + which, n >= 64, (a, n)
read again from the pair record); the root leaf takes no entry at all.  The scenes here put one leaf of a chosen size m where each of
those forms meets it, and make a hit on the wrong triangle of that leaf visible:

* LEAF-FORM SCENES from bvh_corpus.bunch(m), whose m triangles no builder may split.  They are nested, similar and on parallel planes,
  so one ray crosses many of them at different t and the order inside the leaf decides the answer.  "left": the bunch as it is, node 1
  of the tree (the pair's first child, which = 0: stacked only after the d1 > d2 swap); "right": every x negated (exact), node 2
  (which = 1: stacked without the swap); "root": bunch(m, rest=0), one node.  material_id = input index mod 7 over a palette of
  distinct albedo and emission, so a wrong triangle changes prim, material, albedo and the radiance.
* four RAY FAMILIES per left / right scene: (a) from beyond the far end of the remainder into the bunch -- the remainder's box is
  nearer, the bunch is stacked and popped; (b) from just outside the bunch, leaving through the remainder -- the bunch is entered as
  the near child; (c) across the root's box between the two children; (d) family (a) with t_max around the closest hit.  Each in two
  forms: unit directions (ray_safe's fast quotient) and un-normalised ones with a component above 2 (the IEEE division of `slab`).
* CORPUS SCENES by name from bvh_corpus.ENTRIES, with rays from outside the bounds towards triangle centroids and through vertices and
  edge midpoints from an eye point.

Left out: special_huge, special_nan and every overflow* entry.  Their coordinates pass 2^40 or are NaN; whether a resident scene takes
them is another question than traversal.

tests/test_traverse_cases_model.py holds all of this to what it is for on the models alone (which node the bunch is, that it is
stacked and popped, entered directly, hit and missed), so that tests/test_gpu_traverse_corpus.py cannot pass by never reaching a case."""
import numpy as np

import bvh_corpus as bc
import query_model as Q

F32 = np.float32
LEAF_SIZES = (62, 63, 64, 65, 300)                    # both sides of `n < 64u` and of the 6-bit field, and a leaf far past it
LEAF_SIZE_BIG = 3000                                  # the queries and the trace kernel only: the Python models pay per triangle test
SHAPES = ("left", "right", "root")
PALETTE = ((0.80, 0.30, 0.20), (0.10, 0.90, 0.40), (0.25, 0.35, 0.85), (0.70, 0.70, 0.10), (0.60, 0.15, 0.75), (0.15, 0.65, 0.70),
           (0.90, 0.55, 0.35))                        # base colour of material k; its emission is the colour of material (k + 3) % 7 * (k + 1) / 4
CORPUS = ("size513_copies", "size2049_copies", "size2049_ties", "size2049_zero_area", "size2049_flat", "special_zeros", "special_denormal",
          "spiral", "spiral_small", "chain_x", "bunch100_cost", "bunch300_z", "halves100")


def materials():
    from rust_ray_tracing_amd import synth
    n = len(PALETTE)
    return [synth.material(base=PALETTE[k], emission=tuple(F32(c) * F32(k + 1) / F32(4.0) for c in PALETTE[(k + 3) % n])) for k in range(n)]


def _geometric_normals(t):
    p = t["vertices"]["position"].astype(np.float64)
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    ln = np.linalg.norm(n, axis=1)
    n = np.where((ln > 0)[:, None], n / np.where(ln > 0, ln, 1.0)[:, None], np.array([0.0, 1.0, 0.0]))
    t["vertices"]["normal"] = n.astype(F32)[:, None, :]


def dress(tris):
    """material_id = input index (carried in tex_coord_x) mod the palette; vertex normals = the triangle's own"""
    t = tris.copy()
    t["material_id"] = t["vertices"]["tex_coord_x"][:, 0].astype(np.uint32) % len(PALETTE)
    _geometric_normals(t)
    return t


def leaf_tris(m, shape):
    """TRIANGLE records of a leaf-form scene, in input order"""
    pos = bc.bunch(m, rest=0) if shape == "root" else bc.bunch(m)
    if shape == "right":
        pos = pos.copy()
        pos[:, :, 0] = -pos[:, :, 0]
    return dress(bc.triangles(pos))


def corpus_tris(name):
    assert name in CORPUS
    return dress(bc.make(name))


# ---- what a tree holds ----------------------------------------------------------------------------------------------------------------
def as_nodes(nodes):
    from rust_ray_tracing_amd import NODE
    return np.ascontiguousarray(nodes).view(NODE).reshape(-1)


def bunch_node(nodes, m):
    """index of the one leaf of m triangles"""
    idx = np.flatnonzero(as_nodes(nodes)["num_tris"] == m)
    assert len(idx) == 1, idx
    return int(idx[0])


def tiny_axes(nodes):
    """DevScene::tiny_axes restated: bit a is set when a bounding plane of the tree has a coordinate 0 < |p| < 2^-76 on axis a"""
    nd = as_nodes(nodes)
    p = np.abs(np.concatenate([nd["bounds_min"], nd["bounds_max"]]))
    return sum(1 << a for a in range(3) if np.any((p[:, a] > 0) & (p[:, a] < F32(2.0 ** -76))))


def ray_safe(rays, tiny=0):
    """ray_safe (csrc/pt_traverse.h) restated: bool [n], True where the slab test takes the exact fast quotient"""
    with np.errstate(all="ignore"):
        d, o = np.abs(rays["direction"]), np.abs(rays["origin"])
        zero_ok = np.array([not (tiny >> a) & 1 for a in range(3)])
        origin = (o >= F32(2.0 ** -70)) | ((o == 0) & zero_ok[None, :])
        return np.all((d >= F32(2.0 ** -60)) & (d <= F32(2.0)), axis=1) & np.all(o <= F32(2.0 ** 40), axis=1) & np.all(origin, axis=1)


# ---- rays for a left / right scene -------------------------------------------------------------------------------------------------------
def _two_forms(o, d, rng):
    """directions of even rays unit, of odd rays un-normalised with their largest component between 2.5 and 6"""
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    odd = np.arange(len(d)) % 2 == 1
    d[odd] *= (rng.uniform(2.5, 6.0, len(d)) / np.abs(d).max(axis=1))[odd, None]
    return Q.make_rays(o.astype(F32), d.astype(F32))


def _boxes(tris, nodes, m):
    nd = as_nodes(nodes)
    b = bunch_node(nodes, m)
    assert b in (1, 2) and nd["num_tris"][0] == 0 and nd["first_tri_or_child"][0] == 1
    r = 3 - b
    bunch = tris[nd["first_tri_or_child"][b]: nd["first_tri_or_child"][b] + m]
    return ((nd["bounds_min"][b].astype(np.float64), nd["bounds_max"][b].astype(np.float64)),
            (nd["bounds_min"][r].astype(np.float64), nd["bounds_max"][r].astype(np.float64)),
            (nd["bounds_min"][0].astype(np.float64), nd["bounds_max"][0].astype(np.float64)), bunch["vertices"]["position"].astype(np.float64))


def _on_bunch(rng, P, n, box):
    """n points: most ON a triangle of the bunch (uniform barycentric), every fourth anywhere in its box"""
    k = rng.integers(0, len(P), n)
    bary = rng.dirichlet((1.0, 1.0, 1.0), n)
    pts = (P[k] * bary[:, :, None]).sum(axis=1)
    off = np.arange(n) % 4 == 3
    pts[off] = rng.uniform(box[0], box[1], (n, 3))[off]
    return pts


def leaf_rays(tris, nodes, m, n=96, seed=1):
    """Rays of families (a), (b), (c) for a left / right scene (tree-ordered `tris`, its `nodes`): -> (RAY records, family letter [n]).
    Family (d) is made from (a) by `with_t_max` once the closest hits are known.  n is split 3 : 2 : 1."""
    rng = np.random.default_rng([seed, m])
    (blo, bhi), (rlo, rhi), (wlo, whi), P = _boxes(tris, nodes, m)
    n_a, n_b = n // 2, n // 3
    n_c = n - n_a - n_b
    side = 1.0 if rlo[0] > bhi[0] else -1.0                      # the remainder lies on +x (left scene) or -x (right scene)
    far_x = (rhi[0] if side > 0 else rlo[0]) + side * 0.1 * (rhi[0] - rlo[0])
    centre, shrink = 0.5 * (rlo + rhi), 0.4 * (rhi - rlo)
    # (a) through a point of the remainder's box, from beyond its far end, at a point of the bunch
    tg = _on_bunch(rng, P, n_a, (blo, bhi))
    via = rng.uniform(centre - shrink, centre + shrink, (n_a, 3))
    o_a = tg + (via - tg) * ((far_x - tg[:, 0]) / (via[:, 0] - tg[:, 0]))[:, None]
    rays_a = _two_forms(o_a, tg - o_a, rng)
    # (b) from behind the bunch (two box diagonals back), through a point of the bunch, at a point of the remainder's box
    tg = _on_bunch(rng, P, n_b, (blo, bhi))
    via = rng.uniform(centre - shrink, centre + shrink, (n_b, 3))
    d_b = (via - tg) / np.linalg.norm(via - tg, axis=1, keepdims=True)
    o_b = tg - d_b * (2.0 * np.linalg.norm(bhi - blo))
    rays_b = _two_forms(o_b, d_b, rng)
    # (c) across the root's box in the gap between the children, nearly at right angles to x
    gap_lo, gap_hi = (bhi[0], rlo[0]) if side > 0 else (rhi[0], blo[0])
    x = rng.uniform(gap_lo + 0.1 * (gap_hi - gap_lo), gap_hi - 0.1 * (gap_hi - gap_lo), n_c)
    through = np.stack([x, rng.uniform(wlo[1], whi[1], n_c), rng.uniform(wlo[2], whi[2], n_c)], axis=1)
    ang = rng.uniform(0.0, 2.0 * np.pi, n_c)
    d_c = np.stack([rng.uniform(0.01, 0.05, n_c) * rng.choice([-1.0, 1.0], n_c), np.cos(ang), np.sin(ang)], axis=1)
    d_c[np.abs(d_c) < 1e-3] = 1e-3                                # no component near zero: the unit form stays inside ray_safe
    rays_c = _two_forms(through - d_c * 20.0, d_c, rng)
    return np.concatenate([rays_a, rays_b, rays_c]), np.array(["a"] * n_a + ["b"] * n_b + ["c"] * n_c)


def with_t_max(rays, family, closest, every=2):
    """family (d): every `every`-th ray of family (a) again, with t_max around its closest hit (query_model.occlusion_t_max)
    -> (all rays, family letters)"""
    pick = np.flatnonzero(family == "a")[::every]
    d = Q.occlusion_t_max(rays[pick], closest[pick])
    return np.concatenate([rays, d]), np.concatenate([family, np.array(["d"] * len(pick))])


def root_rays(tris, n=48, seed=2):
    """for a root scene: from a shell around the bunch at points of it, both forms"""
    rng = np.random.default_rng([seed, len(tris)])
    P = tris["vertices"]["position"].astype(np.float64)
    lo, hi = P.reshape(-1, 3).min(0), P.reshape(-1, 3).max(0)
    tg = _on_bunch(rng, P, n, (lo, hi))
    out = rng.normal(size=(n, 3))
    out /= np.linalg.norm(out, axis=1, keepdims=True)
    o = 0.5 * (lo + hi) + out * (1.5 * np.linalg.norm(hi - lo))
    return _two_forms(o, tg - o, rng)


# ---- rays for a corpus scene ---------------------------------------------------------------------------------------------------------
def corpus_rays(tris, n=64, n_hard=16, n_near=16, seed=5):
    """n rays from outside the bounds towards triangle centroids (both forms), then, from one eye point outside the bounds, rays through
    n_hard vertices and n_hard edge midpoints (as tests/test_gpu_query.py::test_hard_rays aims them), then n_near rays that start
    half a triangle's size off a triangle and point at it, so that nothing stands in between: the first four at input triangle 0,
    the one a `copies` soup repeats hundreds of times.  `tris` in INPUT order: the rays do not depend on who built the tree."""
    rng = np.random.default_rng([seed, len(tris)])
    P32 = tris["vertices"]["position"]
    P = P32.astype(np.float64)
    lo, hi = P.reshape(-1, 3).min(0), P.reshape(-1, 3).max(0)
    centre, radius = 0.5 * (lo + hi), 0.5 * float(np.linalg.norm(hi - lo))
    k = rng.integers(0, len(P), n)
    tg = P[k].mean(axis=1)
    out = rng.normal(size=(n, 3))
    out /= np.linalg.norm(out, axis=1, keepdims=True)
    o = centre + 1.5 * radius * out
    rays = _two_forms(o, tg - o, rng)
    eye = (centre + radius * np.array([1.3, 0.7, 0.9])).astype(F32)
    pick = rng.choice(len(P), n_hard, replace=False)
    with np.errstate(all="ignore"):
        v = [P32[t, 0] - eye for t in pick] + [F32(0.5) * (P32[t, 0] + P32[t, 1]) - eye for t in pick]
    hard = Q.make_rays(np.tile(eye, (2 * n_hard, 1)), np.stack(v))
    t = np.concatenate([np.zeros(4, dtype=np.int64), rng.integers(0, len(P), n_near - 4)])
    on = (P[t] * rng.dirichlet((2.0, 2.0, 2.0), n_near)[:, :, None]).sum(axis=1)
    nrm = np.cross(P[t, 1] - P[t, 0], P[t, 2] - P[t, 0])
    area = np.linalg.norm(nrm, axis=1)
    nrm = np.where((area > 0)[:, None], nrm / np.where(area > 0, area, 1.0)[:, None], np.array([0.0, 1.0, 0.0]))
    size = np.maximum(np.sqrt(area), 1e-3 * np.abs(P[t]).max(axis=(1, 2)))
    off = nrm * (0.5 * size * rng.choice([-1.0, 1.0], n_near))[:, None] + rng.normal(0.0, 0.05, (n_near, 3)) * size[:, None]
    near = _two_forms(on + off, -off, rng)
    return np.concatenate([rays, hard, near])


# ---- the model with its trace ----------------------------------------------------------------------------------------------------------
def trace(orc_lib, tris, nodes, rays, cull=False, margin=0.0, anyhit=False, tri_order=None):
    """query_model.per_ray with the event list of every ray -> (HIT records, occluded [n], per-ray counters, [events of ray i])"""
    tris, nodes = np.ascontiguousarray(tris), as_nodes(nodes)
    hits = np.zeros(len(rays), dtype=Q.HIT)
    words = hits.view(np.uint32).reshape(-1, 4)
    occ = np.zeros(len(rays), dtype=np.uint8)
    per = {k: np.zeros(len(rays), dtype=np.int64) for k in Q.PER_RAY + ("stack_overflows",)}
    events = []
    with np.errstate(all="ignore"):
        for i in range(len(rays)):
            c, ev = {}, []
            Q._record(words, occ, i, Q.traverse(orc_lib, tris, nodes, rays[i], cull, margin, anyhit, c, ev), tri_order)
            events.append(ev)
            for k in per:
                per[k][i] = c.get(k, 0)
    return hits, occ, per, events


def totals(per, n):
    """the five counters of a batch from its per-ray ones (query_model.COUNTERS)"""
    out = {k: int(per[k].sum()) for k in ("inner_steps", "tri_tests", "hits")}
    out.update(rays=n, max_stack=int(per["max_stack"].max()) if n else 0)
    return out


def leaf_events(events, node):
    """per ray: was leaf `node` stacked and popped, and was it entered without the stack -> (popped bool [n], entered bool [n],
    swapped flag of its pushes (set))"""
    popped = np.array([any(e[0] == "pop" and e[1] == node for e in ev) for ev in events])
    entered = np.array([any(e[0] == "enter" and e[1] == node for e in ev) for ev in events])
    swaps = {e[3] for ev in events for e in ev if e[0] == "push" and e[1] == node}
    return popped, entered, swaps


# ---- cameras ------------------------------------------------------------------------------------------------------------------------
def camera(position, target, half_width):
    """A CAMERA record at `position` whose central ray points at `target` and whose frame is 2 * half_width wide there: the rows of
    look_at that take the screen's x and y are scaled down, which the renderers multiply through like any other matrix.  A frame of
    24 x 16 pixels then covers a leaf a few units wide from thousands of units away."""
    from rust_ray_tracing_amd import _lib as L
    position, target = np.asarray(position, np.float64), np.asarray(target, np.float64)
    w = target - position
    dist = np.linalg.norm(w)
    w = w / dist
    r = np.cross([0.0, 1.0, 0.0], w)
    r /= np.linalg.norm(r)
    u = np.cross(w, r)
    c = np.zeros((), dtype=L.CAMERA)
    s = half_width / dist
    c["look_at"][0, :3], c["look_at"][1, :3], c["look_at"][2, :3] = (r * s).astype(F32), (u * s).astype(F32), w.astype(F32)
    c["look_at"][3, :3], c["look_at"][3, 3] = position.astype(F32), 1.0
    c["position"] = position.astype(F32)
    return c


def leaf_cameras(tris, nodes, m):
    """Two CAMERA records for a left / right scene: [0] beyond the far end of the remainder, looking through its box at the bunch (the
    pixels' rays meet the remainder's box first: the bunch is stacked); [1] close to the bunch on its other side (entered directly).
    For a root scene (one node): two sides of the bunch."""
    nd = as_nodes(nodes)
    if len(nd) == 1:
        lo, hi = nd["bounds_min"][0].astype(np.float64), nd["bounds_max"][0].astype(np.float64)
        c, size = 0.5 * (lo + hi), float(np.linalg.norm(hi - lo))
        return [camera(c + np.array([3.0, 0.4, 0.3]) * size, c, 0.45 * size), camera(c - np.array([2.5, -0.6, 0.5]) * size, c, 0.45 * size)]
    (blo, bhi), (rlo, rhi), _, _ = _boxes(tris, nodes, m)
    c, size = 0.5 * (blo + bhi), float(np.linalg.norm(bhi - blo))
    rc = 0.5 * (rlo + rhi)
    far = c + (rc - c) * 2.2
    near = c - (rc - c) / np.linalg.norm(rc - c) * (2.5 * size) + np.array([0.0, 0.3, -0.2]) * size
    return [camera(far, c, 0.5 * size), camera(near, c, 0.5 * size)]


CORE_VIEW = {"spiral": (1.1, 0.5, 0.8), "spiral_small": (0.9, -1.1, 0.7)}    # chosen on the CPU: from there the central ray hits a core
                                                                               # triangle (tests/test_traverse_cases_model.py asserts it)


def corpus_camera(tris, through_core=None, at_first=False):
    """One CAMERA record outside a corpus scene's bounds, the whole scene in its frame; or, `at_first`, close to input triangle 0.  `through_core` (a key of CORE_VIEW: the
    spirals, whose core of most of the triangles is a point at f32's resolution from outside the bounds): aimed at the median centroid, with a frame 2^-40
    of the distance wide, so that every pixel's ray is the central one to the last bit or two and goes down all the levels of the
    tree into the core -- the rays that reach the deepest stack."""
    P = tris["vertices"]["position"].astype(np.float64)
    if at_first:                                             # a `copies` soup: a fifth of its size off input triangle 0, the one it repeats, facing it
        nrm = np.cross(P[0, 1] - P[0, 0], P[0, 2] - P[0, 0])
        size = np.sqrt(np.linalg.norm(nrm))
        return camera(P[0].mean(axis=0) + nrm / np.linalg.norm(nrm) * (0.2 * size), P[0].mean(axis=0), 0.8 * size)
    lo, hi = P.reshape(-1, 3).min(0), P.reshape(-1, 3).max(0)
    c, size = 0.5 * (lo + hi), float(np.linalg.norm(hi - lo))
    position = c + np.array([1.1, 0.5, 0.8]) * size
    if through_core:
        position = c + np.array(CORE_VIEW[through_core]) * size
        target = np.median(P.mean(axis=1), axis=0)
        return camera(position, target, np.linalg.norm(target - position) * 2.0 ** -40)
    return camera(position, c, 0.4 * size)


# ---- the cases, made once and left unchanged -----------------------------------------------------------------------------------------
RAYS_PER_SCENE = {LEAF_SIZE_BIG: 40}                  # before family (d); 96 otherwise
CORPUS_RAYS = {"spiral": (24, 4, 8)}                  # (towards centroids, hard of each kind, near); (64, 16, 16) otherwise: a ray through
                                                      # the spiral's core tests all of its 5 000 triangles
_leaf_cases, _corpus_inputs = {}, {}


def leaf_case(rrt, orc, m, shape):
    """A leaf-form scene with the HOST builder's tree and its rays -> dict: sc (Scene, not uploaded), node (the bunch), first (its
    first triangle), rays, family (letter per ray; "r" throughout for a root scene), ref (the reference arm's `trace` of them)."""
    key = (m, shape)
    if key not in _leaf_cases:
        sc = rrt.Scene.from_arrays(leaf_tris(m, shape), materials())
        node = bunch_node(sc.bvh_nodes, m)
        lib = orc.load()
        if shape == "root":
            rays = root_rays(sc.tris)
            family = np.array(["r"] * len(rays))
        else:
            rays, family = leaf_rays(sc.tris, sc.bvh_nodes, m, RAYS_PER_SCENE.get(m, 96))
            rays, family = with_t_max(rays, family, trace(lib, sc.tris, sc.bvh_nodes, rays)[0])
        for a in (rays, family, sc.tris, sc.bvh_nodes):
            a.setflags(write=False)
        _leaf_cases[key] = dict(sc=sc, node=node, first=int(as_nodes(sc.bvh_nodes)["first_tri_or_child"][node]), rays=rays, family=family,
                                ref=trace(lib, sc.tris, sc.bvh_nodes, rays))
    return _leaf_cases[key]


def corpus_input(name):
    """(input triangles of corpus scene `name`, its rays), made once"""
    if name not in _corpus_inputs:
        tris = corpus_tris(name)
        rays = corpus_rays(tris, *CORPUS_RAYS.get(name, (64, 16, 16)))
        for a in (tris, rays):
            a.setflags(write=False)
        _corpus_inputs[name] = (tris, rays)
    return _corpus_inputs[name]


def in_bunch(case, hits, m):
    """bool [n]: the hit is a triangle of the bunch (tree order = the caller's on a host-built scene)"""
    prim = hits["prim"] & 0x01FFFFFF
    return (hits["prim"] != Q.NONE) & (prim >= case["first"]) & (prim < case["first"] + m)
