"""Hard inputs for the three entries whose caller hands over a path's first segment: rays for mipt_query_radiance, surface points for
mipt_bake_gather, probes for mipt_probe_bake.  Pure numpy, shared by tests/test_hard_inputs_model.py (CPU: the models alone),
tests/test_gpu_radiance_hard.py, tests/test_gpu_bake_hard.py and tests/test_gpu_probe_hard.py.  Every input is legal per
include/mipt.h; the oracle decides what each is worth.

hard_rays():  both sides of every boundary of ray_safe (csrc/pt_traverse.h: |d| in [2^-60, 2], |o| <= 2^40, |o| >= 2^-70 or 0), zero,
denormal, huge and non-finite components, rays in a triangle's plane and rays through vertices and edges, with the seeds 0 (the
stuck stream), 1, 0x80000000 and 0xffffffff among the default ones.  hard_points(): barycentrics that are no barycentrics, normals
that cannot be normalised, a zero-area triangle, the seeds at which the sample seed formula gives 0, prim words with the ignored
bits set, the first and the last triangle, and no point in between.  hard_probes(): an origin on both sides of every origin
clause of the guard, shared by all of a probe's samples, and origins on vertices, edges, triangles, node planes and corners."""
import numpy as np

from bake_model import FRONT, NONE, POINT, TRI_MASK, M32
from radiance_model import RAY, default_seeds

F = np.float32
CULL_MARGIN_SAFE = 2.0 ** -7                    # MIPT_CULL_MARGIN_SAFE

DIR_SPECIALS = [("0", 0.0), ("-0", -0.0), ("1e-42", 1e-42), ("2^-70", 2.0 ** -70), ("2^-61", 2.0 ** -61), ("2^-60", 2.0 ** -60), ("2", 2.0),
                ("next(2)", float(np.nextafter(F(2), F(3)))), ("4", 4.0), ("2^100", 2.0 ** 100), ("nan", np.nan), ("+inf", np.inf), ("-inf", -np.inf)]
ORIGIN_SMALL = [("2^-71", 2.0 ** -71), ("2^-70", 2.0 ** -70), ("1e-42", 1e-42)]
ORIGIN_BIG = [("2^40", 2.0 ** 40), ("next(2^40)", float(np.nextafter(F(2.0 ** 40), F(np.inf)))), ("2^41", 2.0 ** 41)]
ORIGIN_BAD = [("nan", np.nan), ("+inf", np.inf), ("-inf", -np.inf)]
HARD_SEEDS = (0, 1, 0x80000000, 0xFFFFFFFF)
N_PLANE, N_AIMED = 8, 24

RAY_CLASSES = ([f"d{'xyz'[a]}={n}" for n, _ in DIR_SPECIALS for a in range(3)] + ["d=0"] +
               [f"o{'xyz'[a]}={n}" for n, _ in ORIGIN_SMALL + ORIGIN_BIG + ORIGIN_BAD for a in range(3)] +
               [f"plane{k}" for k in range(N_PLANE)] + [f"{w}{k}" for k in range(N_AIMED) for w in ("vertex", "edge01_", "edge12_")])


def _keeps_sign(value):
    return np.isfinite(value) and value != 0.0


def hard_rays(tris, eye, seed):
    """-> (rays [147] RAY, tags [147] of str, one of RAY_CLASSES each).  tris: the scene's triangles; eye: a point outside the
    geometry that sees it; seed: picks the triangles of the in-plane and the aimed rays.  t_max is 0: the radiance entry ignores it."""
    P = np.asarray(tris["vertices"]["position"], dtype=np.float32)
    eye = np.asarray(eye, dtype=np.float32)
    flat = P.reshape(-1, 3)
    lo, hi = flat.min(0), flat.max(0)
    centre = ((lo + hi) * F(0.5)).astype(np.float32)
    skew = (hi - lo) * np.float32([0.013, -0.027, 0.041])
    base = (centre - eye) + skew                                                    # towards the scene, no component 0
    base = (base / np.abs(base).max()).astype(np.float32)                           # the largest component is 1: inside ray_safe's range
    assert np.all(np.abs(base) >= 2.0 ** -20)
    rng = np.random.default_rng(seed)
    pick = rng.choice(len(P), N_AIMED, replace=len(P) < N_AIMED)          # the cornell box has 12 triangles
    o, d, tags = [], [], []

    def add(tag, oo, dd):
        tags.append(tag); o.append(np.asarray(oo, dtype=np.float32)); d.append(np.asarray(dd, dtype=np.float32))
    with np.errstate(all="ignore"):
        for name, value in DIR_SPECIALS:
            for axis in range(3):
                dd = base.copy()
                dd[axis] = np.copysign(F(value), base[axis]) if _keeps_sign(value) else F(value)
                add(f"d{'xyz'[axis]}={name}", eye, dd)
        add("d=0", eye, (0.0, 0.0, 0.0))
        for name, value in ORIGIN_SMALL:                                            # the eye with one tiny coordinate, aimed at the centre
            for axis in range(3):
                oo = eye.copy(); oo[axis] = F(value)
                dd = (centre - oo) + skew
                add(f"o{'xyz'[axis]}={name}", oo, dd / np.abs(dd).max())
        for name, value in ORIGIN_BIG:                                              # far out on one axis, aimed back: the tilt keeps every
            for axis in range(3):                                                   # direction component inside [2^-60, 2]
                oo = centre.copy(); oo[axis] = F(value)
                dd = np.float32([2.0 ** -45, -(2.0 ** -45), 2.0 ** -45]); dd[axis] = F(-1.0)
                add(f"o{'xyz'[axis]}={name}", oo, dd)
        for name, value in ORIGIN_BAD:
            for axis in range(3):
                oo = eye.copy(); oo[axis] = F(value)
                add(f"o{'xyz'[axis]}={name}", oo, base)
        for k, t in enumerate(pick[:N_PLANE]):                                      # in the plane of a triangle (det = 0 up to rounding)
            v0, v1, v2 = P[t]
            add(f"plane{k}", v0 - (v1 - v0), (v1 - v0) + F(0.5) * (v2 - v0))
        for k, t in enumerate(pick):                                                # through a vertex and two edge midpoints; the edge rays
            v0, v1, v2 = P[t]                                                       # scaled by a power of two into the guard's range
            add(f"vertex{k}", eye, v0 - eye)
            add(f"edge01_{k}", eye, ((F(0.5) * (v0 + v1)) - eye) * F(0.125)); add(f"edge12_{k}", eye, ((F(0.5) * (v1 + v2)) - eye) * F(0.125))
    n = len(tags)
    assert tags == RAY_CLASSES
    rays = np.zeros(n, dtype=RAY)
    rays["origin"], rays["direction"] = np.stack(o), np.stack(d)
    rays["reserved"] = default_seeds(n, first=70000)
    first_aimed = n - 3 * N_AIMED                                                   # the hard seeds go to rays that see the scene
    for k, s in enumerate(HARD_SEEDS):
        rays["reserved"][first_aimed + 1 + 17 * k] = s
    return rays, np.array(tags)


RAY_SEED = 31                                   # hard_rays' seed in every test, so that the CPU test sees the GPU tests' rays


def eye_for(tris, kind):
    """the eye of hard_rays for the scene kinds of tests/test_gpu_radiance.py: inside the cornell box, whose walls face inwards, and
    outside the others"""
    if kind != "cornell":
        return np.float32([3.0, 0.55, 0.0])
    P = np.asarray(tris["vertices"]["position"], dtype=np.float32).reshape(-1, 3)
    lo, hi = P.min(0), P.max(0)
    return (lo + (hi - lo) * np.float32([0.31, 0.57, 0.23])).astype(np.float32)


def ray_safe(rays, tiny_axes=0):
    """bool [n]: ray_safe of csrc/pt_traverse.h restated -- the rays whose FIRST segment takes the fast quotient"""
    o, d = np.asarray(rays["origin"], dtype=np.float32), np.asarray(rays["direction"], dtype=np.float32)
    with np.errstate(all="ignore"):
        ok = np.all((np.abs(d) >= F(2.0 ** -60)) & (np.abs(d) <= F(2.0)), axis=1) & np.all(np.abs(o) <= F(2.0 ** 40), axis=1)
    m = np.ascontiguousarray(o).view(np.uint32) & np.uint32(0x7FFFFFFF)
    zero_ok = np.array([not tiny_axes & 1, not tiny_axes & 2, not tiny_axes & 4])
    return ok & np.all((m >= np.uint32(0x1C800000)) | ((m == 0) & zero_ok[None, :]), axis=1)


def spread(hard, pool):
    """one hard ray per four pool rays (h p p p p h p p p p ...): every wave holds lanes on both quotient paths.  -> (rays, the
    indices of the hard rays, the indices of the pool rays); needs 4 len(hard) pool rays"""
    n = len(hard)
    assert len(pool) >= 4 * n
    out = np.zeros(5 * n, dtype=hard.dtype)                                       # rays, or the probes of hard_probes
    at = 5 * np.arange(n)
    rest = np.setdiff1d(np.arange(5 * n), at)
    out[at], out[rest] = hard, pool[: 4 * n]
    return out, at, rest


def splice(pool, hard, stride):
    """the pool with hard[k] spliced in at index k * stride of the result: -> (rays, index of every hard ray, index of every pool ray)"""
    n = len(pool) + len(hard)
    assert stride > 1 and (len(hard) - 1) * stride < n
    at = np.arange(len(hard)) * stride
    rest = np.setdiff1d(np.arange(n), at)
    out = np.zeros(n, dtype=RAY)
    out[at], out[rest] = hard, pool
    return out, at, rest


# ---- surface points -------------------------------------------------------------------------------------------------------------------
SPECIAL_KINDS = ("zero_normals", "nan_corner_normal", "huge_normals", "tiny_normals", "zero_area")
_NAN, _INF = np.nan, np.inf
UV_SPECIALS = [(_NAN, .2), (.2, _NAN), (_INF, .1), (.1, -_INF), (1e30, 0.0), (-.5, .25), (2.0, 2.0), (0.0, 0.0), (-0.0, -0.0), (1.0, 0.0), (0.0, 1.0),
               (.5, .5), (1e-42, 1e-42), (3e38, 3e38)]
ZERO_SEEDS = ((1 << 31) - 87636354, (1 << 32) - 87636354)        # 987612486 = 2 x an odd number: the formula is 0 iff seed + g stride + 87636354 = 0 mod 2^31
HARD_FIRST_SAMPLE, HARD_STRIDE = 5, 0x30000001                   # the options the "late zero" point is made for: g = 6 is its second sample there
LATE_ZERO_SEED = (ZERO_SEEDS[0] - ((6 * HARD_STRIDE) & M32)) & M32
PRIM_JUNK = 0x7E000000                                           # bits 25 ... 30: ignored by the entry


def with_special_triangles(tris):
    """-> (a copy of tris in which five triangles carry SPECIAL_KINDS' normals and positions, their five indices)"""
    t = np.ascontiguousarray(tris).copy()
    n = len(t)
    assert n >= 64
    idx = np.array([(k + 1) * n // 7 + 1 for k in range(5)])
    nrm, pos = t["vertices"]["normal"], t["vertices"]["position"]
    nrm[idx[0]] = 0.0
    nrm[idx[1], 1] = np.nan
    nrm[idx[2]] = 1e30
    nrm[idx[3]] = np.float32([1e-30, -1e-30, 1e-30])
    pos[idx[4], 2] = pos[idx[4], 1]                                                 # a segment: edge_2 == edge_1, area exactly 0
    return t, idx


def find_special(tris):
    """the indices of with_special_triangles' five triangles in `tris`, in SPECIAL_KINDS' order, found by what they carry -- for an
    array that a builder has reordered since"""
    nrm, pos = np.asarray(tris["vertices"]["normal"]), np.asarray(tris["vertices"]["position"])
    flat = nrm.reshape(len(nrm), -1)
    with np.errstate(all="ignore"):
        found = [np.flatnonzero(~flat.any(axis=1)), np.flatnonzero(np.isnan(flat).any(axis=1)), np.flatnonzero((flat == F(1e30)).all(axis=1)),
                 np.flatnonzero((np.abs(flat) == F(1e-30)).all(axis=1)), np.flatnonzero((pos[:, 2] == pos[:, 1]).all(axis=1))]
    assert [len(f) for f in found] == [1] * 5, [len(f) for f in found]
    return np.array([int(f[0]) for f in found])


def hard_points(caller_tris, special):
    """-> (points POINT, tags of str).  caller_tris: the array in the caller's order; special: with_special_triangles' indices into
    it.  A MIPT_HIT_NONE record follows every sixth point."""
    n = len(caller_tris)
    special = [int(k) for k in special]
    sound = [k for k in (n // 3, n // 2 + 5) if k not in special]
    assert len(sound) == 2 and len(special) == len(SPECIAL_KINDS) and 0 not in special and n - 1 not in special
    rec, tags = [], []

    def add(tag, seed, u, v, prim):
        rec.append((int(seed) & M32, F(u), F(v), int(prim) & M32)); tags.append(tag)
    with np.errstate(all="ignore"):
        for kind, k in zip(SPECIAL_KINDS, special):
            add(kind + ":front", 11 + k, .3, .3, k | FRONT); add(kind + ":back", 12 + k, .3, .3, k)
        for j, k in enumerate(sound):
            for i, (u, v) in enumerate(UV_SPECIALS):
                add(f"uv{i}", 100 * j + i, u, v, k | (FRONT if (i + j) % 2 else 0))
        add("zero_seed0", ZERO_SEEDS[0], .25, .25, sound[0] | FRONT); add("zero_seed1", ZERO_SEEDS[1], .25, .25, sound[1])
        add("late_zero_seed", LATE_ZERO_SEED, .25, .5, sound[0] | FRONT)
        add("seed_ffffffff", 0xFFFFFFFF, .5, .25, sound[1] | FRONT)
        add("prim_junk:front", 41, .2, .3, sound[0] | PRIM_JUNK | FRONT); add("prim_junk:back", 42, .2, .3, sound[1] | PRIM_JUNK)
        add("tri0:front", 43, .3, .2, 0 | FRONT); add("tri0:back", 44, .3, .2, 0)
        add("tri_last:front", 45, .6, .2, (n - 1) | FRONT); add("tri_last:back", 46, .6, .2, n - 1)
    out, out_tags = [], []
    for i, (r, t) in enumerate(zip(rec, tags)):
        out.append(r); out_tags.append(t)
        if i % 6 == 5:
            out.append((1000 + i, F(.1), F(.1), NONE)); out_tags.append("none")
    pts = np.array(out, dtype=POINT)
    assert not np.any((pts["prim"] != NONE) & ((pts["prim"] & TRI_MASK) >= n))
    return pts, np.array(out_tags)


POINT_CLASSES = ([k + s for k in SPECIAL_KINDS for s in (":front", ":back")] + [f"uv{i}" for i in range(len(UV_SPECIALS))] +
                 ["zero_seed0", "zero_seed1", "late_zero_seed", "seed_ffffffff", "prim_junk:front", "prim_junk:back", "tri0:front", "tri0:back",
                  "tri_last:front", "tri_last:back", "none"])


def interleave(a, b):
    """a[0] b[0] a[1] b[1] ... then what is left of the longer: -> (array, indices of a's items, indices of b's items)"""
    m = min(len(a), len(b))
    n = len(a) + len(b)
    ia = np.concatenate([2 * np.arange(m), np.arange(2 * m, 2 * m + len(a) - m)]).astype(np.int64)
    ib = np.setdiff1d(np.arange(n), ia)
    out = np.zeros(n, dtype=a.dtype)
    out[ia], out[ib] = a, b
    return out, ia, ib


# ---- probes ---------------------------------------------------------------------------------------------------------------------------
# A probe is the origin of all its samples' first segments: with s samples it puts s consecutive lanes of the ray kernel on the same
# side of ray_safe's origin clauses (the directions are unit vectors as drawn, and pass theirs).
PROBE = np.dtype([("position", "<f4", 3), ("seed", "<u4")])       # MiptProbe (probe_model.PROBE)
PROBE_AXIS_VALUES = ORIGIN_SMALL + ORIGIN_BIG + ORIGIN_BAD + [("0", 0.0), ("-0", -0.0)]
N_PROBE_TRIS, N_PROBE_PLANES, N_PROBE_CORNERS = 6, 6, 4
PROBE_CLASSES = ([f"p{'xyz'[a]}={n}" for n, _ in PROBE_AXIS_VALUES for a in range(3)] + ["p=0", "p=2^-71"] +
                 [f"{w}{k}" for k in range(N_PROBE_TRIS) for w in ("on_vertex", "on_edge", "on_centroid")] +
                 [f"on_node_plane{k}" for k in range(N_PROBE_PLANES)] + [f"on_corner{k}" for k in range(N_PROBE_CORNERS)])
PROBE_SEED = 41                                 # hard_probes' seed in every test, so that the CPU test sees the GPU tests' probes


def hard_probes(tris, nodes, seed):
    """-> (probes [63] PROBE, tags [63] of str, PROBE_CLASSES in order).  tris, nodes: the scene's triangles and its mirrored tree;
    seed: picks the triangles, the inner nodes and the corners.  Per axis every value of PROBE_AXIS_VALUES with the other two
    coordinates inside the scene; all three coordinates 0 and 2^-71; on a vertex, on an edge's midpoint and at the f32 centroid of
    some triangles; on a bounding plane of an inner node; on a corner of the scene's bounds.  Seeds 13 i + 7 but for HARD_SEEDS, both
    ZERO_SEEDS and LATE_ZERO_SEED (whose second sample under HARD_FIRST_SAMPLE / HARD_STRIDE runs on stream 1), which go to probes
    on geometry."""
    P = np.asarray(tris["vertices"]["position"], dtype=np.float32)
    flat = P.reshape(-1, 3)
    lo, hi = flat.min(0), flat.max(0)
    centre = ((lo + hi) * F(0.5)).astype(np.float32)
    inside = (centre + np.clip((hi - lo) * np.float32([0.11, 0.17, -0.13]), F(-0.5), F(0.5))).astype(np.float32)
    assert np.all(inside > lo) and np.all(inside < hi) and np.all(np.abs(inside) >= 2.0 ** -20)
    rng = np.random.default_rng(seed)
    pick = rng.choice(len(P), N_PROBE_TRIS, replace=False)
    inner = np.flatnonzero(np.asarray(nodes["num_tris"]) == 0)
    assert len(inner) >= N_PROBE_PLANES
    pick_nodes = rng.choice(inner, N_PROBE_PLANES, replace=False)
    pick_corners = rng.choice(8, N_PROBE_CORNERS, replace=False)
    pos, tags = [], []

    def add(tag, p):
        tags.append(tag); pos.append(np.asarray(p, dtype=np.float32))
    for name, value in PROBE_AXIS_VALUES:
        for axis in range(3):
            p = inside.copy(); p[axis] = F(value)
            add(f"p{'xyz'[axis]}={name}", p)
    add("p=0", (0.0, 0.0, 0.0)); add("p=2^-71", (2.0 ** -71,) * 3)
    for k, t in enumerate(pick):
        v0, v1, v2 = P[t]
        add(f"on_vertex{k}", (v0, v1, v2)[k % 3]); add(f"on_edge{k}", F(0.5) * ((v0, v1, v2)[k % 3] + (v0, v1, v2)[(k + 1) % 3]))
        add(f"on_centroid{k}", ((v0 + v1) + v2) / F(3.0))
    for k, j in enumerate(pick_nodes):                                              # the middle of the node's box, moved onto one of its six planes
        b0, b1 = np.asarray(nodes["bounds_min"][j], dtype=np.float32), np.asarray(nodes["bounds_max"][j], dtype=np.float32)
        p = ((b0 + b1) * F(0.5)).astype(np.float32)
        p[k % 3] = (b0, b1)[(k // 3) % 2][k % 3]
        add(f"on_node_plane{k}", p)
    for k, c in enumerate(pick_corners):
        add(f"on_corner{k}", [(lo, hi)[(c >> a) & 1][a] for a in range(3)])
    n = len(tags)
    assert tags == PROBE_CLASSES
    probes = np.zeros(n, dtype=PROBE)
    probes["position"] = np.stack(pos)
    probes["seed"] = 13 * np.arange(n, dtype=np.uint32) + 7
    first = tags.index("on_vertex0")
    for k, s in enumerate(HARD_SEEDS + ZERO_SEEDS + (LATE_ZERO_SEED,)):             # on_vertex0, on_edge0, on_centroid0, on_vertex1, ...
        probes["seed"][first + k] = s
    return probes, np.array(tags)


def tiny_plane_probes(copies=3):
    """the origins of tests/test_gpu_radiance_hard.py::test_hard_rays_on_a_scene_with_tiny_planes as probes: a coordinate of 0, 2^-71
    or 2^-70 on each axis and on two pairs of axes, the rest of (0.5, -2, -7); `copies` probes of each with seeds of their own"""
    o = []
    for value in (0.0, 2.0 ** -71, 2.0 ** -70):
        for axis in range(3):
            oo = np.float32([0.5, -2.0, -7.0]); oo[axis] = value; o.append(oo)
        o.append(np.float32([value, -2.0, value])); o.append(np.float32([value, value, -7.0]))
    probes = np.zeros(len(o) * copies, dtype=PROBE)
    probes["position"] = np.tile(np.stack(o), (copies, 1))
    probes["seed"] = 29 * np.arange(len(probes), dtype=np.uint32) + 300
    return probes


def probe_rays(probes, dirs):
    """the first segments of a bake as RAY records, for ray_safe: probes [n], dirs [n, samples, 3] -> [n * samples]"""
    dirs = np.asarray(dirs, dtype=np.float32)
    rays = np.zeros(dirs.shape[0] * dirs.shape[1], dtype=RAY)
    rays["origin"] = np.repeat(np.asarray(probes["position"], dtype=np.float32), dirs.shape[1], axis=0)
    rays["direction"] = dirs.reshape(-1, 3)
    return rays


def origin_safe(probes, tiny_axes=0):
    """bool [n]: the probes whose position passes ray_safe's origin clauses"""
    return ray_safe(probe_rays(probes, np.ones((len(probes), 1, 3), dtype=np.float32)), tiny_axes)


# ---- comparisons and what the model must show before anything is compared with it -----------------------------------------------------
def _words(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32), np.isnan(a.view(np.float32))


def differing(a, b):
    """bool array of a's shape: the f32 words that differ, two NaNs counting as equal.  IEEE 754 leaves the sign and payload of a NaN
    an operation PRODUCES to the implementation (x86 SSE and gfx950 differ); everything else is compared bit for bit."""
    (wa, na), (wb, nb) = _words(a), _words(b)
    assert wa.shape == wb.shape, (wa.shape, wb.shape)
    return (wa != wb) & ~(na & nb)


def same_bits_or_both_nan(a, b):
    return not differing(a, b).any()


def bad_rows(got, want):
    bad = np.flatnonzero(differing(got, want).reshape(len(want), -1).any(axis=1))
    g, w = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    return len(bad), [(int(i), g[i].tolist(), w[i].tolist()) for i in bad[:4]]


def nan_rows(x):
    return int(np.isnan(np.asarray(x)).reshape(len(x), -1).any(axis=1).sum())


def few_nan_rows(model_out):
    """at most a tenth of the model's rows are NaN: a comparison that counts two NaNs as equal still compares numbers"""
    for k in ("sum", "mean"):
        assert 10 * nan_rows(model_out[k]) <= len(model_out[k]), (k, nan_rows(model_out[k]), len(model_out[k]))
