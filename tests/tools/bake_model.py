"""The models of include/mipt.h "baking" for tests/test_bake_abi.py, tests/test_bake_model.py, tests/test_gpu_bake.py and
tests/test_cpp_host_bake.py.

texels(): mipt_bake_texels in numpy f32 -- a brute force over ALL triangles of the caller's array per texel, every operator one
rounded f32 operation in the header's order.  texels_indexed(): the same definition stated a second time, over the (triangle,
texel) pairs that pass the box clause, for inputs of 10^6 triangles.  gather(): mipt_bake_gather as a Python loop over the oracle's orc_rand_in_unit_sphere
and orc_trace_ray_m / orc_trace_ray_wgsl_m (the one-ray entries with a cull margin and counters); the interpolation and `normalized` in numpy f32, the seed arithmetic in Python integers
(checked against orc_pixel_seed).  Nothing of the library under test is used here."""
import ctypes as C

import numpy as np

POINT = np.dtype([("seed", "<u4"), ("u", "<f4"), ("v", "<f4"), ("prim", "<u4")])       # MiptSurfacePoint
NONE, FRONT, TRI_MASK = 0xFFFFFFFF, 0x80000000, 0x01FFFFFF
M32 = (1 << 32) - 1
_F3 = C.c_float * 3
F = np.float32


def corner_uvs(tris):
    """[n, 3, 2] f32: tex_coord_x, tex_coord_y of vertices 0, 1, 2"""
    v = tris["vertices"]
    return np.stack([np.asarray(v["tex_coord_x"], dtype=np.float32), np.asarray(v["tex_coord_y"], dtype=np.float32)], axis=-1)


def texel_centres(width, height, index):
    """s, t of the texels `index` (u32 array): ((float)x + 0.5f) / (float)width, ((float)y + 0.5f) / (float)height"""
    index = np.asarray(index, dtype=np.uint32)
    x, y = index % np.uint32(width), index // np.uint32(width)
    s = (x.astype(np.float32) + F(0.5)) / F(width)
    t = (y.astype(np.float32) + F(0.5)) / F(height)
    return s, t


def texels(tris, width, height, index=None, box=True):
    """-> (points [len(index)] POINT, info dict).  tris: the caller's array, in the caller's order.  index: the texels wanted
    (default: all, in order).  info: covered (of the texels asked for) and degenerate (triangles whose d is 0 or not finite).
    box=False drops the box clause of "covered": NOT the header's definition, only what a test measures its inputs with (how
    many texels the clause decides)."""
    if index is None:
        index = np.arange(width * height, dtype=np.uint32)
    index = np.asarray(index, dtype=np.uint32)
    s, t = texel_centres(width, height, index)
    uv = corner_uvs(tris)
    out = np.zeros(len(index), dtype=POINT)
    out["seed"], out["prim"] = index, NONE
    free = np.ones(len(index), dtype=bool)
    with np.errstate(all="ignore"):
        # what depends on the triangle alone, for all of them at once (the loop below is what takes the time at 10^6 triangles)
        ax, ay = uv[:, 0, 0], uv[:, 0, 1]
        bx, by, cx, cy = uv[:, 1, 0] - ax, uv[:, 1, 1] - ay, uv[:, 2, 0] - ax, uv[:, 2, 1] - ay
        d = (bx * cy) - (cx * by)
        usable = np.isfinite(d) & (d != 0)
        lo = np.minimum(np.minimum(uv[:, 0], uv[:, 1]), uv[:, 2])           # [n, 2]; the corners of a usable triangle are no NaNs
        hi = np.maximum(np.maximum(uv[:, 0], uv[:, 1]), uv[:, 2])
        assert d.dtype == np.float32
        for k in np.flatnonzero(usable):                                    # ascending: the first to cover a texel keeps it
            if box:                                                         # the box clause first: most triangles hold no texel asked for
                sel = np.flatnonzero((s >= lo[k, 0]) & (s <= hi[k, 0]) & (t >= lo[k, 1]) & (t <= hi[k, 1]) & free)
            else:
                sel = np.flatnonzero(free)
            if len(sel) == 0:
                continue
            px, py = s[sel] - ax[k], t[sel] - ay[k]
            u = ((px * cy[k]) - (cx[k] * py)) / d[k]
            v = ((bx[k] * py) - (px * by[k])) / d[k]
            take = (u >= 0) & (v >= 0) & ((u + v) <= 1)
            if take.any():
                assert u.dtype == np.float32 and v.dtype == np.float32
                sel = sel[take]
                out["u"][sel], out["v"][sel], out["prim"][sel] = u[take], v[take], np.uint32(int(k) | FRONT)
                free[sel] = False
    return out, dict(covered=int((~free).sum()), degenerate=int((~usable).sum()))


def centre_lines(width, height):
    """the centres of the columns [width] and of the rows [height], by texel_centres' own expression"""
    return texel_centres(width, 1, np.arange(width))[0], texel_centres(1, height, np.arange(height))[1]


def boxes(tris, width, height):
    """Per triangle, the texel columns [x0, x1) and rows [y0, y1) whose f32 centre passes the box clause, and `usable` (d finite and
    not 0; the ranges of the others are empty): the centres are monotone in the texel index, so the clause is two binary searches
    per axis -- `left` for lo (the first centre >= lo), `right` for hi (one past the last centre <= hi).  Exact: no estimate."""
    uv = corner_uvs(tris)
    a, b, c = uv[:, 0], uv[:, 1], uv[:, 2]
    with np.errstate(all="ignore"):
        d = ((b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1])) - ((c[:, 0] - a[:, 0]) * (b[:, 1] - a[:, 1]))
        usable = np.isfinite(d) & (d != 0)
    cen_x, cen_y = centre_lines(width, height)
    assert np.all(np.diff(cen_x) >= 0) and np.all(np.diff(cen_y) >= 0)
    out = []
    for cen, axis in ((cen_x, 0), (cen_y, 1)):
        lo = np.minimum(np.minimum(a[:, axis], b[:, axis]), c[:, axis])
        hi = np.maximum(np.maximum(a[:, axis], b[:, axis]), c[:, axis])
        first = np.where(usable, np.searchsorted(cen, np.where(usable, lo, 0), "left"), 0)
        end = np.where(usable, np.searchsorted(cen, np.where(usable, hi, 0), "right"), 0)
        out += [first.astype(np.int64), np.maximum(end, first).astype(np.int64)]
    return out[0], out[1], out[2], out[3], usable


def _uv_of(uv, tri, s, t):
    """d, u, v of the pairs (triangle tri[i], centre s[i], t[i]): the header's expression tree, every operator one f32 operation"""
    ax, ay = uv[tri, 0, 0], uv[tri, 0, 1]
    bx, by, cx, cy = uv[tri, 1, 0] - ax, uv[tri, 1, 1] - ay, uv[tri, 2, 0] - ax, uv[tri, 2, 1] - ay
    d = (bx * cy) - (cx * by)
    px, py = s - ax, t - ay
    u = ((px * cy) - (cx * py)) / d
    v = ((bx * py) - (px * by)) / d
    assert u.dtype == np.float32 and v.dtype == np.float32
    return u, v


def texels_indexed(tris, width, height, chunk=1 << 22, stats=None):
    """texels() of every texel, stated a second time and fast enough for 10^6 triangles: the (triangle, texel) pairs that pass the box
    clause are enumerated from boxes() in ascending triangle order, at most `chunk` <= 2^24 at a time, u and v are evaluated on the
    pairs, and a texel goes to the first pair that covers it.  Nothing of the kernel's walk (its estimate of the box, its padding)
    is used.  stats, a dict, receives `pairs` and per-triangle `owned` counts.  tests/test_bake_model.py holds it to texels()."""
    assert 0 < chunk <= 1 << 24
    n_tex = width * height
    uv = corner_uvs(tris)
    x0, x1, y0, y1, usable = boxes(tris, width, height)
    nx = x1 - x0
    count = nx * (y1 - y0)
    end = np.cumsum(count)
    start = end - count
    total = int(end[-1]) if len(end) else 0
    cen_x, cen_y = centre_lines(width, height)
    owner = np.full(n_tex, -1, dtype=np.int64)
    with np.errstate(all="ignore"):
        for p0 in range(0, total, chunk):
            p1 = min(p0 + chunk, total)
            first, last = int(np.searchsorted(end, p0, "right")), int(np.searchsorted(end, p1 - 1, "right"))
            part = np.minimum(end[first: last + 1], p1) - np.maximum(start[first: last + 1], p0)
            tri = np.repeat(np.arange(first, last + 1), part)
            local = np.arange(p0, p1) - start[tri]
            x, y = x0[tri] + local % nx[tri], y0[tri] + local // nx[tri]
            u, v = _uv_of(uv, tri, cen_x[x], cen_y[y])
            cov = (u >= 0) & (v >= 0) & ((u + v) <= 1)
            tri, tex = tri[cov], (y * width + x)[cov]
            new = owner[tex] < 0                                            # earlier chunks hold lower triangles
            owner[tex[new][::-1]] = tri[new][::-1]                          # a repeated index keeps the LAST value assigned: the lowest triangle
    out = np.zeros(n_tex, dtype=POINT)
    out["seed"], out["prim"] = np.arange(n_tex, dtype=np.uint32), NONE
    has = np.flatnonzero(owner >= 0)
    s, t = texel_centres(width, height, has)
    with np.errstate(all="ignore"):
        out["u"][has], out["v"][has] = _uv_of(uv, owner[has], s, t)         # the same operations on the same operands as in the loop
    out["prim"][has] = owner[has].astype(np.uint32) | np.uint32(FRONT)
    if stats is not None:
        stats["pairs"], stats["owned"] = total, np.bincount(owner[has], minlength=len(uv))
    return out, dict(covered=len(has), degenerate=int((~usable).sum()))


def sliver_uvs(width, height, n, k, seed):
    """[n, 3, 2] f32: slivers laid ALONG LINES OF TEXEL CENTRES, so that centres outside a sliver's box fall within rounding noise of
    its line and only the box clause keeps them out.  Corner a is the centre (x0, y0), b the centre (x0 + m, y0 +- m), c the centre
    (x0 + j, y0 +- j) between them with each coordinate's bit pattern moved by -k ... +k ulps; m in 3 ... min(width, height) / 4,
    x0, y0 in the middle half of the atlas, 0 < j < m, either diagonal.  (Random slivers off the centre lines are decided by the
    clause on no texel at all.)"""
    rng = np.random.default_rng(seed)
    cen_x, cen_y = centre_lines(width, height)
    m = rng.integers(3, min(width, height) // 4 + 1, n)
    x0 = rng.integers(width // 4, width - width // 4, n)
    y0 = rng.integers(height // 4, height - height // 4, n)
    j = rng.integers(1, m)
    sign = np.where(rng.random(n) < 0.5, 1, -1)
    uv = np.zeros((n, 3, 2), dtype=np.float32)
    for corner, step in ((0, 0 * m), (1, m), (2, j)):
        uv[:, corner, 0], uv[:, corner, 1] = cen_x[x0 + step], cen_y[y0 + sign * step]
    moved = uv[:, 2].view(np.int32) + rng.integers(-k, k + 1, (n, 2)).astype(np.int32)      # positive floats: + 1 is the next one up
    uv[:, 2] = moved.view(np.float32)
    return uv


def sample_seed(seed, g, stride):
    """rng of sample g of a point: cpu.rs:28-29 with the point as the pixel and the sample as the frame, 1 in place of 0"""
    return (987612486 * ((int(seed) + (int(g) & M32) * int(stride) + 87636354) & M32)) & M32 or 1


def _normalized(a):
    length = np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])             # vec3.rs:93-97, f32 throughout
    return a / length                                                        # vec3.rs:105-109


def surface(tris, point):
    """P, N of one point on the caller's triangles, f32 [3] each (include/mipt.h "mipt_bake_gather")"""
    k = int(point["prim"]) & TRI_MASK
    pos = np.asarray(tris["vertices"]["position"][k], dtype=np.float32)
    nrm = np.asarray(tris["vertices"]["normal"][k], dtype=np.float32)
    u, v = F(point["u"]), F(point["v"])
    e1, e2 = pos[1] - pos[0], pos[2] - pos[0]                               # ray.rs:24-25
    P = (pos[0] + e1 * u) + e2 * v
    w = (F(1.0) - u) - v                                                    # ray.rs:45
    N = (nrm[0] * w + nrm[1] * u) + nrm[2] * v
    if not int(point["prim"]) & FRONT:
        N = -N                                                              # ray.rs:46-48
    assert P.dtype == np.float32 and N.dtype == np.float32
    return P, N


class Gather:
    """The scene as the oracle takes it (sc.tris and sc.bvh_nodes in the TREE's order) and the caller's triangle array, kept alive.

    Counters.  Every path of a real point is one call of the one-ray entry, counted as that entry counts.  A path of a MIPT_HIT_NONE
    point is "a ray that misses" (include/mipt.h): bake_rays_kernel writes it as a placeholder ray -- origin 0, direction (NaN, NaN,
    NaN), seed 1 -- and the trace loop runs it like any other.  Every slab quotient of it is a NaN and every triangle test's t is one,
    so it counts one ray, the one step at the root (one inner step, or the root's triangle tests where the root is a leaf), no hit and
    no texel fetch, whatever the depth, the shading or the traversal.  The model states this by handing that very ray to the oracle."""

    def __init__(self, orc, sc, caller_tris):
        self.orc, self.lib = orc, orc.load()
        self.tris, self.nodes = np.ascontiguousarray(sc.tris), np.ascontiguousarray(sc.bvh_nodes)
        self.mats = np.ascontiguousarray(sc.materials_array())
        self.texs = [np.ascontiguousarray(t) for t in sc.textures]
        self.tex_array = orc._tex_array(self.texs)
        self.caller = np.ascontiguousarray(caller_tris)
        assert len(self.caller) == len(self.tris)

    def run(self, points, samples, depth, shading=0, cull=0, first_sample=0, stride=None, margin=0.0):
        """-> dict: "sum" [n, 3] f32 (the samples added in order from +0), "mean" [n, 3] f32 (sum / f32(samples); 0 for a point
        without a surface, like the sum), "first_hit" [n, samples] bool (the first scatter ray hit something; False for no point) and
        "counters" [n, 5] int64 in the order of radiance_model.COUNTERS.  margin: the culled traversal's cull_margin."""
        lib, n = self.lib, len(points)
        stride = n if stride is None else stride
        args = (self.tris.ctypes.data, self.tris.nbytes // 112, self.nodes.ctypes.data, self.nodes.nbytes // 32, self.mats.ctypes.data,
                self.mats.nbytes // 80, self.tex_array, len(self.texs))
        total = np.zeros((n, 3), dtype=np.float32)
        first_hit = np.zeros((n, samples), dtype=bool)
        counters = np.zeros((n, 5), dtype=np.int64)
        out, rs, cnt = _F3(), _F3(), (C.c_uint64 * 5)()
        entry = lib.orc_trace_ray_m if shading == 0 else lib.orc_trace_ray_wgsl_m
        nan = float("nan")
        with np.errstate(all="ignore"):
            for i in range(n):
                if int(points["prim"][i]) == NONE:
                    o, d, st = _F3(0.0, 0.0, 0.0), _F3(nan, nan, nan), C.c_uint32(1)             # the placeholder ray (class docstring)
                    entry(*args, C.byref(o), C.byref(d), depth, C.byref(st), cull, C.c_float(margin), self.orc.LIBM_GLIBC235, C.byref(out), C.byref(cnt))
                    assert cnt[0] == 1 and cnt[3] == 0 and cnt[4] == 0 and cnt[1] + cnt[2] > 0
                    counters[i] = samples * np.array(list(cnt), dtype=np.int64)
                    continue
                P, N = surface(self.caller, points[i])
                acc = np.zeros(3, dtype=np.float32)
                for s in range(samples):
                    g = (first_sample + s) & M32
                    rng = sample_seed(points["seed"][i], g, stride)
                    assert rng == (lib.orc_pixel_seed((int(points["seed"][i]) + g * stride) & M32) or 1)
                    st = C.c_uint32(rng)
                    lib.orc_rand_in_unit_sphere(C.byref(st), self.orc.LIBM_GLIBC235, C.byref(rs))
                    new_dir = _normalized(N + np.array(list(rs), dtype=np.float32))            # ray.rs:179-180
                    origin = P + new_dir * F(0.0001)                                             # ray.rs:181
                    o, d = _F3(*[float(x) for x in origin]), _F3(*[float(x) for x in new_dir])
                    probe = C.c_uint32(st.value)                                                 # the first segment alone: did it hit?
                    lib.orc_trace_ray_wgsl(*args, C.byref(o), C.byref(d), 1, C.byref(probe), 0, self.orc.LIBM_GLIBC235, C.byref(out), C.byref(cnt))
                    first_hit[i, s] = cnt[3] > 0
                    entry(*args, C.byref(o), C.byref(d), depth, C.byref(st), cull, C.c_float(margin), self.orc.LIBM_GLIBC235, C.byref(out), C.byref(cnt))
                    counters[i] += np.array(list(cnt), dtype=np.int64)
                    acc = acc + np.array(list(out), dtype=np.float32)                            # f32 + f32, rounded once
                total[i] = acc
        none = points["prim"] == NONE
        mean = total / F(samples)
        mean[none] = 0
        return dict(sum=total, mean=mean, first_hit=first_hit, counters=counters)


def conditions(model_out, points):
    """What every scene-backed gather case asserts of the MODEL's output before anything is compared with it"""
    for k in ("sum", "mean"):
        assert not np.any(np.isnan(model_out[k])), k
    real = points["prim"] != NONE
    hits, n = int(model_out["first_hit"][real].sum()), int(real.sum()) * model_out["first_hit"].shape[1]
    assert 4 * hits >= n, (hits, n)                                          # at least a quarter of the first scatter rays hit
    assert 10 * (n - hits) >= n, (n - hits, n)                               # at least a tenth escape


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()
