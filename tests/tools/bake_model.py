"""The models of include/mipt.h "baking" for tests/test_bake_abi.py, tests/test_gpu_bake.py and tests/test_cpp_host_bake.py.

texels(): mipt_bake_texels in numpy f32 -- a brute force over ALL triangles of the caller's array per texel, every operator one
rounded f32 operation in the header's order.  gather(): mipt_bake_gather as a Python loop over the oracle's orc_rand_in_unit_sphere
and orc_trace_ray / orc_trace_ray_wgsl; the interpolation and `normalized` in numpy f32, the seed arithmetic in Python integers
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


def texels(tris, width, height, index=None):
    """-> (points [len(index)] POINT, info dict).  tris: the caller's array, in the caller's order.  index: the texels wanted
    (default: all, in order).  info: covered (of the texels asked for) and degenerate (triangles whose d is 0 or not finite)."""
    if index is None:
        index = np.arange(width * height, dtype=np.uint32)
    index = np.asarray(index, dtype=np.uint32)
    s, t = texel_centres(width, height, index)
    uv = corner_uvs(tris)
    out = np.zeros(len(index), dtype=POINT)
    out["seed"], out["prim"] = index, NONE
    free = np.ones(len(index), dtype=bool)
    degenerate = 0
    with np.errstate(all="ignore"):
        for k in range(len(uv)):                                            # ascending: the first to cover a texel keeps it
            a, b, c = uv[k]
            bx, by, cx, cy = b[0] - a[0], b[1] - a[1], c[0] - a[0], c[1] - a[1]
            d = (bx * cy) - (cx * by)
            if not (np.isfinite(d) and d != 0):
                degenerate += 1
                continue
            px, py = s - a[0], t - a[1]
            u = ((px * cy) - (cx * py)) / d
            v = ((bx * py) - (px * by)) / d
            lo_x, hi_x = min(a[0], b[0], c[0]), max(a[0], b[0], c[0])
            lo_y, hi_y = min(a[1], b[1], c[1]), max(a[1], b[1], c[1])
            cov = (u >= 0) & (v >= 0) & ((u + v) <= 1) & (s >= lo_x) & (s <= hi_x) & (t >= lo_y) & (t <= hi_y)
            take = cov & free
            if take.any():
                assert u.dtype == np.float32 and v.dtype == np.float32
                out["u"][take], out["v"][take], out["prim"][take] = u[take], v[take], np.uint32(k | FRONT)
                free &= ~take
    return out, dict(covered=int((~free).sum()), degenerate=degenerate)


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
    """The scene as the oracle takes it (sc.tris and sc.bvh_nodes in the TREE's order) and the caller's triangle array, kept alive"""

    def __init__(self, orc, sc, caller_tris):
        self.orc, self.lib = orc, orc.load()
        self.tris, self.nodes = np.ascontiguousarray(sc.tris), np.ascontiguousarray(sc.bvh_nodes)
        self.mats = np.ascontiguousarray(sc.materials_array())
        self.texs = [np.ascontiguousarray(t) for t in sc.textures]
        self.tex_array = orc._tex_array(self.texs)
        self.caller = np.ascontiguousarray(caller_tris)
        assert len(self.caller) == len(self.tris)

    def run(self, points, samples, depth, shading=0, cull=0, first_sample=0, stride=None):
        """-> dict: "sum" [n, 3] f32 (the samples added in order from +0), "mean" [n, 3] f32 (sum / f32(samples); 0 for a point
        without a surface, like the sum) and "first_hit" [n, samples] bool (the first scatter ray hit something; False for no point)"""
        lib, n = self.lib, len(points)
        stride = n if stride is None else stride
        args = (self.tris.ctypes.data, self.tris.nbytes // 112, self.nodes.ctypes.data, self.nodes.nbytes // 32, self.mats.ctypes.data,
                self.mats.nbytes // 80, self.tex_array, len(self.texs))
        total = np.zeros((n, 3), dtype=np.float32)
        first_hit = np.zeros((n, samples), dtype=bool)
        out, rs, cnt = _F3(), _F3(), (C.c_uint64 * 5)()
        with np.errstate(all="ignore"):
            for i in range(n):
                if int(points["prim"][i]) == NONE:
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
                    if shading == 0:
                        lib.orc_trace_ray(*args, C.byref(o), C.byref(d), depth, C.byref(st), cull, self.orc.LIBM_GLIBC235, C.byref(out))
                    else:
                        lib.orc_trace_ray_wgsl(*args, C.byref(o), C.byref(d), depth, C.byref(st), cull, self.orc.LIBM_GLIBC235, C.byref(out), C.byref(cnt))
                    acc = acc + np.array(list(out), dtype=np.float32)                            # f32 + f32, rounded once
                total[i] = acc
        none = points["prim"] == NONE
        mean = total / F(samples)
        mean[none] = 0
        return dict(sum=total, mean=mean, first_hit=first_hit)


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
